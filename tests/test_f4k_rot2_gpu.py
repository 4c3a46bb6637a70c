"""The "rot H" order at look-ahead two (csrc/f4k_rot.h, fft4096_rot2_kernel; the draw behind the row stores, the one form kept)
and, now that it is no longer what a plan takes unasked, at look-ahead three (fft4096_rot_kernel) against the grid-stride order:
plans created under SDRK_F4K_ORDER=ticket with SDRK_F4K_TICKET_FORM=rot2 / rot4 / rot8 and SDRK_F4K_ROT_AHEAD=2top / 3 must give
the bits of the grid-stride plan for every row — Hann and rectangular, dB rows and complex spectra, from one
frame (a grid of 8 workgroups, seven of which find no frame at all) over counts beside a multiple of 8 and beside the
768-workgroup grid to eight grids and a few — write nothing past the last row, and leave the heads at zero from call to call:
the same plan is called three times without a sync between and once more on a second stream, each call into rows of its own,
so that a frame some call skipped stays NaN.  The grid-stride rows are computed once per window (row f does not depend on the
length of the call) and shared.  The two no-arithmetic probes must run under each look-ahead."""
import ctypes

import numpy as np
import pytest

from oracle import cpu_ref
from tests.parity import assert_db_parity
from tests.test_f4k_ticket_gpu import _Dev, _HipStream, _frame, N, SEED

pytestmark = pytest.mark.gpu

COUNTS = (1, 7, 9, 767, 769, 2309, 6157)
FORMS = ("rot2", "rot4", "rot8")
AHEADS = ("2top", "3")
GUARD = 2
TOP = max(COUNTS)

_stride = {}


def _plan(monkeypatch, order, window, form=None, ahead=None):
    from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
    monkeypatch.setenv("SDRK_F4K_ORDER", order)
    for name, value in (("SDRK_F4K_TICKET_FORM", form), ("SDRK_F4K_ROT_AHEAD", ahead)):
        if value:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    return SpectrumPlan(N, window=window)


def _stride_rows(monkeypatch, window):
    """dB rows of the grid-stride plan for frames 0 .. TOP - 1 (read-only), once per window."""
    key = ("db", window)
    if key not in _stride:
        dev = _Dev()
        try:
            d_in = dev.alloc(TOP * N * 8)
            d_s = dev.alloc((TOP + GUARD) * N * 4)
            dev.ffi.check(dev.lib.sdrk_synth_fill(0, SEED, 0, TOP, N, ctypes.c_void_p(d_in), None))
            dev.put(d_s + TOP * N * 4, np.full((GUARD, N), np.nan, dtype=np.float32))
            with _plan(monkeypatch, "stride", window) as ps:
                ps.exec_device(d_in, TOP, d_s)
                ps.sync()
            ref = dev.rows(d_s, 0, TOP + GUARD)
        finally:
            dev.free()
        assert np.isfinite(ref[:TOP]).all() and np.isnan(ref[TOP:]).all()
        ref.setflags(write=False)
        _stride[key] = ref
    return _stride[key]


def _stride_spectra(monkeypatch, window, x):
    key = ("c64", window)
    if key not in _stride:
        with _plan(monkeypatch, "stride", window) as ps:
            ref = ps.fft(x)
        assert ref.shape == (TOP, N) and np.isfinite(ref.view(np.float32)).all()
        ref.setflags(write=False)
        _stride[key] = ref
    return _stride[key]


@pytest.mark.parametrize("window", ["hann", None])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ahead", AHEADS)
def test_rot2_rows_equal_stride_rows_call_after_call(monkeypatch, ahead, form, window):
    ref = _stride_rows(monkeypatch, window)
    what = f"{form} {ahead}"
    dev = _Dev()
    second = None
    region = TOP + GUARD                       # rows per call
    calls = 4                                  # three on the plan's stream, one on a second stream
    try:
        d_in = dev.alloc(TOP * N * 8)
        d_t = dev.alloc(calls * region * N * 4)
        dev.ffi.check(dev.lib.sdrk_synth_fill(0, SEED, 0, TOP, N, ctypes.c_void_p(d_in), None))
        second = _HipStream()
        w = np.hanning(N) if window == "hann" else None
        with _plan(monkeypatch, "ticket", window, form, ahead) as pt:
            for n in COUNTS:
                nan = np.full((n + GUARD, N), np.nan, dtype=np.float32)
                for c in range(calls):
                    dev.put(d_t + c * region * N * 4, nan)
                for c in range(3):
                    pt.exec_device(d_in, n, d_t + c * region * N * 4)
                pt.exec_device(d_in, n, d_t + 3 * region * N * 4, stream=second.handle.value)
                second.synchronize()
                pt.sync()
                for c in range(calls):
                    got = dev.rows(d_t, c * region, n + GUARD)
                    assert np.isnan(got[n:]).all(), f"{what}, {n} frames, call {c}: rows written past the end"
                    assert np.array_equal(got[:n].view(np.uint32), ref[:n].view(np.uint32)), \
                        f"{what}, {n} frames, call {c}: rows differ from grid-stride rows"
                for f in sorted({0, n - 1}):
                    assert_db_parity(got[f], cpu_ref.spectrum_db(_frame(f, N), window=w), what=f"{what}: frame {f} of {n}")
    finally:
        if second is not None:
            second.destroy()
        dev.free()


@pytest.mark.parametrize("window", ["hann", None])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ahead", AHEADS)
def test_rot2_complex_spectra_equal_stride_spectra(monkeypatch, ahead, form, window):
    from sdr_iq_visualizer_amd import synth
    what = f"{form} {ahead}"
    x = synth.synth_iq(SEED, 0, TOP, N)
    ref = _stride_spectra(monkeypatch, window, x)
    with _plan(monkeypatch, "ticket", window, form, ahead) as pt:
        for n in COUNTS:
            a = pt.fft(x[:n])
            assert a.shape == (n, N)
            assert np.array_equal(a.view(np.uint32), ref[:n].view(np.uint32)), f"{what}, {n} frames: spectra differ"
        a2 = pt.fft(x[:769])                                     # the heads were left at zero
        assert np.array_equal(a2.view(np.uint32), ref[:769].view(np.uint32)), f"{what}: a call after the longest"


@pytest.mark.parametrize("ahead", AHEADS)
def test_probes_run_under_each_look_ahead(monkeypatch, ahead):
    """sdrk_stream_ceiling_probe and sdrk_copy_probe over 2309 frame-equivalents (three grids and a few) and over one; the
    2:1 probe's output is the pairwise sum of its input whatever the order of the frames."""
    monkeypatch.setenv("SDRK_F4K_ORDER", "ticket")
    monkeypatch.delenv("SDRK_F4K_TICKET_FORM", raising=False)
    monkeypatch.setenv("SDRK_F4K_ROT_AHEAD", ahead)
    dev = _Dev()
    try:
        frames = 2309
        d_in = dev.alloc(frames * N * 8)
        d_out = dev.alloc((2 * frames + GUARD) * N * 4)
        dev.ffi.check(dev.lib.sdrk_synth_fill(0, SEED, 0, frames, N, ctypes.c_void_p(d_in), None))
        x = dev.rows(d_in, 0, 2 * frames)                        # a frame's 8 bytes per sample as two float32 rows
        mixed = x.reshape(frames, 8, 256, 4)
        mixed = (mixed[:, 0::2] + mixed[:, 1::2]).reshape(frames, N)
        ms = (ctypes.c_float * 3)()
        for n in (1, frames):
            dev.put(d_out, np.full((2 * n + GUARD, N), np.nan, dtype=np.float32))
            dev.ffi.check(dev.lib.sdrk_stream_ceiling_probe(0, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n, 3, ms))
            assert all(t > 0.0 for t in ms), list(ms)
            got = dev.rows(d_out, 0, n + GUARD)
            assert np.isnan(got[n:]).all() and np.array_equal(got[:n].view(np.uint32), mixed[:n].view(np.uint32)), f"2:1 probe, {n} frames"
            dev.ffi.check(dev.lib.sdrk_copy_probe(0, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n * N * 8, 3, ms))
            assert all(t > 0.0 for t in ms), list(ms)
            got = dev.rows(d_out, 0, 2 * n + GUARD)
            assert np.isnan(got[2 * n:]).all() and np.array_equal(got[:2 * n].view(np.uint32), x[:2 * n].view(np.uint32)), f"copy probe, {n} frames"
    finally:
        dev.free()

"""The "rot H" order at look-ahead two with the row stores left in flight across the turn (SDRK_F4K_ROT_AHEAD=2flow,
fft4096_flow2_kernel, csrc/fft4096.hip): the draw goes out ahead of the row stores, the first frame runs ahead of the steady loop
and a workgroup whose frame is at or past the end leaves for a drain loop, so that no wait of the steady loop covers the stores.
Plans created under SDRK_F4K_ORDER=ticket with SDRK_F4K_TICKET_FORM=rot2 / rot4 / rot8 must give the bits of the grid-stride plan
for every row — Hann and rectangular, dB rows and complex spectra — at the smallest counts at which that shape can go wrong:
one frame (a grid of 8 in which seven workgroups find nothing: the exit from the prologue, and the drain loop alone), counts
beside a multiple of 8 and beside the 768-workgroup grid (skipped frames, and frames that follow one), and three grids and a few
(several steady turns for every workgroup: a wait that is too lax would show as words of frame i + 1 read before they landed).
Nothing is written past the last row, a skipped frame stays NaN, and the heads are left at zero from call to call: the same plan
is called three times without a sync between and once more on a second stream, each call into rows of its own.  The grid-stride
rows are computed once per window and shared.  The two no-arithmetic probes must run under the new value."""
import ctypes

import numpy as np
import pytest

from oracle import cpu_ref
from tests.parity import assert_db_parity
from tests.test_f4k_ticket_gpu import _Dev, _HipStream, _frame, N, SEED

pytestmark = pytest.mark.gpu

COUNTS = (1, 7, 9, 767, 769, 2309)
FORMS = ("rot2", "rot4", "rot8")
AHEAD = "2flow"
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
def test_flow_rows_equal_stride_rows_call_after_call(monkeypatch, form, window):
    ref = _stride_rows(monkeypatch, window)
    what = f"{form} {AHEAD}"
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
        with _plan(monkeypatch, "ticket", window, form, AHEAD) as pt:
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
                    assert not np.isnan(got[:n]).any(), f"{what}, {n} frames, call {c}: a frame was skipped"
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
def test_flow_complex_spectra_equal_stride_spectra(monkeypatch, form, window):
    from sdr_iq_visualizer_amd import synth
    what = f"{form} {AHEAD}"
    x = synth.synth_iq(SEED, 0, TOP, N)
    ref = _stride_spectra(monkeypatch, window, x)
    with _plan(monkeypatch, "ticket", window, form, AHEAD) as pt:
        for n in COUNTS:
            a = pt.fft(x[:n])
            assert a.shape == (n, N)
            assert np.array_equal(a.view(np.uint32), ref[:n].view(np.uint32)), f"{what}, {n} frames: spectra differ"
        a2 = pt.fft(x[:769])                                     # the heads were left at zero
        assert np.array_equal(a2.view(np.uint32), ref[:769].view(np.uint32)), f"{what}: a call after the longest"


def test_probes_run_under_the_flow_look_ahead(monkeypatch):
    """sdrk_stream_ceiling_probe (in its form that leaves the stores in flight) and sdrk_copy_probe over 2309 frame-equivalents
    (three grids and a few) and over one; the 2:1 probe's output is the pairwise sum of its input whatever the order of the frames."""
    monkeypatch.setenv("SDRK_F4K_ORDER", "ticket")
    monkeypatch.delenv("SDRK_F4K_TICKET_FORM", raising=False)
    monkeypatch.setenv("SDRK_F4K_ROT_AHEAD", AHEAD)
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

"""The ticket order of the N = 4096 kernel (csrc/f4k_ticket.h, fft4096_ticket_kernel) against the grid-stride order: plans
created under SDRK_F4K_ORDER=ticket and =stride must give the same bits for every row — Hann and rectangular, dB rows and
complex spectra, from one frame (a grid of 8 workgroups, seven of which find no frame at all) over counts beside a multiple
of 8 and beside the 768-workgroup grid to a call of 128 grids — write nothing past the last row, and carry the heads from
call to call: the same plan is called three times without a sync between and once more on a second stream, each call into rows of
its own, so that a frame some call skipped stays NaN."""
import ctypes

import numpy as np
import pytest

from oracle import cpu_ref
from tests.parity import assert_db_parity

pytestmark = pytest.mark.gpu

N = 4096
COUNTS = (1, 7, 9, 767, 769, 2309)
GUARD = 2
SEED = 77


def _plan(monkeypatch, order, window):
    from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
    monkeypatch.setenv("SDRK_F4K_ORDER", order)
    return SpectrumPlan(N, window=window)


class _HipStream:
    """A second stream of the HIP runtime the library itself runs on: the symbols are looked up through the library's own
    handle, so they are those of the runtime it is linked against, whatever else the process has loaded."""

    def __init__(self):
        from sdr_iq_visualizer_amd import _ffi
        lib = _ffi.lib()
        self.create, self.sync, self.free = lib.hipStreamCreate, lib.hipStreamSynchronize, lib.hipStreamDestroy
        for fn in (self.create, self.sync, self.free):
            fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
        self.handle = ctypes.c_void_p()
        assert self.create(ctypes.byref(self.handle)) == 0

    def synchronize(self):
        assert self.sync(self.handle) == 0

    def destroy(self):
        assert self.free(self.handle) == 0


class _Dev:
    """A few device buffers, freed together."""

    def __init__(self):
        from sdr_iq_visualizer_amd import _ffi
        self.ffi, self.lib, self.bufs = _ffi, _ffi.lib(), []
        _ffi.require_device(0)

    def alloc(self, nbytes):
        d = ctypes.c_void_p()
        self.ffi.check(self.lib.sdrk_dev_alloc(0, nbytes, ctypes.byref(d)))
        self.bufs.append(d)
        return d.value

    def put(self, d, a):
        self.ffi.check(self.lib.sdrk_memcpy_h2d(0, ctypes.c_void_p(d), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def rows(self, d, f0, n):
        a = np.empty((n, N), dtype=np.float32)
        self.ffi.check(self.lib.sdrk_memcpy_d2h(0, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d + f0 * N * 4), a.nbytes))
        return a

    def free(self):
        for d in reversed(self.bufs):
            self.lib.sdrk_dev_free(0, d)


def _frame(f, hop):
    from sdr_iq_visualizer_amd import synth
    s0 = f * hop
    return synth.synth_iq(SEED, s0 // N, 2, N).reshape(-1)[s0 % N: s0 % N + N]


@pytest.mark.parametrize("window", ["hann", None])
def test_ticket_rows_equal_stride_rows_call_after_call(monkeypatch, window):
    dev = _Dev()
    second = None
    top = max(COUNTS)
    region = top + GUARD                       # rows per call
    calls = 4                                  # three on the plan's stream, one on a second stream
    try:
        d_in = dev.alloc(top * N * 8)
        d_t = dev.alloc(calls * region * N * 4)
        d_s = dev.alloc(region * N * 4)
        dev.ffi.check(dev.lib.sdrk_synth_fill(0, SEED, 0, top, N, ctypes.c_void_p(d_in), None))
        nan = np.full((region, N), np.nan, dtype=np.float32)
        second = _HipStream()
        w = np.hanning(N) if window == "hann" else None
        with _plan(monkeypatch, "ticket", window) as pt, _plan(monkeypatch, "stride", window) as ps:
            for n in COUNTS:
                for c in range(calls):
                    dev.put(d_t + c * region * N * 4, nan)
                dev.put(d_s, nan)
                for c in range(3):
                    pt.exec_device(d_in, n, d_t + c * region * N * 4)
                pt.exec_device(d_in, n, d_t + 3 * region * N * 4, stream=second.handle.value)
                ps.exec_device(d_in, n, d_s)
                second.synchronize()
                pt.sync()
                ps.sync()
                ref = dev.rows(d_s, 0, region)
                assert np.isfinite(ref[:n]).all() and np.isnan(ref[n:]).all()
                for c in range(calls):
                    got = dev.rows(d_t, c * region, region)
                    assert np.isnan(got[n:]).all(), f"{n} frames, call {c}: rows written past the end"
                    assert np.array_equal(got[:n].view(np.uint32), ref[:n].view(np.uint32)), \
                        f"{n} frames, call {c}: ticketed rows differ from grid-stride rows"
                for f in sorted({0, n - 1}):
                    assert_db_parity(ref[f], cpu_ref.spectrum_db(_frame(f, N), window=w), what=f"frame {f} of {n}")
    finally:
        if second is not None:
            second.destroy()
        dev.free()


@pytest.mark.parametrize("window", ["hann", None])
def test_ticket_complex_spectra_equal_stride_spectra(monkeypatch, window):
    from sdr_iq_visualizer_amd import synth
    x = synth.synth_iq(SEED, 0, max(COUNTS), N)
    with _plan(monkeypatch, "ticket", window) as pt, _plan(monkeypatch, "stride", window) as ps:
        for n in COUNTS:
            a, b = pt.fft(x[:n]), ps.fft(x[:n])
            assert a.shape == (n, N) and np.isfinite(b.view(np.float32)).all()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{n} frames: ticketed spectra differ"
            a2 = pt.fft(x[:n])                                   # the heads carry over
            assert np.array_equal(a2.view(np.uint32), b.view(np.uint32)), f"{n} frames, second call"


def test_ticket_long_call_equals_stride(monkeypatch):
    """98304 frames at hop 2048 (1.6 GB of input): 128 grids' worth of tickets in one launch, and the length at which the
    grid-stride call it is compared with is first cut into two.  The rows beside that cut, the first and the last go against
    the oracle."""
    n_frames, hop = 98304, 2048
    block = 8192
    dev = _Dev()
    try:
        samples = (n_frames - 1) * hop + N
        gen = -(-samples // N)
        d_in = dev.alloc(gen * N * 8)
        d_t = dev.alloc((n_frames + GUARD) * N * 4)
        d_s = dev.alloc(n_frames * N * 4)
        dev.ffi.check(dev.lib.sdrk_synth_fill(0, SEED, 0, gen, N, ctypes.c_void_p(d_in), None))
        dev.put(d_t + n_frames * N * 4, np.full((GUARD, N), np.nan, dtype=np.float32))
        with _plan(monkeypatch, "ticket", "hann") as pt, _plan(monkeypatch, "stride", "hann") as ps:
            pt.exec_device(d_in, n_frames, d_t, frame_stride=hop)
            ps.exec_device(d_in, n_frames, d_s, frame_stride=hop)
            pt.sync()
            ps.sync()
        assert np.isnan(dev.rows(d_t, n_frames, GUARD)).all(), "rows written past the end of the call"
        for f0 in range(0, n_frames, block):
            a, b = dev.rows(d_t, f0, block), dev.rows(d_s, f0, block)
            assert np.isfinite(b).all()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"rows {f0}..{f0 + block}: ticketed rows differ"
        w = np.hanning(N)
        for f in (0, n_frames // 2 - 1, n_frames // 2, n_frames - 1):
            assert_db_parity(dev.rows(d_t, f, 1)[0], cpu_ref.spectrum_db(_frame(f, hop), window=w), what=f"frame {f} (hop {hop})")
    finally:
        dev.free()

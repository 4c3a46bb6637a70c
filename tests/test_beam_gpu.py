"""The filter-and-sum beamformer on the GPU (sdrk_plan_set_beam, sdrk_exec_device_beam* / sdrk_exec_host_beam*): C coherent channels
filtered by their own taps, summed, tuned and decimated in one pass.  Against the down-converter where the two coincide (C = 1: bit
for bit), against itself (the integer forms are the complex64 form on the widened elements, the host entry is the device entry,
decimation is selection from D = 1, two channels commute: bit for bit) and against float64 numpy on the same elements —

    s = nearest bin;  v = sum_c np.convolve(x_c, h_c exp(+2 pi i s t / 4096), "valid");  out = v[i] exp(-2 pi i phase_i / 2^32),
    phase_i = freq_word * ((index0 + i) mod 2^32) mod 2^32 in exact integers, for the i with (index0 + i) % D == 0

never against the library.  The bound is the FIR bound added over the channels by the triangle inequality,
max |out - ref| <= REL_TOL * sum_c ||h_c||_1 * max|x_c| (tests/parity.py's 1e-5; the mixer's share is inside it, as in
tests/test_ddc_gpu.py).  Every check prints its worst err/tol.

Shapes: n_in = 2 L + 1000 + M - 1 is three blocks with a short last one; 40 blocks under SDRK_NUM_CUS=8 (16 workgroups) make every
workgroup walk two or three blocks of the grid-stride."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd import sigmf_io
from sdr_iq_visualizer_amd.spectrum import BeamStream, SpectrumPlan, beam_taps, ddc_taps, freq_word, iq8_to_c64
from tests.gpu_helpers import DevBuf, same_bits
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
GUARD = 64                                         # complex64 behind the last output, which must stay as they were
FAR = (1 << 40) + 3
FINE = 0x12345678                                  # bin 291.27
ON_A_BIN = (517 << 20) & 0xFFFFFFFF
SHAPES = [(1, 1), (33, 7), (257, 50), (2049, 200), (2049, 256)]     # (M, D)
CHANNELS = (1, 2, 3, 5, 8)
EDGE16 = np.array([[-32768, 32767], [32767, -32768], [-1, 0], [0, -1], [0, 0], [255, -256]], np.int16)


def block_len(m):
    return (4097 - m) // 256 * 256


def n_in_of(m, blocks=3):
    return (blocks - 1) * block_len(m) + 1000 + m - 1


def bin_of(word):
    return ((word + 0x80000) >> 20) & 4095


def filters(seed, c, m):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((c, m)) + 1j * rng.standard_normal((c, m))) / np.sqrt(2 * m)).astype(np.complex64)


def noise(seed, n, c):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n, c)) + 1j * rng.standard_normal((n, c))) / np.sqrt(2)).astype(np.complex64)


def elements16(seed, n, c):
    """(n, C, 2) int16 with the edge values planted in every channel, at the start, across a block boundary and at the end."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3000, 3000, (n, c, 2)).astype(np.int16)
    for at in (0, n // 2, n - len(EDGE16)):
        x[at:at + len(EDGE16)] = EDGE16[:, None, :]
    return x


def elements8(seed, n, c, dtype):
    """(n, C, 2) int8 / uint8, every byte value present, the edge bytes planted at both ends."""
    rng = np.random.default_rng(seed)
    lo, hi = (-128, 127) if dtype == np.int8 else (0, 255)
    x = rng.integers(lo, hi + 1, (n, c, 2)).astype(dtype)
    x[0], x[1], x[-2], x[-1] = lo, hi, hi, lo
    x[2, :, 0], x[2, :, 1] = lo, hi
    return x


def widen_elements(x):
    """(n, C, 2) int16 / int8 / uint8 -> (n, C) complex64, exactly as the library widens."""
    if x.dtype == np.int16:
        return np.ascontiguousarray(x).astype(np.float32).view(np.complex64).reshape(x.shape[0], x.shape[1])
    return iq8_to_c64(x)


def ref_beam(x, h, word, d, index0):
    """float64: per channel the valid convolution with its filter on the nearest bin, summed; the mixer; the kept."""
    c, m = h.shape
    rot = np.exp(2j * np.pi * bin_of(word) * np.arange(m) / N)
    v = sum(np.convolve(x[:, k].astype(np.complex128), h[k].astype(np.complex128) * rot, "valid") for k in range(c))
    i = np.arange(v.shape[0], dtype=np.uint64)
    idx32 = (np.uint64(index0) + i) & np.uint64(0xFFFFFFFF)
    phase = (np.uint64(word) * idx32) & np.uint64(0xFFFFFFFF)
    y = v * np.exp(-2j * np.pi * (phase.astype(np.float64) / 2.0 ** 32))
    return y[((np.uint64(index0 % d) + i) % np.uint64(d)) == 0]


def tol_of(x, h):
    x, h = x.astype(np.complex128), h.astype(np.complex128)
    return REL_TOL * float(sum(np.abs(h[k]).sum() * np.abs(x[:, k]).max() for k in range(h.shape[0])))


WORST = {}


def check(got, ref, tol, what):
    assert got.shape == ref.shape and got.dtype == np.complex64, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), what
    w = float(np.abs(got.astype(np.complex128) - ref).max()) / tol
    WORST[what] = w
    print(f"{what}: err/tol {w:.2e}")
    assert w <= 1.0, (what, w)
    return w


class _HipStream:
    """A second stream of the HIP runtime the library itself runs on (looked up through the library's own handle)."""

    def __init__(self):
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


class Dev:
    """Elements resident on the device — their first element `skip` SAMPLES past the allocation's start, so the stream is aligned
    to a sample and not to an element — and an output buffer whose GUARD samples behind the last output must stay untouched."""

    def __init__(self, x, skip=0):
        self.x, self.n_in = np.ascontiguousarray(x), x.shape[0]
        self.kind = "" if x.dtype == np.complex64 else "_ci16" if x.dtype == np.int16 else "_ci8"
        self.sample = 8 if self.kind == "" else 4 if self.kind == "_ci16" else 2
        self.d_in, self.d_out = DevBuf(self.x.nbytes + skip * self.sample), DevBuf((self.n_in + GUARD) * 8)
        self.p_in = self.d_in.p.value + skip * self.sample
        _ffi.check(_ffi.lib().sdrk_memcpy_h2d(0, ctypes.c_void_p(self.p_in), self.x.ctypes.data_as(ctypes.c_void_p), self.x.nbytes))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.d_in.__exit__()
        self.d_out.__exit__()

    def beam(self, plan, word, d, index0=0, stream=None):
        n_out = plan.beam_outputs(self.n_in, d, index0)
        self.d_out.put(np.full(n_out + GUARD, np.nan + 1j * np.nan, np.complex64))
        kw = {"unsigned": self.x.dtype == np.uint8} if self.kind == "_ci8" else {}
        getattr(plan, "exec_device_beam" + self.kind)(self.p_in, self.n_in, self.d_out.p.value, word, decim=d, index0=index0,
                                                      stream=stream.handle.value if stream else 0, **kw)
        if stream:
            stream.synchronize()
        plan.sync()
        got = self.d_out.get(n_out + GUARD, np.complex64)
        assert np.all(np.isnan(got[n_out:].real)), "stored past n_out"
        return got[:n_out]

    def ddc(self, plan, word, d, index0=0):
        """The single-channel down-converter on the same buffer (C = 1 elements are samples)."""
        n_out = plan.ddc_outputs(self.n_in, d, index0)
        self.d_out.put(np.full(n_out + GUARD, np.nan + 1j * np.nan, np.complex64))
        kw = {"unsigned": self.x.dtype == np.uint8} if self.kind == "_ci8" else {}
        getattr(plan, "exec_device_ddc" + self.kind)(self.p_in, self.n_in, self.d_out.p.value, word, decim=d, index0=index0, **kw)
        plan.sync()
        return self.d_out.get(n_out, np.complex64)


@pytest.fixture(params=[None, "8"], ids=["all_cus", "8_cus"])
def cus(request, monkeypatch):
    """The plans made in the test size their grids for the whole device, or for 8 CUs (read when a plan is made)."""
    if request.param:
        monkeypatch.setenv("SDRK_NUM_CUS", request.param)
    else:
        monkeypatch.delenv("SDRK_NUM_CUS", raising=False)
    return request.param


def sizes_of(m, cus):
    return [n_in_of(m)] + ([n_in_of(m, 40)] if cus else [])


# ---- 1. one channel is the down-converter --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", SHAPES)
def test_one_channel_gives_the_bits_of_the_down_converter(m, d, cus):
    """C = 1 against ddc / ddc_ci16 / ddc_ci8 on a plan with set_fir(h_0): bit for bit.  A stream of -0.0 keeps the signs of its
    zeros (channel 0 starts the sum as it is, it is not added to +0.0); an Inf reaches the outputs at word 0 (no mixer runs)."""
    h = filters(m, 1, m)
    for n_in in sizes_of(m, cus):
        x = noise(m + 1, n_in, 1)
        x[5, 0] = np.complex64(complex(-0.0, -0.0))
        minus = np.full((n_in, 1), np.complex64(complex(-0.0, -0.0)), np.complex64)
        inputs = (x, minus, elements16(m + 2, n_in, 1), elements8(m + 3, n_in, 1, np.int8), elements8(m + 4, n_in, 1, np.uint8))
        with SpectrumPlan(N) as plan:
            plan.set_beam(h)
            plan.set_fir(h[0])
            assert (plan.beam_channels, plan.beam_taps, plan.fir_taps) == (1, m, m)
            for xin in inputs:
                with Dev(xin) as dev:
                    for word in (0, ON_A_BIN, FINE):
                        for index0 in (0, d + 1 if d > 1 else 1, FAR):
                            a, b = dev.beam(plan, word, d, index0), dev.ddc(plan, word, d, index0)
                            assert a.shape[0] == plan.beam_outputs(n_in, d, index0)
                            assert same_bits(a, b), (m, d, xin.dtype, hex(word), index0)
            x[n_in - 3, 0] = np.complex64(complex(np.inf, 1.0))
            with Dev(x) as dev:
                assert np.isnan(dev.beam(plan, 0, 1, 0)[-1].real) and np.isnan(dev.ddc(plan, 0, 1, 0)[-1].real)


# ---- 2. the integer forms are the complex64 form on the widened elements -------------------------------------------------------------
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("m,d", SHAPES)
def test_integer_forms_give_the_bits_of_the_complex64_form_and_float64_parity(m, d, c, cus):
    h = filters(10 * m + c, c, m)
    for n_in in sizes_of(m, cus):
        narrow = (elements16(m + c, n_in, c), elements8(m + c + 1, n_in, c, np.int8), elements8(m + c + 2, n_in, c, np.uint8))
        with SpectrumPlan(N) as plan:
            plan.set_beam(h)
            for xin in narrow:
                wide = widen_elements(xin)
                with Dev(xin, skip=1) as dn, Dev(wide, skip=1) as dw:           # one sample past the allocation's start
                    for word, index0 in ((0, 0), (ON_A_BIN, d // 2 + 1), (FINE, FAR)):
                        a, b = dn.beam(plan, word, d, index0), dw.beam(plan, word, d, index0)
                        assert a.shape[0] > 0 and same_bits(a, b), (m, d, c, xin.dtype, hex(word), index0)
                    if n_in == n_in_of(m):
                        check(b, ref_beam(wide, h, FINE, d, FAR), tol_of(wide, h), f"C={c} M={m} D={d} {xin.dtype}")
            if n_in == n_in_of(m):
                x = noise(m + c + 3, n_in, c)
                with Dev(x) as dx:
                    for word, index0 in ((0, 1), (FINE, 0)):
                        check(dx.beam(plan, word, d, index0), ref_beam(x, h, word, d, index0), tol_of(x, h),
                              f"C={c} M={m} D={d} unit noise word={word:#x}")


# ---- 3. the host entry is the device entry on prefix || iq ---------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("c,m,d", [(1, 33, 7), (3, 257, 50), (8, 2049, 200), (5, 1, 1)])
def test_host_entry_gives_the_bits_of_the_device_entry(c, m, d, pinned, monkeypatch):
    import sdr_iq_visualizer_amd as pkg
    monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "3")
    h = filters(c + m, c, m)
    n = 7 * block_len(m) + 321                                                   # three chunks, the last one short
    with SpectrumPlan(N) as plan:
        plan.set_beam(h)
        for xin in (noise(c, n + m - 1, c), elements16(c + 1, n + m - 1, c), elements8(c + 2, n + m - 1, c, np.uint8)):
            kind = "" if xin.dtype == np.complex64 else "_ci16" if xin.dtype == np.int16 else "_ci8"
            pre, iq = xin[:m - 1], xin[m - 1:]
            if pinned:
                keep = pkg.pinned_empty(iq.shape, iq.dtype)
                keep[...] = iq
                iq = keep
            for word, s0 in ((FINE, FAR), (0, 0)):
                got = getattr(plan, "beam" + kind)(iq, word, decim=d, prefix=pre if m > 1 else None, sample0=s0)
                with Dev(xin) as dev:
                    assert same_bits(got, dev.beam(plan, word, d, s0)), (c, m, d, kind, hex(word))
            # a NULL prefix: elements of byte 0, of byte 0x80 for cu8
            silent = np.full((m - 1,) + xin.shape[1:], 128 if xin.dtype == np.uint8 else 0, xin.dtype)
            with Dev(np.concatenate((silent, xin[m - 1:]))) as dev:
                assert same_bits(getattr(plan, "beam" + kind)(xin[m - 1:], FINE, decim=d, sample0=3), dev.beam(plan, FINE, d, 3))


# ---- 4. decimation is selection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,m", [(2, 33), (5, 257), (8, 2049)])
def test_decimation_is_selection_from_the_undecimated_call(c, m, cus):
    h = filters(c * m, c, m)
    for n_in in sizes_of(m, cus):
        with SpectrumPlan(N) as plan, Dev(noise(c + m, n_in, c)) as dx, Dev(elements8(c + m, n_in, c, np.int8)) as d8:
            plan.set_beam(h)
            for index0 in (0, 1, FAR):
                for dev in (dx, d8):
                    full = dev.beam(plan, FINE, 1, index0)
                    assert full.shape[0] == n_in - m + 1
                    for d in (7, 50, 200, 256):
                        got = dev.beam(plan, FINE, d, index0)
                        assert same_bits(got, full[(d - index0 % d) % d::d]), (c, m, d, index0)


# ---- 5. / 6. the sum: two channels commute, a silent filter adds only zeros ---------------------------------------------------------
@pytest.mark.parametrize("m,d", [(33, 7), (2049, 200)])
def test_two_channels_commute_and_a_zero_filter_changes_signs_of_zero_only(m, d, cus):
    n_in = sizes_of(m, cus)[-1]
    h2, x2 = filters(m, 2, m), noise(m + 9, n_in, 2)
    with SpectrumPlan(N) as plan:
        plan.set_beam(h2)
        with Dev(x2) as dev:
            a = dev.beam(plan, FINE, d, 5)
        plan.set_beam(h2[::-1])
        with Dev(x2[:, ::-1]) as dev:
            assert same_bits(a, dev.beam(plan, FINE, d, 5)), "a float add commutes"
        x3 = noise(m + 10, n_in, 3)
        h3 = filters(m + 1, 3, m)
        h3[1] = 0
        plan.set_beam(h3)
        with Dev(x3) as dev:
            three = dev.beam(plan, 0, d, 0)
        plan.set_beam(h3[[0, 2]])
        with Dev(x3[:, [0, 2]]) as dev:
            two = dev.beam(plan, 0, d, 0)
        assert np.all(np.isfinite(three.view(np.float32))) and np.array_equal(three, two)


# ---- 7. streams, streams of the caller, repeated calls ------------------------------------------------------------------------------
def test_beam_stream_in_uneven_pieces_equals_one_call():
    """Ragged pieces: every push is a call of its own on tail || piece, its blocks cut from the piece's first element, so the pieces
    equal one call within the bound (the header promises no equal bits between different cuts of a stream, as for DdcStream); one
    push is one call, bit for bit.  Pieces of uneven numbers of whole blocks, which see the blocks of one call, are the next test."""
    c, m, d = 3, 257, 50
    h = filters(77, c, m)
    n = 5 * block_len(m) + 77
    for xin in (noise(1, n, c), elements16(2, n, c), elements8(3, n, c, np.int8), elements8(4, n, c, np.uint8)):
        kind = "" if xin.dtype == np.complex64 else "_ci16" if xin.dtype == np.int16 else "_ci8"
        with SpectrumPlan(N) as plan:
            with BeamStream(plan, h, d, 123456.0, 2.4e6) as bs:
                cuts = [0, 1, 300, 300, 4097, 9000, n]
                pieces = [bs.push(xin[a:b]) for a, b in zip(cuts, cuts[1:])]
                assert bs.sample_index == n and bs.channels == c
            whole = getattr(plan, "beam" + kind)(xin, freq_word(123456.0, 2.4e6), decim=d)
            # every piece is a call of its own on tail || piece: the bound holds per piece, the bits for the first one
            assert np.concatenate(pieces).shape == whole.shape
            one = BeamStream(plan, h, d, 123456.0, 2.4e6).push(xin)
            assert same_bits(one, whole)
            wide = xin if kind == "" else widen_elements(xin)
            pad = np.full((m - 1, c), 0.5 + 0.5j if xin.dtype == np.uint8 else 0, np.complex64)
            ref = ref_beam(np.concatenate((pad, wide)), h, freq_word(123456.0, 2.4e6), d, 0)
            check(np.concatenate(pieces), ref, tol_of(wide, h), f"BeamStream pieces {xin.dtype}")
            check(whole, ref, tol_of(wide, h), f"BeamStream whole {xin.dtype}")


def test_pieces_cut_on_block_boundaries_give_the_bits_of_one_call():
    """Pieces of whole blocks of outputs see the blocks one call sees: BeamStream fed in uneven multiples of L equals one call."""
    c, m, d = 2, 257, 7
    L, h = block_len(m), filters(5, c, m)
    x = noise(6, 6 * L + 99, c)
    with SpectrumPlan(N) as plan:
        with BeamStream(plan, h, d, -40e3, 1e6) as bs:
            cuts = [0, L, 3 * L, 4 * L, x.shape[0]]
            got = np.concatenate([bs.push(x[a:b]) for a, b in zip(cuts, cuts[1:])])
        assert same_bits(got, plan.beam(x, freq_word(-40e3, 1e6), decim=d))


def test_a_callers_stream_repeated_calls_and_a_ddc_call_between_them():
    c, m, d = 5, 257, 50
    h, x = filters(8, c, m), noise(9, n_in_of(m), c)
    rows_in = noise(10, 4 * N, 1).reshape(4, N)
    with SpectrumPlan(N) as plan, Dev(x) as dev, Dev(np.ascontiguousarray(x[:, :1])) as one:
        rows = plan.spectrum_db(rows_in)
        plan.set_beam(h)
        plan.set_fir(h[2])
        first = dev.beam(plan, FINE, d, FAR)
        side = _HipStream()
        try:
            assert same_bits(dev.beam(plan, FINE, d, FAR, stream=side), first)
        finally:
            side.destroy()
        between = one.ddc(plan, FINE, d, FAR)
        assert same_bits(dev.beam(plan, FINE, d, FAR), first)
        assert same_bits(one.ddc(plan, FINE, d, FAR), between)
        assert (plan.beam_channels, plan.beam_taps, plan.fir_taps) == (c, m, m)
        assert same_bits(plan.spectrum_db(rows_in), rows), "rows of a plain spectrum call are unchanged around a beam call"
        ms = plan.exec_device_beam_timed_each(dev.p_in, dev.n_in, dev.d_out.p.value, FINE, 2, decim=d, index0=FAR)
        assert len(ms) == 2 and all(v > 0 for v in ms)
        assert same_bits(dev.d_out.get(first.shape[0], np.complex64), first)


# ---- known answers: a plane wave on a uniform line ----------------------------------------------------------------------------------
def _line(phi, amp, tone_bin, n, c=5):
    s = amp * np.exp(2j * np.pi * tone_bin * np.arange(n) / N)
    return s[:, None] * np.exp(1j * phi * np.arange(c))[None, :], np.exp(1j * phi * np.arange(c))


def test_known_plane_wave_steered_nulled_and_a_second_source_behind_the_null():
    c, m, d, B = 5, 257, 8, 517
    n = n_in_of(m)
    taps = ddc_taps(d, m)
    word = (B << 20) & 0xFFFFFFFF                                                # the tone lands at DC
    gain = abs(np.sum(taps.astype(np.complex128)))                               # the low-pass at DC
    x1, a1 = _line(0.7, 100.0, B, n)
    x2, a2 = _line(-1.1, 1.0, B, n)                                              # 40 dB down, from another direction
    steer = a1 / c                                                               # w^H a1 = 1
    null = np.array([1.0, -np.exp(0.7j), 0, 0, 0]) / 2                           # w^H a1 = (1 - 1) / 2 = 0
    assert abs(np.vdot(steer, a1) - 1) < 1e-12 and abs(np.vdot(null, a1)) < 1e-12
    with SpectrumPlan(N) as plan:
        def run(x, w):
            plan.set_beam(beam_taps(w, taps))
            x = x.astype(np.complex64)
            with Dev(x) as dev:
                return dev.beam(plan, word, d, 0), tol_of(x, beam_taps(w, taps))
        y, tol = run(x1, steer)
        assert np.abs(np.abs(y) - 100.0 * gain).max() <= tol, "weights a/C return the tone at its single-channel amplitude"
        for k in range(c):                                                       # each channel alone carries the tone
            y, tol = run(x1, np.eye(c)[k])
            assert np.abs(np.abs(y) - 100.0 * gain).max() <= tol
        y, tol = run(x1, null)
        print(f"nulled: |out| max {np.abs(y).max():.3e}, bound {tol:.3e}")
        assert np.abs(y).max() <= tol, "weights orthogonal to a leave nothing but rounding"
        y, tol = run(x1 + x2, null)
        left = abs(np.vdot(null, a2)) * 1.0 * gain
        assert left > 50 * tol and np.abs(np.abs(y) - left).max() <= tol, "the second source comes through at |w^H a2|"


# ---- refusals, the CLI ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_working():
    lib = _ffi.lib()
    c, m = 3, 33
    h, x = filters(1, c, m), noise(2, N, c)
    n_out, each = ctypes.c_size_t(0), (ctypes.c_float * 2)()
    out = np.empty(N, np.complex64)

    def invalid(rc, word):
        return rc == _ffi.SDRK_ERR_INVALID and word in lib.sdrk_last_error()

    with SpectrumPlan(N) as p, SpectrumPlan(8192) as big, DevBuf(x.nbytes + N * 8) as d:
        d.put(x)
        d_out = ctypes.c_void_p(d.p.value + x.nbytes)
        hp = h.ctypes.data_as(ctypes.c_void_p)
        assert lib.sdrk_plan_beam_channels(p.handle) == 0 and lib.sdrk_plan_beam_taps(p.handle) == 0
        assert invalid(lib.sdrk_exec_device_beam(p.handle, d.p, N, FINE, 7, 0, d_out, None), b"sdrk_plan_set_beam")
        assert invalid(lib.sdrk_exec_host_beam(p.handle, None, x.ctypes.data_as(ctypes.c_void_p), N, FINE, 7, 0,
                                               out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_out)), b"sdrk_plan_set_beam")
        for bad in (0, 9):
            assert invalid(lib.sdrk_plan_set_beam(p.handle, bad, m, hp), b"channels")
        for bad in (0, 2050):
            assert invalid(lib.sdrk_plan_set_beam(p.handle, c, bad, hp), b"ntaps")
        assert invalid(lib.sdrk_plan_set_beam(p.handle, c, m, None), b"NULL")
        assert lib.sdrk_plan_set_beam(big.handle, c, m, hp) == _ffi.SDRK_ERR_UNSUPPORTED
        with SpectrumPlan(N, precision="double") as dbl:
            assert lib.sdrk_plan_set_beam(dbl.handle, c, m, hp) == _ffi.SDRK_ERR_INVALID
        p.set_beam(h)
        assert lib.sdrk_plan_beam_channels(p.handle) == c and lib.sdrk_plan_beam_taps(p.handle) == m
        for bad in (0, 257):
            assert invalid(lib.sdrk_exec_device_beam(p.handle, d.p, N, FINE, bad, 0, d_out, None), b"decim")
        assert invalid(lib.sdrk_exec_device_beam(p.handle, d.p, m - 1, FINE, 7, 0, d_out, None), b"taps")
        assert invalid(lib.sdrk_exec_device_beam(p.handle, None, N, FINE, 7, 0, d_out, None), b"NULL")
        assert invalid(lib.sdrk_exec_device_beam_ci16(p.handle, d.p, N, FINE, 7, 0, None, None), b"NULL")
        assert lib.sdrk_exec_device_beam_iq8(p.handle, d.p, 2, N, FINE, 7, 0, d_out, None) == _ffi.SDRK_ERR_INVALID
        assert b"iq8_format" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_beam_timed_each(p.handle, d.p, N, FINE, 7, 0, d_out, 0, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_beam(p.handle, None, x.ctypes.data_as(ctypes.c_void_p), N, FINE, 7, 0,
                                       out.ctypes.data_as(ctypes.c_void_p), None) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError, match="channels"):
            p.beam(x[:, :2], FINE)
        got = p.beam(x, FINE, decim=7)
        check(got, ref_beam(np.concatenate((np.zeros((m - 1, c)), x)), h, FINE, 7, 0), tol_of(x, h), "after the refusals")


def test_cli_extract_with_weights_on_cu8_matches_the_same_samples_as_cf32(tmp_path):
    c, d, fs = 3, 50, 2.4e6
    x8 = elements8(31, 3 * N + 500, c, np.uint8)
    w = np.exp(0.4j * np.arange(c)) / c
    np.save(tmp_path / "w.npy", w)
    sigmf_io.write_sigmf(str(tmp_path / "rec8"), x8, fs, 100e6, datatype="cu8", num_channels=c)
    sigmf_io.write_sigmf(str(tmp_path / "rec32"), iq8_to_c64(x8), fs, 100e6, num_channels=c)
    env = dict(os.environ, PYTHONPATH=REPO)
    outs = []
    for name in ("rec8", "rec32"):
        r = subprocess.run([sys.executable, "-m", "sdr_iq_visualizer_amd.cli", "extract", str(tmp_path / name), "--weights",
                            str(tmp_path / "w.npy"), "--offset-hz", "250e3", "--decim", str(d), "--exact", "--out",
                            str(tmp_path / (name + "_out"))], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        report = json.loads(r.stdout.strip().splitlines()[-1])
        assert report["channels"] == c and report["decim"] == d and report["freq_word"] == freq_word(250e3, fs)
        outs.append(sigmf_io.read_sigmf(str(tmp_path / (name + "_out")))[0])
    # the cu8 stream starts from bytes of 128 (+0.5 + 0.5j), the cf32 one from zeros: the first BLOCK's transform sees other
    # samples (every output of it differs in rounding, those within M - 1 of the start in value); equal from the second block on
    m = ddc_taps(d).shape[0]
    skip = -(-block_len(m) // d)
    tol = REL_TOL * float(np.abs(beam_taps(w, ddc_taps(d))).sum()) * 128 * np.sqrt(2)
    assert np.abs(outs[0][(m - 1 + d - 1) // d:skip] - outs[1][(m - 1 + d - 1) // d:skip]).max() <= 2 * tol
    assert outs[0].shape == outs[1].shape and outs[0].shape[0] == (x8.shape[0] + d - 1) // d
    assert same_bits(outs[0][skip:], outs[1][skip:])
    r = subprocess.run([sys.executable, "-m", "sdr_iq_visualizer_amd.cli", "extract", str(tmp_path / "rec8"), "--offset-hz", "0",
                        "--decim", "2", "--out", str(tmp_path / "no")], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "extract takes a single-channel recording" in r.stderr

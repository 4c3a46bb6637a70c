"""The digital down-converter on the GPU (sdrk_exec_device_ddc* / sdrk_exec_host_ddc* / sdrk_exec_*_ddcbank*): tuning by a 32-bit
frequency word and any integer decimation in one pass, against the FIR call where the two coincide (bit for bit), against itself
(decimation is selection from D = 1, the bank is the single call, the host entry is the device entry: bit for bit) and against
float64 numpy on the same samples — the definition of include/sdrk.h:

    s = nearest bin;  v = np.convolve(x, h exp(+2 pi i s t / 4096), "valid");  out = v[i] exp(-2 pi i phase_i / 2^32),
    phase_i = freq_word * ((index0 + i) mod 2^32) mod 2^32 in exact integers, for the i with (index0 + i) % D == 0

never against the library.  The bound is the FIR call's: max |out - ref| <= REL_TOL * ||h||_1 * max|x| (tests/parity.py's 1e-5); the
NCO adds at most about 1.5e-7 |v| to the FIR call's error, 1.5 % of the bound.  Every check prints its worst err/tol.

Filter lengths M = 1, 257, 801, 2049 (L = 4096, 3840, 3072, 2048) and inputs of three blocks plus a ragged tail, n_in = M and a
600-block run: the smallest that cover a block boundary with b L % D != 0, a clipped last block, lanes with rel0 < 0 and D > 128
against L = 2048, where the number of outputs varies per block.

Measured on the device (profiles/ddc/SUMMARY.md): worst err/tol 7.6e-2 (M = 1), 8.3e-3 to 1.2e-2 at the longer
filters and 2.0e-3 over 600 blocks; the known tone's worst deviation from its first output 2.7e-2 of 2 tol, 69.35 turns under bin tuning."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd.spectrum import DdcBankStream, DdcStream, SpectrumPlan, ddc_taps, freq_word, freq_word_hz
from tests.gpu_helpers import DevBuf, same_bits, stream16_planted, widen_flat
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
GUARD = 64   # complex64 behind the last output, which must stay as they were
TAPS = (1, 257, 801, 2049)
FAR = (1 << 40) + 3
FINE = 0x12345678                                  # bin 291.27
SUBSET_FOR_8_CUS = "not everything_above"          # (not this test itself)


def block_len(m):
    return (4097 - m) // 256 * 256


def n_in_of(m):
    return 3 * block_len(m) + m - 1 + 123          # three whole blocks of outputs and a ragged fourth


def bin_of(word):
    return ((word + 0x80000) >> 20) & 4095


def ref_ddc(x, h, word, d, index0):
    """float64: the valid convolution with the filter on the nearest bin, the mixer with its phase in exact integers, the kept."""
    m = h.shape[0]
    hs = h.astype(np.complex128) * np.exp(2j * np.pi * bin_of(word) * np.arange(m) / N)
    v = np.convolve(x.astype(np.complex128), hs, "valid")
    i = np.arange(v.shape[0], dtype=np.uint64)
    idx32 = (np.uint64(index0) + i) & np.uint64(0xFFFFFFFF)
    phase = (np.uint64(word) * idx32) & np.uint64(0xFFFFFFFF)                   # (< 2^64: exact)
    y = v * np.exp(-2j * np.pi * (phase.astype(np.float64) / 2.0 ** 32))
    return y[((np.uint64(index0 % d) + i) % np.uint64(d)) == 0]


def tol_of(x, h):
    return REL_TOL * float(np.abs(h.astype(np.complex128)).sum()) * float(np.abs(x.astype(np.complex128)).max())


def random_taps(seed, m):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2 * m)).astype(np.complex64)


def noise(seed, n):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def brute(n_in, m, d, index0):
    i_first = (d - index0 % d) % d
    return 0 if i_first > n_in - m else (n_in - m - i_first) // d + 1


class Dev:
    """An input resident on the device and an output buffer behind it: the device entries of a plan, with the GUARD samples behind
    the last output checked to be untouched."""

    def __init__(self, x, planes=1):
        self.x, self.n_in, self.ci16 = x, x.shape[0], x.dtype == np.int16
        self.room = planes * (self.n_in + GUARD)
        self.d_in, self.d_out = DevBuf(x.nbytes), DevBuf(self.room * 8)
        self.d_in.put(x)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.d_in.__exit__()
        self.d_out.__exit__()

    def _fresh(self, n):
        self.d_out.put(np.full(n, np.nan + 1j * np.nan, np.complex64))

    def ddc(self, plan, word, d, index0=0):
        n_out = plan.ddc_outputs(self.n_in, d, index0)
        self._fresh(n_out + GUARD)
        (plan.exec_device_ddc_ci16 if self.ci16 else plan.exec_device_ddc)(self.d_in.p.value, self.n_in, self.d_out.p.value, word,
                                                                          decim=d, index0=index0)
        plan.sync()
        got = self.d_out.get(n_out + GUARD, np.complex64)
        assert np.all(np.isnan(got[n_out:].real)), "stored past n_out"
        return got[:n_out]

    def fir(self, plan, d, s, phase0):
        n_out = plan.fir_outputs(self.n_in, d)
        self._fresh(n_out + GUARD)
        (plan.exec_device_fir_ci16 if self.ci16 else plan.exec_device_fir)(self.d_in.p.value, self.n_in, self.d_out.p.value, decim=d,
                                                                          shift_bins=s, phase0=phase0)
        plan.sync()
        return self.d_out.get(n_out, np.complex64)

    def bank(self, plan, words, d, index0=0, pad=0):
        n_out = plan.ddc_outputs(self.n_in, d, index0)
        stride = n_out + pad
        self._fresh(len(words) * stride + GUARD)
        (plan.exec_device_ddc_bank_ci16 if self.ci16 else plan.exec_device_ddc_bank)(
            self.d_in.p.value, self.n_in, self.d_out.p.value, words, decim=d, index0=index0, out_stride=stride if pad else None)
        plan.sync()
        got = self.d_out.get(len(words) * stride + GUARD, np.complex64)
        planes = got[: len(words) * stride].reshape(len(words), stride)
        assert np.all(np.isnan(planes[:, n_out:].real)) and np.all(np.isnan(got[len(words) * stride:].real)), "stored outside the planes"
        return planes[:, :n_out]


def check(got, ref, tol, what):
    assert got.shape == ref.shape and got.dtype == np.complex64, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), what
    if got.shape[0] == 0:
        return 0.0
    w = float(np.abs(got.astype(np.complex128) - ref).max()) / tol
    print(f"{what}: err/tol {w:.2e}")
    assert w <= 1.0, (what, w)
    return w


# ---- 1. the bits of the existing call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TAPS)
def test_a_word_on_a_bin_gives_the_bits_of_the_fir_call(m):
    """freq_word = s << 20, D a power of two, index0 a multiple of D: sdrk_exec_device_fir with phase0 = s index0 mod 4096, bit
    for bit, from complex64 and from int16; at s = 0 with -0.0 and Inf among the samples (no mixer runs: they pass as they are)."""
    n_in = n_in_of(m)
    x = noise(m, n_in)
    special = x.copy()
    special[5] = np.complex64(complex(-0.0, -0.0))
    special[m + 17] = np.complex64(complex(-0.0, 3.0))
    special[n_in - 40] = np.complex64(complex(np.inf, 1.0))                     # (the last block: NaN from there on, in both calls)
    x16 = stream16_planted(m + 1, n_in)
    with SpectrumPlan(N) as plan, Dev(x) as dx, Dev(special) as dsp, Dev(x16) as d16:
        plan.set_fir(random_taps(m, m))
        for d in (1, 2, 16, 256):
            for index0 in (0, (1 << 40) + 256 * 5):
                for s in (0, 1, -7, 2047, -2048):
                    word, phase0 = (s << 20) & 0xFFFFFFFF, (s * index0) % N
                    for dev in (dx, d16) + ((dsp,) if s == 0 else ()):
                        a, b = dev.ddc(plan, word, d, index0), dev.fir(plan, d, s, phase0)
                        assert a.shape[0] == (n_in - m) // d + 1
                        assert same_bits(a, b), (m, d, s, index0, dev.ci16)
        assert np.isnan(dsp.ddc(plan, 0, 1, 0)[-1].real)                        # (the Inf did reach the outputs)


# ---- 2. decimation is selection ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TAPS)
def test_decimation_is_selection_from_the_undecimated_call(m):
    n_in = n_in_of(m)
    with SpectrumPlan(N) as plan, Dev(noise(m + 2, n_in)) as dx, Dev(stream16_planted(m + 3, n_in)) as d16:
        plan.set_fir(random_taps(m + 1, m))
        lib = _ffi.lib()
        for index0 in (0, 1, FAR):
            for dev in (dx, d16):
                full = dev.ddc(plan, FINE, 1, index0)
                assert full.shape[0] == n_in - m + 1
                for d in (3, 5, 6, 7, 10, 12, 50, 100, 125, 200, 255, 256):
                    got = dev.ddc(plan, FINE, d, index0)
                    i_first = (d - index0 % d) % d
                    assert got.shape[0] == lib.sdrk_ddc_outputs(n_in, m, d, index0) == brute(n_in, m, d, index0)
                    assert same_bits(got, full[i_first::d]), (m, d, index0, dev.ci16)


def test_one_output_and_none():
    for m in TAPS:
        x = noise(m + 4, m)
        h = random_taps(m, m)
        with SpectrumPlan(N) as plan, Dev(x) as dx:
            plan.set_fir(h)
            one = dx.ddc(plan, FINE, 1, 0)
            assert one.shape == (1,)
            check(one, ref_ddc(x, h, FINE, 1, 0), tol_of(x, h), f"n_in = M = {m}")
            assert same_bits(dx.ddc(plan, FINE, 255, 255 * 4), dx.ddc(plan, FINE, 1, 255 * 4))   # kept
            assert dx.ddc(plan, FINE, 255, 3).shape == (0,)                     # not kept: n_out = 0, a successful no-op
            assert plan.ddc(x[:1], FINE, decim=7, sample0=1).shape == (0,)      # and through the host entry


def test_six_hundred_blocks():
    """More blocks than the grid has workgroups with the mixer on (two per CU): the block-to-block bookkeeping over many steps, with
    a large index0.  Bits against D = 1; accuracy on 2000 outputs spread over the run."""
    m, d = 2049, 50
    L = block_len(m)
    n_in = 600 * L + m - 1
    x, h = noise(9, n_in), ddc_taps(d, m)
    with SpectrumPlan(N) as plan, Dev(x) as dx:
        plan.set_fir(h)
        got, full = dx.ddc(plan, FINE, d, FAR), dx.ddc(plan, FINE, 1, FAR)
        i_first = (d - FAR % d) % d
        assert got.shape[0] == brute(n_in, m, d, FAR) and same_bits(got, full[i_first::d])
        pick = np.unique(np.concatenate((np.arange(50), got.shape[0] - 1 - np.arange(50),
                                         np.random.default_rng(1).integers(0, got.shape[0], 1900))))
        i = i_first + pick * d
        hs = h.astype(np.complex128) * np.exp(2j * np.pi * bin_of(FINE) * np.arange(m) / N)
        win = x.astype(np.complex128)[i[:, None] + (m - 1 - np.arange(m))[None, :]]
        phase = [(FINE * ((FAR + int(k)) & 0xFFFFFFFF)) & 0xFFFFFFFF for k in i]
        ref = (win * hs[None, :]).sum(axis=1) * np.exp(-2j * np.pi * np.array(phase, dtype=np.float64) / 2.0 ** 32)
        check(got[pick], ref, tol_of(x, h), "600 blocks")


# ---- 3. accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TAPS)
def test_parity_with_float64_numpy(m):
    n_in = n_in_of(m)
    worst = 0.0
    with SpectrumPlan(N) as plan:
        for name, x in (("noise", noise(m + 5, n_in)), ("int16", stream16_planted(m + 6, n_in))):
            h = random_taps(m + 7, m) if name == "noise" else ddc_taps(7, m)
            xc = widen_flat(x) if x.dtype == np.int16 else x
            plan.set_fir(h)
            with Dev(x) as dev:
                for word, d, index0 in ((FINE, 1, 0), (FINE, 7, FAR), (0xFEDCBA98, 50, 12345), (1, 255, 1), (0xFFFFFFFF, 3, FAR),
                                        (0x800, 200, 7), (0, 5, 2)):
                    got = dev.ddc(plan, word, d, index0)
                    worst = max(worst, check(got, ref_ddc(xc, h, word, d, index0), tol_of(xc, h),
                                             f"M={m} {name} word={word:#x} D={d} index0={index0}"))
    print(f"M={m}: worst err/tol {worst:.2e}")


# ---- 4. known answer: fails under bin tuning -----------------------------------------------------------------------------------------
def test_known_a_tone_at_the_word_lands_at_dc_and_does_not_rotate():
    d, n, amp = 50, 1 << 20, 1.0
    h = ddc_taps(d)
    m = h.shape[0]
    t = np.arange(n, dtype=np.uint64)
    phase = (np.uint64(FINE) * t) & np.uint64(0xFFFFFFFF)                       # exact integer phase
    tone = (amp * np.exp(2j * np.pi * (phase.astype(np.float64) / 2.0 ** 32))).astype(np.complex64)
    tol = tol_of(tone, h)
    with SpectrumPlan(N) as plan, Dev(tone) as dev:
        plan.set_fir(h)
        got = dev.ddc(plan, FINE, d, 0)
        assert got.shape[0] == (n - m) // d + 1
        dev_from_first = float(np.abs(got.astype(np.complex128) - complex(got[0])).max())
        print(f"tone at the word: |out| {abs(got[0]):.6f}, worst deviation from the first output {dev_from_first / (2 * tol):.2e} of 2 tol")
        assert dev_from_first <= 2 * tol                                        # no rotation
        frac = (FINE - (bin_of(FINE) << 20)) / 2.0 ** 32                        # the tone's offset from the filter's centre
        resp = abs((h.astype(np.complex128) * np.exp(-2j * np.pi * frac * np.arange(m))).sum())
        assert abs(abs(complex(got[0])) - amp * resp) <= tol and resp > 0.99
        # the same through the FIR call at the nearest bin: 0.27 bins left over, 69 turns over the 2^20 samples
        y = dev.fir(plan, 2, bin_of(FINE), 0)
        turns = float(np.unwrap(np.angle(y.astype(np.complex128)))[-1] - np.angle(complex(y[0]))) / (2 * np.pi)
        print(f"bin tuning: {turns:.2f} turns")
        assert 68.5 <= abs(turns) <= 69.5
        # a tone one output-Nyquist (fs / 2 D) above the word: in the transition band, left at |H(0.5 / D)| as the taps say ...
        for off, what in ((0.5 / d, "one output-Nyquist away"), (0.75 / d, "in the stopband")):
            word2 = (FINE + int(round(off * 2 ** 32))) & 0xFFFFFFFF
            ph2 = (np.uint64(word2) * t) & np.uint64(0xFFFFFFFF)
            dev.d_in.put((amp * np.exp(2j * np.pi * (ph2.astype(np.float64) / 2.0 ** 32))).astype(np.complex64))
            out = dev.ddc(plan, FINE, d, 0)
            f2 = (word2 - (bin_of(FINE) << 20)) / 2.0 ** 32
            want = abs((h.astype(np.complex128) * np.exp(-2j * np.pi * f2 * np.arange(m))).sum())
            level = float(np.abs(out).max())
            print(f"tone {what}: {20 * np.log10(max(level, 1e-30)):.1f} dB (the taps: {20 * np.log10(want):.1f} dB)")
            assert abs(level - amp * want) <= tol
            if off > 0.6 / d:                                                   # ... and from 0.6 / D on below -55 dB, as promised
                assert level <= amp * 10 ** (-55 / 20) + tol


# ---- 5. the bank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d,index0", [(1, 7, 0), (257, 50, 1), (801, 5, FAR), (2049, 200, FAR)])
def test_bank_planes_are_the_single_calls(m, d, index0):
    n_in = n_in_of(m)
    rng = np.random.default_rng(m)
    words64 = [0, FINE, 0xFEDCBA98, FINE, 1 << 20, *rng.integers(0, 1 << 32, 59).tolist()]   # a zero word, a duplicate, a bin
    with SpectrumPlan(N) as plan, Dev(noise(m + 8, n_in), 64) as dx, Dev(stream16_planted(m + 9, n_in), 64) as d16:
        plan.set_fir(random_taps(m + 2, m))
        for dev in (dx, d16):
            for words, pad in (([FINE], 0), ([0], 3), (words64[:3], 0), (words64[:3], 5), (words64, 0), (words64, 1)):
                planes = dev.bank(plan, words, d, index0, pad)
                assert planes.shape == (len(words), brute(n_in, m, d, index0))
                for c in (range(len(words)) if len(words) <= 3 else (0, 1, 2, 3, 4, 31, 62, 63)):
                    assert same_bits(planes[c], dev.ddc(plan, words[c], d, index0)), (m, d, len(words), c, pad, dev.ci16)
            assert same_bits(planes[3], planes[1])
        ms = plan.exec_device_ddc_bank_timed_each(dx.d_in.p.value, n_in, dx.d_out.p.value, words64[:3], 2, decim=d, index0=index0)
        one = plan.exec_device_ddc_timed_each(dx.d_in.p.value, n_in, dx.d_out.p.value, FINE, 2, decim=d, index0=index0)
        assert len(ms) == len(one) == 2 and all(v > 0 for v in ms + one)


# ---- 6. the host entries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(257, 7), (801, 50), (2049, 7), (1, 50)])
def test_host_entries_equal_the_device_entries_across_chunks(m, d, monkeypatch):
    n = 11 * block_len(m) + 77
    x, h, pre = noise(m + d, n), random_taps(m + 1, m), noise(m + d + 1, m - 1)
    x16, pre16 = stream16_planted(m + d, n), stream16_planted(m + d + 1, max(m - 1, 1))[: m - 1]
    words = [FINE, 0, 0xFEDCBA98]
    with SpectrumPlan(N) as plan:
        plan.set_fir(h)
        for sample0 in (0, 12345, FAR):
            for prefix in (pre, None):
                virt = np.concatenate((pre if prefix is not None else np.zeros(m - 1, np.complex64), x))
                with Dev(virt, 3) as dv:
                    dev, dev_bank = dv.ddc(plan, FINE, d, sample0), dv.bank(plan, words, d, sample0)
                assert dev.shape[0] == brute(n + m - 1, m, d, sample0)
                for chunk in ("3", "5", None):
                    if chunk is None:
                        monkeypatch.delenv("SDRK_FIR_CHUNK_BLOCKS", raising=False)
                    else:
                        monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", chunk)
                    host = plan.ddc(x, FINE, decim=d, prefix=prefix, sample0=sample0)
                    assert same_bits(host, dev), (m, d, sample0, chunk, prefix is not None)
                    assert same_bits(plan.ddc_bank(x, words, decim=d, prefix=prefix, sample0=sample0), dev_bank), (m, d, sample0, chunk)
                assert same_bits(plan.ddc(x, FINE, decim=d, prefix=prefix, sample0=sample0), host)      # repeated: the same bits
            check(host, ref_ddc(virt, h, FINE, d, sample0), tol_of(virt, h), f"host M={m} D={d} sample0={sample0}")
        monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "3")
        a = plan.ddc_ci16(x16, FINE, decim=d, prefix=pre16 if m > 1 else None, sample0=FAR)
        assert same_bits(a, plan.ddc(widen_flat(x16), FINE, decim=d, prefix=widen_flat(pre16) if m > 1 else None, sample0=FAR))
        b = plan.ddc_bank_ci16(x16, words, decim=d, sample0=12345)
        assert same_bits(b, plan.ddc_bank(widen_flat(x16), words, decim=d, sample0=12345)) and same_bits(b[0], plan.ddc_ci16(
            x16, FINE, decim=d, sample0=12345))


def test_existing_rows_and_the_fir_call_are_unchanged_around_a_ddc_call():
    x = noise(3, 8 * N)
    with SpectrumPlan(N) as plan:
        plan.set_fir(ddc_taps(8))
        row, y = plan.spectrum_db(x[:N]), plan.fir(x, decim=8, shift_bins=100)
        z = plan.ddc(x, FINE, decim=7)
        assert same_bits(plan.spectrum_db(x[:N]), row) and same_bits(plan.fir(x, decim=8, shift_bins=100), y)
        assert same_bits(plan.ddc(x, FINE, decim=7), z) and plan.fir_taps == 129


# ---- 7. streams --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci16", [False, True])
def test_ddc_streams_in_ragged_pieces_equal_the_float64_reference_of_the_whole_stream(ci16):
    pieces, d, fs = (1, 3, 4095, 4097, 10000, 49), 50, 2.4e6
    n = sum(pieces)
    x = stream16_planted(21, n) if ci16 else noise(21, n)
    xc = widen_flat(x) if ci16 else x
    h = ddc_taps(d, 257)
    offs = [300.4 * fs / N, 0.0, -123456.789]
    virt = np.concatenate((np.zeros(256, np.complex64), xc))                    # lfilter: a zero prefix
    tol = tol_of(xc, h)
    with DdcStream(None, h, d, offs[0], fs) as ch, DdcBankStream(None, h, d, offs, fs) as bank:
        assert ch.freq_word == freq_word(offs[0], fs) and ch.tuned_hz == freq_word_hz(ch.freq_word, fs) and ch.out_rate == fs / d
        out, rows, at = [], [], 0
        for p in pieces:
            out.append(ch.push(x[at:at + p]))
            rows.append(bank.push(x[at:at + p]))
            at += p
            assert out[-1].shape[0] == rows[-1].shape[1] == len(range(-(-(at - p) // d) * d, at, d))
        got, planes = np.concatenate(out), np.concatenate(rows, axis=1)
    assert got.shape[0] == planes.shape[1] == len(range(0, n, d))               # the multiples of D in the stream
    check(got, ref_ddc(virt, h, freq_word(offs[0], fs), d, 0), tol, f"DdcStream in pieces {pieces}")
    for c, f in enumerate(offs):
        check(planes[c], ref_ddc(virt, h, freq_word(f, fs), d, 0), tol, f"DdcBankStream channel {c}")
    assert same_bits(planes[0], got)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device():
    lib = _ffi.lib()
    h = ddc_taps(7)
    n_out = ctypes.c_size_t()
    each = (ctypes.c_float * 2)()
    w3 = (ctypes.c_uint32 * 3)(0, FINE, 5)
    w65 = (ctypes.c_uint32 * 65)()
    x = noise(1, N)
    single = (lib.sdrk_exec_device_ddc, lib.sdrk_exec_device_ddc_ci16)
    banks = (lib.sdrk_exec_device_ddcbank, lib.sdrk_exec_device_ddcbank_ci16)
    with SpectrumPlan(1024) as p, DevBuf(1 << 16) as d:
        assert lib.sdrk_exec_device_ddc(p.handle, d.p, 1024, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_UNSUPPORTED
        assert b"4096" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_ddcbank(p.handle, d.p, 1024, 3, w3, 7, 0, d.p, 1024, None) == _ffi.SDRK_ERR_UNSUPPORTED
        assert lib.sdrk_exec_host_ddc(p.handle, None, d.p, 1024, FINE, 7, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_UNSUPPORTED
        assert p.spectrum_db(x[:1024]).shape == (1024,)                           # a plan that has refused still works
    with SpectrumPlan(N, precision="double") as p64, DevBuf(1 << 16) as d:
        for fn in single:
            assert fn(p64.handle, d.p, N, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        for fn in banks:
            assert fn(p64.handle, d.p, N, 3, w3, 7, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError):
            p64.ddc(x, FINE)
        assert p64.spectrum_db(x.astype(np.complex128)).shape == (N,)
    with SpectrumPlan(N) as p, DevBuf(1 << 17) as d:
        for fn in single:
            assert fn(p.handle, d.p, N, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"no FIR filter" in lib.sdrk_last_error()
        for fn in banks:
            assert fn(p.handle, d.p, N, 3, w3, 7, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"no FIR filter" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_ddc_timed_each(p.handle, d.p, N, FINE, 7, 0, d.p, 2, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ddc(p.handle, None, d.p, N, FINE, 7, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError):
            p.ddc(x, FINE)
        p.set_fir(h)
        m = h.shape[0]
        for fn in single:
            for decim in (0, 257, -4):
                assert fn(p.handle, d.p, N, FINE, decim, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"decim" in lib.sdrk_last_error()
            assert fn(p.handle, None, N, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, FINE, 7, 0, None, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, m - 1, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"n_in" in lib.sdrk_last_error()
            assert fn(None, d.p, N, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
        for fn in banks:
            for decim in (0, 257):
                assert fn(p.handle, d.p, N, 3, w3, decim, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"decim" in lib.sdrk_last_error()
            for chans in (0, 65):
                assert fn(p.handle, d.p, N, chans, w65, 7, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"n_chan" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 3, None, 7, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"freq_word" in lib.sdrk_last_error()
            short = brute(N, m, 7, 0) - 1
            assert fn(p.handle, d.p, N, 3, w3, 7, 0, d.p, short, None) == _ffi.SDRK_ERR_INVALID and b"out_stride" in lib.sdrk_last_error()
            assert fn(p.handle, None, N, 3, w3, 7, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 3, w3, 7, 0, None, N, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_ddc_timed_each(p.handle, d.p, N, FINE, 7, 0, d.p, 0, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ddc(p.handle, None, d.p, N, FINE, 7, 0, d.p, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ddc(p.handle, None, None, N, FINE, 7, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ddcbank(p.handle, None, d.p, N, 3, w3, 7, 0, d.p, (N + 6) // 7 - 1, ctypes.byref(n_out)) == \
            _ffi.SDRK_ERR_INVALID and b"out_stride" in lib.sdrk_last_error()
        # after all the refusals the plan still works: 4096 samples in (32 KiB), their outputs behind them
        ms = p.exec_device_ddc_timed_each(d.p.value, N, d.p.value + (1 << 15), FINE, launches=3, decim=7)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        check(p.ddc(x, FINE, decim=7), ref_ddc(np.concatenate((np.zeros(m - 1), x)), h, FINE, 7, 0), tol_of(x, h), "after the refusals")


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8: many blocks per workgroup at every size, so the loads in flight across iterations and the block-to-block keep
    bookkeeping are covered at every shape — in a child process, as the plans read the variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", SUBSET_FOR_8_CUS],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

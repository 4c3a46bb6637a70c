"""The down-converter from 8-bit I,Q on the GPU (sdrk_exec_*_downconv_iq8 / sdrk_exec_*_downconvbank_iq8, csrc/downconv_iq8.hip):
an 8-bit call returns THE BITS of the existing complex64 call on spectrum.iq8_to_c64(samples) — every tap count, word, D, index0
and C, device and host entries, however the host call is chunked, the last (short) block of a call included, where positions past
n_in count as +0.0 for unsigned bytes too.  Inputs are random bytes over all 256 values per format from fixed seeds; comparisons
are array_equal on uint32 views (same_bits) unless a tolerance is named: the project's FIR bound 1e-5 ||h||_1 max|x| against
float64 numpy (tol_of of test_ddc_gpu.py), for the stream as a whole and the known answer.

Sizes: n_in = 2 L + 1234 + M - 1 is three blocks with a short last one; under SDRK_NUM_CUS=8 (24 / 16 workgroups) a second input
of 61 blocks makes every workgroup iterate, so the loads in flight across iterations and the keep bookkeeping carry.

Measured on the device: every bit identity holds; DdcStream in pieces err/tol 5.8e-3 (int8) and 5.0e-3 (uint8); the cu8 tone's
worst deviation from its first output 8.7e-2 LSB of an allowed 2.26, the half-LSB offset leaves 7.2e-5 of an allowed 2.9e-3."""
import numpy as np
import pytest

from sdr_iq_visualizer_amd.spectrum import (ChannelBankStream, ChannelStream, DdcBankStream, DdcStream, SpectrumPlan, channel_taps,
                                            ddc_taps, freq_word, iq8_to_c64)
from tests.gpu_helpers import DevBuf, same_bits, stream16_planted
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

N = 4096
GUARD = 64
FAR = (1 << 40) + 12345
FINE = 0x12345678
ON_A_BIN = (0x7F3 << 20) & 0xFFFFFFFF
DTYPES = (np.int8, np.uint8)


def block_len(m):
    return (4097 - m) // 256 * 256


def raw_bytes(seed, n, dtype):
    """(n, 2) byte pairs over all 256 values: the extremes planted at both ends (the last block is the short one)."""
    x = np.random.default_rng(seed).integers(0, 256, size=(n, 2)).astype(np.uint8)
    plant = np.array([[0, 255], [128, 127], [255, 0], [127, 128]], np.uint8)[: n]
    x[: plant.shape[0]] = plant
    x[n - plant.shape[0]:] = plant[::-1]
    if n >= 4096:
        assert np.unique(x).shape[0] == 256
    return x.view(dtype)


def random_taps(seed, m):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2 * m)).astype(np.complex64)


def bin_of(word):
    return ((word + 0x80000) >> 20) & 4095


def ref_ddc(x, h, word, d, index0):
    """float64: the definition of include/sdrk.h (as in test_ddc_gpu.py)."""
    m = h.shape[0]
    hs = h.astype(np.complex128) * np.exp(2j * np.pi * bin_of(word) * np.arange(m) / N)
    v = np.convolve(x.astype(np.complex128), hs, "valid")
    i = np.arange(v.shape[0], dtype=np.uint64)
    idx32 = (np.uint64(index0) + i) & np.uint64(0xFFFFFFFF)
    phase = (np.uint64(word) * idx32) & np.uint64(0xFFFFFFFF)
    y = v * np.exp(-2j * np.pi * (phase.astype(np.float64) / 2.0 ** 32))
    return y[((np.uint64(index0 % d) + i) % np.uint64(d)) == 0]


def tol_of(x, h):
    return REL_TOL * float(np.abs(h.astype(np.complex128)).sum()) * float(np.abs(x.astype(np.complex128)).max())


class Dev8:
    """Byte pairs and their widened form resident on the device, one output buffer: the 8-bit and the complex64 device entries,
    each on a buffer filled with NaN first and checked to be untouched behind the last output."""

    def __init__(self, raw, planes=1):
        self.raw, self.n_in, self.unsigned = raw, raw.shape[0], raw.dtype == np.uint8
        self.d8, self.d64, self.d_out = DevBuf(raw.nbytes), DevBuf(raw.shape[0] * 8), DevBuf(planes * (self.n_in + GUARD) * 8)
        self.d8.put(raw)
        self.d64.put(iq8_to_c64(raw))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in (self.d8, self.d64, self.d_out):
            d.__exit__()

    def _read(self, plan, n):
        plan.sync()
        got = self.d_out.get(n + GUARD, np.complex64)
        return got[:n], got[n:]

    def one(self, plan, word, d, index0, narrow=True, n_in=None):
        n_in = self.n_in if n_in is None else n_in
        n_out = plan.ddc_outputs(n_in, d, index0)
        self.d_out.put(np.full(n_out + GUARD, np.nan + 1j * np.nan, np.complex64))
        if narrow:
            plan.exec_device_ddc_ci8(self.d8.p.value, n_in, self.d_out.p.value, word, unsigned=self.unsigned, decim=d, index0=index0)
        else:
            plan.exec_device_ddc(self.d64.p.value, n_in, self.d_out.p.value, word, decim=d, index0=index0)
        got, guard = self._read(plan, n_out)
        assert np.all(np.isnan(guard.real)), "stored past n_out"
        return got

    def bank(self, plan, words, d, index0, narrow=True, pad=0):
        n_out = plan.ddc_outputs(self.n_in, d, index0)
        stride, c = n_out + pad, len(words)
        self.d_out.put(np.full(c * stride + GUARD, np.nan + 1j * np.nan, np.complex64))
        if narrow:
            plan.exec_device_ddc_bank_ci8(self.d8.p.value, self.n_in, self.d_out.p.value, words, unsigned=self.unsigned, decim=d,
                                          index0=index0, out_stride=stride if pad else None)
        else:
            plan.exec_device_ddc_bank(self.d64.p.value, self.n_in, self.d_out.p.value, words, decim=d, index0=index0,
                                      out_stride=stride if pad else None)
        got, guard = self._read(plan, c * stride)
        planes = got.reshape(c, stride)
        assert np.all(np.isnan(planes[:, n_out:].real)) and np.all(np.isnan(guard.real)), "stored outside the planes"
        return planes[:, :n_out]


@pytest.fixture(params=[None, "8"], ids=["all_cus", "8_cus"])
def cus(request, monkeypatch):
    """The plans made in the test size their grids for the whole device, or for 8 CUs (read when a plan is made)."""
    if request.param:
        monkeypatch.setenv("SDRK_NUM_CUS", request.param)
    else:
        monkeypatch.delenv("SDRK_NUM_CUS", raising=False)
    return request.param


# ---- 1. the bits of the complex64 call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
@pytest.mark.parametrize("m", [1, 257, 2049])
def test_device_entry_returns_the_bits_of_the_complex64_call_on_the_widened_samples(m, dtype, cus):
    L = block_len(m)
    sizes = [2 * L + 1234 + m - 1] + ([60 * L + 1234 + m - 1] if cus else [])     # three blocks, the last one short; 61 under 8 CUs
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m, m))
        for n_in in sizes:
            with Dev8(raw_bytes(m + n_in, n_in, dtype)) as dev:
                for d in (1, 7, 50, 256):
                    for index0 in (0, 1, FAR):
                        for word in (0, ON_A_BIN, FINE):
                            a, b = dev.one(plan, word, d, index0), dev.one(plan, word, d, index0, narrow=False)
                            assert a.shape[0] == plan.ddc_outputs(n_in, d, index0) > 0
                            assert same_bits(a, b), (m, dtype.__name__, n_in, d, index0, hex(word))
                assert np.all(np.isfinite(a.view(np.float32)))
                ms = plan.exec_device_ddc_ci8_timed_each(dev.d8.p.value, n_in, dev.d_out.p.value, FINE, 2, unsigned=dev.unsigned,
                                                         decim=7, index0=1)
                assert len(ms) == 2 and all(v > 0 for v in ms)
                n_out = plan.ddc_outputs(n_in, 7, 1)
                assert same_bits(dev.d_out.get(n_out, np.complex64), dev.one(plan, FINE, 7, 1))


# ---- 2. short inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
def test_one_output_and_none(dtype, cus):
    for m in (1, 257, 2049):
        raw = raw_bytes(m + 4, m, dtype)
        h = random_taps(m, m)
        with SpectrumPlan(N) as plan, Dev8(raw, 3) as dev:
            plan.set_fir(h)
            one = dev.one(plan, FINE, 1, 0)
            assert one.shape == (1,) and same_bits(one, dev.one(plan, FINE, 1, 0, narrow=False))
            assert abs(complex(one[0]) - ref_ddc(iq8_to_c64(raw), h, FINE, 1, 0)[0]) <= tol_of(iq8_to_c64(raw), h)
            assert same_bits(dev.one(plan, FINE, 255, 255 * 4), dev.one(plan, FINE, 1, 255 * 4))      # index0 % D == 0: kept
            assert dev.one(plan, FINE, 255, 3).shape == (0,)                     # not kept: n_out = 0, a successful no-op
            assert dev.bank(plan, [FINE, 0, 5], 255, 3).shape == (3, 0)
            assert same_bits(dev.bank(plan, [FINE, 0, 5], 255, 255)[0], dev.one(plan, FINE, 255, 255))
            assert plan.ddc_ci8(raw[:1], FINE, decim=7, sample0=1).shape == (0,)  # and through the host entry
            assert plan.ddc_bank_ci8(raw[:1], [FINE, 0], decim=7, sample0=1).shape == (2, 0)
            assert plan.ddc_ci8(raw[:1], FINE, decim=7, sample0=7).shape == (1,)


# ---- 3. the bank -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
@pytest.mark.parametrize("m,d,index0", [(1, 7, 0), (257, 50, 1), (801, 5, (1 << 40) + 3), (2049, 200, (1 << 40) + 3)])
def test_bank_planes_are_the_single_8_bit_calls(m, d, index0, dtype, cus):
    L = block_len(m)
    n_in = (40 if cus else 2) * L + 1234 + m - 1
    rng = np.random.default_rng(m)
    words64 = [FINE, 0, 0xFEDCBA98, FINE, 1 << 20, *rng.integers(0, 1 << 32, 59).tolist()]   # a zero word among non-zero ones
    with SpectrumPlan(N) as plan, Dev8(raw_bytes(m + 8, n_in, dtype), 64) as dev:
        plan.set_fir(random_taps(m + 2, m))
        for words, pad in (([FINE], 0), ([0], 3), (words64[:3], 0), (words64[:3], 5), (words64, 0), (words64, 1)):
            planes = dev.bank(plan, words, d, index0, pad=pad)
            assert planes.shape == (len(words), plan.ddc_outputs(n_in, d, index0)) and planes.shape[1] > 0
            for c in (range(len(words)) if len(words) <= 3 else (0, 1, 2, 3, 4, 31, 62, 63)):
                assert same_bits(planes[c], dev.one(plan, words[c], d, index0)), (m, d, len(words), c, pad)
            assert same_bits(planes, dev.bank(plan, words, d, index0, narrow=False, pad=pad)), (m, d, len(words), pad)
        ms = plan.exec_device_ddc_bank_ci8_timed_each(dev.d8.p.value, n_in, dev.d_out.p.value, words64[:3], 2, unsigned=dev.unsigned,
                                                      decim=d, index0=index0)
        assert len(ms) == 2 and all(v > 0 for v in ms)


# ---- 4. the host entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
@pytest.mark.parametrize("m,d", [(257, 7), (257, 50), (2049, 7)])
def test_host_entries_equal_the_device_entries_across_chunks(m, d, dtype, monkeypatch):
    n = 11 * block_len(m) + 77
    raw, pre = raw_bytes(m + d, n, dtype), raw_bytes(m + d + 1, m - 1, dtype)
    silence = np.full((m - 1, 2), 128 if dtype == np.uint8 else 0, dtype)        # what a NULL prefix stands for
    words = [FINE, 0, 0xFEDCBA98]
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m + 1, m))
        for sample0 in (0, FAR):
            for prefix in (pre, None):
                virt = np.concatenate((pre if prefix is not None else silence, raw))
                with Dev8(virt, 3) as dv:
                    dev, dev_bank = dv.one(plan, FINE, d, sample0), dv.bank(plan, words, d, sample0)
                for chunk in ("3", None):
                    if chunk is None:
                        monkeypatch.delenv("SDRK_FIR_CHUNK_BLOCKS", raising=False)
                    else:
                        monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", chunk)
                    host = plan.ddc_ci8(raw, FINE, decim=d, prefix=prefix, sample0=sample0)
                    assert same_bits(host, dev), (m, d, sample0, chunk, prefix is not None)
                    bank = plan.ddc_bank_ci8(raw, words, decim=d, prefix=prefix, sample0=sample0)
                    assert same_bits(bank, dev_bank), (m, d, sample0, chunk, prefix is not None)
                    # the complex64 host call GIVEN the widened prefix (for NULL: the widened 0 / 0x80 bytes)
                    wide_pre = iq8_to_c64(pre if prefix is not None else silence)
                    assert same_bits(host, plan.ddc(iq8_to_c64(raw), FINE, decim=d, prefix=wide_pre, sample0=sample0))
        if dtype == np.uint8:
            assert np.all(iq8_to_c64(silence) == np.complex64(0.5 + 0.5j))
        else:                                                                     # int8: NULL for both calls is the same stream
            assert same_bits(host, plan.ddc(iq8_to_c64(raw), FINE, decim=d, prefix=None, sample0=FAR))


# ---- 5. streams ------------------------------------------------------------------------------------------------------------------------
PIECES = (1, 3, 200, 4095, 4097, 10000, 49)                                       # 1, and lengths below M = 257


@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
def test_ddc_streams_in_ragged_pieces_equal_the_plan_calls_and_the_float64_reference(dtype):
    d, fs = 50, 2.4e6
    n = sum(PIECES)
    raw = raw_bytes(21, n, dtype)
    h = ddc_taps(d, 257)
    offs = [300.4 * fs / N, 0.0, -123456.789]
    words = [freq_word(f, fs) for f in offs]
    tail = np.full((256, 2), 128 if dtype == np.uint8 else 0, dtype)
    with SpectrumPlan(N) as ref, DdcStream(None, h, d, offs[0], fs) as ch, DdcBankStream(None, h, d, offs, fs) as bank:
        ref.set_fir(h)
        out, at = [], 0
        for p in PIECES:
            piece = raw[at:at + p]
            got, rows = ch.push(piece), bank.push(piece)
            kw = dict(decim=d, prefix=iq8_to_c64(tail), sample0=at)
            assert same_bits(got, ref.ddc(iq8_to_c64(piece), words[0], **kw)), (p, at)
            assert same_bits(rows, ref.ddc_bank(iq8_to_c64(piece), words, **kw)), (p, at)
            assert got.shape[0] == len(range(-(-at // d) * d, at + p, d))
            out.append(got)
            tail = np.concatenate((tail, piece))[-256:]
            at += p
            assert ch.sample_index == bank.sample_index == at and np.array_equal(ch._tail, tail) and ch._tail.dtype == dtype
        with pytest.raises(ValueError, match="not both"):
            ch.push(raw[:10].view(np.uint8 if dtype == np.int8 else np.int8))
        with pytest.raises(ValueError, match="not both"):
            bank.push(np.zeros(10, np.complex64))
    whole = np.concatenate(out)
    start = np.full(256, 0.5 + 0.5j if dtype == np.uint8 else 0.0, np.complex64)   # a uint8 stream starts from bytes of 128
    virt = np.concatenate((start, iq8_to_c64(raw)))
    tol = tol_of(virt, h)
    err = float(np.abs(whole.astype(np.complex128) - ref_ddc(virt, h, words[0], d, 0)).max())
    print(f"DdcStream {dtype.__name__} in pieces {PIECES}: err/tol {err / tol:.2e}")
    assert whole.shape[0] == len(range(0, n, d)) and err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["ci8", "cu8"])
def test_channel_streams_take_8_bit_pieces_through_the_call_with_the_bins_word(dtype):
    d, fs = 16, 2.4e6
    n = sum(PIECES)
    raw = raw_bytes(22, n, dtype)
    h = channel_taps(d, 257)
    offs = [300.4 * fs / N, 0.0, -1000.2 * fs / N]
    tail = np.full((256, 2), 128 if dtype == np.uint8 else 0, dtype)
    with SpectrumPlan(N) as ref, ChannelStream(None, h, d, offs[0], fs) as ch, ChannelBankStream(None, h, d, offs, fs) as bank:
        ref.set_fir(h)
        assert ch.shift_bins == 300 and bank.shift_bins == [300, 0, -1000] and ch.tuned_hz == 300 * (fs / N)
        words = [(s % N) << 20 for s in bank.shift_bins]
        at, on_multiple = 0, 0
        for p in PIECES + (3, 1600, 1600, 777):                               # (18445 + 3: pieces that start on multiples of 16)
            piece = raw[at:at + p] if at + p <= n else raw[:p]
            got, rows = ch.push(piece), bank.push(piece)
            kw = dict(decim=d, prefix=iq8_to_c64(tail), sample0=at)
            assert same_bits(got, ref.ddc(iq8_to_c64(piece), words[0], **kw)), (p, at)
            assert same_bits(rows, ref.ddc_bank(iq8_to_c64(piece), words, **kw)), (p, at)
            fir = ref.fir(iq8_to_c64(piece), shift_bins=300, decim=d, prefix=iq8_to_c64(tail), sample0=at)
            if at % d == 0:                                                        # the same blocks: the bits of the FIR call
                assert same_bits(got, fir), (p, at)
                on_multiple += 1
            elif got.shape[0]:                                                     # blocks cut elsewhere: its error bound
                assert np.abs(got - fir).max() <= 2 * tol_of(iq8_to_c64(raw), h)
            tail = np.concatenate((tail, piece))[-256:]
            at += p
            assert ch.sample_index == bank.sample_index == at
        assert on_multiple == 4
        with pytest.raises(ValueError, match="not both"):
            ch.push(np.zeros((10, 2), np.int16))


# ---- 6. known answer -------------------------------------------------------------------------------------------------------------------
def test_known_a_cu8_tone_at_the_word_lands_at_dc_and_does_not_rotate():
    """An RTL-SDR's bytes, 128 + 100 (cos, sin) rounded to integers: s[n] + (0.5 + 0.5i) after the widening about 127.5, with s
    the integer-valued tone.  The tone at the word lands at DC and stands still.  The half-LSB offset is a DC term of the INPUT:
    the mixer moves it to -word, 291 bins from the pass band, where the taps leave less than -55 dB of it (ddc_taps' promise from
    0.6 / D on) — so the outputs equal those of the offset-free samples to that level and the offset shows nowhere else.
    Rounding to integers moves every sample by at most 0.5 a part, an output by at most q = ||h||_1 sqrt(0.5): the allowance
    for 'does not rotate', 1 % of the tone (a rotating tone would move by twice its amplitude)."""
    d, n, amp = 50, 1 << 16, 100.0
    h = ddc_taps(d)
    m = h.shape[0]
    t = np.arange(n, dtype=np.uint64)
    phase = ((np.uint64(FINE) * t) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32
    raw = np.empty((n, 2), np.uint8)
    raw[:, 0] = np.rint(128.0 + amp * np.cos(2 * np.pi * phase))
    raw[:, 1] = np.rint(128.0 + amp * np.sin(2 * np.pi * phase))
    x = iq8_to_c64(raw)
    offset = 0.5 + 0.5j
    s = x.astype(np.complex128) - offset                                          # the integer-valued tone
    assert np.array_equal(s.real, raw[:, 0].astype(np.float64) - 128.0)
    tol = tol_of(x, h)
    q = float(np.abs(h.astype(np.complex128)).sum()) * np.sqrt(0.5)
    stop = abs(offset) * 10 ** (-55 / 20)
    with SpectrumPlan(N) as plan, Dev8(raw) as dev:
        plan.set_fir(h)
        got = dev.one(plan, FINE, d, 0)
        assert got.shape[0] == (n - m) // d + 1 and same_bits(got, dev.one(plan, FINE, d, 0, narrow=False))
    g = got.astype(np.complex128)
    assert np.abs(g - ref_ddc(x, h, FINE, d, 0)).max() <= tol                     # the definition, on the samples as widened
    left = float(np.abs(g - ref_ddc(s, h, FINE, d, 0)).max())                     # what the offset leaves in the outputs
    frac = (FINE - (bin_of(FINE) << 20)) / 2.0 ** 32
    resp = abs((h.astype(np.complex128) * np.exp(-2j * np.pi * frac * np.arange(m))).sum())
    dev_from_first = float(np.abs(g - g[0]).max())
    print(f"cu8 tone at the word: |out| {abs(g[0]):.4f} (amp {amp} x {resp:.4f}); worst deviation from the first output "
          f"{dev_from_first:.3e} (allowed {2 * (q + stop + tol):.3e}); the offset leaves {left:.3e} (allowed {stop + tol:.3e})")
    assert left <= stop + tol
    assert dev_from_first <= 2 * (q + stop + tol)                                 # no rotation
    assert abs(abs(g[0]) - amp * resp) <= q + stop + tol and resp > 0.99


# ---- 7. the existing calls -------------------------------------------------------------------------------------------------------------
def test_existing_calls_give_the_same_bits_before_and_after_an_8_bit_call():
    rng = np.random.default_rng(3)
    x = ((rng.standard_normal(8 * N) + 1j * rng.standard_normal(8 * N)) / np.sqrt(2)).astype(np.complex64)
    x16 = stream16_planted(4, 8 * N)
    raw = raw_bytes(5, 8 * N, np.uint8)
    with SpectrumPlan(N) as plan:
        plan.set_fir(ddc_taps(8))
        before = (plan.spectrum_db(x[:N]), plan.fir(x, decim=8, shift_bins=100), plan.ddc(x, FINE, decim=7),
                  plan.ddc_ci16(x16, FINE, decim=7), plan.ddc_bank(x, [FINE, 0], decim=7))
        z = plan.ddc_ci8(raw, FINE, decim=7)
        zb = plan.ddc_bank_ci8(raw.view(np.int8), [FINE, 0], decim=7)
        after = (plan.spectrum_db(x[:N]), plan.fir(x, decim=8, shift_bins=100), plan.ddc(x, FINE, decim=7),
                 plan.ddc_ci16(x16, FINE, decim=7), plan.ddc_bank(x, [FINE, 0], decim=7))
        for a, b in zip(before, after):
            assert same_bits(a, b)
        assert same_bits(plan.ddc_ci8(raw, FINE, decim=7), z) and same_bits(plan.ddc_bank_ci8(raw.view(np.int8), [FINE, 0], decim=7), zb)
        assert plan.fir_taps == 129

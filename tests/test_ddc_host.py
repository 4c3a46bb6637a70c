"""The digital down-converter without a GPU: header, ctypes table and exports agree on the eleven symbols; sdrk_ddc_outputs
against a brute-force count; the exhaustive checks of the shared arithmetic of csrc/kernels_ddc.h (tests/ddc_arith_check.cpp: the
reciprocal division for every D, the NCO rotation over all 2^20 residues against float64, the block-to-block keep bookkeeping);
freq_word round trips and wrap-around; DdcStream / DdcBankStream bookkeeping with the C call replaced by the float64 numpy
definition; the command line with and without --exact."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import DdcBankStream, DdcStream, channel_taps, ddc_taps, freq_word, freq_word_hz
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
ELEVEN = sorted(["sdrk_ddc_outputs", "sdrk_exec_device_ddc", "sdrk_exec_device_ddc_ci16", "sdrk_exec_device_ddc_timed_each",
                 "sdrk_exec_host_ddc", "sdrk_exec_host_ddc_ci16", "sdrk_exec_device_ddcbank", "sdrk_exec_device_ddcbank_ci16",
                 "sdrk_exec_device_ddcbank_timed_each", "sdrk_exec_host_ddcbank", "sdrk_exec_host_ddcbank_ci16"])


def test_header_table_and_exports_agree_on_the_eleven_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "ddc" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == ELEVEN == sorted(n for n in table if "ddc" in n)
    assert not [n for n in ELEVEN if "_fir" in n or "chanbank" in n]          # (the sets the FIR and bank tests pin stay theirs)
    for n in ELEVEN:
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
    assert "#define SDRK_VERSION 500" in text
    section = text.split("digital down-converter (DDC)")[1].split("measurement probes")[0]
    for word in ("within fs/8192", "lands at DC exactly", "(index0 + i) % D == 0", "0x1.921fb6p-30f", "freq_word == 0 runs no mixer",
                 "rational (non-integer) resampling", "per-channel filters or decimation", "n_out = 0\n * is a successful no-op"):
        assert word in section, word
    handle = ctypes.CDLL(_ffi.library_path())
    assert all(hasattr(handle, n) for n in ELEVEN)
    for name in ("ddc", "ddc_bank", "ddc_taps", "freq_word", "freq_word_hz", "DdcStream", "DdcBankStream"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def brute(n_in, m, d, index0):
    return sum(1 for i in range(0, n_in - m + 1) if (index0 + i) % d == 0)


def test_ddc_outputs_against_a_brute_force_count():
    lib = _ffi.lib()
    zero = 0
    for m in (1, 2, 5):
        for d in (1, 2, 3, 7, 50, 255, 256):
            for index0 in (0, 1, d - 1, d, 12345, (1 << 40) + 3):
                for n_in in (m, m + 1, m + d - 1, m + d, m + 3 * d + 1, 700):
                    got = lib.sdrk_ddc_outputs(n_in, m, d, index0)
                    want = brute(n_in, m, d, index0)
                    zero += want == 0
                    assert got == want, (n_in, m, d, index0)
                    i_first = (d - index0 % d) % d
                    assert want == (0 if i_first > n_in - m else (n_in - m - i_first) // d + 1)
    assert zero > 20                                                          # n_out = 0 is among the cases
    for bad in ((8, 9, 1, 0), (9, 0, 1, 0), (100, 9, 0, 0), (100, 9, 257, 0), (100, 9, -1, 0)):
        assert lib.sdrk_ddc_outputs(*bad) == 0
    plan = bare_plan(N)
    plan.fir_taps = 9
    assert plan.ddc_outputs(100, 7, 3) == brute(100, 9, 7, 3) and plan.ddc_outputs(9, 7, 3) == 0


@pytest.fixture(scope="module")
def arith():
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    import tempfile
    with tempfile.TemporaryDirectory(prefix="sdrk_ddc_") as tmp:
        exe = os.path.join(tmp, "ddc_arith_check")
        subprocess.run([gxx, "-O2", "-std=c++17", "-I", os.path.join(REPO, "tests", "fake_hip"),
                        os.path.join(REPO, "tests", "ddc_arith_check.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    return {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in out.splitlines()}


def test_reciprocal_division_is_exact_for_every_decimation(arith):
    assert arith["div"]["bad"] == "0"


def test_nco_rotation_is_within_half_an_ulp_of_unit_scale_over_all_residues(arith):
    """Truncating the series costs below 2.3e-13; what is left is one rounding at unit scale: each part within 2^-24.
    Found: cosine 2.98e-8 (2^-25), sine 1.57e-10."""
    assert float(arith["nco"]["worst_cos"]) <= 2.0 ** -24 and float(arith["nco"]["worst_sin"]) <= 2.0 ** -24
    assert arith["bits"]["same"] == "1"                                       # r == 0: the table entry itself, -0.0 included


def test_keep_bookkeeping_of_a_persistent_workgroup_matches_the_definition(arith):
    assert arith["keep"]["bad"] == "0" and int(arith["keep"]["kept"]) > 10_000_000


def test_freq_word_round_trips_and_wraps():
    fs = 61.44e6
    assert freq_word(0.0, fs) == 0 and freq_word(fs / 4096, fs) == 1 << 20 and freq_word(-fs / 4096, fs) == (1 << 32) - (1 << 20)
    assert freq_word(fs / 2, fs) == 1 << 31 == freq_word(-fs / 2, fs)       # the two ends of the band are one frequency
    assert freq_word(fs, fs) == 0 and freq_word(1.25 * fs, fs) == 1 << 30     # beyond the band: wraps as sampled frequencies do
    assert freq_word_hz(1 << 31, fs) == -fs / 2 and freq_word_hz(-1, fs) == -fs / 2 ** 32 == freq_word_hz((1 << 32) - 1, fs)
    rng = np.random.default_rng(7)
    for w in [1, 0x12345678, 0xFEDCBA98, (1 << 32) - 1, *rng.integers(0, 1 << 32, 200).tolist()]:
        assert freq_word(freq_word_hz(w, fs), fs) == w                        # hertz and back: the same word
    for f in rng.uniform(-fs / 2, fs / 2, 200):
        assert abs(freq_word_hz(freq_word(f, fs), fs) - f) <= fs / 2 ** 33 * (1 + 1e-9)   # to the nearest word
    assert fs / 2 ** 32 < 0.0144                                              # 0.014 Hz at 61.44 Msps
    with pytest.raises(ValueError):
        freq_word(1.0, 0.0)


def test_python_argument_checks_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    words = (ctypes.c_uint32 * 3)(0, 1, 2)
    n_out = ctypes.c_size_t()
    assert lib.sdrk_exec_device_ddc(None, p, 8, 5, 7, 0, p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_exec_host_ddcbank(None, None, p, 8, 3, words, 7, 0, p, 8, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
    plan = bare_plan(N)
    plan.fir_taps = 0
    x = np.zeros(100, np.complex64)
    with pytest.raises(ValueError, match="set_fir"):
        plan.ddc(x, 5)
    plan.fir_taps = 9
    for kw in ({"decim": 0}, {"decim": 257}, {"sample0": -1}, {"prefix": np.zeros(7, np.complex64)}):
        with pytest.raises(ValueError):
            plan.ddc(x, 5, **kw)
        with pytest.raises(ValueError):
            plan.ddc_bank(x, [5, 6], **kw)
    for bad in ([], list(range(65))):
        with pytest.raises(ValueError, match="1..64"):
            plan.ddc_bank(x, bad)
    for entry in ("exec_device_ddc", "exec_device_ddc_ci16", "exec_device_ddc_timed_each"):
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 100, 0x2000, 5, decim=300)
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 8, 0x2000, 5)
    with pytest.raises(ValueError, match="out_stride"):
        plan.exec_device_ddc_bank(0x1000, 100, 0x2000, [1, 2], decim=7, out_stride=3)
    with pytest.raises(ValueError):
        spectrum.ddc(x, np.ones(3), 0.0, 1e6, decim=300)
    assert np.array_equal(ddc_taps(16), channel_taps(16)) and ddc_taps(50).shape == (801,) and ddc_taps(3, 33).shape == (33,)
    assert abs(ddc_taps(50).astype(np.complex128).sum() - 1) < 1e-6
    for bad in (0, 257):
        with pytest.raises(ValueError):
            ddc_taps(bad)


class NumpyDdcPlan:
    """What the DDC streams ask of a plan, answered by the float64 definition of include/sdrk.h."""

    def __init__(self):
        self.calls = []

    def set_fir(self, taps):
        self.h = np.asarray(taps, np.complex128)
        return self.h.shape[0]

    def ddc(self, x, word, *, decim, prefix, sample0):
        m = self.h.shape[0]
        self.calls.append((x.shape[0], None if prefix is None else prefix.copy(), sample0))
        pre = np.zeros(m - 1, np.complex128) if prefix is None else prefix.astype(np.complex128)
        assert pre.shape == (m - 1,)
        s = ((word + 0x80000) >> 20) & 4095
        hs = self.h * np.exp(2j * np.pi * s * np.arange(m) / N)
        v = np.convolve(np.concatenate((pre, x.astype(np.complex128))), hs, "valid")
        idx = [sample0 + j for j in range(v.shape[0])]
        phase = np.array([(word * (j & 0xFFFFFFFF)) & 0xFFFFFFFF for j in idx], dtype=np.float64)
        y = v * np.exp(-2j * np.pi * phase / 2.0 ** 32)
        return y[np.array([j % decim == 0 for j in idx], dtype=bool)].astype(np.complex64)

    def ddc_ci16(self, x, word, *, decim, prefix, sample0):
        assert x.dtype == np.int16 and (prefix is None or prefix.dtype == np.int16)
        wide = lambda a: None if a is None else a.astype(np.float32).view(np.complex64).reshape(-1)   # noqa: E731
        return self.ddc(wide(x), word, decim=decim, prefix=wide(prefix), sample0=sample0)

    def ddc_bank(self, x, words, *, decim, prefix, sample0):
        return np.stack([self.ddc(x, w, decim=decim, prefix=prefix, sample0=sample0) for w in words])

    def ddc_bank_ci16(self, x, words, *, decim, prefix, sample0):
        return np.stack([self.ddc_ci16(x, w, decim=decim, prefix=prefix, sample0=sample0) for w in words])


def test_ddc_stream_keeps_the_tail_the_index_and_the_exact_offset():
    fs, d = 2.4e6, 7
    h = ddc_taps(d, 33)
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    plan = NumpyDdcPlan()
    off = -100.6 * fs / N
    ch = DdcStream(plan, h, d, off, fs)
    assert ch.freq_word == freq_word(off, fs) and ch.tuned_hz == freq_word_hz(ch.freq_word, fs) and abs(ch.tuned_hz - off) <= fs / 2 ** 33
    assert ch.out_rate == fs / d and ch.ntaps == 33
    out, at = [], 0
    for p in (1, 0, 3, 31, 32, 33, 1000, 3900):
        out.append(ch.push(x[at:at + p]))
        at += p
        assert ch.sample_index == at
        assert out[-1].shape == (len(range(-(-(at - p) // d) * d, at, d)),)      # the multiples of D that fall into the piece
    assert at == 5000 and out[1].shape == (0,) and len(plan.calls) == 7           # an empty piece makes no call
    assert out[2].shape == (0,)                                                   # samples 1..3 hold no multiple of 7: a call, no output
    assert plan.calls[0][1] is None and plan.calls[0][2] == 0                     # no samples yet: a zero prefix
    for (n, pre, s0), start in zip(plan.calls[1:], (1, 4, 35, 67, 100, 1100)):
        want = np.concatenate((np.zeros(32, np.complex64), x[:start]))[-32:]      # the 32 samples before the piece
        assert s0 == start and np.array_equal(pre, want)
    whole = NumpyDdcPlan()
    whole.set_fir(h)
    ref = whole.ddc(x, ch.freq_word, decim=d, prefix=None, sample0=0)
    got = np.concatenate(out)
    assert got.shape == ref.shape == (715,) and np.abs(got - ref).max() < 1e-5    # 715 multiples of 7 below 5000
    ch.close()                                                                    # (a plan that was handed in is not closed)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            DdcStream(plan, h, bad, 0.0, fs)
    ch = DdcStream(plan, h, d, 0.6 * fs, fs)                                      # beyond the band: wraps
    assert ch.tuned_hz == pytest.approx(-0.4 * fs, abs=1e-3)
    ch.push(x[:10])
    with pytest.raises(ValueError, match="not both"):
        ch.push(np.zeros((10, 2), np.int16))


def test_ddc_bank_stream_rows_are_the_single_streams():
    fs, d = 1.0e6, 50
    h = ddc_taps(d, 65)
    rng = np.random.default_rng(5)
    i16 = rng.integers(-2048, 2048, size=(3000, 2)).astype(np.int16)
    offs = [0.0, 1234.5, -250000.25]
    bank = DdcBankStream(NumpyDdcPlan(), h, d, offs, fs)
    singles = [DdcStream(NumpyDdcPlan(), h, d, f, fs) for f in offs]
    assert bank.freq_words == [s.freq_word for s in singles] and bank.tuned_hz == [s.tuned_hz for s in singles]
    at, total = 0, 0
    for p in (10, 0, 49, 1000, 1941):
        got = bank.push(i16[at:at + p])
        assert got.shape[0] == 3
        for c, s in enumerate(singles):
            assert np.array_equal(got[c], s.push(i16[at:at + p]))
        at += p
        total += got.shape[1]
    assert at == 3000 and total == 60 and bank.sample_index == 3000
    with pytest.raises(ValueError):
        DdcBankStream(NumpyDdcPlan(), h, d, [], fs)
    with pytest.raises(ValueError):
        DdcBankStream(NumpyDdcPlan(), h, d, [0.0] * 65, fs)


class _FakeDdcStream(DdcStream):
    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(NumpyDdcPlan(), taps, decim, offset_hz, sample_rate)


class _FakeDdcBankStream(DdcBankStream):
    def __init__(self, plan, taps, decim, offsets_hz, sample_rate, *, device=0):
        super().__init__(NumpyDdcPlan(), taps, decim, offsets_hz, sample_rate)


class _Forbidden:
    def __init__(self, *a, **k):
        raise AssertionError("--exact must not take the bin-tuned stream (nor the other way round)")


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_cli_extract_exact_tunes_to_the_word_and_takes_any_decimation(tmp_path, capsys, monkeypatch, datatype):
    fs, fc, d = 1.0e6, 1.0e9, 5
    rng = np.random.default_rng(5)
    i16 = rng.integers(-2048, 2048, size=(9000, 2)).astype(np.int16)
    x = i16 if datatype == "ci16_le" else i16.astype(np.float32).view(np.complex64).reshape(-1)
    base, out = str(tmp_path / "rec"), str(tmp_path / "chan")
    sigmf_io.write_sigmf(base, x, fs, fc, datatype=datatype)
    monkeypatch.setattr(spectrum, "DdcStream", _FakeDdcStream)
    monkeypatch.setattr(spectrum, "DdcBankStream", _FakeDdcBankStream)
    monkeypatch.setattr(spectrum, "ChannelStream", _Forbidden)
    monkeypatch.setattr(spectrum, "ChannelBankStream", _Forbidden)
    monkeypatch.setattr(cli, "EXTRACT_PIECE", 4001)                               # three pieces, cut off the multiples of D
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000.3", "--decim", str(d), "--exact", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    word = freq_word(100000.3, fs)
    assert report["freq_word"] == word and "shift_bins" not in report
    assert report["tuned_offset_hz"] == freq_word_hz(word, fs) and abs(report["tuned_offset_hz"] - 100000.3) < fs / 2 ** 33
    assert report["samples_in"] == 9000 and report["samples_out"] == 1800 and report["taps"] == 81 and report["decim"] == 5
    y, meta = sigmf_io.read_sigmf(out)
    assert y.dtype == np.complex64 and y.shape == (1800,) and meta["sample_rate"] == fs / d
    whole = NumpyDdcPlan()
    whole.set_fir(ddc_taps(d))
    wide = i16.astype(np.float32).view(np.complex64).reshape(-1)
    assert np.abs(y - whole.ddc(wide, word, decim=d, prefix=None, sample0=0)).max() < 1e-2
    # several offsets: the bank, one recording each
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000.3", "-7.5", "--decim", "50", "--exact", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [c["freq_word"] for c in report["channels"]] == [word, freq_word(-7.5, fs)] and report["samples_out"] == 180
    assert all("shift_bins" not in c for c in report["channels"])
    y1, _ = sigmf_io.read_sigmf(out + "_1")
    assert y1.shape == (180,)
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "0", "--decim", "300", "--exact", "--out", out]) == 2
    assert "1..256" in capsys.readouterr().err


class _BinPlan:
    """What ChannelStream asks of a plan: the bin-tuned call is the DDC's definition with the word on the bin."""

    def set_fir(self, taps):
        self.ddc = NumpyDdcPlan()
        return self.ddc.set_fir(taps)

    def fir(self, x, *, decim, shift_bins, prefix, sample0):
        return self.ddc.ddc(x, (shift_bins << 20) & 0xFFFFFFFF, decim=decim, prefix=prefix, sample0=sample0)


class _FakeStream(spectrum.ChannelStream):
    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(_BinPlan(), taps, decim, offset_hz, sample_rate)


def test_cli_extract_without_exact_is_what_it_was(tmp_path, capsys, monkeypatch):
    fs, fc, d = 1.0e6, 1.0e9, 4
    rng = np.random.default_rng(5)
    x = rng.integers(-2048, 2048, size=(9000, 2)).astype(np.int16).astype(np.float32).view(np.complex64).reshape(-1)
    base, out = str(tmp_path / "rec"), str(tmp_path / "chan")
    sigmf_io.write_sigmf(base, x, fs, fc)
    monkeypatch.setattr(spectrum, "ChannelStream", _FakeStream)
    monkeypatch.setattr(spectrum, "DdcStream", _Forbidden)
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000", "--decim", str(d), "--out", out]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    report = json.loads(line)
    assert list(report) == ["wrote", "samples_in", "samples_out", "sample_rate", "center_freq", "tuned_offset_hz", "shift_bins", "decim",
                            "taps"]                                               # the keys and their order: byte for byte what it was
    assert report["shift_bins"] == 410 and "freq_word" not in report
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "0", "--decim", "3", "--out", out]) == 2
    assert "power of two" in capsys.readouterr().err

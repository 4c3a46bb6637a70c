"""The 8-bit down-converter without a GPU: header, ctypes table and exports agree on the six names, their signatures are those of
the _ci16 twins (the timed ones: of the complex64 entries) plus ``int iq8_format`` behind the samples pointer; the refusals through
ctypes; the Python argument checks (dtype rules, one dtype throughout a stream, the first tail of bytes 0 / 128) with the C call
replaced by the float64 numpy definition; and ``cli.py extract`` on synthetic ci8 / cu8 recordings, whose bytes reach the 8-bit
method unwidened."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, processing, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import (ChannelBankStream, ChannelStream, DdcBankStream, DdcStream, SpectrumPlan, channel_taps,
                                            ddc_taps, freq_word, freq_word_hz, iq8_to_c64)
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
TWINS = {"sdrk_exec_device_downconv_iq8": "sdrk_exec_device_ddc_ci16",
         "sdrk_exec_device_downconv_iq8_timed_each": "sdrk_exec_device_ddc_timed_each",
         "sdrk_exec_host_downconv_iq8": "sdrk_exec_host_ddc_ci16",
         "sdrk_exec_device_downconvbank_iq8": "sdrk_exec_device_ddcbank_ci16",
         "sdrk_exec_device_downconvbank_iq8_timed_each": "sdrk_exec_device_ddcbank_timed_each",
         "sdrk_exec_host_downconvbank_iq8": "sdrk_exec_host_ddcbank_ci16"}


def test_header_table_and_exports_agree_on_the_six_names():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "downconv" in n)
    table = {name: (res, args) for name, res, args in _ffi.SYMBOLS}
    assert declared == sorted(TWINS) == sorted(n for n in table if "downconv" in n)
    handle = ctypes.CDLL(_ffi.library_path())
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    for name, twin in TWINS.items():
        assert hasattr(handle, name) and getattr(_ffi.lib(), name).argtypes == table[name][1]
        at = 3 if "_host_" in name else 2                                        # behind the samples pointer (host: prefix, iq)
        res, args = table[twin]
        assert table[name] == (res, [*args[:at], ctypes.c_int, *args[at:]]), name
        decl = norm(re.search(rf"int {name}\(([^;]*)\);", header).group(1)).split(", ")
        want = norm(re.search(rf"int {twin}\(([^;]*)\);", header).group(1)).split(", ")
        assert decl[at] == "int iq8_format" and len(decl) == len(want) + 1, name
        rest = [re.sub(r"_(iq8|ci16|c64)\b", "", p) for p in decl[:at] + decl[at + 1:]]
        assert rest == [re.sub(r"_(iq8|ci16|c64)\b", "", p) for p in want], name
        for fragment in ("ddc", "_fir", "chanbank", "_xspec"):                    # the sets the other ABI tests pin stay theirs
            assert fragment not in name
        assert not re.search(r"_sk(_|$)", name)
    assert "#define SDRK_VERSION 500" in text and _ffi.lib().sdrk_version() == 500   # additions do not bump it
    assert text.count("digital down-converter (DDC)") == 1
    section = text.split("the down-converter from 8-bit input")[1].split("measurement probes")[0]
    for word in ("2*4096/L + 8/D", "0x80", "+0.5 + 0.5i", "+0.0 + 0.0i", "NULL prefix", "bits of the complex64 call"):
        assert word in section, word
    for name in ("ddc_ci8", "ddc_bank_ci8"):
        assert getattr(pkg, name) is getattr(spectrum, name) is getattr(processing, name)
        assert name in pkg.__all__ and name in processing.__all__
    for name in ("ddc_ci8", "ddc_bank_ci8", "exec_device_ddc_ci8", "exec_device_ddc_ci8_timed_each", "exec_device_ddc_bank_ci8",
                 "exec_device_ddc_bank_ci8_timed_each"):
        assert callable(getattr(SpectrumPlan, name))


def test_refusals_through_ctypes_need_no_device():
    lib = _ffi.lib()
    INVALID = _ffi.SDRK_ERR_INVALID
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    words = (ctypes.c_uint32 * 3)(0, 1, 2)
    n_out = ctypes.c_size_t()
    calls = (lambda pl, fmt: lib.sdrk_exec_device_downconv_iq8(pl, p, fmt, 8, 5, 7, 0, p, None),
             lambda pl, fmt: lib.sdrk_exec_device_downconv_iq8_timed_each(pl, p, fmt, 8, 5, 7, 0, p, 2, each),
             lambda pl, fmt: lib.sdrk_exec_host_downconv_iq8(pl, None, p, fmt, 8, 5, 7, 0, p, ctypes.byref(n_out)),
             lambda pl, fmt: lib.sdrk_exec_device_downconvbank_iq8(pl, p, fmt, 8, 3, words, 7, 0, p, 8, None),
             lambda pl, fmt: lib.sdrk_exec_device_downconvbank_iq8_timed_each(pl, p, fmt, 8, 3, words, 7, 0, p, 8, 2, each),
             lambda pl, fmt: lib.sdrk_exec_host_downconvbank_iq8(pl, None, p, fmt, 8, 3, words, 7, 0, p, 8, ctypes.byref(n_out)))
    for call in calls:
        for fmt in (2, -1, 255):                                                  # the text of the 8-bit spectra's refusal
            assert call(None, fmt) == INVALID
            assert f"iq8_format {fmt} is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED".encode() == lib.sdrk_last_error()
        for fmt in (0, 1):
            assert call(None, fmt) == INVALID and b"NULL" in lib.sdrk_last_error()
    for launches, ms in ((0, each), (4097, each), (2, None)):
        assert lib.sdrk_exec_device_downconv_iq8_timed_each(None, p, 0, 8, 5, 7, 0, p, launches, ms) == INVALID
        assert b"launches" in lib.sdrk_last_error()
    # (taps unset, D out of range, n_chan, out_stride and NULL pointers on a plan: tests/host_api_downconv_iq8_stress.cpp, which
    # has a stand-in device to make plans on)


class NumpyPlan:
    """What the streams ask of a plan, answered by the float64 definition of include/sdrk.h; records what reached it."""

    def __init__(self):
        self.calls = []

    def set_fir(self, taps):
        self.h = np.asarray(taps, np.complex128)
        return self.h.shape[0]

    def _run(self, x, word, decim, prefix, sample0):
        m = self.h.shape[0]
        pre = np.zeros(m - 1, np.complex128) if prefix is None else prefix.astype(np.complex128)
        assert pre.shape == (m - 1,)
        s = ((word + 0x80000) >> 20) & 4095
        hs = self.h * np.exp(2j * np.pi * s * np.arange(m) / N)
        v = np.convolve(np.concatenate((pre, x.astype(np.complex128))), hs, "valid")
        idx = [sample0 + j for j in range(v.shape[0])]
        phase = np.array([(word * (j & 0xFFFFFFFF)) & 0xFFFFFFFF for j in idx], dtype=np.float64)
        y = v * np.exp(-2j * np.pi * phase / 2.0 ** 32)
        return y[np.array([j % decim == 0 for j in idx], dtype=bool)].astype(np.complex64)

    def ddc(self, x, word, *, decim, prefix, sample0):
        self.calls.append(("ddc", x.dtype, x.shape[0], prefix, sample0))
        return self._run(x, word, decim, prefix, sample0)

    def ddc_ci8(self, x, word, *, decim, prefix, sample0):
        assert x.dtype in (np.int8, np.uint8) and x.ndim == 2 and (prefix is None or prefix.dtype == x.dtype)
        self.calls.append(("ddc_ci8", x.dtype, x.shape[0], None if prefix is None else prefix.copy(), sample0))
        if prefix is None and self.h.shape[0] > 1:                               # what the C entry takes a NULL prefix for
            prefix = np.full((self.h.shape[0] - 1, 2), 128 if x.dtype == np.uint8 else 0, x.dtype)
        return self._run(iq8_to_c64(x), word, decim, None if prefix is None else iq8_to_c64(prefix), sample0)

    def ddc_bank_ci8(self, x, words, *, decim, prefix, sample0):
        return np.stack([self.ddc_ci8(x, w, decim=decim, prefix=prefix, sample0=sample0) for w in words])

    def fir(self, x, *, decim, shift_bins, prefix, sample0):
        self.calls.append(("fir", x.dtype, x.shape[0], prefix, sample0))
        return self._run(x, (shift_bins << 20) & 0xFFFFFFFF, decim, prefix, sample0)


def raw_bytes(seed, n, dtype):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 2)).astype(np.uint8).view(dtype)


@pytest.mark.parametrize("dtype,silence", [(np.int8, 0), (np.uint8, 128)])
def test_streams_take_8_bit_pieces_one_dtype_throughout_from_a_first_tail_of_mid_scale_bytes(dtype, silence):
    fs, d = 2.4e6, 7
    h = ddc_taps(d, 33)
    raw = raw_bytes(4, 5000, dtype)
    plan = NumpyPlan()
    ch = DdcStream(plan, h, d, -100.6 * fs / N, fs)
    out, at = [], 0
    for p in (1, 0, 3, 31, 32, 33, 1000, 3900):
        out.append(ch.push(raw[at:at + p]))
        at += p
        assert ch.sample_index == at
    assert at == 5000 and out[1].shape == (0,) and len(plan.calls) == 7            # an empty piece makes no call
    assert all(c[0] == "ddc_ci8" and c[1] == dtype for c in plan.calls)           # the bytes reach the 8-bit method as they are
    assert plan.calls[0][3] is None and plan.calls[0][4] == 0                     # no samples yet: the NULL prefix
    for (_, _, n, pre, s0), start in zip(plan.calls[1:], (1, 4, 35, 67, 100, 1100)):
        want = np.concatenate((np.full((32, 2), silence, dtype), raw[:start]))[-32:]   # the first tail: bytes of 0 / 128
        assert s0 == start and pre.dtype == dtype and np.array_equal(pre, want)
    whole = NumpyPlan()
    whole.set_fir(h)
    start = np.full(32, complex(iq8_to_c64(np.full((1, 2), silence, dtype))[0]), np.complex64)
    assert start[0] == (0.5 + 0.5j if dtype == np.uint8 else 0.0)
    ref = whole._run(iq8_to_c64(raw), ch.freq_word, d, start, 0)
    got = np.concatenate(out)
    assert got.shape == ref.shape == (715,) and np.abs(got - ref).max() < 1e-3
    # one dtype throughout: the other 8-bit dtype, int16 and complex are refused as mixing is today
    other = np.uint8 if dtype == np.int8 else np.int8
    for bad in (raw[:10].view(other), np.zeros((10, 2), np.int16), np.zeros(10, np.complex64)):
        with pytest.raises(ValueError, match="not both"):
            ch.push(bad)
    for bad in (raw[:10, :1], raw[:10].reshape(5, 2, 2), raw[:10].reshape(-1)):    # the dtype rules of _as_ci8
        with pytest.raises(ValueError, match="8-bit"):
            ch.push(bad)
    assert ch.sample_index == 5000 and len(plan.calls) == 7                       # a refused piece changes nothing
    # the bank: rows are the single streams; a stream that began complex refuses bytes
    offs = [0.0, 1234.5, -250000.25]
    bank = DdcBankStream(NumpyPlan(), h, d, offs, fs)
    singles = [DdcStream(NumpyPlan(), h, d, f, fs) for f in offs]
    at = 0
    for p in (10, 0, 49, 1000, 1941):
        rows = bank.push(raw[at:at + p])
        for c, one in enumerate(singles):
            assert np.array_equal(rows[c], one.push(raw[at:at + p]))
        at += p
    assert bank._tail.dtype == dtype and bank.sample_index == 3000
    started = DdcStream(NumpyPlan(), h, d, 0.0, fs)
    started.push(np.zeros(40, np.complex64))
    with pytest.raises(ValueError, match="not both"):
        started.push(raw[:10])


@pytest.mark.parametrize("dtype,silence", [(np.int8, 0), (np.uint8, 128)])
def test_channel_streams_route_8_bit_pieces_through_the_call_with_the_bins_word(dtype, silence):
    fs, d = 1.0e6, 4
    h = channel_taps(d, 33)
    raw = raw_bytes(6, 3000, dtype)
    plan = NumpyPlan()
    ch = ChannelStream(plan, h, d, -100000.0, fs)
    assert ch.shift_bins == -410 and ch.tuned_hz == -410 * (fs / N)               # reported as now
    out = [ch.push(raw[:1001]), ch.push(raw[1001:])]
    assert [c[0] for c in plan.calls] == ["ddc_ci8", "ddc_ci8"] and plan.calls[1][4] == 1001 == ch.sample_index - 1999
    assert np.array_equal(plan.calls[1][3], np.concatenate((np.full((32, 2), silence, dtype), raw[:1001]))[-32:])
    word = ((-410) % N) << 20
    whole = NumpyPlan()
    whole.set_fir(h)
    start = np.full(32, complex(iq8_to_c64(np.full((1, 2), silence, dtype))[0]), np.complex64)
    assert np.abs(np.concatenate(out) - whole._run(iq8_to_c64(raw), word, d, start, 0)).max() < 1e-3
    with pytest.raises(ValueError, match="not both"):
        ch.push(np.zeros((10, 2), np.int16))
    for bad in (3, 0, 512):
        with pytest.raises(ValueError):                                           # the decimation stays a power of two up to 256
            ChannelStream(plan, h, bad, 0.0, fs)
    bank = ChannelBankStream(NumpyPlan(), h, d, [-100000.0, 0.0], fs)
    rows = bank.push(raw[:1001])
    assert bank.shift_bins == [-410, 0] and np.array_equal(rows[0], out[0]) and rows.shape == (2, out[0].shape[0])
    complex_first = ChannelStream(NumpyPlan(), h, d, 0.0, fs)
    complex_first.push(np.zeros(40, np.complex64))
    assert complex_first.plan.calls[0][0] == "fir"                                 # complex pieces go where they went
    with pytest.raises(ValueError, match="not both"):
        complex_first.push(raw[:10])


def test_plan_methods_check_dtype_shape_and_prefix_before_any_call():
    plan = bare_plan(N)
    plan.fir_taps = 0
    good = np.zeros((100, 2), np.uint8)
    with pytest.raises(ValueError, match="set_fir"):
        plan.ddc_ci8(good, 5)
    plan.fir_taps = 9
    for bad in (np.zeros(100, np.complex64), good.astype(np.int16), good.astype(np.float32), np.zeros(100, np.int8),
                np.zeros((100, 3), np.uint8), np.zeros((100, 4), np.uint8)[:, ::2], np.zeros((2, 50, 2), np.int8), good.tolist()):
        for call in (lambda: plan.ddc_ci8(bad, 5), lambda: plan.ddc_bank_ci8(bad, [5, 6]),
                     lambda: spectrum.ddc_ci8(bad, np.ones(3), 0.0, 1e6), lambda: spectrum.ddc_bank_ci8(bad, np.ones(3), [0.0], 1e6)):
            with pytest.raises(ValueError, match="8-bit"):
                call()
    for kw in ({"decim": 0}, {"decim": 257}, {"sample0": -1}, {"prefix": np.zeros((7, 2), np.uint8)},
               {"prefix": np.zeros((8, 2), np.int8)}, {"prefix": np.zeros(8, np.complex64)}):   # short, the other dtype, complex
        with pytest.raises(ValueError):
            plan.ddc_ci8(good, 5, **kw)
        with pytest.raises(ValueError):
            plan.ddc_bank_ci8(good, [5, 6], **kw)
    for bad in ([], list(range(65))):
        with pytest.raises(ValueError, match="1..64"):
            plan.ddc_bank_ci8(good, bad)
    for entry in ("exec_device_ddc_ci8", "exec_device_ddc_ci8_timed_each"):
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 100, 0x2000, 5, decim=300)
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 8, 0x2000, 5, unsigned=True)
    with pytest.raises(ValueError, match="out_stride"):
        plan.exec_device_ddc_bank_ci8(0x1000, 100, 0x2000, [1, 2], decim=7, out_stride=3)
    with pytest.raises(ValueError):
        spectrum.ddc_ci8(good, np.ones(3), 0.0, 1e6, decim=300)
    double = bare_plan(N, double=True)
    double.fir_taps = 9
    with pytest.raises(ValueError):
        double.ddc_ci8(good, 5)


class _FakeDdcStream(DdcStream):
    seen = []

    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offset_hz, sample_rate)
        _FakeDdcStream.seen.append(self.plan)


class _FakeDdcBankStream(DdcBankStream):
    def __init__(self, plan, taps, decim, offsets_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offsets_hz, sample_rate)
        _FakeDdcStream.seen.append(self.plan)


class _FakeChannelStream(ChannelStream):
    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offset_hz, sample_rate)
        _FakeDdcStream.seen.append(self.plan)


class _FakeChannelBankStream(ChannelBankStream):
    def __init__(self, plan, taps, decim, offsets_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offsets_hz, sample_rate)
        _FakeDdcStream.seen.append(self.plan)


@pytest.mark.parametrize("dtype,datatype", [(np.int8, "ci8"), (np.uint8, "cu8")])
def test_cli_extract_pushes_the_bytes_of_an_8_bit_recording_as_they_are(tmp_path, capsys, monkeypatch, dtype, datatype):
    fs, fc, d = 1.0e6, 1.0e9, 5
    raw = raw_bytes(5, 9000, dtype)
    base, out = str(tmp_path / "rec"), str(tmp_path / "chan")
    sigmf_io.write_sigmf(base, raw, fs, fc, datatype=datatype)
    monkeypatch.setattr(spectrum, "DdcStream", _FakeDdcStream)
    monkeypatch.setattr(spectrum, "DdcBankStream", _FakeDdcBankStream)
    monkeypatch.setattr(spectrum, "ChannelStream", _FakeChannelStream)
    monkeypatch.setattr(spectrum, "ChannelBankStream", _FakeChannelBankStream)
    monkeypatch.setattr(cli, "EXTRACT_PIECE", 4001)                               # three pieces, cut off the multiples of D
    silence = np.full(1, 0.5 + 0.5j if dtype == np.uint8 else 0.0, np.complex64)

    def calls():
        made = [c for p in _FakeDdcStream.seen for c in p.calls]
        _FakeDdcStream.seen.clear()
        return made

    calls()
    # --exact, one offset
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000.3", "--decim", str(d), "--exact", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    word = freq_word(100000.3, fs)
    assert list(report) == ["wrote", "samples_in", "samples_out", "sample_rate", "center_freq", "tuned_offset_hz", "freq_word", "decim",
                            "taps"]                                               # the report is what it was
    assert report["freq_word"] == word and report["tuned_offset_hz"] == freq_word_hz(word, fs)
    assert report["samples_in"] == 9000 and report["samples_out"] == 1800 and report["taps"] == 81 and report["decim"] == 5
    made = calls()
    assert [(c[0], c[1], c[2]) for c in made] == [("ddc_ci8", np.dtype(dtype), 4001), ("ddc_ci8", np.dtype(dtype), 4001),
                                                  ("ddc_ci8", np.dtype(dtype), 998)]          # unwidened, 2 bytes a sample
    y, meta = sigmf_io.read_sigmf(out)
    assert y.dtype == np.complex64 and y.shape == (1800,) and meta["sample_rate"] == fs / d
    whole = NumpyPlan()
    whole.set_fir(ddc_taps(d))
    assert np.abs(y - whole._run(iq8_to_c64(raw), word, d, np.repeat(silence, 80), 0)).max() < 1e-2
    # --exact, several offsets: the bank, one recording each
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000.3", "-7.5", "--decim", "50", "--exact", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [c["freq_word"] for c in report["channels"]] == [word, freq_word(-7.5, fs)] and report["samples_out"] == 180
    assert list(report) == ["channels", "samples_in", "samples_out", "sample_rate", "decim", "taps"]
    made = calls()
    assert made and all(c[0] == "ddc_ci8" and c[1] == dtype for c in made)
    assert sigmf_io.read_sigmf(out + "_1")[0].shape == (180,)
    # without --exact: the bin-tuned streams, single and several offsets
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000", "--decim", "4", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(report) == ["wrote", "samples_in", "samples_out", "sample_rate", "center_freq", "tuned_offset_hz", "shift_bins", "decim",
                            "taps"]
    assert report["shift_bins"] == 410 and report["samples_out"] == 2250 and "freq_word" not in report
    made = calls()
    assert [(c[0], c[1]) for c in made] == [("ddc_ci8", np.dtype(dtype))] * 3
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000", "0", "--decim", "4", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [c["shift_bins"] for c in report["channels"]] == [410, 0] and report["samples_out"] == 2250
    made = calls()
    assert made and all(c[0] == "ddc_ci8" and c[1] == dtype for c in made)
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "0", "--decim", "3", "--out", out]) == 2
    assert "power of two" in capsys.readouterr().err

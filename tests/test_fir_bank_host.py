"""The channel bank without a GPU: header and ctypes table agree on the five symbols, the refusals that need no device, the Python
argument checks and output shapes, ChannelBankStream's bookkeeping against ChannelStream's with the C call replaced by the float64
numpy reference, and the command line's naming for one offset and for several."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import ChannelBankStream, ChannelStream, channel_taps
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
FIVE = sorted(["sdrk_exec_device_chanbank", "sdrk_exec_device_chanbank_ci16", "sdrk_exec_device_chanbank_timed_each",
               "sdrk_exec_host_chanbank", "sdrk_exec_host_chanbank_ci16"])


def test_header_and_ctypes_table_agree_on_the_five_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "chanbank" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == FIVE == sorted(n for n in table if "chanbank" in n)
    for n in FIVE:
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
    assert "#define SDRK_VERSION 500" in text
    section = text.split("channel bank: C tuned channels")[1].split("measurement probes")[0]
    for word in ("out_stride >= n_out", "phase0 = NULL", "EXACTLY THE BITS", "per-channel filters or decimation", "more than 64 channels"):
        assert word in section, word
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in FIVE)
    for name in ("fir_bank", "ChannelBankStream"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    shifts = (ctypes.c_int * 3)(0, 5, -5)
    each = (ctypes.c_float * 2)()
    n_out = ctypes.c_size_t()
    for fn in (lib.sdrk_exec_device_chanbank, lib.sdrk_exec_device_chanbank_ci16):
        assert fn(None, p, 8, 1, 3, shifts, None, p, 8, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_exec_device_chanbank_timed_each(None, p, 8, 1, 3, shifts, None, p, 8, 0, each) == _ffi.SDRK_ERR_INVALID
    assert b"launches" in lib.sdrk_last_error()
    assert lib.sdrk_exec_device_chanbank_timed_each(None, p, 8, 1, 3, shifts, None, p, 8, 2, each) == _ffi.SDRK_ERR_INVALID
    for fn in (lib.sdrk_exec_host_chanbank, lib.sdrk_exec_host_chanbank_ci16):
        assert fn(None, None, p, 8, 1, 3, shifts, 0, p, 8, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_last_error() == b"plan is NULL"


def test_python_argument_checks():
    plan = bare_plan(N)
    plan.fir_taps = 0
    x = np.zeros(100, np.complex64)
    with pytest.raises(ValueError, match="set_fir"):
        plan.fir_bank(x, [0, 1])
    with pytest.raises(ValueError, match="set_fir"):
        plan.exec_device_fir_bank(0x1000, 100, 0x2000, [0, 1])
    plan.fir_taps = 9
    for shifts in ([], list(range(65)), [0, 2048], [-2049], [[1, 2], [3, 5000]]):
        with pytest.raises(ValueError):
            plan.fir_bank(x, shifts)
        with pytest.raises(ValueError):
            plan.fir_bank_ci16(np.zeros((100, 2), np.int16), shifts)
        for entry in ("exec_device_fir_bank", "exec_device_fir_bank_ci16", "exec_device_fir_bank_timed_each"):
            with pytest.raises(ValueError):
                getattr(plan, entry)(0x1000, 100, 0x2000, shifts)
        with pytest.raises(ValueError):
            spectrum.fir_bank(x, np.ones(3), shifts)
    for kw in ({"decim": 3}, {"decim": 0}, {"decim": 512}, {"sample0": -1}, {"prefix": np.zeros(7, np.complex64)}):
        with pytest.raises(ValueError):
            plan.fir_bank(x, [0, 1], **kw)
    with pytest.raises(ValueError):
        plan.fir_bank_ci16(np.zeros((100, 2), np.int32), [0, 1])
    with pytest.raises(ValueError):
        plan.fir_bank_ci16(np.zeros((100, 2), np.int16), [0, 1], prefix=np.zeros((9, 2), np.int16))
    for entry in ("exec_device_fir_bank", "exec_device_fir_bank_ci16", "exec_device_fir_bank_timed_each"):
        with pytest.raises(ValueError, match="power of two"):
            getattr(plan, entry)(0x1000, 100, 0x2000, [0, 1], decim=6)
        with pytest.raises(ValueError, match="out_stride"):
            getattr(plan, entry)(0x1000, 100, 0x2000, [0, 1], out_stride=91)       # 92 outputs
        with pytest.raises(ValueError, match="phase0"):
            getattr(plan, entry)(0x1000, 100, 0x2000, [0, 1], phase0=[1, 2, 3])
        with pytest.raises(ValueError, match="taps"):
            getattr(plan, entry)(0x1000, 8, 0x2000, [0, 1])                        # n_in < M
    args = plan._device_fir_bank_args(0x1000, 100, 0x2000, [7, -7, 7], 4, [-1, 4096, 5], None)
    assert args[2:4] == [4, 3] and list(args[4]) == [7, -7, 7] and list(args[5]) == [4095, 0, 5] and args[7].value == 23
    assert plan._device_fir_bank_args(0x1000, 100, 0x2000, [7], 1, None, 200)[5] is None
    double = bare_plan(N, double=True)
    with pytest.raises(ValueError, match="double"):
        double.fir_bank(x.astype(np.complex128), [0])
    with pytest.raises(ValueError):
        spectrum.fir_bank(x, np.ones(3), [0, 1], decim=5)


class NumpyPlan:
    """What ChannelStream and ChannelBankStream ask of a plan, answered by the float64 definition of include/sdrk.h."""

    def __init__(self):
        self.calls = []

    def set_fir(self, taps):
        self.h = np.asarray(taps, np.complex128)
        return self.h.shape[0]

    def _one(self, x, decim, shift_bins, prefix, sample0):
        m = self.h.shape[0]
        pre = np.zeros(m - 1, np.complex128) if prefix is None else prefix.astype(np.complex128)
        assert pre.shape == (m - 1,)
        hs = self.h * np.exp(2j * np.pi * shift_bins * np.arange(m) / N)
        v = np.convolve(np.concatenate((pre, x.astype(np.complex128))), hs, "valid")
        j = sample0 + np.arange(v.shape[0])
        y = v * np.exp(-2j * np.pi * ((shift_bins * j) % N) / N)
        return y[j % decim == 0].astype(np.complex64)

    def fir(self, x, *, decim, shift_bins, prefix, sample0):
        self.calls.append((x.shape[0], None if prefix is None else prefix.copy(), sample0))
        return self._one(x, decim, shift_bins, prefix, sample0)

    def fir_ci16(self, x, *, decim, shift_bins, prefix, sample0):
        return self.fir_bank_ci16(x, [shift_bins], decim=decim, prefix=prefix, sample0=sample0)[0]

    def fir_bank(self, x, shift_bins, *, decim, prefix, sample0):
        self.calls.append((x.shape[0], None if prefix is None else prefix.copy(), sample0))
        return np.stack([self._one(x, decim, s, prefix, sample0) for s in shift_bins])

    def fir_bank_ci16(self, x, shift_bins, *, decim, prefix, sample0):
        assert x.dtype == np.int16 and (prefix is None or prefix.dtype == np.int16)
        wide = lambda a: None if a is None else a.astype(np.float32).view(np.complex64).reshape(-1)   # noqa: E731
        return self.fir_bank(wide(x), shift_bins, decim=decim, prefix=wide(prefix), sample0=sample0)


def test_channel_bank_stream_keeps_one_tail_and_index_and_equals_channel_streams():
    fs, d = 2.4e6, 8
    h = channel_taps(d, 33)
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    offsets = (-100.6 * fs / N, 0.0, 611.2 * fs / N, -100.6 * fs / N)
    plan = NumpyPlan()
    bank = ChannelBankStream(plan, h, d, offsets, fs)
    assert bank.shift_bins == [-101, 0, 611, -101] and bank.tuned_hz == [s * fs / N for s in bank.shift_bins]
    assert bank.out_rate == fs / d and bank.ntaps == 33
    singles = [ChannelStream(NumpyPlan(), h, d, f, fs) for f in offsets]
    assert [s.shift_bins for s in singles] == bank.shift_bins
    out, at = [], 0
    for p in (1, 0, 7, 31, 32, 33, 1000, 3896):
        got = bank.push(x[at:at + p])
        want = [s.push(x[at:at + p]) for s in singles]
        at += p
        assert bank.sample_index == at == singles[0].sample_index
        assert got.shape == (4, want[0].shape[0]) and got.dtype == np.complex64
        for c in range(4):
            assert np.array_equal(got[c], want[c]), (p, c)
        out.append(got)
    assert out[1].shape == (4, 0) and len(plan.calls) == 7                        # an empty piece makes no call
    assert plan.calls[0][1] is None and plan.calls[0][2] == 0                     # no samples yet: a zero prefix
    for mine, theirs in zip(plan.calls, singles[2].plan.calls):                   # ONE tail, the one a single stream keeps
        assert mine[0] == theirs[0] and mine[2] == theirs[2]
        assert (mine[1] is None and theirs[1] is None) or np.array_equal(mine[1], theirs[1])
    assert np.concatenate(out, axis=1).shape == (4, 625)
    bank.close()                                                                  # (a plan that was handed in is not closed)
    for bad in ((0.6 * fs,), (), tuple(range(65))):
        with pytest.raises(ValueError):
            ChannelBankStream(plan, h, d, bad, fs)
    with pytest.raises(ValueError):
        ChannelBankStream(plan, h, 3, (0.0,), fs)
    bank = ChannelBankStream(plan, h, d, (0.0, 1e5), fs)
    bank.push(x[:10])
    with pytest.raises(ValueError, match="not both"):
        bank.push(np.zeros((10, 2), np.int16))


class _FakeStream(ChannelStream):
    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offset_hz, sample_rate)


class _FakeBank(ChannelBankStream):
    made = 0

    def __init__(self, plan, taps, decim, offsets_hz, sample_rate, *, device=0):
        type(self).made += 1
        super().__init__(NumpyPlan(), taps, decim, offsets_hz, sample_rate)


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_cli_extract_names_one_channel_as_before_and_several_by_index(tmp_path, capsys, monkeypatch, datatype):
    fs, fc, d = 1.0e6, 1.0e9, 4
    rng = np.random.default_rng(5)
    i16 = rng.integers(-2048, 2048, size=(9000, 2)).astype(np.int16)
    x = i16 if datatype == "ci16_le" else i16.astype(np.float32).view(np.complex64).reshape(-1)
    base, out = str(tmp_path / "rec"), str(tmp_path / "chan")
    sigmf_io.write_sigmf(base, x, fs, fc, datatype=datatype)
    monkeypatch.setattr(spectrum, "ChannelStream", _FakeStream)
    monkeypatch.setattr(spectrum, "ChannelBankStream", _FakeBank)
    monkeypatch.setattr(cli, "EXTRACT_PIECE", 4000)                               # three pieces
    made = _FakeBank.made
    # one offset: the single stream, the old names and the old report
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000", "--decim", str(d), "--out", out]) == 0
    one = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert _FakeBank.made == made and one["shift_bins"] == 410 and one["samples_out"] == 2250
    assert sorted(os.path.basename(p) for p in one["wrote"]) == ["chan.sigmf-data", "chan.sigmf-meta"]
    y_one, _ = sigmf_io.read_sigmf(out)
    # several: one bank stream, BASE_0, BASE_1, ...
    offsets = ["100000", "-250000", "0"]
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", *offsets, "--decim", str(d), "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert _FakeBank.made == made + 1
    assert report["samples_in"] == 9000 and report["samples_out"] == 2250 and report["taps"] == 65 and report["sample_rate"] == fs / d
    assert [c["shift_bins"] for c in report["channels"]] == [410, -1024, 0]
    for c, ch in enumerate(report["channels"]):
        assert sorted(os.path.basename(p) for p in ch["wrote"]) == [f"chan_{c}.sigmf-data", f"chan_{c}.sigmf-meta"]
        y, meta = sigmf_io.read_sigmf(f"{out}_{c}")
        assert y.dtype == np.complex64 and y.shape == (2250,)
        assert ch["center_freq"] == fc + ch["shift_bins"] * fs / N and ch["tuned_offset_hz"] == ch["shift_bins"] * fs / N
        assert meta["sample_rate"] == fs / d and meta["center_freq"] == int(ch["center_freq"])
    assert np.array_equal(sigmf_io.read_sigmf(out + "_0")[0], y_one)              # channel 0 is the single extraction's channel
    # refusals keep their form
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "0", "6e5", "--decim", str(d), "--out", out]) == 2
    assert "shift_bins" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "--decim", str(d), "--out", out])

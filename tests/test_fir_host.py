"""FIR filtering and channel extraction without a GPU: header and ctypes table agree on the seven symbols, the refusals that need
no device, channel_taps against its stated gain and stopband, ChannelStream's bookkeeping with the C call replaced by the float64
numpy reference, and the command line's metadata and refusal."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import ChannelStream, channel_taps
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
SEVEN = sorted(["sdrk_plan_set_fir", "sdrk_plan_fir_taps", "sdrk_exec_device_fir", "sdrk_exec_device_fir_ci16",
                "sdrk_exec_device_fir_timed_each", "sdrk_exec_host_fir", "sdrk_exec_host_fir_ci16"])


def test_header_and_ctypes_table_agree_on_the_seven_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "_fir" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == SEVEN == sorted(n for n in table if "_fir" in n)
    for n in SEVEN:
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
    assert "#define SDRK_VERSION 500" in text
    section = text.split("FIR filtering and channel extraction")[1].split("measurement probes")[0]
    for word in ("other block lengths", "double precision", "rational resampling", "fine (sub-bin) tuning"):
        assert word in section, word                                       # said not to be provided
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in SEVEN)
    for name in ("channel_taps", "fir_filter", "ChannelStream"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    n_out = ctypes.c_size_t()
    assert lib.sdrk_plan_set_fir(None, 1, p) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_plan_fir_taps(None) == _ffi.SDRK_ERR_INVALID
    for fn in (lib.sdrk_exec_device_fir, lib.sdrk_exec_device_fir_ci16):
        assert fn(None, p, 8, 1, 0, 0, p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_exec_device_fir_timed_each(None, p, 8, 1, 0, 0, p, 0, each) == _ffi.SDRK_ERR_INVALID
    assert b"launches" in lib.sdrk_last_error()
    assert lib.sdrk_exec_device_fir_timed_each(None, p, 8, 1, 0, 0, p, 2, each) == _ffi.SDRK_ERR_INVALID
    for fn in (lib.sdrk_exec_host_fir, lib.sdrk_exec_host_fir_ci16):
        assert fn(None, None, p, 8, 1, 0, 0, p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_last_error() == b"plan is NULL"


def test_python_argument_checks():
    plan = bare_plan(N)
    plan.fir_taps = 0
    x = np.zeros(100, np.complex64)
    with pytest.raises(ValueError, match="set_fir"):
        plan.fir(x)
    with pytest.raises(ValueError, match="set_fir"):
        plan.exec_device_fir(0x1000, 100, 0x2000)
    plan.fir_taps = 9
    for kw in ({"decim": 3}, {"decim": 0}, {"decim": 512}, {"shift_bins": 2048}, {"shift_bins": -2049}, {"sample0": -1},
               {"prefix": np.zeros(7, np.complex64)}):
        with pytest.raises(ValueError):
            plan.fir(x, **kw)
    with pytest.raises(ValueError):
        plan.fir_ci16(np.zeros((100, 2), np.int32))
    with pytest.raises(ValueError):
        plan.fir_ci16(np.zeros((100, 2), np.int16), prefix=np.zeros((9, 2), np.int16))
    for entry in ("exec_device_fir", "exec_device_fir_ci16", "exec_device_fir_timed_each"):
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 100, 0x2000, decim=6)
        with pytest.raises(ValueError):
            getattr(plan, entry)(0x1000, 100, 0x2000, shift_bins=4000)
    assert plan.fir_outputs(100, 4) == (100 - 9) // 4 + 1
    with pytest.raises(ValueError):
        plan.fir_outputs(8)
    for bad in (np.zeros(0), np.zeros(2050), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            plan.set_fir(bad)
    double = bare_plan(N, double=True)
    with pytest.raises(ValueError, match="double"):
        double.set_fir(np.ones(3))
    with pytest.raises(ValueError):
        spectrum.fir_filter(x, np.ones(3), decim=5)


@pytest.mark.parametrize("window,floor_db", [("hann", -55.0), ("blackman", -75.0)])
def test_channel_taps_has_unit_dc_gain_and_the_stated_stopband(window, floor_db):
    """From 0.6/D on the response lies below -55 dB under Hann and below -75 dB under Blackman at the default length, for D up to
    128 (a Hann-windowed sinc of 16 D + 1 taps does not reach -60 dB: its worst case here is -56.4 dB); at D = 256 the 2049-tap
    limit leaves -43 dB under Hann."""
    for d in (1, 2, 4, 16, 128, 256):
        h = channel_taps(d, window=window)
        assert h.dtype == np.complex64 and h.shape == (min(16 * d + 1, 2049),) and np.all(h.imag == 0)
        assert abs(h.astype(np.complex128).sum() - 1) < 1e-6
        assert np.allclose(h, h[::-1])                                      # linear phase
        if d == 1:
            continue
        n = 1 << 19
        resp = np.abs(np.fft.fft(h.astype(np.complex128), n))
        f = np.abs(np.fft.fftfreq(n))
        stop = 20 * np.log10(resp[f >= 0.6 / d].max())
        want = floor_db if d <= 128 else (-43.0 if window == "hann" else -28.0)
        print(f"{window} D={d}: stopband {stop:.1f} dB")
        assert stop <= want, (window, d, stop)
        if d <= 128:
            assert abs(20 * np.log10(resp[f <= 0.2 / d].min())) < 0.1          # flat over the inner half of the passband
    assert channel_taps(1, 1).tolist() == [1] and channel_taps(4, 33).shape == (33,)
    assert np.allclose(channel_taps(4, 33, np.hanning(35)[1:-1]), channel_taps(4, 33))
    for bad in ((3, None), (0, None), (512, None), (4, 0), (4, 2050)):
        with pytest.raises(ValueError):
            channel_taps(*bad)
    with pytest.raises(ValueError):
        channel_taps(4, 33, "kaiser")


class NumpyPlan:
    """What ChannelStream asks of a plan, answered by the float64 definition of include/sdrk.h."""

    def __init__(self):
        self.calls = []

    def set_fir(self, taps):
        self.h = np.asarray(taps, np.complex128)
        return self.h.shape[0]

    def fir(self, x, *, decim, shift_bins, prefix, sample0):
        m = self.h.shape[0]
        self.calls.append((x.shape[0], None if prefix is None else prefix.copy(), sample0))
        pre = np.zeros(m - 1, np.complex128) if prefix is None else prefix.astype(np.complex128)
        assert pre.shape == (m - 1,)
        hs = self.h * np.exp(2j * np.pi * shift_bins * np.arange(m) / N)
        v = np.convolve(np.concatenate((pre, x.astype(np.complex128))), hs, "valid")
        j = sample0 + np.arange(v.shape[0])
        y = v * np.exp(-2j * np.pi * ((shift_bins * j) % N) / N)
        return y[j % decim == 0].astype(np.complex64)

    def fir_ci16(self, x, *, decim, shift_bins, prefix, sample0):
        assert x.dtype == np.int16 and (prefix is None or prefix.dtype == np.int16)
        wide = lambda a: None if a is None else a.astype(np.float32).view(np.complex64).reshape(-1)   # noqa: E731
        return self.fir(wide(x), decim=decim, shift_bins=shift_bins, prefix=wide(prefix), sample0=sample0)


def test_channel_stream_keeps_the_tail_the_index_and_the_rounded_offset():
    fs, d = 2.4e6, 8
    h = channel_taps(d, 33)
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    plan = NumpyPlan()
    ch = ChannelStream(plan, h, d, -100.6 * fs / N, fs)
    assert ch.shift_bins == -101 and ch.tuned_hz == -101 * fs / N and ch.out_rate == fs / d and ch.ntaps == 33
    out, at = [], 0
    for p in (1, 0, 7, 31, 32, 33, 1000, 3896):
        out.append(ch.push(x[at:at + p]))
        at += p
        assert ch.sample_index == at
    assert at == 5000 and out[1].shape == (0,) and len(plan.calls) == 7           # an empty piece makes no call
    assert plan.calls[0][1] is None and plan.calls[0][2] == 0                     # no samples yet: a zero prefix
    for (n, pre, s0), start in zip(plan.calls[1:], (1, 8, 39, 71, 104, 1104)):
        want = np.concatenate((np.zeros(32, np.complex64), x[:start]))[-32:]      # the 32 samples before the piece
        assert s0 == start and np.array_equal(pre, want)
    whole = NumpyPlan()
    whole.set_fir(h)
    ref = whole.fir(x, decim=d, shift_bins=-101, prefix=None, sample0=0)
    got = np.concatenate(out)
    assert got.shape == ref.shape == (625,) and np.abs(got - ref).max() < 1e-5
    ch.close()                                                                    # (a plan that was handed in is not closed)
    with pytest.raises(ValueError):
        ChannelStream(plan, h, d, 0.6 * fs, fs)                                   # beyond the band
    with pytest.raises(ValueError):
        ChannelStream(plan, h, 3, 0.0, fs)
    ch = ChannelStream(plan, h, d, 0.0, fs)
    ch.push(x[:10])
    with pytest.raises(ValueError, match="not both"):
        ch.push(np.zeros((10, 2), np.int16))


class _FakeStream(ChannelStream):
    def __init__(self, plan, taps, decim, offset_hz, sample_rate, *, device=0):
        super().__init__(NumpyPlan(), taps, decim, offset_hz, sample_rate)


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_cli_extract_writes_the_channel_with_its_rate_and_centre(tmp_path, capsys, monkeypatch, datatype):
    fs, fc, d = 1.0e6, 1.0e9, 4
    rng = np.random.default_rng(5)
    i16 = rng.integers(-2048, 2048, size=(9000, 2)).astype(np.int16)
    x = i16 if datatype == "ci16_le" else i16.astype(np.float32).view(np.complex64).reshape(-1)
    base, out = str(tmp_path / "rec"), str(tmp_path / "chan")
    sigmf_io.write_sigmf(base, x, fs, fc, datatype=datatype)
    monkeypatch.setattr(spectrum, "ChannelStream", _FakeStream)
    monkeypatch.setattr(cli, "EXTRACT_PIECE", 4000)                               # three pieces
    assert cli.main(["extract", base + ".sigmf-meta", "--offset-hz", "100000", "--decim", str(d), "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    bins = round(100000 / (fs / N))
    assert report["shift_bins"] == bins == 410 and report["tuned_offset_hz"] == bins * fs / N
    assert report["samples_in"] == 9000 and report["samples_out"] == 2250 and report["taps"] == 65
    y, meta = sigmf_io.read_sigmf(out)
    assert y.dtype == np.complex64 and y.shape == (2250,)
    assert report["sample_rate"] == fs / d and report["center_freq"] == fc + bins * fs / N
    assert meta["sample_rate"] == fs / d and meta["center_freq"] == int(fc + bins * fs / N)   # (the metadata holds whole hertz)
    assert meta["global"]["core:datatype"] == "cf32_le"
    whole = NumpyPlan()
    whole.set_fir(channel_taps(d))
    wide = i16.astype(np.float32).view(np.complex64).reshape(-1)
    assert np.abs(y - whole.fir(wide, decim=d, shift_bins=bins, prefix=None, sample0=0)).max() < 1e-2


def test_cli_extract_refuses_a_multi_channel_recording_and_bad_arguments(tmp_path, capsys):
    two = str(tmp_path / "two")
    sigmf_io.write_sigmf(two, np.zeros((8192, 2), np.complex64), 1e6, 1e9, num_channels=2)
    assert cli.main(["extract", two + ".sigmf-meta", "--offset-hz", "0", "--decim", "4", "--out", str(tmp_path / "o")]) == 2
    assert "single-channel" in capsys.readouterr().err
    one = str(tmp_path / "one")
    sigmf_io.write_sigmf(one, np.zeros(8192, np.complex64), 1e6, 1e9)
    assert cli.main(["extract", one + ".sigmf-meta", "--offset-hz", "0", "--decim", "3", "--out", str(tmp_path / "o")]) == 2
    assert "power of two" in capsys.readouterr().err
    assert cli.main(["extract", one + ".sigmf-meta", "--offset-hz", "6e5", "--decim", "4", "--out", str(tmp_path / "o")]) == 2
    assert "shift_bins" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "o") + ".sigmf-meta")
    with pytest.raises(SystemExit):
        cli.main(["extract", one + ".sigmf-meta", "--decim", "4", "--out", "x"])  # no --offset-hz

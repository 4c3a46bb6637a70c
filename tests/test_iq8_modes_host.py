"""The 8-bit filter-bank and spectral-kurtosis entry points without a GPU: the thirteen names in the header, the exports and
the ctypes table, each with its int16 twin's argument list plus the format; argument refusals through ctypes; dtype, shape and
argument refusals of the Python layer before any call; the frame / group arithmetic with the library stubbed (counts follow
the samples, not the bytes); and cli.py psd on stubbed spectrum functions: an 8-bit recording goes in as it is for --pfb and
--sk, and only the Welch leg widens it."""
import ctypes
import json
import os
import re
import threading

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# new name -> its int16 twin
TWINS = {
    "sdrk_exec_device_pfb_iq8": "sdrk_exec_device_pfb_ci16",
    "sdrk_exec_device_pfb_iq8_timed_each": "sdrk_exec_device_pfb_ci16_timed_each",
    "sdrk_exec_host_pfb_iq8": "sdrk_exec_host_pfb_ci16",
    "sdrk_exec_fft_host_pfb_iq8": "sdrk_exec_fft_host_pfb_ci16",
    "sdrk_exec_device_pfb_integrated_iq8": "sdrk_exec_device_pfb_integrated_ci16",
    "sdrk_exec_device_pfb_integrated_iq8_timed_each": "sdrk_exec_device_pfb_integrated_ci16_timed_each",
    "sdrk_exec_host_pfb_integrated_iq8": "sdrk_exec_host_pfb_integrated_ci16",
    "sdrk_exec_device_kurtosis_iq8": "sdrk_exec_device_sk_ci16",
    "sdrk_exec_device_kurtosis_iq8_timed_each": "sdrk_exec_device_sk_ci16_timed_each",
    "sdrk_exec_host_kurtosis_iq8": "sdrk_exec_host_sk_ci16",
    "sdrk_exec_device_pfb_kurtosis_iq8": "sdrk_exec_device_pfb_sk_ci16",
    "sdrk_exec_device_pfb_kurtosis_iq8_timed_each": "sdrk_exec_device_pfb_sk_ci16_timed_each",
    "sdrk_exec_host_pfb_kurtosis_iq8": "sdrk_exec_host_pfb_sk_ci16",
}


def test_thirteen_names_in_header_exports_and_ctypes_table():
    assert len(TWINS) == 13
    table = {s[0]: s for s in _ffi.SYMBOLS}
    header = open(os.path.join(REPO, "include", "sdrk.h")).read()
    handle = ctypes.CDLL(_ffi.library_path())
    norm = lambda s: re.sub(r"\s+", " ", s)
    for name, twin in TWINS.items():
        res, args = table[name][1:]
        assert res is table[twin][1] and list(args) == [*table[twin][2][:2], ctypes.c_int, *table[twin][2][2:]], name
        assert getattr(_ffi.lib(), name).argtypes == args and hasattr(handle, name)
        decl = norm(re.search(rf"int {name}\(([^;]*)\);", header).group(1))
        want = norm(re.search(rf"int {twin}\(([^;]*)\);", header).group(1))
        assert re.match(r"sdrk_plan\* plan, const void\* \w+, int iq8_format,", decl), name
        assert decl.replace(", int iq8_format", "").replace("iq8", "iq_ci16") == want, name     # the twin's list plus the format
        # the names keep clear of the sets other tests hold on the header's symbols
        assert not re.search(r"_sk(_|$)|ddc|downconv|_fir|chanbank|_xspec", name)
    assert "#define SDRK_VERSION 500" in header and _ffi.lib().sdrk_version() == 500    # additions do not bump it
    for fn in ("pfb_db_ci8", "pfb_integrated_db_ci8", "spectral_kurtosis_ci8"):
        assert getattr(pkg, fn) is getattr(spectrum, fn) and fn in pkg.__all__
    for fn in ("pfb_db_ci8", "pfb_fft_ci8", "pfb_integrate_ci8", "exec_device_pfb_ci8", "exec_device_pfb_ci8_timed_each",
               "exec_device_pfb_integrated_ci8", "exec_device_pfb_integrated_ci8_timed_each", "spectral_kurtosis_ci8",
               "pfb_spectral_kurtosis_ci8", "exec_device_sk_ci8", "exec_device_sk_ci8_timed_each", "exec_device_pfb_sk_ci8",
               "exec_device_pfb_sk_ci8_timed_each"):
        assert callable(getattr(SpectrumPlan, fn))
    m8, m16 = spectrum._PFB_CI8, spectrum._PFB_CI16
    assert m8.iq8 and m8.pfb and not m8.ci16 and all(spectrum._CI8[9:12])
    for field in m8._fields[2:12]:                                           # every slot of the mode table is the twin's
        assert TWINS[getattr(m8, field)] == getattr(m16, field), field
    for field in ("sk_host", "sk_device", "sk_timed_each"):
        assert TWINS[getattr(spectrum._CI8, field)] == getattr(spectrum._CI16, field), field


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    INVALID = _ffi.SDRK_ERR_INVALID
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    frames = (lambda fmt: lib.sdrk_exec_device_pfb_iq8(None, p, fmt, 1, 16, p, None),
              lambda fmt: lib.sdrk_exec_device_pfb_iq8_timed_each(None, p, fmt, 1, 16, p, 2, each),
              lambda fmt: lib.sdrk_exec_host_pfb_iq8(None, p, fmt, 1, 16, p),
              lambda fmt: lib.sdrk_exec_fft_host_pfb_iq8(None, p, fmt, 1, 16, p),
              lambda fmt: lib.sdrk_exec_device_pfb_integrated_iq8(None, p, fmt, 1, 2, 16, 0, 0, 1.0, p, None),
              lambda fmt: lib.sdrk_exec_device_pfb_integrated_iq8_timed_each(None, p, fmt, 1, 2, 16, 0, 0, 1.0, p, 2, each),
              lambda fmt: lib.sdrk_exec_host_pfb_integrated_iq8(None, p, fmt, 1, 2, 16, 0, 0, 1.0, p),
              lambda fmt: lib.sdrk_exec_device_pfb_kurtosis_iq8(None, p, fmt, 1, 2, 16, 0, 1.0, p, None),
              lambda fmt: lib.sdrk_exec_device_pfb_kurtosis_iq8_timed_each(None, p, fmt, 1, 2, 16, 0, 1.0, p, 2, each),
              lambda fmt: lib.sdrk_exec_host_pfb_kurtosis_iq8(None, p, fmt, 1, 2, 16, 0, 1.0, p))
    for call in frames:      # behind the filter bank the plan is looked at first, as the twins do: no plan, whatever the format
        for fmt in (0, 1, 2, -1):
            assert call(fmt) == INVALID and lib.sdrk_last_error() == b"plan is NULL"
    plain = (lambda fmt, g, k, s, form: lib.sdrk_exec_device_kurtosis_iq8(None, p, fmt, g, k, s, form, 1.0, p, None),
             lambda fmt, g, k, s, form: lib.sdrk_exec_device_kurtosis_iq8_timed_each(None, p, fmt, g, k, s, form, 1.0, p, 2, each),
             lambda fmt, g, k, s, form: lib.sdrk_exec_host_kurtosis_iq8(None, p, fmt, g, k, s, form, 1.0, p))
    for call in plain:
        for fmt in (2, -1, 255):
            assert call(fmt, 1, 2, 16, 0) == INVALID and f"iq8_format {fmt} is neither".encode() in lib.sdrk_last_error()
        for fmt in (0, 1):      # every refusal of the int16 twin, in its words
            twin_says = {}
            for what, args in (("form", (1, 2, 16, 2)), ("groups", (0, 2, 16, 0)), ("k", (1, 1, 16, 0)), ("range", (1 << 40, 1 << 40, 16, 0)),
                               ("stride", (1, 2, 0, 0)), ("plan", (1, 2, 16, 0))):
                assert lib.sdrk_exec_host_sk_ci16(None, p, *args, 1.0, p) == INVALID
                twin_says[what] = lib.sdrk_last_error()
                assert call(fmt, *args) == INVALID and lib.sdrk_last_error() == twin_says[what], what
            assert twin_says["plan"] == b"plan is NULL" and b"out_form 2" in twin_says["form"]
    for launches, ms in ((0, each), (4097, each), (2, None)):
        assert lib.sdrk_exec_device_kurtosis_iq8_timed_each(None, p, 0, 1, 2, 16, 0, 1.0, p, launches, ms) == INVALID
        assert b"launches" in lib.sdrk_last_error()
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.spectral_kurtosis_ci8(np.zeros((8192, 2), np.uint8), 4096, 2)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


class _Lib:
    """Stands where _ffi.lib() stands: records each host call with the format behind the input pointer."""

    def __init__(self):
        self.calls = []

    def _frames(name):
        def f(self, handle, iq, fmt, frames, stride, out):
            self.calls.append((name, fmt.value, frames.value, stride.value))
            return 0
        return f

    def _rows(name):
        def f(self, handle, iq, fmt, groups, k, hop, *rest):
            codes, scale = rest[:-2], rest[-2]
            self.calls.append((name, fmt.value, groups.value, k.value, hop.value, *codes, scale.value))
            return 0
        return f

    sdrk_exec_host_pfb_iq8 = _frames("pfb")
    sdrk_exec_fft_host_pfb_iq8 = _frames("pfb_fft")
    sdrk_exec_host_pfb_integrated_iq8 = _rows("pfb_int")
    sdrk_exec_host_kurtosis_iq8 = _rows("sk")
    sdrk_exec_host_pfb_kurtosis_iq8 = _rows("pfb_sk")

    def __getattr__(self, name):
        raise AssertionError(f"unexpected library call {name}")


class _Plan(SpectrumPlan):
    """The arithmetic of the SpectrumPlan methods without a device behind it."""

    def __init__(self, nfft, taps=0, wkey="rect"):     # (SpectrumPlan.__init__ needs a device)
        self.nfft, self._double, self._handle, self._lock, self._wkey = nfft, False, ctypes.c_void_p(1), threading.Lock(), wkey
        self.pfb_taps = taps

    def close(self):
        pass


@pytest.fixture
def stub(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(spectrum, "lib", lambda: fake)
    return fake


def test_frame_and_group_counts_follow_the_samples_not_the_bytes(stub):
    p = _Plan(64, taps=3)
    for dtype, fmt in ((np.int8, 0), (np.uint8, 1)):
        z = lambda samples: np.zeros((samples, 2), dtype)
        assert p.pfb_db_ci8(z(64 * 10)).shape == (8, 64) and stub.calls[-1] == ("pfb", fmt, 8, 64)          # 10 blocks, T = 3: 8 frames
        assert p.pfb_db_ci8(z(64 * 3 + 16 * 5 + 3), 16).shape == (6, 64) and stub.calls[-1] == ("pfb", fmt, 6, 16)
        spec = p.pfb_fft_ci8(z(64 * 4 + 63), 1)
        assert spec.shape == (128, 64) and spec.dtype == np.complex64 and stub.calls[-1] == ("pfb_fft", fmt, 128, 1)
        assert p.pfb_integrate_ci8(z(64 * 12), 3).shape == (3, 64)                                            # 10 frames: 3 groups, 1 dropped
        assert stub.calls[-1] == ("pfb_int", fmt, 3, 3, 64, 0, 0, 1.0)
        assert p.pfb_integrate_ci8(z(64 * 3 + 32 * 7), 4, hop=32, detector="min", out="power", scale=0.25).shape == (2, 64)
        assert stub.calls[-1] == ("pfb_int", fmt, 2, 4, 32, 2, 1, 0.25)
        mean, sk = p.spectral_kurtosis_ci8(z(64 * 10 + 63), 3)                                                # 10 frames of 64
        assert mean.shape == sk.shape == (3, 64) and mean.dtype == np.float32 and mean.base is sk.base
        assert stub.calls[-1] == ("sk", fmt, 3, 3, 64, 0, 1.0)                                                # (no detector argument)
        mean, sk = p.pfb_spectral_kurtosis_ci8(z(64 * 12), 5, out="power", scale=2.0)
        assert sk.shape == (2, 64) and stub.calls[-1] == ("pfb_sk", fmt, 2, 5, 64, 1, 2.0)
        n_calls = len(stub.calls)
        assert p.pfb_db_ci8(z(64 * 3 - 1)).shape == (0, 64) and p.pfb_integrate_ci8(z(64 * 4), 3).shape == (0, 64)
        assert p.spectral_kurtosis_ci8(z(64), 2)[1].shape == (0, 64) and p.pfb_spectral_kurtosis_ci8(z(64 * 3), 2)[0].shape == (0, 64)
        assert len(stub.calls) == n_calls                                                                    # nothing to run


def test_wrong_dtype_shape_or_arguments_are_refused_before_any_call(stub):
    p = _Plan(64, taps=2)
    good = np.zeros((512, 2), np.uint8)
    bad_inputs = (np.zeros(512, np.complex64), good.astype(np.int16), good.astype(np.float32), np.zeros(512, np.int8),
                  np.zeros((2, 256, 2), np.int8), np.zeros((512, 3), np.uint8), np.zeros((512, 4), np.uint8)[:, ::2], good.tolist())
    for bad in bad_inputs:
        for call in (lambda: p.pfb_db_ci8(bad), lambda: p.pfb_fft_ci8(bad), lambda: p.pfb_integrate_ci8(bad, 2),
                     lambda: p.spectral_kurtosis_ci8(bad, 2), lambda: p.pfb_spectral_kurtosis_ci8(bad, 2),
                     lambda: spectrum.pfb_db_ci8(bad, 64, 2), lambda: spectrum.pfb_integrated_db_ci8(bad, 64, 2, 2),
                     lambda: spectrum.spectral_kurtosis_ci8(bad, 64, 2)):      # (refused before a plan, and so a device, is asked for)
            with pytest.raises(ValueError, match="8-bit"):
                call()
    for dtype in (np.int8, np.uint8):            # byte pairs pick the 8-bit mode of pfb_spectral_kurtosis, as int16 picks its mode
        for bad in (np.zeros(512, dtype), np.zeros((512, 3), dtype)):
            with pytest.raises(ValueError, match="8-bit"):
                spectrum.pfb_spectral_kurtosis(bad, 64, 2, 2)
        with pytest.raises(ValueError, match="k must be >= 2"):
            spectrum.pfb_spectral_kurtosis(np.zeros((512, 2), dtype), 64, 2, 1)
    for kw in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median"), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            p.pfb_integrate_ci8(good, **kw)
    for kw in (dict(k=1), dict(k=2, hop=0), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            p.spectral_kurtosis_ci8(good, **kw)
        with pytest.raises(ValueError):
            p.pfb_spectral_kurtosis_ci8(good, **kw)
    for call in (lambda: p.exec_device_sk_ci8(1, 1, 1, 1), lambda: p.exec_device_pfb_sk_ci8(1, 1, 1, 1, unsigned=True),
                 lambda: p.exec_device_pfb_integrated_ci8(1, 0, 2, 1), lambda: p.exec_device_sk_ci8_timed_each(1, 2, 2, 1, frame_stride=0)):
        with pytest.raises(ValueError):
            call()
    # no prototype; a windowed plan behind the filter bank; a double plan
    bare, windowed = _Plan(64), _Plan(64, taps=2, wkey="hann")
    for call in (lambda: bare.pfb_db_ci8(good), lambda: bare.pfb_integrate_ci8(good, 2), lambda: bare.pfb_spectral_kurtosis_ci8(good, 2),
                 lambda: bare.exec_device_pfb_ci8(1, 1, 1), lambda: bare.exec_device_pfb_sk_ci8(1, 1, 2, 1)):
        with pytest.raises(ValueError, match="set_pfb"):
            call()
    for call in (lambda: windowed.pfb_integrate_ci8(good, 2), lambda: windowed.pfb_spectral_kurtosis_ci8(good, 2),
                 lambda: windowed.exec_device_pfb_integrated_ci8(1, 1, 2, 1)):
        with pytest.raises(ValueError, match="rectangular"):
            call()
    p._double = True
    for call in (lambda: p.pfb_db_ci8(good), lambda: p.pfb_fft_ci8(good), lambda: p.pfb_integrate_ci8(good, 2),
                 lambda: p.spectral_kurtosis_ci8(good, 2), lambda: p.pfb_spectral_kurtosis_ci8(good, 2),
                 lambda: p.exec_device_pfb_ci8(1, 1, 1), lambda: p.exec_device_pfb_ci8_timed_each(1, 1, 1),
                 lambda: p.exec_device_pfb_integrated_ci8(1, 1, 1, 1), lambda: p.exec_device_pfb_integrated_ci8_timed_each(1, 1, 1, 1),
                 lambda: p.exec_device_sk_ci8(1, 1, 2, 1), lambda: p.exec_device_sk_ci8_timed_each(1, 1, 2, 1),
                 lambda: p.exec_device_pfb_sk_ci8(1, 1, 2, 1), lambda: p.exec_device_pfb_sk_ci8_timed_each(1, 1, 2, 1)):
        with pytest.raises(ValueError, match="double"):
            call()
    assert stub.calls == []


def test_device_methods_pass_the_format_behind_the_input_pointer(monkeypatch):
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(handle, iq, fmt, *rest):
                seen.append((name, iq.value, fmt.value, len(rest)))
                return 0
            return f

    monkeypatch.setattr(spectrum, "lib", lambda: Lib())
    p = _Plan(64, taps=2)
    p.exec_device_pfb_ci8(11, 3, 12)
    p.exec_device_pfb_ci8_timed_each(11, 3, 12, 2, unsigned=True)
    p.exec_device_pfb_integrated_ci8(11, 3, 2, 12, unsigned=True)
    p.exec_device_pfb_integrated_ci8_timed_each(11, 3, 2, 12)
    p.exec_device_sk_ci8(11, 3, 2, 12, unsigned=True)
    p.exec_device_sk_ci8_timed_each(11, 3, 2, 12)
    p.exec_device_pfb_sk_ci8(11, 3, 2, 12)
    p.exec_device_pfb_sk_ci8_timed_each(11, 3, 2, 12, unsigned=True)
    # (arguments behind the format: the twin's, with the stream or the launch count and the milliseconds at the end)
    assert seen == [("sdrk_exec_device_pfb_iq8", 11, 0, 4), ("sdrk_exec_device_pfb_iq8_timed_each", 11, 1, 5),
                    ("sdrk_exec_device_pfb_integrated_iq8", 11, 1, 8), ("sdrk_exec_device_pfb_integrated_iq8_timed_each", 11, 0, 9),
                    ("sdrk_exec_device_kurtosis_iq8", 11, 1, 7), ("sdrk_exec_device_kurtosis_iq8_timed_each", 11, 0, 8),
                    ("sdrk_exec_device_pfb_kurtosis_iq8", 11, 0, 7), ("sdrk_exec_device_pfb_kurtosis_iq8_timed_each", 11, 1, 8)]


def test_cli_psd_pushes_an_8_bit_recording_as_it_is(tmp_path, monkeypatch, capsys):
    """--pfb, --pfb --integrate, --integrate --sk and --pfb --integrate --sk take the bytes as they are; --welch widens on the
    host and gets complex64, also when --pfb is given with it; a cf32_le recording goes where it went."""
    seen = []

    def fake(name, shape_of, pair=False):
        def f(x, *a, **kw):
            x = np.asarray(x)
            seen.append((name, x.dtype, x.shape))
            rows = np.zeros(shape_of(x, *a), np.float32) + 1.0
            return (rows, rows) if pair else rows
        return f

    n = lambda x: x.shape[0]
    monkeypatch.setattr(spectrum, "iq8_to_c64", (lambda real: lambda a: (seen.append(("iq8_to_c64", a.dtype, a.shape)), real(a))[1])(spectrum.iq8_to_c64))
    for name in ("spectrum_db_ci8", "spectrum_db"):
        monkeypatch.setattr(spectrum, name, fake(name, lambda x, **kw: (n(x),)))
    for name in ("integrated_db_ci8", "integrated_db"):
        monkeypatch.setattr(spectrum, name, fake(name, lambda x, nfft, k: (n(x) // nfft // k, nfft)))
    for name in ("pfb_db_ci8", "pfb_db"):
        monkeypatch.setattr(spectrum, name, fake(name, lambda x, nfft, t: (n(x) // nfft - t + 1, nfft)))
    for name in ("pfb_integrated_db_ci8", "pfb_integrated_db"):
        monkeypatch.setattr(spectrum, name, fake(name, lambda x, nfft, t, k: ((n(x) // nfft - t + 1) // k, nfft)))
    for name in ("spectral_kurtosis_ci8", "spectral_kurtosis"):
        monkeypatch.setattr(spectrum, name, fake(name, lambda x, nfft, k: (n(x) // nfft // k, nfft), pair=True))
    monkeypatch.setattr(spectrum, "pfb_spectral_kurtosis", fake("pfb_spectral_kurtosis", lambda x, nfft, t, k: ((n(x) // nfft - t + 1) // k, nfft), pair=True))
    monkeypatch.setattr(spectrum, "welch_psd", fake("welch_psd", lambda x, nfft, fs: (nfft,)))
    rng = np.random.default_rng(2)

    def run(base, *opts):
        seen.clear()
        assert cli.main(["psd", base + ".sigmf-meta", "--nfft", "64", *opts]) == 0
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    for dtype, datatype in ((np.int8, "ci8"), (np.uint8, "cu8")):
        raw = rng.integers(0, 256, size=(64 * 9, 2)).astype(np.uint8).view(dtype)
        base = str(tmp_path / datatype)
        sigmf_io.write_sigmf(base, raw, 1e6, 1e8, datatype=datatype)
        d, row, stream = np.dtype(dtype), (64, 2), (64 * 9, 2)
        report = run(base, "--pfb", "4")
        assert report["samples"] == 64 * 9 and report["pfb_rows"] == 6 and report["pfb_taps"] == 4
        assert seen == [("spectrum_db_ci8", d, row), ("pfb_db_ci8", d, stream)]
        report = run(base, "--pfb", "4", "--integrate", "3")
        assert report["pfb_integrated_rows"] == 2 and report["integrated_rows"] == 3
        assert seen == [("spectrum_db_ci8", d, row), ("integrated_db_ci8", d, stream), ("pfb_db_ci8", d, stream),
                        ("pfb_integrated_db_ci8", d, stream)]
        report = run(base, "--integrate", "3", "--sk")
        assert report["sk_rows"] == 3
        assert seen == [("spectrum_db_ci8", d, row), ("integrated_db_ci8", d, stream), ("spectral_kurtosis_ci8", d, stream)]
        report = run(base, "--pfb", "4", "--integrate", "3", "--sk")
        assert report["sk_rows"] == 2
        assert seen == [("spectrum_db_ci8", d, row), ("integrated_db_ci8", d, stream), ("pfb_db_ci8", d, stream),
                        ("pfb_integrated_db_ci8", d, stream), ("pfb_spectral_kurtosis", d, stream)]
        # the Welch leg alone widens, for itself; the filter bank beside it still takes the bytes
        report = run(base, "--welch", "32", "--pfb", "4")
        assert report["welch_segments"] == 18 and report["samples"] == 64 * 9 and report["pfb_rows"] == 6
        assert seen == [("spectrum_db_ci8", d, row), ("iq8_to_c64", d, stream), ("welch_psd", np.dtype(np.complex64), (64 * 9,)),
                        ("pfb_db_ci8", d, stream)]
    sigmf_io.write_sigmf(str(tmp_path / "c"), np.zeros(64 * 9, np.complex64), 1e6, 1e8)
    c64 = np.dtype(np.complex64)
    run(str(tmp_path / "c"), "--pfb", "4", "--integrate", "3", "--sk")
    assert seen == [("spectrum_db", c64, (64,)), ("integrated_db", c64, (64 * 9,)), ("pfb_db", c64, (64 * 9,)),
                    ("pfb_integrated_db", c64, (64 * 9,)), ("pfb_spectral_kurtosis", c64, (64 * 9,))]
    run(str(tmp_path / "c"), "--integrate", "3", "--sk")
    assert seen == [("spectrum_db", c64, (64,)), ("integrated_db", c64, (64 * 9,)), ("spectral_kurtosis", c64, (64 * 9,))]

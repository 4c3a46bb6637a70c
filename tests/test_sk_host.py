"""The spectral-kurtosis entry points without a GPU: header and ctypes table agree on the twelve symbols, the argument refusals
through ctypes, the Python argument checks, sk_limits, and the reference estimator itself on Gaussian noise (numpy)."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("sk", "sk_ci16", "pfb_sk", "pfb_sk_ci16")
TWELVE = sorted(f"sdrk_exec_{kind.format(m)}" for m in MODES for kind in ("device_{}", "device_{}_timed_each", "host_{}"))


def test_header_and_ctypes_table_agree_on_the_twelve_symbols():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sdrk.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if re.search(r"_sk(_|$)", n))
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == TWELVE == sorted(n for n in table if re.search(r"_sk(_|$)", n))
    for n in TWELVE:                                  # the argument lists of the header: no detector, then what each kind adds
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
        assert not any("detector" in p for p in params), n
    assert "#define SDRK_VERSION 500" in open(os.path.join(REPO, "include", "sdrk.h")).read()
    assert _ffi.DETECTORS == {"mean": 0, "max": 1, "min": 2}          # "sk" is not a detector
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in TWELVE)
    for n in ("spectral_kurtosis", "spectral_kurtosis_ci16", "pfb_spectral_kurtosis", "sk_limits"):
        assert getattr(pkg, n) is getattr(spectrum, n) and n in pkg.__all__


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    for m in MODES:
        def dev(g, k, stride, form):
            return getattr(lib, f"sdrk_exec_device_{m}")(None, p, g, k, stride, form, 1.0, p, None)

        def host(g, k, stride, form):
            return getattr(lib, f"sdrk_exec_host_{m}")(None, p, g, k, stride, form, 1.0, p)

        def timed(g, k, stride, form):
            return getattr(lib, f"sdrk_exec_device_{m}_timed_each")(None, p, g, k, stride, form, 1.0, p, 2, each)

        for call in (dev, host, timed):
            if m.startswith("pfb"):                   # the filter-bank forms look at the plan first
                assert call(1, 2, 64, 0) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
                continue
            assert call(1, 2, 64, 2) == _ffi.SDRK_ERR_INVALID and b"out_form 2" in lib.sdrk_last_error()
            assert call(0, 2, 64, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(1, 0, 64, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(1 << 40, 1 << 40, 64, 0) == _ffi.SDRK_ERR_INVALID and b"out of range" in lib.sdrk_last_error()
            assert call(1, 2, 0, 0) == _ffi.SDRK_ERR_INVALID and b"frame_stride" in lib.sdrk_last_error()
            assert call(1, 2, 64, 0) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
        if not m.startswith("pfb"):
            fn = getattr(lib, f"sdrk_exec_device_{m}_timed_each")
            assert fn(None, p, 1, 2, 64, 0, 1.0, p, 0, each) == _ffi.SDRK_ERR_INVALID and b"launches" in lib.sdrk_last_error()
    # detector 3 stays refused by the existing call, with its present message
    assert lib.sdrk_exec_device_integrated(None, p, 1, 1, 64, 3, 0, 1.0, p, None) == _ffi.SDRK_ERR_INVALID
    assert b"detector 3 is none of SDRK_DET_MEAN / _MAX / _MIN" in lib.sdrk_last_error()
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.spectral_kurtosis(np.zeros(8192, np.complex64), 4096, 2)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


class _Plan(SpectrumPlan):
    """The arithmetic of SpectrumPlan.spectral_kurtosis without a library handle behind it."""

    def __init__(self, nfft):     # (SpectrumPlan.__init__ needs a device)
        self.nfft, self._double, self._handle, self._lock, self._wkey = nfft, False, None, threading.Lock(), "rect"
        self.pfb_taps = 0


def test_python_argument_checks_and_shapes():
    p = _Plan(64)
    mean_rows, sk_rows = p.spectral_kurtosis(np.zeros(64 * 2, np.complex64), 3)      # no full group: nothing to run
    assert mean_rows.shape == sk_rows.shape == (0, 64) and mean_rows.dtype == sk_rows.dtype == np.float32
    assert mean_rows.base is sk_rows.base
    x, x16 = np.zeros(64 * 4, np.complex64), np.zeros((64 * 4, 2), np.int16)
    for bad in (dict(k=1), dict(k=0), dict(k=2, hop=0), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            p.spectral_kurtosis(x, **bad)
        with pytest.raises(ValueError):
            p.spectral_kurtosis_ci16(x16, **bad)
    with pytest.raises(TypeError):
        p.spectral_kurtosis(x, 2, detector="sk")                                     # not a detector, not an argument
    with pytest.raises(ValueError, match="detector"):
        p.integrate(x, 2, detector="sk")
    with pytest.raises(ValueError, match="int16"):
        p.spectral_kurtosis_ci16(x, 2)
    with pytest.raises(ValueError, match="prototype"):
        p.pfb_spectral_kurtosis(x, 2)
    with pytest.raises(ValueError, match="prototype"):
        p.pfb_spectral_kurtosis_ci16(x16, 2)
    for entry in ("exec_device_sk", "exec_device_sk_ci16"):
        for bad in (dict(n_groups=1, k=1), dict(n_groups=0, k=2), dict(n_groups=1, k=2, frame_stride=0), dict(n_groups=1, k=2, out="x")):
            with pytest.raises(ValueError):
                getattr(p, entry)(8, d_out=8, **bad)
    with pytest.raises(ValueError, match="prototype"):
        p.exec_device_pfb_sk(8, 1, 2, 8)
    p._double = True
    with pytest.raises(ValueError, match="double"):
        p.spectral_kurtosis(x, 2)
    with pytest.raises(ValueError, match="double"):
        p.exec_device_sk_timed_each(8, 1, 2, 8)
    # the module functions check before a plan is made for a prototype
    for bad in (dict(k=1), dict(k=2, hop=0), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            spectrum.pfb_spectral_kurtosis(x, 64, 2, **bad)


def test_cli_sk_needs_an_integration_of_at_least_two_frames(capsys):
    for argv in (["psd", "x.sigmf-meta", "--sk"], ["psd", "x.sigmf-meta", "--integrate", "1", "--sk"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert "K >= 2" in capsys.readouterr().err


def test_sk_limits_is_the_formula():
    for k in (2, 3, 16, 256, 4096):
        sd = np.sqrt(4.0 * k * k / ((k - 1.0) * (k + 2.0) * (k + 3.0)))
        for sigmas in (3.0, 1.0, 4.5):
            lo, hi = pkg.sk_limits(k, sigmas)
            assert lo == pytest.approx(1 - sigmas * sd, rel=1e-14) and hi == pytest.approx(1 + sigmas * sd, rel=1e-14)
    assert pkg.sk_limits(64) == pkg.sk_limits(64, 3.0)
    for bad in (1, 0, -2):
        with pytest.raises(ValueError):
            pkg.sk_limits(bad)


def test_the_reference_estimator_on_gaussian_noise():
    """What the GPU tests compare with, on the case its theory is stated for: K = 256, 4096 bins x 16 groups of complex Gaussian
    noise.  The mean is within 0.01 of 1 and the variance within 10 % of 4K^2/((K-1)(K+2)(K+3))."""
    k, n, groups = 256, 4096, 16
    rng = np.random.default_rng(256)
    x = (rng.standard_normal((groups, k, n)) + 1j * rng.standard_normal((groups, k, n))) / np.sqrt(2)
    p = np.abs(np.fft.fft(x, axis=-1)) ** 2
    s1, s2 = p.sum(axis=1), (p * p).sum(axis=1)
    sk = (k + 1.0) / (k - 1.0) * (k * s2 / s1 ** 2 - 1.0)
    var = 4.0 * k * k / ((k - 1.0) * (k + 2.0) * (k + 3.0))
    print(f"SK of Gaussian noise: mean {sk.mean():.4f}, variance {sk.var():.4f} (theory {var:.4f})")
    assert abs(sk.mean() - 1.0) <= 0.01
    assert abs(sk.var() - var) <= 0.1 * var
    lo, hi = pkg.sk_limits(k)
    assert np.mean((sk < lo) | (sk > hi)) < 0.02                 # (3 sigma: a fraction of a percent, the tail is skewed)

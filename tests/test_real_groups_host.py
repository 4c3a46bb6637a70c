"""CPU: the Python side of the integrated real-input spectra — what rintegrate / rintegrated_db / rwelch_psd and the
device-pointer form refuse before any library call, group counting, the one-sided doubling of rwelch_psd against a float64
numpy reference (the plan call replaced by a numpy stand-in), the agreement of header, _ffi and library on the new entries, and
numpy's own float32 rfft on the inputs of the GPU amplitude-bound cases.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.real_groups_helpers import (K4096_HOP, bound_stream, frames_of, k4096_stream, kahan_mean32, numpy_rintegrate, ref_power,
                                       window64)

NEW = ("sdrk_exec_device_real_integrated", "sdrk_exec_device_real_integrated_timed_each", "sdrk_exec_host_real_integrated")


def bare_plan(nfft):
    """A SpectrumPlan that never met the library: enough for the argument handling in front of a call."""
    p = object.__new__(SpectrumPlan)
    p.nfft, p._double = nfft, False
    return p


def test_the_package_exports_the_two_functions():
    for name in ("rintegrated_db", "rwelch_psd"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def test_header_ffi_and_library_agree_on_the_new_entries():
    header = open(os.path.join(os.path.dirname(_ffi.library_path()), "..", "..", "include", "sdrk.h")).read()
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    for name in NEW:
        proto = re.search(rf"int {name}\(([^;]*)\);", header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(table[name]), name
    assert len(table[NEW[0]]) == 11 and len(table[NEW[1]]) == 12 and len(table[NEW[2]]) == 10
    assert "SDRK_VERSION 500" in header.replace("  ", " ") or _ffi.ABI_VERSION == 500
    assert "Not provided: filter-bank / kurtosis / cross forms" in header
    if os.path.exists(_ffi.library_path()):
        for name in NEW:
            assert hasattr(_ffi.lib(), name)


@pytest.mark.parametrize("bad", [
    np.zeros(4096, np.float64),                 # not silently narrowed
    np.zeros(4096, np.complex64),
    np.zeros(4096, np.int32),
    np.zeros((4, 1024), np.float32),            # a stream is flat
    np.zeros(8192, np.float32)[::2],            # not contiguous
    [0.0] * 4096,                               # not an array
])
def test_streams_refused_before_any_library_call(bad, monkeypatch):
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "SpectrumPlan", lambda *a, **k: pytest.fail("a plan was made"))
    with pytest.raises(ValueError):
        pkg.rintegrated_db(bad, 64, 2)
    with pytest.raises(ValueError):
        pkg.rwelch_psd(bad, 64, 1000.0)
    with pytest.raises(ValueError):
        bare_plan(32).rintegrate(bad, 2)


@pytest.mark.parametrize("hop", [0, 1, 33, -2])
def test_hops_and_counts_refused_before_any_library_call(hop, monkeypatch):
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "SpectrumPlan", lambda *a, **k: pytest.fail("a plan was made"))
    x = np.zeros(4096, np.int16)
    for call in (lambda: pkg.rintegrated_db(x, 64, 2, hop=hop), lambda: pkg.rwelch_psd(x, 64, 1000.0, hop=hop),
                 lambda: bare_plan(32).rintegrate(x, 2, hop=hop), lambda: bare_plan(32).rintegrated_groups(4096, 2, hop),
                 lambda: bare_plan(32).exec_device_real_integrated(8, 1, 2, 8, fmt="s16", frame_stride=hop)):
        with pytest.raises(ValueError):
            call()


def test_the_other_arguments_refused_before_any_library_call(monkeypatch):
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "lib", lambda: pytest.fail("the library was called"))
    x, p = np.zeros(4096, np.uint8), bare_plan(32)
    for call in (lambda: p.rintegrate(x, 0), lambda: p.rintegrate(x, 2, detector="median"), lambda: p.rintegrate(x, 2, out="complex"),
                 lambda: p.rintegrate(x[:100], 2),                                    # fewer samples than one group
                 lambda: p.exec_device_real_integrated(8, 1, 2, 8, fmt="f64"),
                 lambda: p.exec_device_real_integrated(8, 0, 2, 8, fmt="f32"),
                 lambda: p.exec_device_real_integrated(8, 1, 0, 8, fmt="f32"),
                 lambda: p.exec_device_real_integrated_timed_each(8, 1, 2, 8, fmt="f32", detector="peak"),
                 lambda: pkg.rintegrated_db(x, 64, 0), lambda: pkg.rintegrated_db(x, 48, 2), lambda: pkg.rwelch_psd(x, 16, 1.0)):
        with pytest.raises(ValueError):
            call()
    p._double = True
    with pytest.raises(ValueError):
        p.rintegrate(x, 2)


def test_group_counting():
    p = bare_plan(32)                                   # real frames of 64
    assert p.rintegrated_groups(64, 1) == 1 and p.rintegrated_groups(63, 1) == 0
    assert p.rintegrated_groups(64 * 7, 2) == 3         # the seventh frame fills no group
    assert p.rintegrated_groups(64 + 5 * 32, 3, hop=32) == 2 and p.rintegrated_groups(64 + 5 * 32 - 1, 3, hop=32) == 1
    assert p.rintegrated_groups(64 + 4 * 70, 5, hop=70) == 1
    with pytest.raises(ValueError):
        p.rintegrated_groups(640, 0)


@pytest.mark.parametrize("window", ["hann", None])
def test_rwelch_psd_doubles_the_interior_bins(window, monkeypatch):
    n, fs, hop = 64, 8000.0, 32
    monkeypatch.setattr(spectrum, "_cached_real_plan", lambda nfft_real, w, eps, device: bare_plan(nfft_real // 2))
    monkeypatch.setattr(SpectrumPlan, "rintegrate", numpy_rintegrate(n // 2, window))
    x = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    got = pkg.rwelch_psd(x, n, fs, hop=hop, window=window)
    frames = 1 + (1000 - n) // hop
    w = window64(window, n)
    spec = np.fft.rfft(frames_of(x.astype(np.float64), n, frames, hop) * w, axis=-1)
    ref = (np.abs(spec) ** 2).mean(axis=0) / (fs * np.sum(w ** 2))
    ref[1:-1] *= 2.0                                    # one-sided: every bin but 0 and fs/2 stands for two
    assert got.shape == (n // 2 + 1,) and got.dtype == np.float32
    assert np.allclose(got, ref, rtol=1e-6, atol=0)
    # Parseval: the one-sided PSD integrates to the windowed mean power
    power = np.mean((frames_of(x.astype(np.float64), n, frames, hop) * w) ** 2) * n / np.sum(w ** 2)
    assert abs(np.sum(got.astype(np.float64)) * fs / n - power) <= 1e-5 * power


def test_the_replayed_mean_is_the_mean():
    p = np.random.default_rng(5).random((12, 33)).astype(np.float32) + 1
    got = kahan_mean32(p, 3, 4)
    assert got.dtype == np.float32 and np.abs(got - p.astype(np.float64).reshape(3, 4, -1).mean(axis=1)).max() < 3e-7
    assert np.array_equal(kahan_mean32(p, 12, 1), p)    # K = 1: the powers themselves


@pytest.mark.parametrize("n", [16, 256, 4096, 8192])
def test_numpys_float32_rfft_of_the_bound_inputs_stays_within_the_bound(n):
    """The inputs of test_real_groups_gpu.py's amplitude-bound cases are ones on which a float32 transform can hold 1e-5 of
    the peak: numpy's own (pocketfft in single precision) does, with a wide margin."""
    x = bound_stream(n, 100 if n <= 4096 else 12, seed=n)
    for window in (None, "hann"):
        z = np.fft.rfft(x * window64(window, 2 * n).astype(np.float32), axis=-1)
        assert z.dtype == np.complex64
        p = ref_power(x, window)
        err = (np.abs(np.abs(z) - np.sqrt(p)).max(axis=1) / np.sqrt(p.max(axis=1))).max()
        assert err <= 2e-6, (n, window, err)


def test_numpys_float32_rfft_of_the_k_4096_input_stays_within_the_bound():
    x = k4096_stream()
    f = frames_of(x, 8192, 64, K4096_HOP * 64)          # every 64th of the 4096 frames
    z = np.fft.rfft(f * np.hanning(8192).astype(np.float32), axis=-1)
    p = ref_power(f, "hann")
    assert (np.abs(np.abs(z) - np.sqrt(p)).max(axis=1) / np.sqrt(p.max(axis=1))).max() <= 2e-6
    assert p.max(axis=1).max() / p.max(axis=1).min() < 1.001    # nearly equal powers, frame after frame

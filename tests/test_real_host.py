"""CPU: the Python side of the real-input spectra — what the argument handling accepts and refuses before any library call,
rfreq_axis, the SigMF round trips of the four real datatypes, read_sigmf still refusing them, and the refusals of cli psd on a
real-sampled recording.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum

REAL = (("rf32_le", np.float32), ("ri16_le", np.int16), ("ri8", np.int8), ("ru8", np.uint8))


def test_the_package_exports_the_three_functions():
    for name in ("rspectrum_db", "rfft", "rfreq_axis"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def test_the_dtype_is_the_format():
    for (_, dt), code in zip(REAL, (_ffi.REAL_F32, _ffi.REAL_S16, _ffi.REAL_S8, _ffi.REAL_U8)):
        assert spectrum._real_format(spectrum._as_real(np.zeros((2, 64), dt), 64)) == code
    assert (_ffi.REAL_F32, _ffi.REAL_S16, _ffi.REAL_S8, _ffi.REAL_U8) == (0, 1, 2, 3)
    header = open(os.path.join(os.path.dirname(_ffi.library_path()), "..", "..", "include", "sdrk.h")).read()
    assert "SDRK_REAL_F32 = 0, SDRK_REAL_S16 = 1, SDRK_REAL_S8 = 2, SDRK_REAL_U8 = 3" in header
    assert "SDRK_REAL_OUT_DB = 0, SDRK_REAL_OUT_COMPLEX = 1" in header


@pytest.mark.parametrize("bad", [
    np.zeros((2, 64), np.float64),              # not silently narrowed
    np.zeros((2, 64), np.complex64),
    np.zeros((2, 64), np.int32),
    np.zeros((2, 63), np.float32),              # another frame length
    np.zeros((2, 2, 64), np.float32),
    np.zeros(100, np.float32),                  # flat, not whole frames
    np.zeros(0, np.float32),
    np.zeros((4, 128), np.float32)[:, ::2],     # not contiguous
    [0.0] * 64,                                 # not an array
])
def test_frames_refused_before_any_library_call(bad, monkeypatch):
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(spectrum, "lib", lambda: pytest.fail("the library was called"))
    with pytest.raises(ValueError):
        spectrum._as_real(bad, 64)
    for fn in (pkg.rspectrum_db, pkg.rfft):
        with pytest.raises(ValueError):
            fn(bad, 64)


def test_accepted_shapes():
    assert spectrum._as_real(np.zeros((3, 64), np.int8), 64).shape == (3, 64)
    assert spectrum._as_real(np.zeros(192, np.uint8), 64).shape == (192,)
    assert spectrum._as_real(np.zeros(1000, np.int16), 64, stream=True).shape == (1000,)
    with pytest.raises(ValueError):
        spectrum._as_real(np.zeros((3, 64), np.int16), 64, stream=True)


def test_frame_lengths_and_windows_refused_before_a_plan_is_made(monkeypatch):
    monkeypatch.setattr(spectrum, "SpectrumPlan", lambda *a, **k: pytest.fail("a plan was made"))
    x = np.zeros((1, 48), np.float32)
    with pytest.raises(ValueError, match="powers of two"):
        pkg.rfft(x, 48)
    with pytest.raises(ValueError, match="powers of two"):
        pkg.rspectrum_db(np.zeros((1, 16), np.float32), 16)
    with pytest.raises(ValueError, match="window must have shape"):
        pkg.rfft(np.zeros((1, 64), np.float32), 64, window=np.ones(32, np.float32))
    with pytest.raises(ValueError, match="unknown window"):
        pkg.rfft(np.zeros((1, 64), np.float32), 64, window="kaiser")
    w = spectrum._real_window("hann", 64)
    assert w.dtype == np.float32 and np.array_equal(w, np.hanning(64).astype(np.float32))
    assert spectrum._real_window(None, 64) is None and spectrum._real_window("rect", 64) is None


def test_rfreq_axis():
    for n, fs, fc in ((8192, 2.4e6, 0.0), (32, 48000.0, 1e6), (2, 1.0, 0.0)):
        ax = pkg.rfreq_axis(n, fs, fc)
        assert ax.dtype == np.float64 and ax.shape == (n // 2 + 1,)
        assert np.array_equal(ax, np.fft.rfftfreq(n, 1 / fs) + fc)
        assert ax[0] == fc and abs(ax[-1] - (fc + fs / 2)) <= 1e-9 * (fc + fs)
    for bad in (0, 7, -4):
        with pytest.raises(ValueError):
            pkg.rfreq_axis(bad, 1.0)


@pytest.mark.parametrize("datatype,dtype", REAL)
def test_sigmf_round_trip(tmp_path, datatype, dtype):
    rng = np.random.default_rng(4)
    x = rng.standard_normal(1000).astype(dtype) if dtype == np.float32 else \
        rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1, size=1000).astype(dtype)
    base = str(tmp_path / "rec")
    data, meta_path = sigmf_io.write_sigmf(base, x, 48000, 7_100_000, datatype=datatype)
    assert os.path.getsize(data) == x.nbytes
    assert json.load(open(meta_path))["global"]["core:datatype"] == datatype
    y, meta = sigmf_io.read_sigmf_real(base)
    assert y.dtype == dtype and y.shape == x.shape and np.array_equal(y.view(np.uint8), x.view(np.uint8))
    assert meta["sample_rate"] == 48000.0 and meta["center_freq"] == 7_100_000.0
    assert sigmf_io.read_sigmf_real(meta_path, max_samples=10)[0].shape == (10,)
    assert sigmf_io.sigmf_datatype(data) == datatype
    with pytest.raises(ValueError):                       # read_sigmf returns complex samples: a real datatype is refused
        sigmf_io.read_sigmf(base)
    with pytest.raises(ValueError):                       # the array's dtype must be the datatype's
        sigmf_io.write_sigmf(base + "x", x.astype(np.float64), 48000, 0, datatype=datatype)
    with pytest.raises(ValueError):
        sigmf_io.write_sigmf(base + "x", x.reshape(-1, 2), 48000, 0, datatype=datatype)


def test_read_sigmf_real_refuses_complex_recordings(tmp_path):
    base = str(tmp_path / "c")
    sigmf_io.write_sigmf(base, np.zeros(16, np.complex64), 1e6, 0)
    with pytest.raises(ValueError, match="read_sigmf_real reads"):
        sigmf_io.read_sigmf_real(base)


@pytest.mark.parametrize("flags", [["--pfb", "4"], ["--integrate", "4"], ["--integrate", "4", "--sk"],
                                   ["--integrate", "4", "--cross"], ["--integrate", "4", "--correlate"]])
def test_cli_psd_refuses_the_other_forms_on_a_real_recording(tmp_path, capsys, monkeypatch, flags):
    monkeypatch.setattr(spectrum, "rspectrum_db", lambda *a, **k: pytest.fail("computed"))
    base = str(tmp_path / "r")
    sigmf_io.write_sigmf(base, np.zeros(20000, np.int16), 48000, 0, datatype="ri16_le")
    assert cli.main(["psd", base, *flags]) == 2
    err = capsys.readouterr().err
    assert "real-sampled recording" in err and flags[-1 if flags[-1].startswith("--") else 0] in err


def test_cli_psd_refuses_a_bad_real_frame_length_and_a_short_recording(tmp_path, capsys):
    base = str(tmp_path / "r")
    sigmf_io.write_sigmf(base, np.zeros(100, np.uint8), 48000, 0, datatype="ru8")
    assert cli.main(["psd", base, "--nfft", "4097"]) == 2
    assert "real frame length" in capsys.readouterr().err
    assert cli.main(["psd", base]) == 2
    assert "need 8192" in capsys.readouterr().err

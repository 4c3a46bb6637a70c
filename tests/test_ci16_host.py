"""CPU: the host-side pieces of the int16 I,Q input path — argument validation that never reaches a device, the SigMF ci16_le
round trip, the generator's int16 form, the ABI table, and the loud failure without a GPU."""
import json

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, sigmf_io, synth
from sdr_iq_visualizer_amd import spectrum as sp


def _frames(b=3, n=256):
    return np.random.default_rng(b * n).integers(-2048, 2048, size=(b, n, 2), dtype=np.int64).astype(np.int16)


def test_wrong_dtype_or_shape_is_refused_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_ffi, "require_device", no_device)
    monkeypatch.setattr(_ffi, "lib", no_device)
    monkeypatch.setattr(sp, "lib", no_device)
    x = _frames()
    wide = (x[..., 0] + 1j * x[..., 1]).astype(np.complex64)
    bad = [wide,                                   # complex64: that is spectrum_db's input
           x.astype(np.int32), x.astype(np.float32), x.astype(np.int8),
           x[..., 0],                              # no (I, Q) axis
           x.reshape(3, 2, 256),                   # planar, not interleaved
           x[:, ::2],                              # not C-contiguous
           x[..., ::-1],                           # a reversed view: not interleaved I, Q in memory
           np.zeros((2, 2, 256, 2), np.int16),     # too many axes
           np.zeros((256,), np.int16),
           x.tolist()]                             # not an array: nothing is converted
    for a in bad:
        for fn in (pkg.spectrum_db_ci16, pkg.fft_ci16):
            with pytest.raises(ValueError, match="ci16"):
                fn(a)
    for a in (wide.reshape(-1), x, x.reshape(-1, 2).astype(np.int32), x.reshape(-1, 2)[::2], x.reshape(-1)):
        with pytest.raises(ValueError, match="ci16"):
            pkg.stft_db_ci16(a, 256)
    # spectrum_db itself keeps treating integers as numpy's FFT does: double
    assert sp.resolve_precision("auto", x) == "double"


def test_exports_and_abi_table():
    from sdr_iq_visualizer_amd import processing
    for name in ("spectrum_db_ci16", "fft_ci16", "stft_db_ci16"):
        assert getattr(pkg, name) is getattr(sp, name) is getattr(processing, name)
        assert name in pkg.__all__ and name in processing.__all__
    for m in ("spectrum_db_ci16", "fft_ci16", "stft_db_ci16", "exec_device_ci16", "exec_device_ci16_timed_each",
              "exec_device_ci16_timed"):
        assert callable(getattr(sp.SpectrumPlan, m))
    table = {name for name, _, _ in _ffi.SYMBOLS}
    assert {"sdrk_exec_host_ci16", "sdrk_exec_fft_host_ci16", "sdrk_exec_device_ci16", "sdrk_exec_device_ci16_timed_each",
            "sdrk_synth_fill_ci16"} <= table
    lib = _ffi.lib()                                 # every one of them is exported by the built library
    assert lib.sdrk_version() == 500
    assert lib.sdrk_exec_host_ci16(None, None, 1, 1, None) == _ffi.SDRK_ERR_INVALID and b"plan is NULL" in lib.sdrk_last_error()
    assert lib.sdrk_synth_fill_ci16(0, 1, 0, 0, 4096, None, None) == _ffi.SDRK_OK      # nothing to fill


def test_no_gpu_means_an_error_not_a_host_computation():
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    x = _frames()
    with pytest.raises(pkg.SdrkError):
        pkg.spectrum_db_ci16(x)
    with pytest.raises(pkg.SdrkError):
        pkg.fft_ci16(x[0])
    with pytest.raises(pkg.SdrkError):
        pkg.stft_db_ci16(x.reshape(-1, 2), 256, 128)


@pytest.mark.parametrize("seed,first,n_frames,n", [(1234, 0, 8, 4096), (7, (1 << 32) - 2, 5, 64), (0, 1 << 40, 2, 1000)])
def test_synth_int16_form_equals_the_float_form_cast(seed, first, n_frames, n):
    c = synth.synth_iq(seed, first, n_frames, n)
    x = synth.synth_iq_ci16(seed, first, n_frames, n)
    assert x.dtype == np.int16 and x.shape == (n_frames, n, 2) and x.flags.c_contiguous
    assert np.array_equal(x[..., 0], c.real.astype(np.int16)) and np.array_equal(x[..., 1], c.imag.astype(np.int16))
    assert x.min() >= -2048 and x.max() <= 2047
    wide = (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)
    assert np.array_equal(wide.view(np.uint32), c.view(np.uint32))          # widening back: the float form's bits


def test_sigmf_ci16_round_trip_and_unchanged_defaults(tmp_path):
    x = synth.synth_iq_ci16(5, 0, 3, 512).reshape(-1, 2)
    x[0] = (-32768, 32767)
    base = str(tmp_path / "rec16")
    data_path, meta_path = sigmf_io.write_sigmf(base, x, 1_000_000, 2_400_000_000, datatype="ci16_le")
    assert open(data_path, "rb").read() == x.astype("<i2").tobytes()
    assert json.load(open(meta_path))["global"]["core:datatype"] == "ci16_le"
    raw, meta = sigmf_io.read_sigmf(base, native=True)
    assert raw.dtype == np.int16 and raw.shape == x.shape and np.array_equal(raw, x)
    assert meta["sample_rate"] == 1e6 and meta["center_freq"] == 2.4e9
    sp._as_ci16(raw, stream=True)                                    # what stft_db_ci16 takes, as it is
    sp._as_ci16(np.ascontiguousarray(raw[:1024]).reshape(2, 512, 2), 512)
    # the default reader still widens
    wide, _ = sigmf_io.read_sigmf(base)
    assert wide.dtype == np.complex64 and np.array_equal(wide, (x[:, 0] + 1j * x[:, 1]).astype(np.complex64))
    part, _ = sigmf_io.read_sigmf(meta_path, max_samples=100, native=True)
    assert np.array_equal(part, x[:100])
    # integer-valued complex samples are accepted for writing, anything lossy is not
    sigmf_io.write_sigmf(base + "b", wide, 1e6, 0, datatype="ci16_le")
    assert np.array_equal(sigmf_io.read_sigmf(base + "b", native=True)[0], x)
    with pytest.raises(ValueError):
        sigmf_io.write_sigmf(base + "c", wide * 0.5 + 0.25, 1e6, 0, datatype="ci16_le")
    with pytest.raises(ValueError):
        sigmf_io.write_sigmf(base + "c", wide * 4, 1e6, 0, datatype="ci16_le")
    with pytest.raises(ValueError):
        sigmf_io.write_sigmf(base + "c", wide, 1e6, 0, datatype="ci8")
    # cf32_le: writer and reader as before, with or without native=True
    c = synth.synth_iq(9, 0, 2, 256).reshape(-1)
    d32, m32 = sigmf_io.write_sigmf(str(tmp_path / "rec32"), c, 1e6, 1e9)
    assert open(d32, "rb").read() == c.tobytes() and json.load(open(m32))["global"]["core:datatype"] == "cf32_le"
    for native in (False, True):
        got, _ = sigmf_io.read_sigmf(str(tmp_path / "rec32"), native=native)
        assert got.dtype == np.complex64 and np.array_equal(got, c)
    assert sigmf_io.make_metadata(1e6, 1e9)["global"]["core:datatype"] == "cf32_le"

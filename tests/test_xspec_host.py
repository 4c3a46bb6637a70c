"""The two-channel cross-spectrum entry points without a GPU: header and ctypes table agree on the six symbols, the argument
refusals through ctypes, the Python layer's argument checks and input stacking, CrossSpectrum's derived quantities on hand-made
planes, the multi-channel SigMF round trip, and the command line's refusal."""
import ctypes
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import CrossSpectrum
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = sorted(f"sdrk_exec_{kind.format(m)}" for m in ("xspec", "xspec_ci16") for kind in ("device_{}", "device_{}_timed_each", "host_{}"))


def test_header_and_ctypes_table_agree_on_the_six_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "_xspec" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == SIX == sorted(n for n in table if "_xspec" in n)
    for n in SIX:                                     # no detector, no out_form: plan, input, three counts, scale, output, ...
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
        assert not any("detector" in p or "out_form" in p for p in params), n
    assert "#define SDRK_VERSION 500" in text
    for word in ("filter-bank forms", "double precision", "more than two channels", "waterfall appends"):
        assert word in text.split("two-channel cross-spectra")[1].split("measurement probes")[0], word   # said not to be provided
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in SIX)
    assert pkg.cross_spectrum is spectrum.cross_spectrum and pkg.CrossSpectrum is CrossSpectrum
    assert "cross_spectrum" in pkg.__all__ and "CrossSpectrum" in pkg.__all__


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    for m in ("xspec", "xspec_ci16"):
        def dev(g, k, stride):
            return getattr(lib, f"sdrk_exec_device_{m}")(None, p, g, k, stride, 1.0, p, None)

        def host(g, k, stride):
            return getattr(lib, f"sdrk_exec_host_{m}")(None, p, g, k, stride, 1.0, p)

        def timed(g, k, stride):
            return getattr(lib, f"sdrk_exec_device_{m}_timed_each")(None, p, g, k, stride, 1.0, p, 2, each)

        for call in (dev, host, timed):
            assert call(0, 2, 64) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(1, 0, 64) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(1 << 40, 1 << 40, 64) == _ffi.SDRK_ERR_INVALID and b"out of range" in lib.sdrk_last_error()
            assert call(1, 2, 0) == _ffi.SDRK_ERR_INVALID and b"frame_stride" in lib.sdrk_last_error()
            assert call(1, 1, 64) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"   # (K = 1 itself is fine)
        fn = getattr(lib, f"sdrk_exec_device_{m}_timed_each")
        assert fn(None, p, 1, 2, 64, 1.0, p, 0, each) == _ffi.SDRK_ERR_INVALID and b"launches" in lib.sdrk_last_error()


def test_python_argument_checks_and_input_stacking():
    plan = bare_plan(64)
    rng = np.random.default_rng(0)
    a, b = (rng.standard_normal(200) + 1j * rng.standard_normal(200) for _ in range(2))
    stacked = spectrum._as_iq2_c64((a, b))
    assert stacked.shape == (200, 2) and stacked.dtype == np.complex64 and stacked.flags.c_contiguous
    assert np.array_equal(stacked[:, 0], a.astype(np.complex64)) and np.array_equal(stacked[:, 1], b.astype(np.complex64))
    assert spectrum._as_iq2_c64(stacked) is stacked                             # what is ready goes in as it is
    assert "copy" in spectrum.SpectrumPlan.cross_spectrum.__doc__ and "copy" in spectrum.SpectrumPlan.cross_spectrum_ci16.__doc__
    for bad in (a, np.zeros((10, 3), np.complex64), np.zeros((10, 2), np.float32), (a, b[:-1]), (stacked, stacked)):
        with pytest.raises(ValueError):
            spectrum._as_iq2_c64(bad)
    i16 = rng.integers(-2048, 2048, size=(200, 2, 2)).astype(np.int16)
    assert spectrum._as_iq2_ci16(i16) is i16 and spectrum._as_iq2_ci16(i16.reshape(200, 4)).shape == (200, 4)
    pair = spectrum._as_iq2_ci16((i16[:, 0], i16[:, 1]))
    assert pair.shape == (200, 2, 2) and np.array_equal(pair, i16)
    for bad in (i16.astype(np.int32), i16.reshape(400, 2), i16[:, :, ::-1], i16[::2].reshape(100, 4)[:, ::-1], (i16[:, 0], i16[:5, 1])):
        with pytest.raises(ValueError):
            spectrum._as_iq2_ci16(bad)
    # fewer elements than a group needs: four empty views, before any device call
    for res in (plan.cross_spectrum(stacked[:100], 2), plan.cross_spectrum_ci16(i16[:127], 2), plan.cross_spectrum((a[:63], b[:63]), 1)):
        assert isinstance(res, CrossSpectrum) and all(v.shape == (0, 64) and v.dtype == np.float32 for v in res)
        assert res.coherence.shape == res.phase.shape == res.cross.shape == (0, 64)
    for k, hop in ((0, None), (2, 0), (-1, 64)):
        with pytest.raises(ValueError):
            plan.cross_spectrum(stacked, k, hop)
        with pytest.raises(ValueError):
            plan.cross_spectrum_ci16(i16, k, hop)
    for entry in ("exec_device_xspec", "exec_device_xspec_ci16", "exec_device_xspec_timed_each", "exec_device_xspec_ci16_timed_each"):
        for groups, k, stride in ((0, 2, None), (1, 0, None), (1, 2, 0)):
            with pytest.raises(ValueError):
                getattr(plan, entry)(0x1000, groups, k, 0x2000, frame_stride=stride)
    double = bare_plan(64, double=True)
    with pytest.raises(ValueError, match="double"):
        double.cross_spectrum(stacked, 2)
    with pytest.raises(ValueError, match="double"):
        double.exec_device_xspec(0x1000, 1, 2, 0x2000)
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.cross_spectrum(a.astype(np.complex64), b.astype(np.complex64), 64, 2)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


def test_coherence_and_phase_on_hand_made_planes():
    f = np.float32
    #                 one signal   quarter turn   half power common   dead bin   dead channel 1   denormal product
    paa = np.array([[4.0, 9.0, 2.0, 0.0, 5.0, 1e-30]], f)
    pbb = np.array([[1.0, 9.0, 2.0, 0.0, 0.0, 1e-30]], f)
    cre = np.array([[2.0, 0.0, 1.0, 0.0, 0.0, 0.0]], f)
    cim = np.array([[0.0, -9.0, 1.0, 0.0, 0.0, 1e-30]], f)
    r = CrossSpectrum(paa, pbb, cre, cim)
    coh, phase = r.coherence, r.phase
    assert coh.dtype == np.float64 and phase.dtype == np.float64 and np.all(np.isfinite(coh)) and np.all(np.isfinite(phase))
    assert np.allclose(coh[0, :3], [1.0, 1.0, 0.5], rtol=1e-12) and np.array_equal(coh[0, 3:5], [0.0, 0.0])
    assert abs(coh[0, 5] - 1.0) < 1e-6                               # the quotient is formed in float64: no underflow to 0/0
    assert np.allclose(phase[0, :3], [0.0, -np.pi / 2, np.pi / 4]) and phase[0, 3] == 0.0
    assert r.cross.dtype == np.complex64 and np.array_equal(r.cross, cre + 1j * cim)
    inf = CrossSpectrum(np.array([[np.inf]], f), np.array([[1.0]], f), np.array([[np.inf]], f), np.array([[0.0]], f))
    assert np.array_equal(inf.coherence, [[0.0]])                    # never NaN


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_sigmf_two_channel_round_trip(tmp_path, datatype):
    rng = np.random.default_rng(3)
    i16 = rng.integers(-2048, 2048, size=(300, 2, 2)).astype(np.int16)
    x = i16 if datatype == "ci16_le" else i16.astype(np.float32).view(np.complex64).reshape(300, 2)
    base = str(tmp_path / "two")
    data_path, meta_path = sigmf_io.write_sigmf(base, x, 2e6, 1e9, datatype=datatype, num_channels=2)
    assert os.path.getsize(data_path) == 300 * (8 if datatype == "ci16_le" else 16)
    got, meta = sigmf_io.read_sigmf_channels(meta_path)
    assert got.dtype == x.dtype and np.array_equal(got, x)
    assert meta["num_channels"] == 2 and meta["global"]["core:num_channels"] == 2 and meta["sample_rate"] == 2e6
    flat, _ = sigmf_io.read_sigmf(meta_path, native=True)              # read_sigmf: the file as one stream, as before
    assert flat.shape[0] == 600
    with pytest.raises(ValueError):
        sigmf_io.write_sigmf(base, x[:, 0], 2e6, 1e9, datatype=datatype, num_channels=2)
    # one channel: the metadata has no channel count, and the channel reader gives (n, 1)
    sigmf_io.write_sigmf(base + "1", x[:, 0], 2e6, 1e9, datatype=datatype)
    one, meta1 = sigmf_io.read_sigmf_channels(base + "1")
    assert "core:num_channels" not in meta1["global"] and meta1["num_channels"] == 1
    assert one.shape[:2] == (300, 1) and np.array_equal(one[:, 0], x[:, 0])


def test_cli_refuses_cross_on_anything_but_a_two_channel_recording(tmp_path, capsys):
    base = str(tmp_path / "one")
    sigmf_io.write_sigmf(base, np.zeros(8192, np.complex64), 1e6, 1e9)
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", "2", "--cross"]) == 2
    assert "two-channel" in capsys.readouterr().err
    three = str(tmp_path / "three")
    sigmf_io.write_sigmf(three, np.zeros((8192, 3), np.complex64), 1e6, 1e9, num_channels=3)
    assert cli.main(["psd", three + ".sigmf-meta", "--integrate", "2", "--cross"]) == 2
    assert "core:num_channels = 3" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                   # --cross without --integrate K
        cli.main(["psd", base + ".sigmf-meta", "--cross"])

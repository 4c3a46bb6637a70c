"""The correlation-matrix entry points without a GPU: header and ctypes table agree on the nine symbols, the argument refusals
through ctypes, plane_index and CorrelationMatrix's Hermitian assembly and derived quantities on hand-made planes (the zero-
denominator rule of the coherence among them), the Python layer's shape and dtype refusals, the 8-bit multi-channel SigMF round
trip, and the command line's exit codes — with --cross left as it was on a three-channel file."""
import ctypes
import os
import re
import zipfile

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import CorrelationMatrix, CrossSpectrum, plane_index
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = sorted(f"sdrk_exec_{kind.format(m)}" for m in ("corrmat", "corrmat_ci16", "corrmat_iq8")
              for kind in ("device_{}", "device_{}_timed_each", "host_{}"))


def test_header_and_ctypes_table_agree_on_the_nine_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "_corrmat" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == NINE == sorted(n for n in table if "_corrmat" in n)
    for n in NINE:
        params = [p.strip() for p in re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")]
        assert len(params) == len(table[n]), n
        # channels right after the samples pointer; for the 8-bit form after the format
        assert params[2:4] == (["int iq8_format", "int channels"] if "_iq8" in n else ["int channels", "size_t n_groups"]), n
        assert not any("detector" in p or "out_form" in p for p in params), n
    assert "#define SDRK_VERSION 500" in text
    section = text.split("correlation matrix: 2..8 coherent channels")[1].split("FIR filtering and channel extraction")[0]
    for word in ("filter-bank front end", "double precision", "waterfall appends", "more than 8 channels", "direction-finding"):
        assert word in section.split("Not provided")[1], word
    assert "sdrk_exec_*_corrmat*" in text.split("two-channel cross-spectra")[1].split("correlation matrix: 2..8")[0]
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in NINE)
    assert pkg.correlation_matrix is spectrum.correlation_matrix and pkg.CorrelationMatrix is CorrelationMatrix
    assert "correlation_matrix" in pkg.__all__ and "CorrelationMatrix" in pkg.__all__


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    for m in ("corrmat", "corrmat_ci16", "corrmat_iq8"):
        fmt = (1,) if m == "corrmat_iq8" else ()

        def dev(c, g, k, stride):
            return getattr(lib, f"sdrk_exec_device_{m}")(None, p, *fmt, c, g, k, stride, 1.0, p, None)

        def host(c, g, k, stride):
            return getattr(lib, f"sdrk_exec_host_{m}")(None, p, *fmt, c, g, k, stride, 1.0, p)

        def timed(c, g, k, stride):
            return getattr(lib, f"sdrk_exec_device_{m}_timed_each")(None, p, *fmt, c, g, k, stride, 1.0, p, 2, each)

        for call in (dev, host, timed):
            for c in (1, 9, 0, -2, 1 << 20):
                assert call(c, 1, 2, 64) == _ffi.SDRK_ERR_INVALID and b"channels" in lib.sdrk_last_error(), (m, c)
            assert call(3, 0, 2, 64) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(3, 1, 0, 64) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
            assert call(3, 1 << 40, 1 << 40, 64) == _ffi.SDRK_ERR_INVALID and b"out of range" in lib.sdrk_last_error()
            assert call(3, 1, 2, 0) == _ffi.SDRK_ERR_INVALID and b"frame_stride" in lib.sdrk_last_error()
            for c in (2, 8):
                assert call(c, 1, 1, 64) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"   # (K = 1 is fine)
    for bad_fmt in (2, -1):
        assert lib.sdrk_exec_host_corrmat_iq8(None, p, bad_fmt, 3, 1, 2, 64, 1.0, p) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_last_error() != b"plan is NULL"


def test_plane_index_lists_the_autos_then_the_pairs_in_order():
    for C in range(2, 9):
        seen = [plane_index(C, c, c) for c in range(C)]
        assert seen == list(range(C))
        for i in range(C):
            for j in range(i + 1, C):
                q = plane_index(C, i, j)
                assert q == len(seen) and plane_index(C, j, i) == q
                seen += [q, q + 1]
        assert seen == list(range(C * C))
    assert [plane_index(2, 0, 0), plane_index(2, 1, 1), plane_index(2, 0, 1)] == [0, 1, 2]      # the two-channel layout
    assert plane_index(5, 3, 4) == 23 and plane_index(8, 6, 7) == 62
    for bad in ((1, 0, 0), (9, 0, 0), (3, 3, 0), (3, 0, -1)):
        with pytest.raises(ValueError):
            plane_index(*bad)


def test_matrix_is_the_hermitian_assembly_of_the_planes():
    C, groups, n = 3, 2, 4
    planes = np.arange(groups * C * C * n, dtype=np.float32).reshape(groups, C * C, n) + 1
    cm = CorrelationMatrix(planes, C)
    assert cm.channels == C and cm.planes is planes
    m = cm.matrix()
    assert m.shape == (groups, n, C, C) and m.dtype == np.complex64
    assert np.array_equal(m, np.conj(np.swapaxes(m, 2, 3)))                                     # Hermitian
    for c in range(C):
        assert np.array_equal(m[:, :, c, c], planes[:, c].astype(np.complex64)) and np.shares_memory(cm.auto(c), planes)
    for (i, j), q in (((0, 1), 3), ((0, 2), 5), ((1, 2), 7)):
        assert np.array_equal(m[:, :, i, j], planes[:, q] + 1j * planes[:, q + 1])
        assert np.array_equal(cm.cross(i, j), m[:, :, i, j]) and cm.cross(i, j).dtype == np.complex64
        assert np.array_equal(cm.cross(j, i), np.conj(cm.cross(i, j)))
        assert np.array_equal(cm.phase(i, j), -cm.phase(j, i)) and cm.phase(i, j).dtype == np.float64
    assert np.array_equal(cm.cross(1, 1), planes[:, 1].astype(np.complex64))
    for bad in (planes[:, :8], planes[0], np.zeros((1, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            CorrelationMatrix(bad, C)


def test_coherence_is_zero_where_the_denominator_is_zero():
    f = np.float32
    #                  one signal  quarter turn  half power common  dead bin  dead channel 1  denormal product
    paa = np.array([[4.0, 9.0, 2.0, 0.0, 5.0, 1e-30]], f)
    pbb = np.array([[9.0, 4.0, 4.0, 0.0, 0.0, 1e-30]], f)
    cre = np.array([[6.0, 0.0, 2.0, 0.0, 0.0, 0.0]], f)
    cim = np.array([[0.0, -6.0, 0.0, 0.0, 0.0, 0.0]], f)
    cm = CorrelationMatrix(np.stack([paa, pbb, cre, cim], axis=1), 2)
    coh = cm.coherence(0, 1)
    assert coh.dtype == np.float64 and np.all(np.isfinite(coh))
    assert np.allclose(coh[0, :3], [1.0, 1.0, 0.5]) and np.array_equal(coh[0, 3:], [0.0, 0.0, 0.0])
    assert np.array_equal(cm.coherence(1, 0), coh)
    assert np.allclose(cm.coherence(0, 0)[0, :3], 1.0) and cm.coherence(0, 0)[0, 3] == 0.0
    assert np.allclose(cm.phase(0, 1)[0, :3], [0.0, -np.pi / 2, 0.0])
    old = CrossSpectrum(paa, pbb, cre, cim)                                   # the two-channel class, on the same planes
    assert np.array_equal(coh, old.coherence) and np.array_equal(cm.phase(0, 1), old.phase)
    assert np.array_equal(cm.cross(0, 1), old.cross)


def test_python_shape_and_dtype_refusals():
    plan = bare_plan(64)
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((200, 3)) + 1j * rng.standard_normal((200, 3))).astype(np.complex64)
    assert spectrum._as_iqc_c64(x) is x                                        # what is ready goes in as it is
    for bad in (x[:, 0], x[:, :1], np.zeros((10, 9), np.complex64), np.zeros((10, 3), np.float32), np.zeros((10, 3, 2), np.complex64)):
        with pytest.raises(ValueError):
            plan.correlate(bad, 2)
    i16 = rng.integers(-2048, 2048, size=(200, 3, 2)).astype(np.int16)
    i8 = rng.integers(-128, 128, size=(200, 5, 2)).astype(np.int8)
    for bad in (i16.astype(np.int32), i16.reshape(200, 6), i16[:, :, ::-1], i16[:, :1], i8, np.zeros((10, 9, 2), np.int16)):
        with pytest.raises(ValueError):
            plan.correlate_ci16(bad, 2)
    for bad in (i16, i8.reshape(200, 10), i8[::2, ::2][:, :, ::-1], np.zeros((10, 1, 2), np.uint8), i8.astype(np.float32)):
        with pytest.raises(ValueError):
            plan.correlate_ci8(bad, 2)
    for bad in (i8, i8[:, :3], i16[:, :2]):
        with pytest.raises(ValueError):
            plan.cross_spectrum_ci8(bad, 2)
    # fewer elements than a group needs: an empty result, before any device call
    for res, C in ((plan.correlate(x[:100], 2), 3), (plan.correlate_ci16(i16[:127], 2), 3), (plan.correlate_ci8(i8[:63], 1), 5),
                   (plan.correlate_ci8(i8.view(np.uint8)[:63], 1), 5)):
        assert isinstance(res, CorrelationMatrix) and res.channels == C
        assert res.planes.shape == (0, C * C, 64) and res.planes.dtype == np.float32
        assert res.matrix().shape == (0, 64, C, C) and res.coherence(0, 1).shape == res.phase(1, 0).shape == (0, 64)
    empty = plan.cross_spectrum_ci8(np.ascontiguousarray(i8[:100, :2]), 2)
    assert isinstance(empty, CrossSpectrum) and all(v.shape == (0, 64) for v in empty)
    for k, hop in ((0, None), (2, 0), (-1, 64)):
        for call, arg in ((plan.correlate, x), (plan.correlate_ci16, i16), (plan.correlate_ci8, i8)):
            with pytest.raises(ValueError):
                call(arg, k, hop)
    for entry in ("exec_device_corrmat", "exec_device_corrmat_ci16", "exec_device_corrmat_ci8", "exec_device_corrmat_timed_each",
                  "exec_device_corrmat_ci16_timed_each", "exec_device_corrmat_ci8_timed_each"):
        for C, groups, k, stride in ((3, 0, 2, None), (3, 1, 0, None), (3, 1, 2, 0), (1, 1, 2, None), (9, 1, 2, None)):
            with pytest.raises(ValueError):
                getattr(plan, entry)(0x1000, C, groups, k, 0x2000, frame_stride=stride)
    double = bare_plan(64, double=True)
    with pytest.raises(ValueError, match="double"):
        double.correlate(x, 2)
    with pytest.raises(ValueError, match="double"):
        double.exec_device_corrmat(0x1000, 3, 1, 2, 0x2000)
    with pytest.raises(ValueError):
        spectrum.correlation_matrix([x[:, 0], x[:50, 1]], 64, 2)
    assert "copy" in spectrum.correlation_matrix.__doc__
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.correlation_matrix([x[:, 0], x[:, 1], x[:, 2]], 64, 2)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


@pytest.mark.parametrize("datatype", ["ci8", "cu8"])
def test_sigmf_multi_channel_8_bit_round_trip(tmp_path, datatype):
    rng = np.random.default_rng(3)
    dt = np.int8 if datatype == "ci8" else np.uint8
    x = rng.integers(0, 256, size=(300, 5, 2)).astype(np.uint8).view(dt)
    base = str(tmp_path / "five")
    data, meta_path = sigmf_io.write_sigmf(base, x, 2.4e6, 1e9, datatype=datatype, num_channels=5)
    assert os.path.getsize(data) == x.nbytes and open(data, "rb").read() == x.tobytes()
    back, meta = sigmf_io.read_sigmf_channels(meta_path)
    assert back.dtype == dt and back.shape == (300, 5, 2) and np.array_equal(back, x)
    assert meta["num_channels"] == 5 and meta["global"]["core:datatype"] == datatype and meta["global"]["core:num_channels"] == 5
    with open(data, "ab") as fh:                                                # a trailing partial sample instant is dropped
        fh.write(b"\x01\x02\x03")
    assert np.array_equal(sigmf_io.read_sigmf_channels(base)[0], x)
    other = np.uint8 if dt == np.int8 else np.int8
    for bad in (x.view(other), x[:, :4], x.reshape(300, 10), x.astype(np.complex64)[:, :, 0]):
        with pytest.raises(ValueError):
            sigmf_io.write_sigmf(str(tmp_path / "bad"), bad, 1e6, 1e9, datatype=datatype, num_channels=5)
    # the formats it served before behave as before
    c = (rng.standard_normal((50, 3)) + 1j * rng.standard_normal((50, 3))).astype(np.complex64)
    sigmf_io.write_sigmf(base + "_c", c, 1e6, 1e9, num_channels=3)
    assert np.array_equal(sigmf_io.read_sigmf_channels(base + "_c")[0], c)
    i16 = rng.integers(-2048, 2048, size=(50, 3, 2)).astype(np.int16)
    sigmf_io.write_sigmf(base + "_i", i16, 1e6, 1e9, datatype="ci16_le", num_channels=3)
    got = sigmf_io.read_sigmf_channels(base + "_i")[0]
    assert got.dtype == np.int16 and np.array_equal(got, i16)


def test_cli_exit_codes_of_correlate_and_cross_left_as_it_was(tmp_path, capsys):
    one = str(tmp_path / "one")
    sigmf_io.write_sigmf(one, np.zeros(8192, np.complex64), 1e6, 1e9)
    assert cli.main(["psd", one + ".sigmf-meta", "--integrate", "2", "--correlate"]) == 2
    assert "2..8 channels" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                        # --correlate without --integrate K
        cli.main(["psd", one + ".sigmf-meta", "--correlate"])
    assert e.value.code == 2 and "--correlate needs --integrate" in capsys.readouterr().err
    nine = str(tmp_path / "nine")
    sigmf_io.write_sigmf(nine, np.zeros((8192, 9), np.complex64), 1e6, 1e9, num_channels=9)
    assert cli.main(["psd", nine + ".sigmf-meta", "--integrate", "2", "--correlate"]) == 2
    assert "core:num_channels = 9" in capsys.readouterr().err
    three = str(tmp_path / "three")
    sigmf_io.write_sigmf(three, np.zeros((8192, 3), np.complex64), 1e6, 1e9, num_channels=3)
    zipped = str(tmp_path / "three.zip")
    with zipfile.ZipFile(zipped, "w") as z:
        for ext in (".sigmf-data", ".sigmf-meta"):
            z.write(three + ext, "three" + ext)
    assert cli.main(["psd", zipped, "--integrate", "2", "--correlate"]) == 2
    assert "not zipped" in capsys.readouterr().err
    # --cross on a three-channel file: refused exactly as before
    assert cli.main(["psd", three + ".sigmf-meta", "--integrate", "2", "--cross"]) == 2
    err = capsys.readouterr().err
    assert "--cross needs a two-channel cf32_le or ci16_le recording" in err and "core:num_channels = 3" in err

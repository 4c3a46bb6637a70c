"""The double-precision path on the GPU (precision="double": complex128 in, float64 rows / complex128 spectra out; csrc/fft_f64.hip).

The bar is about seven orders of magnitude tighter than the float32 path's: peak-relative magnitude error <= 1e-12 and
|dB difference| <= 1e-4 on every bin within 160 dB of the frame peak, the same NaN / infinity mask as numpy, and the reference's
dtypes (app/sdr/streamer.py:119-121 computes in float64 on complex128 samples)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from oracle import cpu_ref
from sdr_iq_visualizer_amd import _ffi, synth
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_TOL, DB_TOL, DEPTH_DB = 1e-12, 1e-4, 160.0


def assert_db64(got, ref, mag_tol=MAG_TOL, db_tol=DB_TOL, depth=DEPTH_DB):
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(got)], ref[np.isinf(ref)])
    for g, r in zip(got, ref):
        ok = np.isfinite(r)
        if not ok.any():
            continue
        mg, mr = 10.0 ** (g[ok] / 20), 10.0 ** (r[ok] / 20)
        err = float(np.max(np.abs(mg - mr)) / np.max(mr))
        assert err <= mag_tol, err
        deep = r[ok] >= np.max(r[ok]) - depth
        d = float(np.max(np.abs(g[ok][deep] - r[ok][deep])))
        assert d <= db_tol, d


def assert_c128(got, ref, tol=MAG_TOL):
    assert got.dtype == np.complex128 and got.shape == ref.shape
    peak = np.max(np.abs(ref), axis=-1, keepdims=True)
    err = float(np.max(np.abs(got - ref) / peak))
    assert err <= tol, err


def frames128(seed, n_frames, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_frames, n)) + 1j * rng.standard_normal((n_frames, n))).astype(np.complex128)


def test_golden_n4096_against_the_references_own_float64_rows(golden):
    g = golden["ref_n4096"]
    for name in g["names"]:
        x = g[f"{name}/iq"].astype(np.complex128)
        got = pkg.spectrum_db(x, precision="double")
        ref = g[f"{name}/power_db_c128"]
        assert_db64(got, ref)
        if name == "zeros":
            assert np.all(got == 20 * np.log10(1e-12))


@pytest.mark.parametrize("log2n", range(1, 23))
def test_every_power_of_two_db_and_complex(log2n):
    n = 1 << log2n
    nf = max(1, min(64, (1 << 21) // n))
    x = frames128(100 + log2n, nf, n)
    assert_db64(pkg.spectrum_db(x, precision="double"), cpu_ref.spectrum_db(x))
    assert_c128(pkg.fft_c128(x), cpu_ref.fft(x))
    assert_c128(pkg.fft_c128(x, shift=True), cpu_ref.fft(x, shift=True))


@pytest.mark.parametrize("n", [16, 1024, 4096, 65536])
@pytest.mark.parametrize("shift", [True, False])
def test_windows_and_shift(n, shift):
    x = frames128(7, 3, n)
    han = np.hanning(n)
    assert_db64(pkg.spectrum_db(x, window="hann", shift=shift, precision="double"),
                cpu_ref.spectrum_db(x, window=han, shift=shift))
    custom = np.random.default_rng(3).random(n) + 0.5               # float64: must not be down-cast on a double plan
    assert_db64(pkg.spectrum_db(x, window=custom, shift=shift, precision="double"),
                cpu_ref.spectrum_db(x, window=custom, shift=shift))
    assert_c128(pkg.fft_c128(x, window=custom, shift=shift), cpu_ref.fft(x, window=custom, shift=shift))


@pytest.mark.parametrize("eps", [1e-12, 1e-10, 0.0])
@pytest.mark.parametrize("n", [8, 4096, 16384])
def test_eps_including_zero(eps, n):
    x = frames128(11, 4, n)
    x[2] = 0                                                        # exact zeros: 20*log10(eps), -inf for eps = 0
    got = pkg.spectrum_db(x, eps=eps, precision="double")
    ref = cpu_ref.spectrum_db(x, eps=eps)
    assert_db64(got, ref)
    if eps == 0.0:
        assert np.all(np.isneginf(got[2]))


@pytest.mark.parametrize("n", [4096, 65536])
def test_stft_half_overlap_and_hop_larger_than_frame(n):
    rng = np.random.default_rng(n)
    iq = (rng.standard_normal(n * 6 + 123) + 1j * rng.standard_normal(n * 6 + 123)).astype(np.complex128)
    for hop in (n // 2, n + n // 3):
        got = pkg.stft_db(iq, n, hop, precision="double")
        ref = cpu_ref.stft_db(iq, n, hop)
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert_db64(got, ref)


@pytest.mark.parametrize("n", [4096, 65536])
def test_nan_frame_gives_nan_row_and_leaves_neighbours(n):
    x = frames128(5, 3, n)
    x[1, 17] = np.nan
    got = pkg.spectrum_db(x, precision="double")
    assert np.all(np.isnan(got[1]))
    assert_db64(got[[0, 2]], cpu_ref.spectrum_db(x[[0, 2]]))


def test_dynamic_range_150_db_at_65536_hann():
    n = 65536
    t = np.arange(n)
    x = np.exp(2j * np.pi * 1000 * t / n) + 10 ** (-150 / 20) * np.exp(2j * np.pi * 20000 * t / n)
    got = pkg.spectrum_db(x, window="hann", precision="double")
    ref = cpu_ref.spectrum_db(x, window=np.hanning(n))
    deep = ref >= ref.max() - 160
    assert deep.sum() >= 6
    weak = np.abs(np.arange(n) - (n // 2 + 20000)) <= 1
    assert np.all(deep[weak])
    assert float(np.max(np.abs(got[deep] - ref[deep]))) <= 1e-4
    assert_db64(got, ref)


def test_host_boundary_paths():
    n = 4096
    one = frames128(1, 1, n)[0]                                     # the live call: one frame
    got = pkg.spectrum_db(one, precision="double")
    assert got.shape == (n,) and got.dtype == np.float64
    assert_db64(got, cpu_ref.spectrum_db(one))
    big = frames128(2, 600, n)                                      # 37.5 MiB: more than one 16 MiB host chunk
    assert_db64(pkg.spectrum_db(big, precision="double"), cpu_ref.spectrum_db(big))
    pin_in = pkg.pinned_empty(big.shape, np.complex128)
    pin_in[...] = big
    pin_out = pkg.pinned_empty(big.shape, np.float64)
    plan = SpectrumPlan(n, precision="double")
    try:
        res = plan.spectrum_db(pin_in, out=pin_out)
        assert res is pin_out
        assert_db64(pin_out, cpu_ref.spectrum_db(big))
        small = pkg.pinned_empty((4, n), np.complex128)
        small[...] = big[:4]
        assert_db64(plan.spectrum_db(small), cpu_ref.spectrum_db(big[:4]))
    finally:
        plan.close()


def test_exec_device_on_plan_stream_and_timed_each():
    n, nf = 65536, 5
    x = frames128(9, nf, n)
    lib = _ffi.lib()
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    _ffi.check(lib.sdrk_dev_alloc(0, x.nbytes, ctypes.byref(d_in)))
    _ffi.check(lib.sdrk_dev_alloc(0, nf * n * 8, ctypes.byref(d_out)))
    plan = SpectrumPlan(n, precision="double")
    try:
        _ffi.check(lib.sdrk_memcpy_h2d(0, d_in, x.ctypes.data_as(ctypes.c_void_p), x.nbytes))
        plan.exec_device(d_in.value, nf, d_out.value)
        plan.sync()
        out = np.empty((nf, n), np.float64)
        _ffi.check(lib.sdrk_memcpy_d2h(0, out.ctypes.data_as(ctypes.c_void_p), d_out, out.nbytes))
        assert_db64(out, cpu_ref.spectrum_db(x))
        ms = plan.exec_device_timed_each(d_in.value, nf, d_out.value, launches=3)
        assert len(ms) == 3 and all(v > 0 for v in ms)
    finally:
        plan.close()
        lib.sdrk_dev_free(0, d_in)
        lib.sdrk_dev_free(0, d_out)


def test_exec_device_on_a_caller_stream():
    """A fresh process (torch first, so that both share one HIP runtime): the transform on a torch stream."""
    code = (
        "import torch, numpy as np\n"
        "import sdr_iq_visualizer_amd as pkg\n"
        "from oracle import cpu_ref\n"
        "from sdr_iq_visualizer_amd.spectrum import SpectrumPlan\n"
        "n, nf = 4096, 33\n"
        "rng = np.random.default_rng(4)\n"
        "x = rng.standard_normal((nf, n)) + 1j * rng.standard_normal((nf, n))\n"
        "xt = torch.from_numpy(x).cuda()\n"
        "out = torch.empty((nf, n), dtype=torch.float64, device='cuda')\n"
        "s = torch.cuda.Stream()\n"
        "torch.cuda.current_stream().synchronize()\n"
        "plan = SpectrumPlan(n, precision='double')\n"
        "plan.exec_device(xt.data_ptr(), nf, out.data_ptr(), stream=s.cuda_stream)\n"
        "s.synchronize()\n"
        "got, ref = out.cpu().numpy(), cpu_ref.spectrum_db(x)\n"
        "err = np.max(np.abs(10 ** (got / 20) - 10 ** (ref / 20))) / np.max(10 ** (ref / 20))\n"
        "print('err', err, np.max(np.abs(got - ref)))\n"
        "assert err <= 1e-12 and np.max(np.abs(got - ref)) <= 1e-4\n"
        "plan.close()\n"
        "print('caller stream ok')\n"
    )
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=REPO))
    assert r.returncode == 0 and "caller stream ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


def test_precision_auto():
    x64 = synth.synth_iq(77, 0, 3, 4096)
    assert np.array_equal(pkg.spectrum_db(x64, precision="auto"), pkg.spectrum_db(x64))   # complex64 -> today's rows, bit for bit
    assert pkg.spectrum_db(x64, precision="auto").dtype == np.float32
    x128 = x64.astype(np.complex128)
    got = pkg.spectrum_db(x128, precision="auto")
    assert got.dtype == np.float64
    assert_db64(got, cpu_ref.spectrum_db(x128))
    assert pkg.stft_db(x128.reshape(-1), 4096, 2048, precision="auto").dtype == np.float64
    assert pkg.spectrum_db(x128).dtype == np.float32                                       # the default is unchanged
    d = pkg.process_frame(x128[0], 1_000_000, 2_400_000_000, precision="auto")
    assert list(d) == ["time", "samples", "freqs", "power_db", "sample_rate", "center_freq"]
    assert d["samples"] is x128[0] or d["samples"].base is x128
    assert d["power_db"].dtype == np.float64
    ref = cpu_ref.process_frame(x128[0], 1_000_000, 2_400_000_000)
    assert_db64(d["power_db"], ref["power_db"])
    assert np.array_equal(d["freqs"], ref["freqs"])


def test_process_frame_samples_identity():
    x = synth.synth_iq(1, 0, 1, 4096)[0].astype(np.complex128)
    d = pkg.process_frame(x, 1e6, 2.4e9, precision="auto")
    assert d["samples"] is x


def test_mixing_plan_precisions_with_entry_points_is_refused():
    n = 4096
    x128 = frames128(1, 2, n)
    x64 = x128.astype(np.complex64)
    lib = _ffi.lib()
    p64 = SpectrumPlan(n, precision="double")
    p32 = SpectrumPlan(n)
    try:
        assert lib.sdrk_plan_precision(p64.handle) == 64 and lib.sdrk_plan_precision(p32.handle) == 32
        assert lib.sdrk_plan_nfft(p64.handle) == n and lib.sdrk_plan_device(p64.handle) == 0
        o32 = np.empty((2, n), np.float32)
        o64 = np.empty((2, n), np.float64)
        st = lib.sdrk_exec_host(p64.handle, x64.ctypes.data_as(ctypes.c_void_p), 2, n, o32.ctypes.data_as(ctypes.c_void_p))
        assert st == _ffi.SDRK_ERR_INVALID and b"float64 plan" in lib.sdrk_last_error()
        st = lib.sdrk_exec_host_f64(p32.handle, x128.ctypes.data_as(ctypes.c_void_p), 2, n, o64.ctypes.data_as(ctypes.c_void_p))
        assert st == _ffi.SDRK_ERR_INVALID and b"float32 plan" in lib.sdrk_last_error()
        st = lib.sdrk_welch_psd_host(p64.handle, x64.ctypes.data_as(ctypes.c_void_p), 2, n, ctypes.c_float(1.0),
                                     o32.ctypes.data_as(ctypes.c_void_p))
        assert st == _ffi.SDRK_ERR_INVALID
        wf = ctypes.c_void_p()
        _ffi.check(lib.sdrk_waterfall_create(0, n, 4, ctypes.byref(wf)))
        try:
            st = lib.sdrk_waterfall_append_iq(wf, p64.handle, x64.ctypes.data_as(ctypes.c_void_p), 2, n)
            assert st == _ffi.SDRK_ERR_INVALID
        finally:
            lib.sdrk_waterfall_destroy(wf)
        st = lib.sdrk_plan_create_f64(0, 1000, 1, 0, None, ctypes.c_double(1e-12), 1, ctypes.byref(ctypes.c_void_p()))
        assert st == _ffi.SDRK_ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            p64.welch_psd(x128.reshape(-1), 1e6)
        with pytest.raises(ValueError):                             # check() turns SDRK_ERR_INVALID into ValueError
            _ffi.check(lib.sdrk_exec_host(p64.handle, x64.ctypes.data_as(ctypes.c_void_p), 2, n,
                                          o32.ctypes.data_as(ctypes.c_void_p)))
        # the float32 plan still works after the refused calls
        assert np.array_equal(p32.spectrum_db(x64), pkg.spectrum_db(x64))
    finally:
        p64.close()
        p32.close()

"""int16 I,Q input on the GPU (the ``*_ci16`` entry points: what the radio delivers, SigMF ``ci16_le``).

int16 -> float32 is exact and both paths run the same arithmetic, so the acceptance criterion has no tolerance: a ci16 call
returns exactly the bits the complex64 call returns for the same values — at every frame length, on every route of the numpy
boundary and on the device route.  Independently of our own complex64 path, the rows are also held to the reference's
expression evaluated in float64 on the integer samples (what app/sdr/streamer.py:119-121 computes on what pyadi-iio hands it),
with the float32 path's parity bars (tests/parity.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from oracle import cpu_ref
from sdr_iq_visualizer_amd import _ffi, sigmf_io, synth
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import DevBuf, same_bits, widen
from tests.parity import assert_db_parity, assert_db_parity_deep

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def input_frames(n, seed, count=None):
    """One frame of each kind: the generator's 12-bit codes, full-range random int16, a frame holding -32768 and 32767,
    the all-zero frame, an on-bin tone; `count` keeps the first few (large lengths)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((5, n, 2), np.int16)
    x[0] = synth.synth_iq_ci16(seed, 7, 1, n)[0]
    x[1] = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64).astype(np.int16)
    x[2] = rng.integers(-100, 100, size=(n, 2), dtype=np.int64).astype(np.int16)
    x[2, 0] = (-32768, 32767)
    x[2, n - 1] = (32767, -32768)
    # x[3] stays zero
    k = max(1, n // 8) if n > 2 else 1
    ph = 2.0 * np.pi * k * np.arange(n) / n
    x[4, :, 0] = np.rint(12000 * np.cos(ph)).astype(np.int16)
    x[4, :, 1] = np.rint(12000 * np.sin(ph)).astype(np.int16)
    return x if count is None else np.ascontiguousarray(x[:count])


SETTINGS = [(None, True, 1e-12), ("hann", False, 1e-10), ("custom", True, 0.0), (None, False, 0.0)]


def _window(kind, n):
    if kind != "custom":
        return kind
    return (0.25 + 0.75 * np.random.default_rng(n).random(n)).astype(np.float32)


POW2 = [1 << l for l in range(1, 23)]
NPO2 = [1000, 5000, 100000]


@pytest.mark.parametrize("n", POW2 + NPO2)
def test_bit_identity_with_the_complex64_path_at_every_length(n):
    count = None if n <= (1 << 20) else 4            # (2^21, 2^22: without the tone frame; the zero frame stays)
    x = input_frames(n, 100 + n % 97, count)
    c = widen(x)
    for kind, shift, eps in SETTINGS:
        with SpectrumPlan(n, window=_window(kind, n), eps=eps, shift=shift, max_batch=8) as plan:
            with np.errstate(all="ignore"):
                got, ref = plan.spectrum_db_ci16(x), plan.spectrum_db(c)
                assert got.dtype == np.float32 and same_bits(got, ref), (n, kind, shift, eps, int(np.sum(got != ref)))
                gc, rc = plan.fft_ci16(x), plan.fft(c)
                assert gc.dtype == np.complex64 and same_bits(gc, rc), (n, kind, shift, eps)
                # one frame, (n, 2) -> (n,)
                assert same_bits(plan.spectrum_db_ci16(x[1]), ref[1])
            if eps == 1e-12:
                assert np.all(got[3] == np.float32(-240.00002)), got[3][:4]      # the all-zero frame: 20 log10(1e-12) in float32


@pytest.mark.parametrize("n", [64, 1024, 4096, 65536, 1000])
def test_module_functions_match_their_complex64_counterparts(n):
    x = input_frames(n, 5)
    c = widen(x)
    w = _window("custom", n)
    assert same_bits(pkg.spectrum_db_ci16(x), pkg.spectrum_db(c))
    assert same_bits(pkg.spectrum_db_ci16(x, window="hann", eps=1e-10, shift=False),
                     pkg.spectrum_db(c, window="hann", eps=1e-10, shift=False))
    assert same_bits(pkg.spectrum_db_ci16(x[0], window=w), pkg.spectrum_db(c[0], window=w))
    assert same_bits(pkg.fft_ci16(x, window=w, shift=True), pkg.fft_c64(c, window=w, shift=True))
    out = np.empty((5, n), np.float32)
    assert pkg.spectrum_db_ci16(x, out=out) is out and same_bits(out, pkg.spectrum_db(c))
    from sdr_iq_visualizer_amd import processing
    assert processing.spectrum_db_ci16 is pkg.spectrum_db_ci16 and processing.stft_db_ci16 is pkg.stft_db_ci16


@pytest.mark.parametrize("form", ["direct", "wide"])
def test_both_load_forms_of_the_4096_kernel(form, monkeypatch):
    """SDRK_CI16_FORM picks the load form of the N = 4096 int16 kernel (one dword per lane / 16 bytes per lane through LDS);
    the wide one applies only to 16-byte aligned frame starts, so an odd hop takes the direct form whatever the variable says."""
    monkeypatch.setenv("SDRK_CI16_FORM", form)
    x = np.concatenate([input_frames(4096, 3), _random_frames(700, 4096, 8)])
    c = widen(x)
    for kind, shift, eps in SETTINGS:
        with SpectrumPlan(4096, window=_window(kind, 4096), eps=eps, shift=shift) as plan:
            with np.errstate(all="ignore"):
                assert same_bits(plan.spectrum_db_ci16(x), plan.spectrum_db(c)), (form, kind)
                assert same_bits(plan.fft_ci16(x[:9]), plan.fft(c[:9])), (form, kind)
            for hop in (2048, 2052, 2049, 4100, 6):
                s = x.reshape(-1, 2)[: 4096 + 40 * hop]
                assert same_bits(plan.stft_db_ci16(s, hop), plan.stft_db(widen(s), hop)), (form, kind, hop)
                assert same_bits(plan.stft_db_ci16(s[1:], hop), plan.stft_db(widen(s[1:]), hop)), (form, kind, hop)   # base 4-byte aligned


# ---- every route of the numpy boundary ----------------------------------------------------------------------------
# 4096: the flagship's own int16 kernel; 1024: fft_lds.hip's int16 form; 128 and 65536: widened on the device first
def _random_frames(n_frames, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2048, 2048, size=(n_frames, n, 2), dtype=np.int64).astype(np.int16)


@pytest.mark.parametrize("n", [4096, 1024, 128, 65536])
def test_small_and_mid_size_host_calls(n):
    with SpectrumPlan(n, window="hann") as plan:
        for n_frames in (1, 256):
            if n == 65536 and n_frames == 256:
                n_frames = 40
            x = _random_frames(n_frames, n, n + n_frames)
            assert same_bits(plan.spectrum_db_ci16(x), plan.spectrum_db(widen(x))), (n, n_frames)
            assert same_bits(plan.fft_ci16(x), plan.fft(widen(x))), (n, n_frames)


@pytest.mark.parametrize("n", [4096, 1024, 128, 65536])
def test_three_slot_pipeline_with_a_ragged_last_chunk(n):
    n_frames = (33 << 20) // (4 * n) + 5                      # above 32 MiB of int16 input
    x = _random_frames(n_frames, n, 3 * n)
    assert x.nbytes > (32 << 20)
    with SpectrumPlan(n) as plan:
        assert same_bits(plan.spectrum_db_ci16(x), plan.spectrum_db(widen(x)))


@pytest.mark.parametrize("n", [4096, 1024, 65536])
def test_pinned_and_registered_inputs(n):
    for n_frames in (64, (33 << 20) // (4 * n) + 3):       # one launch on the caller's arrays / chunked straight from them
        if n == 65536 and n_frames == 64:
            n_frames = 16
        src = _random_frames(n_frames, n, 11 + n)
        ref = pkg.spectrum_db(widen(src))
        x = pkg.pinned_empty(src.shape, np.int16)
        x[...] = src
        assert pkg.is_pinned(x)
        out = pkg.pinned_empty((n_frames, n), np.float32)
        assert same_bits(pkg.spectrum_db_ci16(x, out=out), ref)
        assert same_bits(pkg.spectrum_db_ci16(x), ref)                # pinned in, pageable out
        y = src.copy()
        with pkg.registered(y):
            assert same_bits(pkg.spectrum_db_ci16(y), ref)
        del x, out


@pytest.mark.parametrize("n", [4096, 1024, 128, 65536, 1000])
def test_stft_with_half_and_odd_hops(n):
    """hop = nfft / 2 and an odd hop: frame starts that are only 4-byte aligned."""
    rng = np.random.default_rng(n)
    rows = 300 if n <= 4096 else 40
    for hop in (n // 2, n // 2 + 1 if (n // 2) % 2 == 0 else n // 2 + 2, 3):
        length = (rows - 1) * hop + n + 7
        if hop == 3:
            length = n + 3 * 50
        x = rng.integers(-2048, 2048, size=(length, 2), dtype=np.int64).astype(np.int16)
        got = pkg.stft_db_ci16(x, n, hop, window="hann")
        assert got.shape == (1 + (length - n) // hop, n)
        assert same_bits(got, pkg.stft_db(widen(x), n, hop, window="hann")), (n, hop)


# ---- the device route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,first,n_frames", [(4096, 0, 9), (4096, (1 << 33) + 5, 3), (1024, 17, 33), (65536, 2, 3), (1000, 1, 4)])
def test_device_generator_equals_the_numpy_int16_form(n, first, n_frames):
    with DevBuf(n_frames * n * 4) as d:
        _ffi.check(_ffi.lib().sdrk_synth_fill_ci16(0, 4242, first, n_frames, n, d.p, None))
        got = d.get((n_frames, n, 2), np.int16)
    ref = synth.synth_iq_ci16(4242, first, n_frames, n)
    assert np.array_equal(got, ref)
    c = synth.synth_iq(4242, first, n_frames, n)
    assert np.array_equal(ref[..., 0], c.real.astype(np.int16)) and np.array_equal(ref[..., 1], c.imag.astype(np.int16))


def _device_case(n, n_frames, window=None, stride=None, check_rows=None):
    """exec_device_ci16 on generated int16 frames against exec_device on the generator's complex64 frames (the same values)."""
    lib = _ffi.lib()
    stride = n if stride is None else stride
    gen_frames = ((n_frames - 1) * stride + n + n - 1) // n
    with DevBuf(gen_frames * n * 4) as d16, DevBuf(gen_frames * n * 8) as d64, DevBuf(n_frames * n * 4) as da, \
            DevBuf(n_frames * n * 4) as db, SpectrumPlan(n, window=window) as plan:
        _ffi.check(lib.sdrk_synth_fill_ci16(0, 31, 0, gen_frames, n, d16.p, None))
        _ffi.check(lib.sdrk_synth_fill(0, 31, 0, gen_frames, n, d64.p, None))
        plan.exec_device_ci16(d16.p.value, n_frames, da.p.value, frame_stride=stride)
        plan.sync()
        before = plan.fused_status()
        plan.exec_device(d64.p.value, n_frames, db.p.value, frame_stride=stride)
        plan.sync()
        step = max(1, n_frames // (check_rows or n_frames))
        for f in range(0, n_frames, step):
            assert same_bits(da.get((n,), np.float32, f * n * 4), db.get((n,), np.float32, f * n * 4)), (n, f)
        assert same_bits(da.get((n,), np.float32, (n_frames - 1) * n * 4), db.get((n,), np.float32, (n_frames - 1) * n * 4))
        ms = plan.exec_device_ci16_timed_each(d16.p.value, n_frames, da.p.value, launches=2, frame_stride=stride)
        assert len(ms) == 2 and all(v > 0 for v in ms)
        assert plan.exec_device_ci16_timed(d16.p.value, n_frames, da.p.value, launches=1, frame_stride=stride) > 0
        assert same_bits(da.get((n,), np.float32, (n_frames - 1) * n * 4), db.get((n,), np.float32, (n_frames - 1) * n * 4))
        return before, plan.fused_status()


@pytest.mark.parametrize("n,n_frames", [(4096, 1000), (4096, 1), (1024, 4097), (16384, 70), (256, 1001), (128, 5000), (1000, 300)])
def test_exec_device_on_the_plan_stream(n, n_frames):
    _device_case(n, n_frames, window="hann")


def test_exec_device_with_overlapped_and_spaced_frames():
    _device_case(4096, 500, stride=2049)
    _device_case(1024, 500, stride=3)
    _device_case(65536, 50, stride=32769)            # widened as one run, halo carried
    _device_case(128, 3000, stride=131)               # widened frame by frame
    _device_case(32768, 20, stride=40001)


def test_more_frames_than_one_staging_chunk_at_65536_reports_through_fused_status():
    """64 MiB of complex64 staging is 128 frames of 65536: 600 frames are five chunks; the call as a whole is what picks the
    persistent N = 65536 form, and its launches are counted and checked like the complex64 call's."""
    before, after = _device_case(65536, 600, check_rows=12)
    assert before["launches"] >= 5 and not before["fallen_back"], before         # the ci16 call alone
    assert after["launches"] > before["launches"] and not after["fallen_back"], after


def test_more_frames_than_one_staging_chunk_at_2_pow_20():
    _device_case(1 << 20, 19, check_rows=19)          # 8 frames per chunk: 8 + 8 + 3
    _device_case(1 << 20, 12, stride=(1 << 19) + 1, check_rows=12)   # overlapped: 15 frames per chunk would fit, 12 given
    _device_case(1 << 20, 40, stride=(1 << 19), check_rows=10)       # overlapped, three chunks


def test_exec_device_on_a_caller_stream():
    """A fresh process (torch first, so that both share one HIP runtime): int16 frames on a torch stream, at a length with
    its own int16 kernel and at one that goes through the staging."""
    code = (
        "import torch, numpy as np\n"
        "import sdr_iq_visualizer_amd as pkg\n"
        "from sdr_iq_visualizer_amd.spectrum import SpectrumPlan\n"
        "rng = np.random.default_rng(4)\n"
        "for n, nf in ((4096, 333), (65536, 150), (64, 999)):\n"
        "    x = rng.integers(-32768, 32768, size=(nf, n, 2), dtype=np.int64).astype(np.int16)\n"
        "    c = (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)\n"
        "    xt = torch.from_numpy(x).cuda()\n"
        "    out = torch.empty((nf, n), dtype=torch.float32, device='cuda')\n"
        "    s = torch.cuda.Stream()\n"
        "    torch.cuda.current_stream().synchronize()\n"
        "    plan = SpectrumPlan(n)\n"
        "    plan.exec_device_ci16(xt.data_ptr(), nf, out.data_ptr(), stream=s.cuda_stream)\n"
        "    plan.exec_device_ci16(xt.data_ptr(), nf, out.data_ptr())\n"      # then the plan's stream: ordered behind the first
        "    s.synchronize(); plan.sync()\n"
        "    ref = plan.spectrum_db(c)\n"
        "    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), n\n"
        "    plan.close()\n"
        "print('caller stream ok')\n"
    )
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=REPO))
    assert r.returncode == 0 and "caller stream ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])


# ---- oracle parity, independent of our own complex64 path ---------------------------------------------------------------
@pytest.mark.parametrize("n,n_frames", [(4096, 256), (1024, 6), (16384, 5), (65536, 4), (1000, 6)])
def test_rows_against_the_reference_expression_in_float64_on_the_integer_samples(n, n_frames):
    x = _random_frames(n_frames, n, 900 + n)
    x64 = x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)      # what pyadi-iio hands streamer.py:114
    for window, wref in ((None, None), ("hann", np.hanning(n))):
        got = pkg.spectrum_db_ci16(x, window=window)
        ref = cpu_ref.spectrum_db(x64, window=wref)
        assert ref.dtype == np.float64
        assert_db_parity(got, ref, what=f"ci16 n={n} window={window}")
        worst = assert_db_parity_deep(got, ref, what=f"ci16 n={n} window={window}")
        print(f"ci16 n={n} window={window}: worst |delta dB| within 70 dB of the peak {worst:.3e}")


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_match_the_complex64_entry_points():
    lib = _ffi.lib()
    x = _random_frames(4, 4096, 1)
    out = np.empty((4, 4096), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with SpectrumPlan(4096, precision="double") as p64:
        for fn in (p64.spectrum_db_ci16, p64.fft_ci16):
            with pytest.raises(ValueError):
                fn(x)
        with pytest.raises(ValueError):
            p64.stft_db_ci16(x.reshape(-1, 2))
        with pytest.raises(ValueError):
            p64.exec_device_ci16(1, 1, 1)
        # the C ABI itself: an f64 plan is refused with the status the complex64 entries give it
        want = lib.sdrk_exec_host(p64.handle, vp(x), 4, 4096, vp(out))
        assert want == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ci16(p64.handle, vp(x), 4, 4096, vp(out)) == want
        assert lib.sdrk_exec_fft_host_ci16(p64.handle, vp(x), 4, 4096, vp(out)) == want
        assert lib.sdrk_exec_device_ci16(p64.handle, vp(x), 4, 4096, vp(out), None) == want
        ms = (ctypes.c_float * 2)()
        assert lib.sdrk_exec_device_ci16_timed_each(p64.handle, vp(x), 4, 4096, vp(out), 2, ms) == want
        assert b"float64 plan" in lib.sdrk_last_error()
    with SpectrumPlan(4096, max_batch=2) as p:
        assert lib.sdrk_exec_host(p.handle, vp(widen(x)), 4, 4096, vp(out)) == _ffi.SDRK_ERR_INVALID
        text = lib.sdrk_last_error()
        assert lib.sdrk_exec_host_ci16(p.handle, vp(x), 4, 4096, vp(out)) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_last_error() == text and b"max_batch" in text
        with pytest.raises(ValueError, match="max_batch"):
            p.spectrum_db_ci16(x)
        for args in ((None, vp(x), 2, 4096, vp(out)), (p.handle, None, 2, 4096, vp(out)), (p.handle, vp(x), 2, 4096, None),
                     (p.handle, vp(x), 2, 0, vp(out))):
            assert lib.sdrk_exec_host_ci16(*args) == lib.sdrk_exec_host(*args) == _ffi.SDRK_ERR_INVALID
            assert lib.sdrk_exec_fft_host_ci16(*args) == lib.sdrk_exec_fft_host(*args) == _ffi.SDRK_ERR_INVALID
            assert lib.sdrk_exec_device_ci16(*args, None) == lib.sdrk_exec_device(*args, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_ci16_timed_each(p.handle, vp(x), 2, 4096, vp(out), 0, ms) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_ci16_timed_each(p.handle, vp(x), 2, 4096, vp(out), 2, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_ci16(p.handle, None, 0, 4096, None) == _ffi.SDRK_OK          # nothing to do
        assert same_bits(p.spectrum_db_ci16(x[:2]), p.spectrum_db(widen(x[:2])))                # the plan still works
    assert lib.sdrk_synth_fill_ci16(0, 1, 0, 2, 4096, None, None) == _ffi.SDRK_ERR_INVALID
    assert lib.sdrk_synth_fill_ci16(0, 1, 0, 2, 4095, vp(x), None) == _ffi.SDRK_ERR_INVALID
    assert lib.sdrk_synth_fill_ci16(99, 1, 0, 2, 4096, vp(x), None) == _ffi.SDRK_ERR_NO_DEVICE
    for bad in (widen(x), x.astype(np.int32), x[..., 0], x.reshape(4, 2, 4096), x[:, ::2], np.zeros((2, 3, 4096, 2), np.int16),
                x.tolist()):
        with pytest.raises(ValueError):
            pkg.spectrum_db_ci16(bad)
        with pytest.raises(ValueError):
            pkg.fft_ci16(bad)
    with pytest.raises(ValueError):
        pkg.stft_db_ci16(x, 4096)                     # a stream is (n_samples, 2)
    with pytest.raises(ValueError):
        pkg.stft_db_ci16(x.reshape(-1, 2), 4096, 0)
    with SpectrumPlan(1024) as p:
        with pytest.raises(ValueError):
            p.spectrum_db_ci16(x)                     # frames of another length


# ---- SigMF -------------------------------------------------------------------------------------------------------------
def test_sigmf_ci16_recording_gives_the_default_readers_bits(tmp_path):
    x = synth.synth_iq_ci16(77, 0, 6, 4096).reshape(-1, 2)
    base = str(tmp_path / "rec")
    sigmf_io.write_sigmf(base, x, 2_000_000, 915_000_000, datatype="ci16_le")
    raw, meta = sigmf_io.read_sigmf(base, native=True)
    wide, _ = sigmf_io.read_sigmf(base)
    assert raw.dtype == np.int16 and raw.shape == (6 * 4096, 2) and wide.dtype == np.complex64
    assert meta["global"]["core:datatype"] == "ci16_le" and meta["sample_rate"] == 2e6
    assert same_bits(pkg.spectrum_db_ci16(raw.reshape(6, 4096, 2)), pkg.spectrum_db(wide.reshape(6, 4096)))
    assert same_bits(pkg.stft_db_ci16(raw, 1024, 512), pkg.stft_db(wide, 1024, 512))
    from sdr_iq_visualizer_amd import cli
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", base + ".sigmf-meta", "--nfft", "4096", "--welch", "1024", "--out", out]) == 0
    z = np.load(out)
    assert same_bits(z["power_db"], pkg.spectrum_db(wide[:4096]))

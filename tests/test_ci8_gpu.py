"""8-bit I,Q input on the GPU: sdrk_exec_*_ci8, sdrk_exec_*_integrated_ci8 and what sits on them in spectrum.py, sigmf_io.py.

One sentence of semantics, so one kind of assertion: x = I + iQ for int8 pairs (SigMF ci8), (I - 127.5) + i(Q - 127.5) for
uint8 pairs (cu8), exactly, then THE SAME BITS as the complex64 entry of the same plan returns for those widened values — every
assertion below is array_equal on the bit patterns against that entry (the widening is numpy's, tests/ci8_helpers.py), except
the absolute checks against float64 numpy on the converted samples (the float32 path's bars: 1e-5 of the frame peak in
amplitude, 0.01 dB within 70 dB of it), which keep the pair from being wrong together.  Every case runs for int8 and for
uint8; inputs are random over the full byte range with 0, 127, -128 / 255 and 128 planted."""
import ctypes

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from oracle import cpu_ref
from sdr_iq_visualizer_amd import _ffi, sigmf_io
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.ci8_helpers import DTYPES, Pair8, case_4096_integrated, case_4096_per_frame, stream8, widen8
from tests.gpu_helpers import DETECTORS, FORMS, DevBuf, run_child, same_bits, same_bits_f32, stream16_planted, widen_flat
from tests.parity import assert_db_parity, assert_db_parity_deep

pytestmark = pytest.mark.gpu

HOST_CHUNK = 16 << 20      # plan_internal.h HOST_CHUNK_BYTES
ZERO_COPY_MAX = 32 << 20   # plan_internal.h ZERO_COPY_MAX_BYTES
STAGE = 64 << 20           # ci16_api.hip CI16_STAGE_BYTES (the 8-bit unpack route shares the staging)


# ---- 1. the N = 4096 kernel, per frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frames", [1, 3, 777])
def test_4096_per_frame_has_the_complex64_bits(dtype, frames):
    """1 and 3 frames; 777: more than the 768 resident workgroups, so a workgroup takes a second frame with the prefetch
    crossing.  Strides 4096, 2048, 1, 4097 (odd sample offsets: 2-byte alignment only) and 5000; a canary row behind the last."""
    case_4096_per_frame(dtype, frames)


@pytest.mark.parametrize("dtype", DTYPES)
def test_4096_device_buffer_whose_first_sample_sits_at_byte_offset_2(dtype):
    case_4096_per_frame(dtype, 5, offset=2)


# ---- 2. every other length: widened into the plan's staging first -------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,frames", [(2, 9), (64, 9), (256, 9), (1024, 9), (16384, 5), (65536, 2), (1000, 5)])
def test_other_lengths_through_the_unpack_route(dtype, n, frames):
    """Packed, one overlapped stride (widened as one run) and one spaced stride (widened frame by frame); chirp-z at 1000."""
    strides = (n, n // 2 + (n > 2), n + 3)
    iq = stream8(n + frames, (frames - 1) * max(strides) + n, dtype)
    with Pair8(iq, frames, n) as d:
        for window in ("hann", None):
            with SpectrumPlan(n, window=window) as plan:
                for stride in strides:
                    got, ref = d.rows8(plan, frames, stride), d.rows64(plan, frames, stride)
                    assert same_bits_f32(got, ref), (dtype, n, window, stride, int(np.sum(got != ref)))
                x = np.ascontiguousarray(iq[: frames * n].reshape(frames, n, 2))
                assert same_bits(plan.fft_ci8(x), plan.fft(widen8(x))), (dtype, n, window, "spectra")


@pytest.mark.parametrize("dtype", DTYPES)
def test_65536_with_more_frames_than_one_staging_chunk(dtype):
    """64 MiB of complex64 staging is 128 frames of 65536: 130 frames are two chunks, below the 512-frame persistent threshold."""
    n, frames = 65536, 130
    assert frames * n * 8 > STAGE and frames < 512
    iq = stream8(65, frames * n, dtype)
    with Pair8(iq, frames, n) as d, SpectrumPlan(n, window="hann") as plan:
        assert same_bits_f32(d.rows8(plan, frames, n), d.rows64(plan, frames, n))


# ---- 3. integrated ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2, 16])
@pytest.mark.parametrize("groups", [1, 5])
def test_4096_integrated_has_the_complex64_bits(dtype, k, groups):
    case_4096_integrated(dtype, k, groups)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_group_of_3000_frames_is_split_carried_and_finalized(dtype):
    """The device entry cuts the one group into slices (partial rows, the finalize); the host entry also carries a slice's
    state across its chunks of 2048 frames."""
    n, k = 4096, 3000
    iq = stream8(30, k * n, dtype)
    assert iq.nbytes > HOST_CHUNK
    with Pair8(iq, 1, n) as d, SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            want = d.int64(plan, 1, k, n, det, "power", 0.5)
            assert same_bits_f32(d.int8(plan, 1, k, n, det, "power", 0.5), want), (dtype, det, "device")
            assert same_bits_f32(plan.integrate_ci8(iq, k, n, det, "power", 0.5), want), (dtype, det, "host")


@pytest.mark.parametrize("dtype", DTYPES)
def test_1024_integrated_through_the_route(dtype):
    n, k, groups = 1024, 3, 7
    iq = stream8(31, groups * k * n, dtype)
    with Pair8(iq, groups, n) as d, SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            for form in FORMS:
                want = d.int64(plan, groups, k, n, det, form, 0.5)
                assert same_bits_f32(d.int8(plan, groups, k, n, det, form, 0.5), want), (dtype, det, form, "device")
                assert same_bits_f32(plan.integrate_ci8(iq, k, n, det, form, 0.5), want), (dtype, det, form, "host")
    assert same_bits_f32(pkg.integrated_db_ci8(iq, n, k, detector="max"), pkg.integrated_db(widen8(iq), n, k, detector="max"))
    assert same_bits_f32(pkg.welch_psd_streamed_ci8(iq, n, 2.4e6), pkg.welch_psd_streamed(widen8(iq), n, 2.4e6))


# ---- 4. the host entries give the device entries' bits ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_frame_host_calls_of_every_size(dtype):
    """One frame (the small mapped call), 256 frames (chunks the kernel reads in place), and more than 32 MiB of input: at
    least two chunks through the three-slot pipeline with a ragged last one.  Pageable and pinned; repeated calls; a complex64
    and an int16 call around an 8-bit call are unchanged."""
    n = 4096
    big = (ZERO_COPY_MAX + (1 << 20)) // (2 * n) + 5
    x16 = stream16_planted(3, 4 * n).reshape(4, n, 2)
    with SpectrumPlan(n, window="hann", max_batch=big) as plan:
        for frames in (1, 256, big):
            x = stream8(frames, frames * n, dtype).reshape(frames, n, 2)
            assert frames != big or (x.nbytes > ZERO_COPY_MAX and frames % (HOST_CHUNK // (2 * n)) != 0)
            c = widen8(x)
            c64_before, i16_before = plan.spectrum_db(c[:4]), plan.spectrum_db_ci16(x16)
            with Pair8(x.reshape(-1, 2), frames, n) as d:
                dev = d.rows8(plan, frames, n)
            assert same_bits_f32(dev, plan.spectrum_db(c)), (dtype, frames, "device against complex64")
            got = plan.spectrum_db_ci8(x)
            assert same_bits_f32(got, dev), (dtype, frames, "pageable")
            assert same_bits_f32(plan.spectrum_db_ci8(x), got), (dtype, frames, "again")
            xp = pinned_empty(x.shape, dtype)
            xp[...] = x
            outp = pinned_empty((frames, n), np.float32)
            assert same_bits_f32(plan.spectrum_db_ci8(xp, out=outp), dev), (dtype, frames, "pinned in and out")
            assert same_bits_f32(plan.spectrum_db_ci8(xp), dev), (dtype, frames, "pinned in")
            del xp, outp
            if frames <= 256:
                assert same_bits(plan.fft_ci8(x), plan.fft(c)), (dtype, frames, "spectra")
            assert same_bits_f32(plan.spectrum_db(c[:4]), c64_before) and same_bits_f32(plan.spectrum_db_ci16(x16), i16_before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integrated_host_calls_of_every_size(dtype):
    """One frame, a mid-size call, and a call of three chunks of 2048 frames with groups across their boundaries."""
    n = 4096
    with SpectrumPlan(n, window="hann") as plan:
        for k, groups in ((1, 1), (8, 32), (101, 45)):
            iq = stream8(k + groups, groups * k * n, dtype)
            assert (k, groups) != (101, 45) or (iq.nbytes > 2 * HOST_CHUNK and (HOST_CHUNK // (2 * n)) % k != 0)
            iqp = pinned_empty(iq.shape, dtype)
            iqp[:] = iq
            c64_before = plan.integrate(widen8(iq[: 2 * n]), 2)
            with Pair8(iq, groups, n) as d:
                for det in DETECTORS:
                    dev = d.int8(plan, groups, k, n, det, "db")
                    assert same_bits_f32(dev, d.int64(plan, groups, k, n, det, "db")), (dtype, k, det)
                    assert same_bits_f32(plan.integrate_ci8(iq, k, n, det), dev), (dtype, k, det, "pageable")
                    assert same_bits_f32(plan.integrate_ci8(iqp, k, n, det), dev), (dtype, k, det, "pinned")
                    assert same_bits_f32(plan.integrate_ci8(iq, k, n, det), dev), (dtype, k, det, "again")
            assert same_bits_f32(plan.integrate(widen8(iq[: 2 * n]), 2), c64_before)
            del iqp


# ---- 5. absolute: the reference expression in float64 on the converted samples ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,frames", [(4096, 256), (1024, 6), (1000, 6)])
def test_rows_against_the_reference_expression_in_float64(dtype, n, frames):
    """20 log10(|fftshift(fft(x))| + 1e-12) in float64; the bars of the float32 path (tests/parity.py)."""
    x = stream8(900 + n, frames * n, dtype).reshape(frames, n, 2)
    off = 127.5 if dtype == np.uint8 else 0.0
    x64 = (x[..., 0].astype(np.float64) - off) + 1j * (x[..., 1].astype(np.float64) - off)
    for window, wref in ((None, None), ("hann", np.hanning(n))):
        got = pkg.spectrum_db_ci8(x, window=window)
        ref = cpu_ref.spectrum_db(x64, window=wref)
        assert ref.dtype == np.float64
        assert_db_parity(got, ref, what=f"ci8 {np.dtype(dtype).name} n={n} window={window}")
        worst = assert_db_parity_deep(got, ref, what=f"ci8 {np.dtype(dtype).name} n={n} window={window}")
        print(f"ci8 {np.dtype(dtype).name} n={n} window={window}: worst |delta dB| within 70 dB of the peak {worst:.3e}")


# ---- 6. many frames and units per workgroup -----------------------------------------------------------------------------------
CHILD_8_CUS = r"""
import numpy as np
import tests.ci8_helpers as h
for dtype in h.DTYPES:
    for frames in (1, 3, 777):
        h.case_4096_per_frame(dtype, frames)
    for k in (1, 2, 16):
        for groups in (1, 5):
            h.case_4096_integrated(dtype, k, groups)
    h.case_4096_integrated(dtype, 7, 30, windows=("hann",))
print("8 cus ok")
"""


def test_cases_1_and_3_on_the_24_workgroups_of_an_8_cu_grid():
    """SDRK_NUM_CUS=8 (the plans read it when they are made: a child process): 777 frames are 32 per workgroup, 30 unsplit
    units are more than the 24 resident workgroups."""
    run_child(CHILD_8_CUS, "8 cus ok", SDRK_NUM_CUS="8")


# ---- 7. a caller's stream -----------------------------------------------------------------------------------------------------
CHILD_STREAM = r"""
import torch, numpy as np
import tests.ci8_helpers as h
from tests.gpu_helpers import same_bits_f32
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
for dtype in h.DTYPES:
    for n, nf in ((4096, 333), (64, 999)):
        x = h.stream8(n + nf, nf * n, dtype)
        xt = torch.from_numpy(x).cuda()
        a = torch.empty((nf, n), dtype=torch.float32, device="cuda")
        b = torch.empty((nf // 3, n), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.current_stream().synchronize()
        with SpectrumPlan(n, window="hann", max_batch=1024) as plan:
            u = dtype == np.uint8
            plan.exec_device_ci8(xt.data_ptr(), nf, a.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_integrated_ci8(xt.data_ptr(), nf // 3, 3, b.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_ci8(xt.data_ptr(), nf, a.data_ptr(), unsigned=u)       # the plan's stream: ordered behind them
            s.synchronize(); plan.sync()
            c = h.widen8(x)
            assert same_bits_f32(a.cpu().numpy(), plan.spectrum_db(c.reshape(nf, n))), (dtype, n)
            assert same_bits_f32(b.cpu().numpy(), plan.integrate(c, 3)), (dtype, n, "integrated")
print("caller stream ok")
"""


def test_exec_device_ci8_on_a_caller_stream():
    """A fresh process (torch first: one HIP runtime): a torch stream, then the plan's own, at N = 4096 and through the route."""
    run_child(CHILD_STREAM, "caller stream ok")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_through_python_and_ctypes():
    lib = _ffi.lib()
    INVALID = _ffi.SDRK_ERR_INVALID
    ms2 = (ctypes.c_float * 2)()
    with SpectrumPlan(64, precision="double") as p64, DevBuf(1024) as d:
        for st in (lib.sdrk_exec_host_ci8(p64.handle, d.p, 0, 1, 64, d.p), lib.sdrk_exec_fft_host_ci8(p64.handle, d.p, 1, 1, 64, d.p),
                   lib.sdrk_exec_device_ci8(p64.handle, d.p, 0, 1, 64, d.p, None),
                   lib.sdrk_exec_device_ci8_timed_each(p64.handle, d.p, 0, 1, 64, d.p, 2, ms2),
                   lib.sdrk_exec_device_integrated_ci8(p64.handle, d.p, 1, 1, 1, 64, 0, 0, 1.0, d.p, None),
                   lib.sdrk_exec_device_integrated_ci8_timed_each(p64.handle, d.p, 1, 1, 1, 64, 0, 0, 1.0, d.p, 2, ms2),
                   lib.sdrk_exec_host_integrated_ci8(p64.handle, d.p, 0, 1, 1, 64, 0, 0, 1.0, d.p)):
            assert st == INVALID and b"float64" in lib.sdrk_last_error()
        for call in (lambda: p64.spectrum_db_ci8(np.zeros((64, 2), np.int8)), lambda: p64.fft_ci8(np.zeros((64, 2), np.uint8)),
                     lambda: p64.stft_db_ci8(np.zeros((64, 2), np.int8)), lambda: p64.integrate_ci8(np.zeros((64, 2), np.uint8), 1),
                     lambda: p64.exec_device_ci8(d.p.value, 1, d.p.value), lambda: p64.exec_device_integrated_ci8(d.p.value, 1, 1, d.p.value)):
            with pytest.raises(ValueError):
                call()
    with SpectrumPlan(64) as p, DevBuf(1024) as d:
        for fmt in (2, -1, 128):
            for st in (lib.sdrk_exec_host_ci8(p.handle, d.p, fmt, 1, 64, d.p), lib.sdrk_exec_fft_host_ci8(p.handle, d.p, fmt, 1, 64, d.p),
                       lib.sdrk_exec_device_ci8(p.handle, d.p, fmt, 1, 64, d.p, None),
                       lib.sdrk_exec_device_ci8_timed_each(p.handle, d.p, fmt, 1, 64, d.p, 2, ms2),
                       lib.sdrk_exec_device_integrated_ci8(p.handle, d.p, fmt, 1, 1, 64, 0, 0, 1.0, d.p, None),
                       lib.sdrk_exec_device_integrated_ci8_timed_each(p.handle, d.p, fmt, 1, 1, 64, 0, 0, 1.0, d.p, 2, ms2),
                       lib.sdrk_exec_host_integrated_ci8(p.handle, d.p, fmt, 1, 1, 64, 0, 0, 1.0, d.p)):
                assert st == INVALID and b"SDRK_IQ8_SIGNED" in lib.sdrk_last_error()
        # every refusal of the int16 twin, word for word
        for args in ((0, 1, 64, 0, 0), (1, 0, 64, 0, 0), (1, 1, 0, 0, 0), (1, 1, 64, 3, 0), (1, 1, 64, -1, 0), (1, 1, 64, 0, 2)):
            g, k, stride, det, form = args
            assert lib.sdrk_exec_device_integrated_ci8(p.handle, d.p, 1, g, k, stride, det, form, 1.0, d.p, None) == INVALID
            text = lib.sdrk_last_error()
            assert lib.sdrk_exec_device_integrated_ci16(p.handle, d.p, g, k, stride, det, form, 1.0, d.p, None) == INVALID
            assert lib.sdrk_last_error() == text
            assert lib.sdrk_exec_host_integrated_ci8(p.handle, d.p, 0, g, k, stride, det, form, 1.0, d.p) == INVALID
        for a_in, a_out, stride in ((None, d.p, 64), (d.p, None, 64), (d.p, d.p, 0)):
            assert lib.sdrk_exec_device_ci8(p.handle, a_in, 0, 2, stride, a_out, None) == INVALID
            text = lib.sdrk_last_error()
            assert lib.sdrk_exec_device_ci16(p.handle, a_in, 2, stride, a_out, None) == INVALID
            assert lib.sdrk_last_error() == text
            assert lib.sdrk_exec_host_ci8(p.handle, a_in, 1, 2, stride, a_out) == INVALID
        assert lib.sdrk_exec_device_ci8(None, d.p, 0, 1, 64, d.p, None) == INVALID
        assert lib.sdrk_exec_device_ci8_timed_each(p.handle, d.p, 0, 1, 64, d.p, 0, ms2) == INVALID
        for bad in (np.zeros(256, np.complex64), np.zeros((256, 2), np.int16), np.zeros((2, 128, 2), np.int8),
                    np.zeros((256, 4), np.uint8)[:, ::2], np.zeros((256, 2), np.int8).tolist()):
            with pytest.raises(ValueError):
                p.integrate_ci8(bad, 2)
            with pytest.raises(ValueError):
                p.stft_db_ci8(bad)
        for bad in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median"), dict(k=2, out="linear")):
            with pytest.raises(ValueError):
                p.integrate_ci8(np.zeros((256, 2), np.uint8), **bad)
        ms = p.exec_device_integrated_ci8_timed_each(d.p.value, 1, 1, d.p.value + 512, launches=3, unsigned=True)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        ms = p.exec_device_ci8_timed_each(d.p.value, 1, d.p.value + 512, launches=2)
        assert len(ms) == 2 and all(v > 0 for v in ms)
        for dtype in DTYPES:                                           # the refused plan still works
            iq = stream8(7, 6 * 64, dtype)
            assert same_bits_f32(p.integrate_ci8(iq, 3), p.integrate(widen8(iq), 3))
            assert same_bits_f32(p.stft_db_ci8(iq), p.stft_db(widen8(iq)))


# ---- 9. SigMF -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,datatype", [(np.int8, "ci8"), (np.uint8, "cu8")])
def test_sigmf_recording_read_natively_gives_the_default_readers_bits(tmp_path, dtype, datatype):
    n = 4096
    iq = stream8(12, 10 * n, dtype)
    base = str(tmp_path / datatype)
    sigmf_io.write_sigmf(base, iq, 2_400_000, 100_000_000, datatype=datatype)
    raw, meta = sigmf_io.read_sigmf(base, native="all")
    wide, _ = sigmf_io.read_sigmf(base)
    assert raw.dtype == dtype and raw.shape == (10 * n, 2) and np.array_equal(raw, iq)
    assert wide.dtype == np.complex64 and same_bits(wide, widen8(iq)) and meta["global"]["core:datatype"] == datatype
    assert same_bits_f32(pkg.spectrum_db_ci8(raw.reshape(10, n, 2), window="hann"), pkg.spectrum_db(wide.reshape(10, n), window="hann"))
    assert same_bits_f32(pkg.stft_db_ci8(raw, n, n // 2), pkg.stft_db(wide, n, n // 2))
    assert same_bits_f32(pkg.integrated_db_ci8(raw, n, 5), pkg.integrated_db(wide, n, 5))

"""Integrated spectra from int16 I,Q on the GPU: sdrk_exec_device_integrated_ci16 / sdrk_exec_host_integrated_ci16 and what
sits on them in spectrum.py and cli.py.

One sentence of semantics, so one kind of assertion: x = float32(I) + i float32(Q) exactly, then THE SAME BITS as the
complex64 integrated call of the same plan returns for ``iq.astype(float32).view(complex64)`` — every assertion below is
array_equal on the bit patterns against that call, except the absolute checks against float64 numpy on the integer samples
(bounds of tests/test_integrate_gpu.py: 1e-5 of the group's peak in amplitude, 0.01 dB within 70 dB of the row peak), which
keep the pair from being wrong together.  Inputs are random 12-bit int16 pairs with a tone."""
import ctypes
import json

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import (DevBuf, Pair, check_amplitude, ref_power, ref_reduced, run_child, same_bits_f32 as same_bits,
                               stream16_noise_tone as stream16, widen_flat as widen)
from tests.parity import assert_db_parity_deep

pytestmark = pytest.mark.gpu

DETECTORS = ("mean", "max", "min")
FORMS = ("db", "power")
EPS = 1e-12
HOST_CHUNK = 16 << 20      # plan_internal.h HOST_CHUNK_BYTES
INT_STAGE = 64 << 20       # integrate_call.h INT_STAGE_BYTES


# ---- the samples in float64, for the reference expressions of tests/gpu_helpers.py ------------------------------------------
def x64_of(iq):
    return iq[:, 0].astype(np.float64) + 1j * iq[:, 1].astype(np.float64)


# ---- 1. the N = 4096 kernel, device entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,groups,hop", [(1, 37, 4096), (3, 1000, 4096), (16, 5, 1001)])
def test_4096_device_entry_has_the_complex64_bits(k, groups, hop):
    """K = 1; more units than the resident grid; frame starts that are only 4-byte aligned, overlapped."""
    n = 4096
    iq = stream16(100 + k, n, groups * k, hop)
    with Pair(iq, groups, n) as d, DevBuf(groups * n * 4) as d_rows:
        for window, shift in (("hann", True), (None, True), ("hann", False), (None, False)):
            with SpectrumPlan(n, window=window, shift=shift, eps=EPS) as plan:
                rows = None
                if k == 1:
                    plan.exec_device_ci16(d.d16.p.value, groups, d_rows.p.value, frame_stride=hop)
                    plan.sync()
                    rows = d_rows.get((groups, n), np.float32)
                for det in DETECTORS:
                    for form in FORMS:
                        got = d.ci16(plan, groups, k, hop, det, form, 0.5)
                        assert same_bits(got, d.c64(plan, groups, k, hop, det, form, 0.5)), (window, shift, det, form)
                        assert np.all(np.isfinite(got)) and got.std() > 0
                        if rows is not None and form == "db":
                            assert same_bits(got, rows), (window, shift, det, "K = 1 against exec_device_ci16")


# ---- 2. slices, partial rows and the finalize; fewer resident workgroups than units ------------------------------------------
def test_one_group_of_64_frames_is_split_and_finalized():
    n, k = 4096, 64
    iq = stream16(2, n, k, n)
    with Pair(iq, 1, n) as d:
        for window in ("hann", None):
            with SpectrumPlan(n, window=window) as plan:
                for det in DETECTORS:
                    for form in FORMS:
                        assert same_bits(d.ci16(plan, 1, k, n, det, form, 0.5), d.c64(plan, 1, k, n, det, form, 0.5)), (window, det, form)


CHILD_8_CUS = r"""
import ctypes, numpy as np
import tests.gpu_helpers as h
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
n, k, groups = 4096, 7, 30
iq = h.stream16_noise_tone(8, n, groups * k, n)
with h.Pair(iq, groups, n) as d, SpectrumPlan(n, window="hann") as plan:
    for det in h.DETECTORS:
        for form in h.FORMS:
            assert h.same_bits_f32(d.ci16(plan, groups, k, n, det, form, 0.5), d.c64(plan, groups, k, n, det, form, 0.5)), (det, form)
print("8 cus ok")
"""


def test_30_groups_on_the_24_workgroups_of_an_8_cu_grid():
    """SDRK_NUM_CUS=8 (the plans read it when they are made: a child process): 30 unsplit units, 24 resident workgroups."""
    run_child(CHILD_8_CUS, "8 cus ok", SDRK_NUM_CUS="8")


# ---- 3. state carried from launch to launch: the host entry ------------------------------------------------------------------
def test_4096_host_entry_equals_device_entry_across_chunks():
    n, k, groups = 4096, 101, 25
    iq = stream16(3, n, groups * k, n)
    frames_per_chunk = HOST_CHUNK // (n * 4)
    assert iq.nbytes > 2 * HOST_CHUNK and frames_per_chunk == 1024 and frames_per_chunk % k != 0
    iqp = pinned_empty(iq.shape, np.int16)
    iqp[:] = iq
    with Pair(iq, groups, n) as d, SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            for form in FORMS:
                dev = d.ci16(plan, groups, k, n, det, form, 0.5)
                assert same_bits(dev, d.c64(plan, groups, k, n, det, form, 0.5)), (det, form)
                assert same_bits(plan.integrate_ci16(iq, k, n, det, form, 0.5), dev), (det, form, "pageable")
                assert same_bits(plan.integrate_ci16(iqp, k, n, det, form, 0.5), dev), (det, form, "pinned")


# ---- 4. every other length: the plan's int16 transform into the spectrum staging ---------------------------------------------
@pytest.mark.parametrize("n,k,groups", [(1024, 100, 45), (64, 7, 2000), (65536, 3, 4), (1000, 5, 6), (128, 9, 50)])
def test_generic_route_device_and_host_entries(n, k, groups):
    """fft_lds reading int16 (1024), the widening route (64, 128, 65536) and chirp-z (1000)."""
    iq = stream16(n + k, n, groups * k, n)
    with Pair(iq, groups, n) as d, SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            for form in FORMS:
                want = d.c64(plan, groups, k, n, det, form, 0.5)
                assert same_bits(d.ci16(plan, groups, k, n, det, form, 0.5), want), (n, det, form, "device")
                assert same_bits(plan.integrate_ci16(iq, k, n, det, form, 0.5), want), (n, det, form, "host")


def test_generic_route_call_larger_than_the_spectrum_staging():
    n, k, groups = 1024, 3000, 3
    frames, stage_frames = groups * k, INT_STAGE // (n * 8)
    assert frames * n * 8 > INT_STAGE                                  # 70 MiB of complex64 spectra
    assert (stage_frames // k) * k < stage_frames < (stage_frames // k + 1) * k <= frames   # group 2 straddles the boundary
    iq = stream16(5, n, frames, n)
    with Pair(iq, groups, n) as d, SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            want = d.c64(plan, groups, k, n, det, "power", 0.5)
            assert same_bits(d.ci16(plan, groups, k, n, det, "power", 0.5), want), det
            assert same_bits(plan.integrate_ci16(iq, k, n, det, "power", 0.5), want), (det, "host")


# ---- 5. absolute: float64 numpy on the integer samples -----------------------------------------------------------------------
def test_4096_rows_against_numpy_in_float64_on_the_integer_samples():
    n, k, groups = 4096, 16, 3
    iq = stream16(6, n, groups * k, n, tone_db=20.0)
    p = ref_power(x64_of(iq), n, groups * k, n, "hann", True)
    with Pair(iq, groups, n) as d, SpectrumPlan(n, window="hann", eps=EPS) as plan:
        for det in DETECTORS:
            for form in FORMS:
                check_amplitude(d.ci16(plan, groups, k, n, det, form), form, p, groups, k, det, f"ci16 K=16 {det} {form}")
            ref = 20 * np.log10(np.sqrt(ref_reduced(p, groups, k, det)) + EPS)
            got = d.ci16(plan, groups, k, n, det)
            d_db = np.abs(got.astype(np.float64) - ref)[ref >= ref.max(axis=-1, keepdims=True) - 70.0]
            print(f"ci16 K=16 {det}: worst |delta dB| within 70 dB of the row peak {d_db.max():.2e} ({d_db.size} bins)")
            assert_db_parity_deep(got, ref, what=f"ci16 K=16 {det}")
            assert_db_parity_deep(plan.integrate_ci16(iq, k, n, det), ref, what=f"ci16 host K=16 {det}")


# ---- 6. module functions, repeated calls, a caller's stream ------------------------------------------------------------------
def test_module_functions_match_their_complex64_counterparts():
    for n, hop, frames in ((4096, 4096, 40), (4096, 1000, 50), (1024, 512, 90), (1000, 1000, 12)):
        iq = stream16(n + hop, n, frames, hop)
        iq = np.ascontiguousarray(np.concatenate([iq, iq[: hop // 3]]))            # a partial trailing frame: dropped
        wide = widen(iq)
        for det in DETECTORS:
            a = pkg.integrated_db_ci16(iq, n, 8, hop, detector=det, window="hann")
            assert a.shape == (frames // 8, n)
            assert same_bits(a, pkg.integrated_db(wide, n, 8, hop, detector=det, window="hann")), (n, hop, det)
            assert same_bits(a, pkg.integrated_db_ci16(iq, n, 8, hop, detector=det, window="hann")), (n, hop, det, "again")
        for shift in (True, False):
            w = pkg.welch_psd_streamed_ci16(iq, n, 2.4e6, hop=hop, shift=shift)
            assert w.shape == (n,)
            assert same_bits(w, pkg.welch_psd_streamed(wide, n, 2.4e6, hop=hop, shift=shift)), (n, hop, shift)
            assert same_bits(w, pkg.welch_psd_streamed_ci16(iq, n, 2.4e6, hop=hop, shift=shift)), (n, hop, shift, "again")
    with pytest.raises(ValueError, match="shorter"):
        pkg.welch_psd_streamed_ci16(np.zeros((100, 2), np.int16), 1024, 1e6)
    from sdr_iq_visualizer_amd import processing
    assert processing.integrated_db_ci16 is pkg.integrated_db_ci16 and processing.welch_psd_streamed_ci16 is pkg.welch_psd_streamed_ci16


CHILD_STREAM = r"""
import torch, numpy as np
import tests.gpu_helpers as h
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
for n, k, groups in ((4096, 5, 40), (4096, 64, 1), (1024, 9, 30), (64, 4, 100)):
    iq = h.stream16_noise_tone(n + k, n, groups * k, n)
    xt = torch.from_numpy(iq).cuda()
    a = torch.empty((groups, n), dtype=torch.float32, device="cuda")
    b = torch.empty((groups, n), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with SpectrumPlan(n, window="hann") as plan:
        for det in h.DETECTORS:
            plan.exec_device_integrated_ci16(xt.data_ptr(), groups, k, a.data_ptr(), detector=det, stream=s.cuda_stream)
            plan.exec_device_integrated_ci16(xt.data_ptr(), groups, k, b.data_ptr(), detector=det)   # the plan's: ordered behind it
            s.synchronize(); plan.sync()
            ref = plan.integrate(h.widen_flat(iq), k, n, det)
            assert h.same_bits_f32(a.cpu().numpy(), ref) and h.same_bits_f32(b.cpu().numpy(), ref), (n, k, det)
print("caller stream ok")
"""


def test_a_caller_stream_gives_the_plan_streams_bits():
    """A fresh process (torch first: one HIP runtime): a torch stream, then the plan's own, on one plan's state and staging."""
    run_child(CHILD_STREAM, "caller stream ok")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device():
    lib = _ffi.lib()
    with SpectrumPlan(64, precision="double") as p64, DevBuf(1024) as d:
        ms2 = (ctypes.c_float * 2)()
        for st in (lib.sdrk_exec_device_integrated_ci16(p64.handle, d.p, 1, 1, 64, 0, 0, 1.0, d.p, None),
                   lib.sdrk_exec_host_integrated_ci16(p64.handle, d.p, 1, 1, 64, 0, 0, 1.0, d.p),
                   lib.sdrk_exec_device_integrated_ci16_timed_each(p64.handle, d.p, 1, 1, 64, 0, 0, 1.0, d.p, 2, ms2)):
            assert st == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        with pytest.raises(ValueError):
            p64.integrate_ci16(np.zeros((64, 2), np.int16), 1)
        with pytest.raises(ValueError):
            p64.exec_device_integrated_ci16(d.p.value, 1, 1, d.p.value)
    with SpectrumPlan(64) as p, DevBuf(1024) as d:
        for args in ((0, 1, 64, 0, 0), (1, 0, 64, 0, 0), (1, 1, 0, 0, 0), (1, 1, 64, 3, 0), (1, 1, 64, -1, 0), (1, 1, 64, 0, 2)):
            g, k, stride, det, form = args
            assert lib.sdrk_exec_device_integrated_ci16(p.handle, d.p, g, k, stride, det, form, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
            text = lib.sdrk_last_error()
            assert lib.sdrk_exec_device_integrated(p.handle, d.p, g, k, stride, det, form, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
            assert lib.sdrk_last_error() == text                     # the refusals are check_int_args's, word for word
            assert lib.sdrk_exec_host_integrated_ci16(p.handle, d.p, g, k, stride, det, form, 1.0, d.p) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_integrated_ci16(p.handle, None, 1, 1, 64, 0, 0, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_integrated_ci16(p.handle, d.p, 1, 1, 64, 0, 0, 1.0, None, None) == _ffi.SDRK_ERR_INVALID
        for bad in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median"), dict(k=2, out="linear")):
            with pytest.raises(ValueError):
                p.integrate_ci16(np.zeros((256, 2), np.int16), **bad)
        for bad in (np.zeros(256, np.complex64), np.zeros((256, 2), np.int32), np.zeros((2, 128, 2), np.int16),
                    np.zeros((256, 4), np.int16)[:, ::2], np.zeros((256, 2), np.int16).tolist()):
            with pytest.raises(ValueError):
                p.integrate_ci16(bad, 2)
        ms = p.exec_device_integrated_ci16_timed_each(d.p.value, 1, 1, d.p.value + 512, launches=3)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        iq = stream16(7, 64, 6, 64)                                  # the refused plan still works
        assert same_bits(p.integrate_ci16(iq, 3), p.integrate(widen(iq), 3))


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_psd_integrate_on_a_ci16_recording(tmp_path, capsys):
    iq = stream16(8, 4096, 43, 4096)
    base = str(tmp_path / "rec16")
    sigmf_io.write_sigmf(base, iq, 2_000_000, 915_000_000, datatype="ci16_le")
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", "8", "--detector", "max", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["integrated_rows"] == 5 and report["integrate_k"] == 8 and report["integrate_detector"] == "max"
    wide, _ = sigmf_io.read_sigmf(base)
    assert wide.dtype == np.complex64
    with np.load(out) as z:
        assert z["integrated_db"].shape == (5, 4096)
        assert same_bits(z["integrated_db"], pkg.integrated_db(wide, 4096, 8, detector="max"))
        assert same_bits(z["power_db"], pkg.spectrum_db(wide[:4096]))


# ---- 9. device memory does not grow with the stream ------------------------------------------------------------------------------
def test_device_memory_of_a_512_mib_host_call_is_bounded():
    """2^27 int16 samples at N = 4096: three staging slots of 16 MiB input + at most 16 MiB rows, two carry rows and the
    partial rows of split groups — under the 192 MiB cap of the complex64 test (whose input is twice the bytes)."""
    n, k = 4096, 64
    block = stream16(9, n, 32, n, tone_db=20.0)
    iq = np.tile(block, ((1 << 27) // block.shape[0], 1))
    assert iq.shape[0] == 1 << 27 and iq.nbytes == 512 << 20
    groups = iq.shape[0] // n // k
    free0, free1, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    with SpectrumPlan(n, window="hann") as plan:
        plan.integrate_ci16(iq[: n * k], k)                     # (first call: the runtime's own allocations)
        _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free0), ctypes.byref(total)))
        rows = plan.integrate_ci16(iq, k, detector="mean", out="power")
        _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free1), ctypes.byref(total)))
    held = int(free0.value) - int(free1.value)
    print(f"device memory taken by the 512 MiB int16 call: {held / 2**20:.1f} MiB")
    assert held <= 192 << 20, held
    p = ref_power(x64_of(np.concatenate([block, block])), n, k, n, "hann", True)
    assert rows.shape == (groups, n)
    check_amplitude(rows[[0, groups // 2, groups - 1]], "power", np.tile(p, (3, 1)), 3, k, "mean", "512 MiB int16")

"""The polyphase filter bank and spectral kurtosis from 8-bit I,Q on the GPU (sdrk_exec_*_pfb_iq8, _pfb_integrated_iq8,
_kurtosis_iq8, _pfb_kurtosis_iq8): 2 bytes per sample, SigMF ci8 (int8) and cu8 (uint8, mid-scale 127.5), widened exactly, and
then the bits of the complex64 entry points.

Every check is in bits: the 8-bit call against the existing complex64 call of the SAME plan on widen8(x) (tests.ci8_helpers),
for both byte types, on streams over the full byte range with the edge bytes planted (stream8).  One case is also held against
float64 numpy with test_sk_gpu.py's bounds, so that the chain does not rest on the complex64 kernels alone.  The device
buffers start their first sample at byte 2 and end in a canary row (tests.iq8_modes_helpers.Dev8)."""
import ctypes
import json

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
from tests import iq8_modes_helpers as h
from tests.ci8_helpers import DTYPES, EDGE_BYTES, stream8, widen8
from tests.gpu_helpers import EPS, held_during, ref_power, run_child, same_bits, same_bits_f32

pytestmark = pytest.mark.gpu

N4K, G3, SCALE = h.N4K, h.G3, h.SCALE


def test_the_inputs_hold_what_the_checks_rely_on():
    for dtype in DTYPES:
        x = stream8(1, 4096, dtype)
        assert x.dtype == dtype and x.shape == (4096, 2) and set(EDGE_BYTES) <= set(x.view(np.uint8).reshape(-1))
        w = widen8(x)
        off = np.float32(127.5 if dtype == np.uint8 else 0)
        assert np.array_equal(w.real, x[:, 0].astype(np.float32) - off) and np.array_equal(w.imag, x[:, 1].astype(np.float32) - off)


# ---- 1. N = 4096, per frame ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps,frames,hop,shift,proto", h.PER_FRAME_4096)
def test_n4096_per_frame_has_the_complex64_bits(dtype, taps, frames, hop, shift, proto):
    h.case_per_frame(dtype, N4K, taps, frames, hop, shift, proto)


@pytest.mark.parametrize("assign", ["0", "1", "2"])
def test_n4096_rows_do_not_depend_on_the_frame_assignment(assign, monkeypatch):
    monkeypatch.setenv("SDRK_PFB_ASSIGN", assign)     # read when the prototype is set
    for dtype in DTYPES:
        for frames, hop in ((13, N4K // 4), (769, G3)):
            h.case_per_frame(dtype, N4K, 4, frames, hop, True, "random", seed=11, spectra=False)


# ---- 2. N = 4096, integrated ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps,k,groups,hop,shift,proto", h.INTEGRATED_4096)
def test_n4096_integrated_has_the_complex64_bits(dtype, taps, k, groups, hop, shift, proto):
    h.case_integrated(dtype, N4K, taps, k, groups, hop, shift, proto)


# ---- 3. N = 4096, spectral kurtosis --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,groups,hop", h.SK_4096)
def test_n4096_kurtosis_has_the_complex64_bits(dtype, k, groups, hop):
    h.case_sk(dtype, N4K, k, groups, hop)


@pytest.mark.parametrize("dtype", DTYPES)
def test_n4096_kurtosis_against_float64_numpy(dtype):
    k, groups, hop = 5, 40, N4K
    iq = stream8(17, (groups * k - 1) * hop + N4K, dtype)
    p = ref_power(widen8(iq), N4K, groups * k, hop, "hann", True)
    with SpectrumPlan(N4K, window="hann", eps=EPS) as plan:
        with h.Dev8(iq, groups, 2 * N4K) as d:
            for form, scale in (("db", 1.0), ("power", SCALE)):
                got = d.run(plan, groups, 2 * N4K, lambda o: plan.exec_device_sk_ci8(d.p8, groups, k, o, unsigned=d.unsigned, frame_stride=hop,
                                                                                     out=form, scale=scale))
                h.check_planes(got.reshape(groups, 2, N4K), form, scale, p, groups, k, f"{np.dtype(dtype).name} {form}")
        mean_rows, sk_rows = plan.spectral_kurtosis_ci8(iq, k, hop)
        h.check_planes(mean_rows.base, "db", 1.0, p, groups, k, f"{np.dtype(dtype).name} host")


# ---- 4. other lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,taps,frames,hop", [(64, 3, 5, 1), (1000, 3, 7, 1500), (1024, 8, 6, 256), (65536, 3, 5, 32768)])
def test_other_lengths_per_frame_have_the_complex64_bits(dtype, n, taps, frames, hop):
    h.case_per_frame(dtype, n, taps, frames, hop, bool(taps & 1), "random" if n != 1000 else "default")


@pytest.mark.parametrize("dtype", DTYPES)
def test_1024_integrated_over_two_staging_chunks_and_a_carried_unit(dtype):
    h.case_integrated(dtype, 1024, 3, 2, 4500, 512, True, "default")       # 9000 folded frames: two chunks of the 64 MiB staging


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,groups,hop", [(1024, 9, 7, 512), (1000, 4, 3, 1000)])
def test_other_lengths_kurtosis_has_the_complex64_bits(dtype, n, k, groups, hop):
    h.case_sk(dtype, n, k, groups, hop)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,taps,k,groups,hop", [(1024, 4, 6, 5, 512), (1000, 3, 3, 4, 1000), (4096, 4, 5, 6, 4096)])
def test_kurtosis_behind_the_filter_bank_has_the_complex64_bits(dtype, n, taps, k, groups, hop):
    h.case_pfb_sk(dtype, n, taps, k, groups, hop)          # (N = 4096 too: the staged route, there is no folding SK kernel)


# ---- 5. the numpy boundary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entries_return_the_device_entries_bits_in_bounded_memory(dtype):
    """~25 MB of bytes at T = 4: the per-frame boundary aims at a quarter of the call per chunk — four chunks, each carrying
    3 * 4096 samples of overlap.  The integrated calls cut at 16 MiB of input (2048 frames): K = 7 divides no chunk."""
    taps, k, frames, hop = 4, 7, 3000, N4K
    L = (frames - 1) * hop + taps * N4K
    base = stream8(5, 64 * N4K + 1, dtype)
    x = np.ascontiguousarray(np.tile(base, (L // base.shape[0] + 1, 1))[:L])
    groups = frames // k
    plain_groups = (L // N4K) // k
    with SpectrumPlan(N4K, eps=EPS) as plan, h.Dev8(x, frames, N4K) as d:
        plan.set_pfb(pfb_prototype(N4K, taps))
        u = d.unsigned
        small = x[: (k - 1) * hop + taps * N4K]
        rows = lambda call, count, floats: d.run(plan, count, floats, call)
        dev = rows(lambda o: plan.exec_device_pfb_ci8(d.p8, frames, o, unsigned=u, frame_stride=hop), frames, N4K)
        host, held = held_during(lambda: plan.pfb_db_ci8(x, hop), lambda: plan.pfb_db_ci8(x[: taps * N4K]))
        print(f"{np.dtype(dtype).name}: device memory taken by the per-frame host call {held / 2**20:.1f} MiB")
        assert held <= 192 << 20, held
        assert same_bits_f32(host, dev)
        xp = pinned_empty(x.shape, dtype)
        xp[...] = x
        out = pinned_empty((frames, N4K), np.float32)
        assert plan.pfb_db_ci8(xp, hop, out=out) is out and same_bits_f32(out, dev)
        # the device rows are the complex64 call's
        nf = 300
        got, want = d.pfb(plan, nf, hop)
        assert same_bits_f32(got, want) and same_bits_f32(got, dev[:nf])
        for det in ("mean", "max"):
            dev_i = rows(lambda o: plan.exec_device_pfb_integrated_ci8(d.p8, groups, k, o, unsigned=u, frame_stride=hop, detector=det,
                                                                       scale=SCALE), groups, N4K)
            host_i, held = held_during(lambda: plan.pfb_integrate_ci8(x, k, hop, det, "db", SCALE), lambda: plan.pfb_integrate_ci8(small, k, hop, det))
            assert held <= 192 << 20, held
            assert same_bits_f32(host_i, dev_i), det
            assert same_bits_f32(plan.pfb_integrate_ci8(xp, k, hop, det, "db", SCALE), dev_i), det
        dev_s = rows(lambda o: plan.exec_device_pfb_sk_ci8(d.p8, groups, k, o, unsigned=u, frame_stride=hop), groups, 2 * N4K)
        host_s, held = held_during(lambda: plan.pfb_spectral_kurtosis_ci8(x, k, hop)[0].base, lambda: plan.pfb_spectral_kurtosis_ci8(small, k, hop))
        assert held <= 192 << 20, held
        assert same_bits_f32(host_s.reshape(groups, -1), dev_s)
        assert same_bits_f32(plan.pfb_spectral_kurtosis_ci8(xp, k, hop)[0].base.reshape(groups, -1), dev_s)
        dev_k = rows(lambda o: plan.exec_device_sk_ci8(d.p8, plain_groups, k, o, unsigned=u, frame_stride=hop), plain_groups, 2 * N4K)
        host_k, held = held_during(lambda: plan.spectral_kurtosis_ci8(x, k, hop)[0].base, lambda: plan.spectral_kurtosis_ci8(small, k, hop))
        assert held <= 192 << 20, held
        assert same_bits_f32(host_k.reshape(plain_groups, -1), dev_k)
        assert same_bits_f32(plan.spectral_kurtosis_ci8(xp, k, hop)[0].base.reshape(plain_groups, -1), dev_k)
        gp = 40      # ... and the complex64 calls' on a prefix
        for pfb, dev_rows in ((True, dev_s), (False, dev_k)):
            got, want = d.sk(plan, gp, k, hop, "db", pfb=pfb)      # (scale does not touch the dB form)
            assert same_bits_f32(got, want) and same_bits_f32(got, dev_rows[:gp])


# ---- 6. housekeeping -----------------------------------------------------------------------------------------------------------
CHILD_8_CUS = r"""
import tests.iq8_modes_helpers as h
for dtype in h.DTYPES:
    h.cases_4096(dtype)
print("8 cus ok")
"""


def test_the_n4096_cases_on_the_24_workgroups_of_an_8_cu_grid():
    """SDRK_NUM_CUS=8 (the plans read it when they are made: a fresh child process): 1700 frames are 70 per workgroup, 40 and 800
    units are more than the 24 resident workgroups, other split factors."""
    run_child(CHILD_8_CUS, "8 cus ok", SDRK_NUM_CUS="8")


CHILD_STREAM = r"""
import torch, numpy as np
import tests.iq8_modes_helpers as h
from tests.gpu_helpers import same_bits_f32
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
T, K = 3, 4
for dtype in h.DTYPES:
    for n, nf in ((4096, 333), (1024, 999)):
        x = h.stream8(n + nf, (nf + T - 1) * n, dtype)
        xt = torch.from_numpy(x).cuda()
        a = torch.empty((nf, n), dtype=torch.float32, device="cuda")
        b = torch.empty((nf // K, n), dtype=torch.float32, device="cuda")
        c = torch.empty((nf // K, 2, n), dtype=torch.float32, device="cuda")
        e = torch.empty((nf // K, 2, n), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.current_stream().synchronize()
        with SpectrumPlan(n) as plan:
            plan.set_pfb(pfb_prototype(n, T))
            u = dtype == np.uint8
            plan.exec_device_pfb_ci8(xt.data_ptr(), nf, a.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_pfb_integrated_ci8(xt.data_ptr(), nf // K, K, b.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_sk_ci8(xt.data_ptr(), nf // K, K, c.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_pfb_sk_ci8(xt.data_ptr(), nf // K, K, e.data_ptr(), unsigned=u, stream=s.cuda_stream)
            plan.exec_device_pfb_ci8(xt.data_ptr(), nf, a.data_ptr(), unsigned=u)       # the plan's stream: ordered behind them
            s.synchronize(); plan.sync()
            w = h.widen8(x)
            assert same_bits_f32(a.cpu().numpy(), plan.pfb_db(w)), (dtype, n)
            assert same_bits_f32(b.cpu().numpy(), plan.pfb_integrate(w, K)), (dtype, n, "integrated")
            assert same_bits_f32(c.cpu().numpy(), plan.spectral_kurtosis(w[: nf * n], K)[0].base), (dtype, n, "kurtosis")
            assert same_bits_f32(e.cpu().numpy(), plan.pfb_spectral_kurtosis(w, K)[0].base), (dtype, n, "pfb kurtosis")
print("caller stream ok")
"""


def test_the_device_entries_on_a_caller_stream():
    """A fresh process (torch first: one HIP runtime): a torch stream, then the plan's own, at N = 4096 and through the stagings."""
    run_child(CHILD_STREAM, "caller stream ok")


def test_refusals_on_a_device_and_the_plan_still_works():
    lib = _ffi.lib()
    n = 256
    hp = pfb_prototype(n, 2)
    x = stream8(1, 6 * n, np.uint8)
    out = np.empty((2, 2, n), np.float32)
    outc = np.empty((2, n), np.complex64)
    xp, op, ocp = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, out, outc))
    ms = (ctypes.c_float * 2)()
    f = ctypes.c_float(1.0)

    def refused(status, says=None):
        assert status == _ffi.SDRK_ERR_INVALID, status
        assert lib.sdrk_last_error() and (says is None or says in lib.sdrk_last_error()), lib.sdrk_last_error()

    def every_pfb(handle, says=None, fmt=1, iq=xp, frames=2, rows=op, rows_c=ocp, stride=n):
        refused(lib.sdrk_exec_device_pfb_iq8(handle, iq, fmt, frames, stride, rows, None), says)
        refused(lib.sdrk_exec_device_pfb_iq8_timed_each(handle, iq, fmt, frames, stride, rows, 2, ms), says)
        refused(lib.sdrk_exec_host_pfb_iq8(handle, iq, fmt, frames, stride, rows), says)
        refused(lib.sdrk_exec_fft_host_pfb_iq8(handle, iq, fmt, frames, stride, rows_c), says)
        groups, k = (1, 2) if frames == 2 else (0, 2)
        refused(lib.sdrk_exec_device_pfb_integrated_iq8(handle, iq, fmt, groups, k, stride, 0, 0, f, rows, None), says)
        refused(lib.sdrk_exec_device_pfb_integrated_iq8_timed_each(handle, iq, fmt, groups, k, stride, 0, 0, f, rows, 2, ms), says)
        refused(lib.sdrk_exec_host_pfb_integrated_iq8(handle, iq, fmt, groups, k, stride, 0, 0, f, rows), says)
        refused(lib.sdrk_exec_device_pfb_kurtosis_iq8(handle, iq, fmt, groups, k, stride, 0, f, rows, None), says)
        refused(lib.sdrk_exec_device_pfb_kurtosis_iq8_timed_each(handle, iq, fmt, groups, k, stride, 0, f, rows, 2, ms), says)
        refused(lib.sdrk_exec_host_pfb_kurtosis_iq8(handle, iq, fmt, groups, k, stride, 0, f, rows), says)

    def every_plain(handle, says=None, fmt=0, iq=xp, groups=1, k=2, rows=op, stride=n, form=0):
        refused(lib.sdrk_exec_device_kurtosis_iq8(handle, iq, fmt, groups, k, stride, form, f, rows, None), says)
        refused(lib.sdrk_exec_device_kurtosis_iq8_timed_each(handle, iq, fmt, groups, k, stride, form, f, rows, 2, ms), says)
        refused(lib.sdrk_exec_host_kurtosis_iq8(handle, iq, fmt, groups, k, stride, form, f, rows), says)

    with SpectrumPlan(n, window="hann") as windowed, SpectrumPlan(n, precision="double") as f64, SpectrumPlan(n) as plan:
        every_pfb(windowed.handle, b"SDRK_WINDOW_RECT")             # the int16 twins' refusals, in their words
        every_pfb(f64.handle, b"float32 plans only")
        every_pfb(plan.handle, b"sdrk_plan_set_pfb")                # no prototype set
        every_plain(f64.handle)
        assert plan.set_pfb(hp) == 2
        for fmt in (2, -1, 255):
            every_pfb(plan.handle, b"is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED", fmt=fmt)
            every_plain(plan.handle, b"is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED", fmt=fmt)
        every_pfb(None)
        every_pfb(plan.handle, iq=None)
        every_pfb(plan.handle, rows=None, rows_c=None)
        every_pfb(plan.handle, frames=0)
        every_pfb(plan.handle, stride=0)                            # stride 0 with more than one frame
        every_plain(None)
        every_plain(plan.handle, iq=None)
        every_plain(plan.handle, rows=None)
        every_plain(plan.handle, groups=0)
        every_plain(plan.handle, k=1)                               # the estimator divides by K - 1
        every_plain(plan.handle, stride=0)
        every_plain(plan.handle, form=2)
        refused(lib.sdrk_exec_device_pfb_iq8_timed_each(plan.handle, xp, 1, 2, n, op, 0, ms))
        refused(lib.sdrk_exec_device_kurtosis_iq8_timed_each(plan.handle, xp, 1, 1, 2, n, 0, f, op, 2, None))
        refused(lib.sdrk_exec_host_pfb_integrated_iq8(plan.handle, xp, 1, 1, 2, n, 7, 0, f, op))
        refused(lib.sdrk_exec_host_pfb_integrated_iq8(plan.handle, xp, 1, 1, 2, n, 0, 9, f, op))
        refused(lib.sdrk_exec_host_pfb_kurtosis_iq8(plan.handle, xp, 1, 1, 1, n, 0, f, op))
        # the refused plan still works
        w = widen8(x)
        assert lib.sdrk_exec_host_pfb_iq8(plan.handle, xp, 1, 2, n, op) == 0
        assert same_bits_f32(out.reshape(-1)[: 2 * n].reshape(2, n), plan.pfb_db(w)[:2])
        assert lib.sdrk_exec_host_kurtosis_iq8(plan.handle, xp, 1, 2, 3, n, 0, f, op) == 0
        assert same_bits_f32(out, plan.spectral_kurtosis(w, 3)[0].base)
        assert same_bits_f32(windowed.spectral_kurtosis_ci8(x, 3)[1], windowed.spectral_kurtosis(w, 3)[1])
        # Python-side refusals
        with pytest.raises(ValueError):
            windowed.pfb_integrate_ci8(x, 2)
        with pytest.raises(ValueError):
            f64.spectral_kurtosis_ci8(x, 2)
        with pytest.raises(ValueError):
            plan.pfb_db_ci8(w)
        with pytest.raises(ValueError):
            plan.pfb_spectral_kurtosis_ci8(x.astype(np.int16), 2)


def test_existing_rows_of_the_same_plan_are_unchanged_by_the_new_calls():
    taps, frames, k = 4, 12, 3
    x = stream8(31, (frames - 1) * N4K + taps * N4K, np.int8)
    xw = widen8(x)
    x16 = np.ascontiguousarray(x.astype(np.int16))
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(pfb_prototype(N4K, taps))
        existing = lambda: (plan.pfb_db(xw), plan.pfb_db_ci16(x16), plan.integrate_ci8(x, k), plan.spectral_kurtosis(xw, k)[0].base)
        before = existing()
        new = (plan.pfb_db_ci8(x), plan.pfb_fft_ci8(x), plan.pfb_integrate_ci8(x, k, detector="max"), plan.spectral_kurtosis_ci8(x, k)[0].base,
               plan.pfb_spectral_kurtosis_ci8(x, k)[0].base)
        after = existing()
        for b, a in zip(before, after):
            assert same_bits(b, a)
        assert same_bits(new[0], before[0]) and same_bits(new[0], before[1]) and same_bits(new[3], before[3])
        assert same_bits(new[1], plan.pfb_fft(xw)) and same_bits(new[2], plan.pfb_integrate(xw, k, detector="max"))
        assert same_bits(new[4], plan.pfb_spectral_kurtosis(xw, k)[0].base)


def test_cli_psd_pfb_integrate_sk_on_8_bit_recordings_reports_what_cf32_reports(tmp_path, capsys):
    n, taps, k = 4096, 4, 8
    reports, arrays = {}, {}
    for dtype, datatype in ((np.uint8, "cu8"), (np.int8, "ci8")):
        iq = stream8(8, (taps + 2 * k) * n + 100, dtype)
        for name, samples, kw in ((datatype, iq, dict(datatype=datatype)), (datatype + "_cf32", widen8(iq), {})):
            base = str(tmp_path / name)
            sigmf_io.write_sigmf(base, samples, 2_000_000, 915_000_000, **kw)
            out = str(tmp_path / (name + ".npz"))
            assert cli.main(["psd", base + ".sigmf-meta", "--pfb", str(taps), "--integrate", str(k), "--sk", "--out", out]) == 0
            reports[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
            assert reports[name].pop("out") == out
            with np.load(out) as z:
                arrays[name] = {key: z[key] for key in z.files}
        r = reports[datatype]
        assert r == reports[datatype + "_cf32"], (r, reports[datatype + "_cf32"])
        assert r["pfb_taps"] == taps and r["pfb_rows"] == 2 * k + 1 and r["pfb_integrated_rows"] == 2 and r["sk_rows"] == 2
        assert sorted(arrays[datatype]) == sorted(arrays[datatype + "_cf32"])
        for key, a in arrays[datatype].items():
            assert same_bits(a, arrays[datatype + "_cf32"][key]), (datatype, key)
        assert same_bits(arrays[datatype]["pfb_db"], pkg.pfb_db_ci8(iq, n, taps))
        assert same_bits(arrays[datatype]["pfb_integrated_db"], pkg.pfb_integrated_db_ci8(iq, n, taps, k))
        assert same_bits(arrays[datatype]["sk"], pkg.pfb_spectral_kurtosis(iq, n, taps, k)[1])
        assert same_bits(pkg.spectral_kurtosis_ci8(iq, n, k)[1], pkg.spectral_kurtosis(widen8(iq), n, k)[1])

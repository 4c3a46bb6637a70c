"""Polyphase filter bank spectra from int16 I,Q on the GPU (sdrk_exec_*_pfb_ci16, sdrk_exec_*_pfb_integrated_ci16): 4 bytes
per sample, x[n] = float32(I[n]) + i float32(Q[n]) exactly, and then the bits of the complex64 PFB entry points.

Every check is in bits (uint32 views): the int16 call against the complex64 PFB call of the SAME plan on the widened array;
one case also against the plan's spectrum_db of numpy's float32 fold of the widened samples, so that the chain does not rest
on the complex64 PFB alone.  Inputs cover the full int16 range: random values with planted -32768, 32767, -1, 0 and pairs of
opposite sign (I < 0 <= Q and the reverse) — a wrong sign extension of the low half shows in the first row."""
import ctypes
import json

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
from tests.gpu_helpers import (DevBuf, fold32, held_during, prototype, run_child, same_bits, stream16_planted as stream16,
                               widen_flat as widen)

pytestmark = pytest.mark.gpu

EPS = 1e-12
N4K = 4096
G3 = N4K + N4K // 3 + 1          # an odd, gapped hop
DETECTORS = ("mean", "max", "min")
FORMS = ("db", "power")
SCALE = 0.37

def test_the_inputs_hold_what_the_checks_rely_on():
    x = stream16(1, 4096)
    assert x.min() == -32768 and x.max() == 32767
    assert ((x[:, 0] < 0) & (x[:, 1] >= 0)).any() and ((x[:, 0] >= 0) & (x[:, 1] < 0)).any()
    w = widen(x)
    assert np.array_equal(w.real, x[:, 0].astype(np.float32)) and np.array_equal(w.imag, x[:, 1].astype(np.float32))


def dev_rows(plan, x, frames, hop, ci16):
    with DevBuf(x.nbytes) as d_in, DevBuf(frames * plan.nfft * 4) as d_out:
        d_in.put(x)
        (plan.exec_device_pfb_ci16 if ci16 else plan.exec_device_pfb)(d_in.p.value, frames, d_out.p.value, frame_stride=hop)
        plan.sync()
        return d_out.get((frames, plan.nfft), np.float32)


def dev_int_rows(plan, x, groups, k, hop, det, form, ci16):
    with DevBuf(x.nbytes) as d_in, DevBuf(groups * plan.nfft * 4) as d_out:
        d_in.put(x)
        fn = plan.exec_device_pfb_integrated_ci16 if ci16 else plan.exec_device_pfb_integrated
        fn(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, detector=det, out=form, scale=SCALE)
        plan.sync()
        return d_out.get((groups, plan.nfft), np.float32)


def check_per_frame(n, taps, frames, hop, shift, proto, seed=1):
    x16 = stream16(seed, (frames - 1) * hop + taps * n)
    xw = widen(x16)
    h = prototype(proto, n, taps, seed + 7)
    with SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        assert plan.set_pfb(h) == taps
        got = dev_rows(plan, x16, frames, hop, ci16=True)
        want = dev_rows(plan, xw, frames, hop, ci16=False)
        # the spectra of every frame, through the numpy boundary (the only entry that returns them; it launches the
        # complex epilogue on chunks of at most 512 frames, so that epilogue's workgroups take one frame each)
        got_fft = plan.pfb_fft_ci16(x16, hop)
        want_fft = plan.pfb_fft(xw, hop)
    assert got_fft.shape == (frames, n)
    db, ff = same_bits(got, want), same_bits(got_fft, want_fft)
    print(f"N={n} T={taps} frames={frames} hop={hop} shift={shift} {proto}: dB rows identical {db}, spectra identical {ff}")
    assert db and ff


# ---- N = 4096, per frame ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps,frames,hop,shift,proto", [
    (1, 1, N4K, True, "default"),
    (2, 7, G3, False, "random"),            # fewer than 8 frames: empty per-XCD ranges
    (4, 1700, N4K, True, "random"),         # more frames than the 768 workgroups: the persistent loop, prefetch across frames
    (4, 1700, 1, False, "default"),         # 4-byte-aligned starts
    (5, 769, N4K // 4, True, "default"),
    (32, 3, N4K, False, "random"),          # the tap limit
])
def test_n4096_per_frame_has_the_complex64_bits(taps, frames, hop, shift, proto):
    check_per_frame(N4K, taps, frames, hop, shift, proto)


def test_n4096_against_spectrum_db_of_numpys_fold():
    taps, frames, hop = 4, 9, G3
    x16 = stream16(21, (frames - 1) * hop + taps * N4K)
    h = prototype("random", N4K, taps, 5)
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(h)
        got = dev_rows(plan, x16, frames, hop, ci16=True)
        host = plan.pfb_db_ci16(x16, hop)
        want = plan.spectrum_db(fold32(widen(x16), h, N4K, taps, frames, hop))
    assert same_bits(got, want)
    assert same_bits(host, want)


@pytest.mark.parametrize("assign", ["0", "1", "2"])
def test_n4096_rows_do_not_depend_on_the_frame_assignment(assign, monkeypatch):
    monkeypatch.setenv("SDRK_PFB_ASSIGN", assign)     # read when the prototype is set
    for frames, hop in ((13, N4K // 4), (769, G3)):
        x16 = stream16(3, (frames - 1) * hop + 4 * N4K)
        with SpectrumPlan(N4K, eps=EPS) as plan:
            plan.set_pfb(prototype("random", N4K, 4, 11))
            got = dev_rows(plan, x16, frames, hop, ci16=True)
            want = dev_rows(plan, widen(x16), frames, hop, ci16=False)
        assert same_bits(got, want), (assign, frames, hop)


# ---- N = 4096, integrated --------------------------------------------------------------------------------------------------
def check_integrated(n, taps, k, groups, hop, shift, proto, seed=2):
    x16 = stream16(seed, (groups * k - 1) * hop + taps * n)
    xw = widen(x16)
    with SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        plan.set_pfb(prototype(proto, n, taps, seed + 3))
        for det in DETECTORS:
            for form in FORMS:
                got = dev_int_rows(plan, x16, groups, k, hop, det, form, ci16=True)
                want = dev_int_rows(plan, xw, groups, k, hop, det, form, ci16=False)
                assert same_bits(got, want), (n, taps, k, groups, hop, det, form)


@pytest.mark.parametrize("taps,k,groups,hop,shift,proto", [
    (1, 1, 9, N4K, True, "default"),
    (2, 3, 5, G3, False, "random"),
    (4, 2, 800, N4K, True, "random"),          # more units than workgroups
    (4, 16, 40, N4K // 4, False, "default"),
    (4, 1700, 1, N4K, True, "default"),        # slices, partials, finalize
    (5, 100, 2, 1, False, "random"),
    (32, 2, 3, N4K, True, "random"),
])
def test_n4096_integrated_has_the_complex64_bits(taps, k, groups, hop, shift, proto):
    check_integrated(N4K, taps, k, groups, hop, shift, proto)


# ---- other lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,taps,frames,hop", [
    (64, 16, 9, 64), (64, 3, 5, 1), (1000, 3, 7, 1500), (1024, 8, 6, 256), (8192, 2, 5, 2731), (65536, 3, 5, 32768),
])
def test_other_lengths_per_frame_have_the_complex64_bits(n, taps, frames, hop):
    check_per_frame(n, taps, frames, hop, shift=bool(taps & 1), proto="random" if n != 1000 else "default")


@pytest.mark.parametrize("n,taps,k,groups,hop", [
    (64, 3, 4096, 2, 1), (1000, 3, 3, 4, 1500),
    (1024, 3, 2, 4500, 512),               # 9000 folded frames: two chunks of the 64 MiB staging, a carried unit
])
def test_other_lengths_integrated_have_the_complex64_bits(n, taps, k, groups, hop):
    check_integrated(n, taps, k, groups, hop, shift=True, proto="default")


# ---- the numpy boundary ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,hop", [(3000, N4K), (6000, N4K // 2)])
def test_host_entries_return_the_device_entries_bits_in_bounded_memory(frames, hop):
    """~49 MB of int16 input at T = 4.  The boundary aims at a quarter of the call per chunk (at most 16 MiB) and at most
    chunk / 16 KiB rows: 750 frames per chunk at either hop, so 4 and 8 chunks, each carrying 3 * 4096 samples of overlap.
    The integrated call cuts at 16 MiB of input (1024 / 2048 frames): K = 7 divides neither."""
    taps, k = 4, 7
    L = (frames - 1) * hop + taps * N4K
    base = stream16(5, 64 * N4K + 1)
    x16 = np.ascontiguousarray(np.tile(base, (L // base.shape[0] + 1, 1))[:L])
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(pfb_prototype(N4K, taps))
        dev = dev_rows(plan, x16, frames, hop, ci16=True)
        host, held = held_during(lambda: plan.pfb_db_ci16(x16, hop), lambda: plan.pfb_db_ci16(x16[: taps * N4K]))
        print(f"frames={frames} hop={hop}: device memory taken by the host call {held / 2**20:.1f} MiB")
        assert held <= 192 << 20, held
        assert same_bits(host, dev)
        xp = pinned_empty(x16.shape, np.int16)
        xp[...] = x16
        out = pinned_empty((frames, N4K), np.float32)
        assert plan.pfb_db_ci16(xp, hop, out=out) is out
        assert same_bits(out, dev)
        # the device rows are the complex64 call's (a prefix: the widened stream is twice the bytes)
        nf = 300
        Lp = (nf - 1) * hop + taps * N4K
        assert same_bits(dev[:nf], dev_rows(plan, widen(x16[:Lp]), nf, hop, ci16=False))
        groups = frames // k
        for det in ("mean", "max"):
            dev_i = dev_int_rows(plan, x16, groups, k, hop, det, "db", ci16=True)
            host_i, held = held_during(lambda: plan.pfb_integrate_ci16(x16, k, hop, det, "db", SCALE),
                                        lambda: plan.pfb_integrate_ci16(x16[: (k - 1) * hop + taps * N4K], k, hop, det))
            assert held <= 192 << 20, held
            assert same_bits(host_i, dev_i), det
            assert same_bits(plan.pfb_integrate_ci16(xp, k, hop, det, "db", SCALE), dev_i), det
        gp = 40
        Lg = (gp * k - 1) * hop + taps * N4K
        assert same_bits(dev_i[:gp], dev_int_rows(plan, widen(x16[:Lg]), gp, k, hop, "max", "db", ci16=False))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_return_invalid_with_a_message_and_the_plan_still_works():
    lib = _ffi.lib()
    n = 256
    h = pfb_prototype(n, 2)
    hp = h.ctypes.data_as(ctypes.c_void_p)
    x16 = stream16(1, 4 * n)
    out = np.empty((2, n), np.float32)
    outc = np.empty((2, n), np.complex64)
    xp, op, ocp = (a.ctypes.data_as(ctypes.c_void_p) for a in (x16, out, outc))
    ms = (ctypes.c_float * 2)()
    f = ctypes.c_float(1.0)

    def refused(status):
        assert status == _ffi.SDRK_ERR_INVALID, status
        assert lib.sdrk_last_error(), "no message"

    def every_exec(handle, iq=xp, frames=2, rows=op, rows_c=ocp, stride=n):
        refused(lib.sdrk_exec_device_pfb_ci16(handle, iq, frames, stride, rows, None))
        refused(lib.sdrk_exec_device_pfb_ci16_timed_each(handle, iq, frames, stride, rows, 2, ms))
        refused(lib.sdrk_exec_host_pfb_ci16(handle, iq, frames, stride, rows))
        refused(lib.sdrk_exec_fft_host_pfb_ci16(handle, iq, frames, stride, rows_c))
        if frames == 2:
            groups, k = 1, 2
        else:
            groups, k = 0, 2
        refused(lib.sdrk_exec_device_pfb_integrated_ci16(handle, iq, groups, k, stride, 0, 0, f, rows, None))
        refused(lib.sdrk_exec_device_pfb_integrated_ci16_timed_each(handle, iq, groups, k, stride, 0, 0, f, rows, 2, ms))
        refused(lib.sdrk_exec_host_pfb_integrated_ci16(handle, iq, groups, k, stride, 0, 0, f, rows))

    with SpectrumPlan(n, window="hann") as windowed, SpectrumPlan(n, precision="double") as f64, SpectrumPlan(n) as plan:
        for bad in (windowed, f64):
            every_exec(bad.handle)
        every_exec(plan.handle)                                   # no prototype set
        assert lib.sdrk_plan_set_pfb(plan.handle, 2, hp) == 0
        every_exec(None)
        every_exec(plan.handle, iq=None)
        every_exec(plan.handle, rows=None, rows_c=None)
        every_exec(plan.handle, frames=0)
        every_exec(plan.handle, stride=0)                         # stride 0 with more than one frame
        refused(lib.sdrk_exec_device_pfb_ci16_timed_each(plan.handle, xp, 2, n, op, 0, ms))
        refused(lib.sdrk_exec_device_pfb_ci16_timed_each(plan.handle, xp, 2, n, op, 2, None))
        refused(lib.sdrk_exec_host_pfb_integrated_ci16(plan.handle, xp, 1, 2, n, 7, 0, f, op))
        refused(lib.sdrk_exec_host_pfb_integrated_ci16(plan.handle, xp, 1, 2, n, 0, 9, f, op))
        # the refused plan still works
        assert lib.sdrk_exec_host_pfb_ci16(plan.handle, xp, 2, n, op) == 0
        assert same_bits(out, plan.spectrum_db(fold32(widen(x16), h, n, 2, 2, n)))
        # Python-side refusals
        with pytest.raises(ValueError):
            windowed.pfb_db_ci16(x16)
        with pytest.raises(ValueError):
            f64.pfb_integrate_ci16(x16, 2)
        with pytest.raises(ValueError):
            plan.pfb_db_ci16(widen(x16))
        with pytest.raises(ValueError):
            plan.pfb_integrate_ci16(x16.astype(np.int32), 2)


def test_existing_rows_of_the_same_plan_are_unchanged_by_the_new_calls():
    taps, frames, k = 4, 12, 3
    x16 = stream16(31, (frames - 1) * N4K + taps * N4K)
    xw = widen(x16)
    f16 = np.ascontiguousarray(x16[: 3 * N4K].reshape(3, N4K, 2))
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(pfb_prototype(N4K, taps))
        before = (plan.pfb_db(xw), plan.pfb_integrate(xw, k, detector="max"), plan.spectrum_db_ci16(f16), plan.spectrum_db(xw[:N4K]))
        new = (plan.pfb_db_ci16(x16), plan.pfb_integrate_ci16(x16, k, detector="max"))
        after = (plan.pfb_db(xw), plan.pfb_integrate(xw, k, detector="max"), plan.spectrum_db_ci16(f16), plan.spectrum_db(xw[:N4K]))
    for b, a in zip(before, after):
        assert same_bits(b, a)
    assert same_bits(new[0], before[0]) and same_bits(new[1], before[1])


def test_cli_psd_pfb_integrate_on_a_ci16_recording(tmp_path, capsys):
    n, taps, k = 4096, 4, 3
    iq = stream16(8, 14 * n + 100)
    base = str(tmp_path / "rec16")
    sigmf_io.write_sigmf(base, iq, 2_000_000, 915_000_000, datatype="ci16_le")
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", base + ".sigmf-meta", "--pfb", str(taps), "--integrate", str(k), "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["pfb_taps"] == taps and report["pfb_rows"] == 11 and report["pfb_integrated_rows"] == 3
    wide, _ = sigmf_io.read_sigmf(base)
    assert wide.dtype == np.complex64
    with np.load(out) as z:
        assert same_bits(z["pfb_db"], pkg.pfb_db_ci16(iq, n, taps))
        assert same_bits(z["pfb_integrated_db"], pkg.pfb_integrated_db_ci16(iq, n, taps, k))
        assert same_bits(z["pfb_db"], pkg.pfb_db(wide, n, taps))
        assert same_bits(z["pfb_integrated_db"], pkg.pfb_integrated_db(wide, n, taps, k))
        assert same_bits(z["integrated_db"], pkg.integrated_db(wide, n, k))


# ---- one plan's three stagings (int16 unpack, PFB fold, integrate) used in turn and with work in flight ---------------------------
CHILD_STAGINGS = r"""
import torch, numpy as np
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
N, T, K = 128, 2, 3            # below every fused and every int16-reading kernel: each call goes through its staging
rng = np.random.default_rng(20)
x = rng.integers(-32768, 32768, size=(4096, 2), dtype=np.int64).astype(np.int16)
h = rng.standard_normal(T * N).astype(np.float32)
x_int, x_pfb = x[:4 * K * N], x[:(6 - 1) * 64 + T * N]
xt_int, xt_pfb = torch.from_numpy(x_int).cuda(), torch.from_numpy(x_pfb).cuda()
side = torch.cuda.Stream()
torch.cuda.current_stream().synchronize()

def plan():
    p = SpectrumPlan(N)
    p.set_pfb(h)
    return p

def device_pair(p):
    a = torch.empty((4, N), dtype=torch.float32, device="cuda")
    b = torch.empty((6, N), dtype=torch.float32, device="cuda")
    torch.cuda.current_stream().synchronize()
    p.exec_device_integrated_ci16(xt_int.data_ptr(), 4, K, a.data_ptr(), detector="max")               # the plan's stream
    p.exec_device_pfb_ci16(xt_pfb.data_ptr(), 6, b.data_ptr(), frame_stride=64, stream=side.cuda_stream)   # no sync between
    side.synchronize(); p.sync()
    return a.cpu().numpy(), b.cpu().numpy()

calls = [lambda p: p.integrate_ci16(x[:2 * K * N], K),                       # 2 groups
         lambda p: p.pfb_integrate_ci16(x[:(5 * K - 1) * 64 + T * N], K, 64),   # 5 groups at hop 64: the stagings grow
         device_pair,
         lambda p: p.stft_db_ci16(x, 32)]
with plan() as one:
    got = [c(one) for c in calls]
for i, c in enumerate(calls):
    with plan() as fresh:
        want = c(fresh)
    for g, w in zip(*((got[i], want) if isinstance(want, tuple) else ((got[i],), (want,)))):
        assert g.shape == w.shape and g.shape[0] > 0 and np.array_equal(g, w), i
print("stagings ok")
"""


def test_one_plans_stagings_in_turn_and_in_flight_give_a_fresh_plans_rows():
    """nfft = 128, T = 2, K = 3 (a fresh process: torch first, one HIP runtime).  On ONE plan: integrate_ci16 over 2 groups,
    pfb_integrate_ci16 over 5 groups at hop 64 (the stagings grow), exec_device_integrated_ci16 on the plan's stream and
    exec_device_pfb_ci16 on a second stream with no sync between them, stft_db_ci16 at hop 32 — each equal to the same call
    on a fresh plan.  This checks the bits that come through stagings that were used before, grew and are used again; the two
    calls in flight use different stagings (int16 unpack and integrate against the PFB fold), so it does not prove the ordering
    of two streams on ONE staging — the stand-in runtime does, under ThreadSanitizer (tests/test_host_sanitizers_*.py)."""
    run_child(CHILD_STAGINGS, "stagings ok")

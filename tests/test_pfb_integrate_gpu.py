"""Integrated polyphase-filter-bank spectra on the GPU (sdrk_exec_*_pfb_integrated): T blocks folded under the prototype, the
plan's transform, and ONE row per K consecutive folded frames — mean (compensated), maximum or minimum of the power per bin.

The definition is in bits: the row of a group is what sdrk_exec_device_integrated returns on the same rectangular plan for the
packed folded frames (numpy's float32 fold, tests/test_pfb_gpu.py's fold32) with the same groups, K, detector, form and scale.
So the first check compares uint32 views.  The second is the project's amplitude bar against float64 numpy on the same
complex64 samples, per group g with S_g the largest reference |Y_f[k]| of the group,

    max_k | sqrt(R_got[k]) - sqrt(R_ref[k]) |  <=  tests.parity.REL_TOL * S_g

which follows from the per-frame bound of the PFB tests (the float32 fold stays at 1.2-1.4e-7 of the frame peak) by the
triangle-inequality argument of tests/test_integrate_gpu.py: a root-mean-square, a maximum and a minimum over frames are
1-Lipschitz in the per-frame magnitudes, and the compensated mean adds one rounding.
Inputs are those of tests/test_pfb_gpu.py: 12-bit integer noise plus an integer-rounded tone, the default and a random prototype."""
import ctypes
import json

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
from tests.gpu_helpers import DevBuf, fold32, held_during, prototype, ref64, same_bits, stream_synth_tone as stream
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

EPS = 1e-12
N4K = 4096
DETECTORS = ("mean", "max", "min")
FORMS = ("db", "power")
SCALE = 0.37


def device_rows(plan, x, groups, k, hop, detector, out, pfb):
    call = plan.exec_device_pfb_integrated if pfb else plan.exec_device_integrated
    with DevBuf(x.nbytes) as d_in, DevBuf(groups * plan.nfft * 4) as d_out:
        d_in.put(x)
        call(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, detector=detector, out=out, scale=SCALE)
        plan.sync()
        return d_out.get((groups, plan.nfft), np.float32)


def check_bits(n, taps, k, groups, hop, shift, proto, detectors, seed, bound):
    frames = groups * k
    x = stream(seed, (frames - 1) * hop + taps * n)
    h = prototype(proto, n, taps, seed + 7)
    y = fold32(x, h, n, taps, frames, hop)
    what = f"N={n} T={taps} K={k} groups={groups} hop={hop} shift={shift} {proto}"
    got_power = {}
    with SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        plan.set_pfb(h)
        for det in detectors:
            for form in FORMS:
                got = device_rows(plan, x, groups, k, hop, det, form, pfb=True)
                want = device_rows(plan, y, groups, k, n, det, form, pfb=False)
                assert same_bits(got, want), (what, det, form)
                if form == "power":
                    got_power[det] = got.astype(np.float64) / np.float64(np.float32(SCALE))
    if not bound:
        return
    P = (np.abs(ref64(x, h, n, taps, frames, hop, shift)) ** 2).reshape(groups, k, n)
    s_g = np.sqrt(P.max(axis=(1, 2)))
    worst = 0.0
    for det, R in (("mean", P.mean(axis=1)), ("max", P.max(axis=1)), ("min", P.min(axis=1))):
        err = (np.abs(np.sqrt(got_power[det]) - np.sqrt(R)).max(axis=-1) / s_g).max()
        worst = max(worst, float(err))
        print(f"{what} {det}: amplitude error {err:.2e} of the group peak (bound {REL_TOL:.0e})")
        # the power form carries one more float32 rounding (scale * R): half an ulp of the amplitude, far below the bound
        assert err <= REL_TOL, (what, det, err)
    print(f"{what}: worst {worst:.2e}")


G3 = N4K + N4K // 3 + 1
# (taps, K, groups, hop, shift, prototype)
CASES_4096 = [
    (1, 1, 9, N4K, True, "random"),            # K = 1 is the PFB row
    (2, 3, 5, G3, False, "default"),           # gapped hop
    (4, 2, 800, N4K, True, "default"),         # more units than the 768 workgroups: the persistent loop, the prefetch across units
    (4, 16, 40, N4K // 4, True, "random"),     # overlapped hop
    (4, 1700, 1, N4K, False, "default"),       # one group cut into slices, partials, finalize
    (5, 100, 2, 1, True, "random"),            # hop 1
    (5, 3, 1000, N4K // 4, False, "default"),  # many small groups at an overlapped hop
    (32, 2, 3, N4K, True, "default"),          # the tap limit
]


@pytest.mark.parametrize("taps,k,groups,hop,shift,proto", CASES_4096)
def test_n4096_bits_of_integrate_on_the_folded_frames_and_float64_bound(taps, k, groups, hop, shift, proto):
    check_bits(N4K, taps, k, groups, hop, shift, proto, DETECTORS, seed=taps * 100 + k, bound=True)


# (n, taps, K, groups, hop): short, hop 1 with slices, chirp-z, single-pass, above 4096, two-pass; the last is 70 MiB of folded
# frames — two staging chunks with a carried unit
CASES_GENERIC = [
    (64, 16, 100, 3, 64), (64, 3, 4096, 2, 1), (1000, 3, 3, 4, 1500), (1024, 8, 16, 6, 256), (8192, 2, 3, 3, 2731),
    (65536, 3, 2, 2, 32768), (1024, 3, 2, 4500, 512),
]


@pytest.mark.parametrize("n,taps,k,groups,hop", CASES_GENERIC)
def test_other_lengths_bits_of_integrate_on_the_folded_frames(n, taps, k, groups, hop):
    check_bits(n, taps, k, groups, hop, bool(taps & 1), "default" if k & 1 else "random", ("mean", "max" if taps & 1 else "min"),
               seed=n % 1000 + taps, bound=False)


def _long_stream(n_samples):
    return np.tile(stream(5, 64 * N4K + 1), n_samples // (64 * N4K + 1) + 1)[:n_samples]


@pytest.mark.parametrize("frames,hop", [(3000, N4K), (6000, N4K // 2)])
def test_host_entry_returns_the_device_entrys_bits_in_bounded_memory(frames, hop):
    """~98 MB of input at T = 4, K = 7 through the chunked numpy boundary: several chunks, K does not divide a chunk's frames
    (units carried), (T - 1) blocks of overlap across every boundary; from a pageable and from a pinned array."""
    taps, k = 4, 7
    x = _long_stream((frames - 1) * hop + taps * N4K)
    h = pfb_prototype(N4K, taps)
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(h)
        groups = plan.pfb_integrated_groups(x.size, k, hop)
        assert groups == frames // k
        xp = pinned_empty(x.shape, np.complex64)
        xp[...] = x
        for det, form in (("mean", "db"), ("max", "power")):
            dev = device_rows(plan, x, groups, k, hop, det, form, pfb=True)
            host, held = held_during(lambda: plan.pfb_integrate(x, k, hop, det, form, SCALE),
                                      lambda: plan.pfb_integrate(x[: (k - 1) * hop + taps * N4K], k, hop, det, form, SCALE))
            print(f"frames={frames} hop={hop} {det}/{form}: device memory taken by the host call {held / 2**20:.1f} MiB")
            assert held <= 192 << 20, held
            assert same_bits(host, dev), (det, form)
            assert same_bits(plan.pfb_integrate(xp, k, hop, det, form, SCALE), dev), (det, form, "pinned")
        # and the definition, on the first groups
        y = fold32(x, h, N4K, taps, 3 * k, hop)
        assert same_bits(dev[:3], device_rows(plan, y, 3, k, N4K, "max", "power", pfb=False))


def test_host_entry_with_few_groups_splits_and_finalizes():
    taps, k, groups, hop = 4, 1500, 2, N4K
    x = _long_stream((groups * k - 1) * hop + taps * N4K)
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(pfb_prototype(N4K, taps))
        for det in ("mean", "min"):
            dev = device_rows(plan, x, groups, k, hop, det, "db", pfb=True)
            assert same_bits(plan.pfb_integrate(x, k, hop, det), dev), det


def test_refusals_return_invalid_with_a_message_and_the_plan_still_works():
    lib = _ffi.lib()
    n, taps, k, groups = 256, 2, 3, 2
    h = pfb_prototype(n, taps)
    x = stream(1, (groups * k - 1) * n + taps * n)
    out = np.empty((groups, n), np.float32)
    xp, op = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, out))
    ms = (ctypes.c_float * 2)()
    MEAN, DB = _ffi.DETECTORS["mean"], _ffi.INT_OUT_FORMS["db"]
    one = ctypes.c_float(1.0)

    def refused(status):
        assert status == _ffi.SDRK_ERR_INVALID, status
        assert lib.sdrk_last_error(), "no message"

    def every_exec(handle, iq=xp, g=groups, kk=k, stride=n, det=MEAN, form=DB, rows=op):
        refused(lib.sdrk_exec_device_pfb_integrated(handle, iq, g, kk, stride, det, form, one, rows, None))
        refused(lib.sdrk_exec_device_pfb_integrated_timed_each(handle, iq, g, kk, stride, det, form, one, rows, 2, ms))
        refused(lib.sdrk_exec_host_pfb_integrated(handle, iq, g, kk, stride, det, form, one, rows))

    with SpectrumPlan(n, window="hann") as windowed, SpectrumPlan(n, precision="double") as f64, SpectrumPlan(n) as plan:
        every_exec(windowed.handle)
        every_exec(f64.handle)
        every_exec(plan.handle)                                   # no prototype set
        plan.set_pfb(h)
        every_exec(None)
        every_exec(plan.handle, det=3)
        every_exec(plan.handle, det=-1)
        every_exec(plan.handle, form=2)
        every_exec(plan.handle, g=0)
        every_exec(plan.handle, kk=0)
        every_exec(plan.handle, g=1 << 40, kk=1 << 40)
        every_exec(plan.handle, stride=0)
        every_exec(plan.handle, iq=None)
        every_exec(plan.handle, rows=None)
        refused(lib.sdrk_exec_device_pfb_integrated_timed_each(plan.handle, xp, groups, k, n, MEAN, DB, one, op, 0, ms))
        refused(lib.sdrk_exec_device_pfb_integrated_timed_each(plan.handle, xp, groups, k, n, MEAN, DB, one, op, 2, None))
        # the refused plan still works
        assert lib.sdrk_exec_host_pfb_integrated(plan.handle, xp, groups, k, n, MEAN, DB, one, op) == 0
        assert same_bits(out, plan.integrate(fold32(x, h, n, taps, groups * k, n).reshape(-1), k))
        # Python-side refusals of the same plans
        for bad in (windowed, f64):
            with pytest.raises(ValueError):
                bad.pfb_integrate(x, k)


def test_ordinary_entry_points_are_unchanged_and_a_second_prototype_takes_effect():
    n = N4K
    x = stream(21, 14 * n)
    with SpectrumPlan(n, eps=EPS) as plan:
        h4 = prototype("random", n, 4, 1)
        plan.set_pfb(h4)
        before = (plan.spectrum_db(x.reshape(14, n)), plan.stft_db(x, n // 2), plan.integrate(x, 3), plan.pfb_db(x, n))
        a = plan.pfb_integrate(x, 3, n)
        assert a.shape == (plan.pfb_integrated_groups(x.size, 3, n), n) == (3, n)
        assert same_bits(a, plan.integrate(fold32(x, h4, n, 4, 9, n).reshape(-1), 3))
        after = (plan.spectrum_db(x.reshape(14, n)), plan.stft_db(x, n // 2), plan.integrate(x, 3), plan.pfb_db(x, n))
        for b, c in zip(before, after):
            assert same_bits(b, c)
        h2 = prototype("random", n, 2, 2)
        assert plan.set_pfb(h2) == 2
        b = plan.pfb_integrate(x, 3, n, detector="max")
        assert b.shape == (4, n)
        assert same_bits(b, plan.integrate(fold32(x, h2, n, 2, 12, n).reshape(-1), 3, detector="max"))
    assert same_bits(spectrum.pfb_integrated_db(x, n, 2, 3, detector="max", prototype=h2, eps=EPS), b)


def test_cli_psd_pfb_integrate_reproduces_pfb_integrated_db(tmp_path, capsys):
    n, taps, k = 1024, 4, 8
    x = stream(31, 40 * n + 17)
    _, meta = sigmf_io.write_sigmf(str(tmp_path / "rec"), x, 1e6, 2.4e9)
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", meta, "--nfft", str(n), "--pfb", str(taps), "--integrate", str(k), "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    saved = np.load(out)
    rows = saved["pfb_integrated_db"]
    assert report["pfb_taps"] == taps and report["pfb_rows"] == saved["pfb_db"].shape[0] == 37
    assert report["integrate_k"] == k and report["integrated_rows"] == saved["integrated_db"].shape[0] == 5
    assert report["pfb_integrated_rows"] == rows.shape[0] == 4
    assert same_bits(rows, spectrum.pfb_integrated_db(x, n, taps, k))
    with SpectrumPlan(n) as plan:
        assert same_bits(rows, plan.integrate(fold32(x, pfb_prototype(n, taps), n, taps, 32, n).reshape(-1), k))

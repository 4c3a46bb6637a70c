"""Integrated spectra on the GPU: one row per K frames — mean / max / min of |fft(w x_f)|^2 per bin — from
sdrk_exec_device_integrated and sdrk_exec_host_integrated, against float64 numpy on the same complex64 samples.

The amplitude bound is the project's REL_TOL, derived, not new: a per-frame amplitude error of eps * peak gives at most
eps * peak on an RMS over frames (triangle inequality in l2) and on a max or min (|max a - max b| <= max |a - b|).  With S_g
the largest reference |X_f[k]| over the frames and bins of group g,

    max_k | sqrt(R_got) - sqrt(R_ref) |  <=  1e-5 * S_g        for every group, detector and route.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from oracle import cpu_ref
from sdr_iq_visualizer_amd import _ffi, cli
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import DevBuf, check_amplitude, ref_power, ref_reduced, same_bits_u32 as same_bits, stream_noise_tone as stream
from tests.parity import assert_db_parity, assert_db_parity_deep

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECTORS = ("mean", "max", "min")
EPS = 1e-12


def hop_of(kind, n):
    return {"packed": n, "half": n // 2, "gapped": n + n // 3 + 1}[kind]


def device_integrate(plan, x, groups, k, hop, detector, out="db", scale=1.0):
    with DevBuf(x.nbytes) as d_in, DevBuf(groups * plan.nfft * 4) as d_out:
        d_in.put(x)
        plan.exec_device_integrated(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, detector=detector, out=out,
                                    scale=scale)
        plan.sync()
        return d_out.get((groups, plan.nfft), np.float32)


# (n, k, groups, hop, window, shift)
CASES = [
    (64, 1, 5, "packed", None, True), (64, 100, 3, "half", "hann", True), (64, 4096, 2, "packed", "hann", False),
    (64, 2, 3000, "gapped", None, True), (64, 3, 7, "half", None, False), (64, 16, 5, "gapped", "hann", True),
    (1000, 3, 4, "gapped", "hann", True), (1000, 16, 2, "packed", None, False), (1000, 4096, 1, "packed", "hann", True),
    (1000, 1, 6, "half", None, True), (1000, 2, 5, "packed", "hann", False), (1000, 100, 2, "gapped", None, True),
    (1024, 3, 5, "gapped", None, False), (1024, 16, 6, "half", "hann", True),
    (1024, 2, 7, "half", "hann", True), (1024, 100, 3, "packed", None, True), (1024, 4096, 1, "packed", "hann", False),
    (1024, 1, 900, "packed", "hann", True),
    (4096, 1, 9, "packed", None, True), (4096, 2, 800, "packed", "hann", True), (4096, 3, 5, "gapped", "hann", False),
    (4096, 16, 40, "half", "hann", True), (4096, 100, 2, "packed", None, False), (4096, 16, 1, "packed", "hann", True),
    (4096, 3, 1000, "half", None, True),
    (8192, 2, 3, "half", None, True), (8192, 16, 2, "packed", "hann", True), (8192, 100, 1, "gapped", "hann", False),
    (8192, 1, 4, "packed", "hann", True), (8192, 3, 3, "packed", None, False),
    (65536, 1, 3, "packed", None, True), (65536, 3, 2, "gapped", "hann", True), (65536, 16, 2, "half", "hann", False),
    (65536, 100, 1, "packed", None, True), (65536, 2, 2, "packed", "hann", True),
    (100000, 2, 2, "packed", "hann", True), (100000, 3, 1, "half", None, False), (100000, 16, 1, "packed", "hann", True),
    (100000, 1, 2, "gapped", None, True), (100000, 100, 1, "half", "hann", True),
]


@pytest.mark.parametrize("n,k,groups,hop_kind,window,shift", CASES)
def test_amplitude_bound_all_detectors(n, k, groups, hop_kind, window, shift):
    rng = np.random.default_rng(n * 31 + k)
    hop = hop_of(hop_kind, n)
    x = stream(rng, n, groups * k, hop)
    p = ref_power(x, n, groups * k, hop, window, shift)
    with SpectrumPlan(n, window=window, eps=EPS, shift=shift) as plan:
        for det in DETECTORS:
            for form in ("db", "power"):
                got = device_integrate(plan, x, groups, k, hop, det, form)
                check_amplitude(got, form, p, groups, k, det, f"N={n} K={k} G={groups} {hop_kind} {window} {det} {form}")
        got = plan.integrate(x, k, hop, "mean", "db")            # the numpy boundary, same bound
        assert got.shape == (groups, n)
        check_amplitude(got, "db", p, groups, k, "mean", f"host N={n} K={k}")


def test_k_4096_of_near_constant_power_holds_the_bound():
    """A tone plus weak noise: every frame adds nearly the same power to the tone's bins — the case in which plain float32
    summation of 4096 terms drifts past the bound and a compensated sum does not.  One group (split) and 800 (unsplit)."""
    n, k = 4096, 4096
    rng = np.random.default_rng(4096)
    x = stream(rng, n, k, n, tone_db=40.0, noise=1e-3)
    p = ref_power(x, n, k, n, "hann", True)
    with SpectrumPlan(n, window="hann", eps=EPS) as plan:
        for form in ("db", "power"):
            got = device_integrate(plan, x, 1, k, n, "mean", form)
            check_amplitude(got, form, p, 1, k, "mean", f"K=4096 split {form}")
    # unsplit, on the same near-constant bins: 800 groups of 5 are more than the resident grid
    with SpectrumPlan(n, window="hann", eps=EPS) as plan:
        got = device_integrate(plan, x[: 4000 * n], 800, 5, n, "mean", "power")
    check_amplitude(got, "power", p, 800, 5, "mean", "K=5 unsplit")


@pytest.mark.parametrize("n,k,groups,hop_kind,window", [(4096, 2, 6, "packed", "hann"), (4096, 16, 3, "half", None),
                                                         (4096, 100, 1, "packed", "hann"), (1024, 16, 4, "packed", "hann"),
                                                         (65536, 3, 2, "packed", None), (1000, 16, 2, "half", "hann")])
def test_mean_and_max_rows_in_db(n, k, groups, hop_kind, window):
    """Noise plus a tone 20 dB above it: every bin of every reference row lies inside the 70 dB window, so the deep check
    covers all of them (asserted: if not, the input is wrong, not the tolerance)."""
    rng = np.random.default_rng(n + k)
    hop = hop_of(hop_kind, n)
    x = stream(rng, n, groups * k, hop, tone_db=20.0)
    p = ref_power(x, n, groups * k, hop, window, True)
    with SpectrumPlan(n, window=window, eps=EPS) as plan:
        for det in ("mean", "max"):
            ref = 20 * np.log10(np.sqrt(ref_reduced(p, groups, k, det)) + EPS)
            assert np.all(ref >= ref.max(axis=-1, keepdims=True) - 70.0), "input: a reference bin outside the deep window"
            got = device_integrate(plan, x, groups, k, hop, det)
            assert_db_parity(got, ref, what=f"N={n} K={k} {det}")
            worst = assert_db_parity_deep(got, ref, what=f"N={n} K={k} {det}")
            print(f"N={n} K={k} {det}: worst |delta dB| {worst:.2e}")
            assert_db_parity_deep(plan.integrate(x, k, hop, det), ref, what=f"host N={n} K={k} {det}")


def test_welch_psd_streamed_randomised():
    """The cases and the bound of test_parity_gpu.test_welch_psd_randomised, through the integrated path."""
    rng = np.random.default_rng(188)
    for case in range(28):
        n = int(rng.choice([64, 256, 1000, 1024, 4096, 8192, 65536]))
        hop = n if rng.random() < 0.4 else int(rng.integers(1, 2 * n + 1))
        segs = int(rng.integers(1, 61 if n <= 8192 else 9))
        L = n + (segs - 1) * hop + int(rng.integers(0, hop))
        window = "hann" if rng.random() < 0.6 else None
        shift = bool(rng.random() < 0.7)
        fs = float(rng.choice([1e6, 2.4e6, 61.44e6]))
        x = ((rng.standard_normal(L) + 1j * rng.standard_normal(L)) * float(rng.uniform(0.01, 300))).astype(np.complex64)
        x += (rng.uniform(1, 100) * np.exp(2j * np.pi * rng.uniform(-0.5, 0.5) * np.arange(L))).astype(np.complex64)
        got = pkg.welch_psd_streamed(x, n, fs, hop=hop, window=window, shift=shift)
        ref = cpu_ref.welch_psd(x, n, fs, hop=hop, window=None if window else np.ones(n), shift=shift)
        assert got.dtype == np.float32 and got.shape == (n,)
        err = float(np.abs(got - ref).max() / ref.max())
        print(f"welch case {case}: N={n} hop={hop} segs={segs}: {err:.2e}")
        assert err <= 1e-5, (case, n, hop, segs, window, shift, err)


def test_welch_psd_streamed_vs_mlab_golden_and_beyond_max_batch(golden):
    g = golden["ref_welch"]
    fs = float(g["fs"][0])
    for hop, key in ((None, "pxx"), (512, "pxx_noverlap512")):
        got = pkg.welch_psd_streamed(g["iq"], 1024, fs, hop=hop)
        assert got.dtype == np.float32 and got.shape == (1024,)
        assert np.abs(got - g[key]).max() <= 1e-5 * g[key].max()
    with pytest.raises(ValueError):
        pkg.welch_psd_streamed(g["iq"][:100], 1024, fs)
    # more segments than the plan's max_batch: welch_psd refuses, the streamed form serves
    rng = np.random.default_rng(9)
    x = stream(rng, 1024, 100, 1024)
    with SpectrumPlan(1024, window="hann", max_batch=8) as plan:
        with pytest.raises(ValueError, match="max_batch"):
            plan.welch_psd(x, 1e6)
        got = plan.welch_psd_streamed(x, 1e6)
    ref = cpu_ref.welch_psd(x, 1024, 1e6)
    assert np.abs(got - ref).max() <= 1e-5 * ref.max()


def test_k_1_at_4096_is_bit_identical_to_exec_device():
    n, frames = 4096, 1000
    rng = np.random.default_rng(1)
    x = stream(rng, n, frames, n)
    for window, shift in (("hann", True), (None, False)):
        with SpectrumPlan(n, window=window, shift=shift) as plan, DevBuf(x.nbytes) as d_in, DevBuf(frames * n * 4) as d_out:
            d_in.put(x)
            plan.exec_device(d_in.p.value, frames, d_out.p.value)
            plan.sync()
            rows = d_out.get((frames, n), np.float32)
            for det in DETECTORS:
                assert same_bits(device_integrate(plan, x, frames, 1, n, det), rows), (window, det)
                assert same_bits(device_integrate(plan, x, 5, 1, n, det), rows[:5]), (window, det)


def test_repeated_calls_give_identical_bits():
    rng = np.random.default_rng(2)
    for n, k, groups in ((4096, 64, 1), (4096, 7, 900), (1024, 50, 3), (100000, 5, 1)):
        x = stream(rng, n, groups * k, n)
        with SpectrumPlan(n, window="hann") as plan:
            for det in DETECTORS:
                a = device_integrate(plan, x, groups, k, n, det)
                assert same_bits(a, device_integrate(plan, x, groups, k, n, det)), (n, det)
                assert same_bits(a, plan.integrate(x, k, n, det)), (n, det, "host")


def test_max_and_min_from_the_split_path_equal_the_unsplit_path(monkeypatch):
    """One group of 64 frames is cut into slices; the same 64 frames repeated as 24 groups on a plan sized for 8 CUs (24
    resident workgroups) are not.  Order does not matter for max or min: the rows are the same bits."""
    n, k = 4096, 64
    rng = np.random.default_rng(3)
    x = stream(rng, n, k, n)
    with SpectrumPlan(n, window="hann") as plan:
        split = {det: device_integrate(plan, x, 1, k, n, det) for det in ("max", "min")}
    monkeypatch.setenv("SDRK_NUM_CUS", "8")
    with SpectrumPlan(n, window="hann") as plan:
        for det in ("max", "min"):
            rows = device_integrate(plan, np.tile(x, 24), 24, k, n, det)
            for g in range(24):
                assert same_bits(rows[g], split[det][0]), (det, g)


@pytest.mark.parametrize("n,k,groups", [(4096, 101, 12), (4096, 3, 1000), (1024, 100, 45), (65536, 7, 10)])
def test_host_entry_equals_device_entry_across_chunks(n, k, groups):
    """More than one 16 MiB chunk, a group (and, where groups are split, a slice) straddling a chunk boundary: the carried
    state continues the same sums, so pageable and pinned host arrays give the device entry's bits."""
    rng = np.random.default_rng(n + k)
    x = stream(rng, n, groups * k, n)
    assert x.nbytes > 2 * (16 << 20) and ((16 << 20) // (n * 8)) % k != 0
    xp = pinned_empty(x.shape, np.complex64)
    xp[:] = x
    with SpectrumPlan(n, window="hann") as plan:
        for det in DETECTORS:
            for form in ("db", "power"):
                dev = device_integrate(plan, x, groups, k, n, det, form, 0.5)
                assert same_bits(plan.integrate(x, k, n, det, form, 0.5), dev), (det, form, "pageable")
                assert same_bits(plan.integrate(xp, k, n, det, form, 0.5), dev), (det, form, "pinned")


@pytest.mark.parametrize("n,k,groups", [(1024, 100, 100), (1024, 3000, 4), (64, 7, 40000)])
def test_generic_route_device_call_larger_than_the_staging(n, k, groups):
    """More than 64 MiB of spectra in one device-entry call: several transform + reduction launches, groups (and slices, where
    the groups are few) carried across staging boundaries — against numpy, and bit for bit against the host entry."""
    rng = np.random.default_rng(n + k)
    x = stream(rng, n, groups * k, n)
    assert x.nbytes > (64 << 20) and ((64 << 20) // (n * 8)) % k != 0
    p = ref_power(x, n, groups * k, n, "hann", True)
    with SpectrumPlan(n, window="hann", eps=EPS) as plan:
        for det in DETECTORS:
            dev = device_integrate(plan, x, groups, k, n, det, "power")
            check_amplitude(dev, "power", p, groups, k, det, f"staging N={n} K={k} {det}")
            assert same_bits(plan.integrate(x, k, n, det, "power"), dev), (n, k, det)


def test_device_memory_of_a_1_gib_host_call_is_bounded():
    """2^27 samples (1 GiB) at N = 4096: the plan holds three staging slots of 16 MiB input + at most 16 MiB rows, two carry
    rows and the partial rows of split groups (< 2 x 768 rows of 32 KiB = 48 MiB) — capped here at 192 MiB in all."""
    n, k = 4096, 64
    rng = np.random.default_rng(5)
    block = stream(rng, n, 32, n)
    x = np.tile(block, (1 << 27) // block.size)
    assert x.nbytes >= 1 << 30
    groups = x.size // n // k
    free0, total = ctypes.c_size_t(), ctypes.c_size_t()
    free1 = ctypes.c_size_t()
    with SpectrumPlan(n, window="hann") as plan:
        plan.integrate(x[: n * k], k)                      # (first call: the runtime's own allocations)
        _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free0), ctypes.byref(total)))
        rows = plan.integrate(x, k, detector="mean", out="power")
        _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free1), ctypes.byref(total)))
    held = int(free0.value) - int(free1.value)
    print(f"device memory taken by the 1 GiB call: {held / 2**20:.1f} MiB")
    assert held <= 192 << 20, held
    p = ref_power(np.concatenate([block, block]), n, k, n, "hann", True)
    assert rows.shape == (groups, n)
    check_amplitude(rows[[0, groups // 2, groups - 1]], "power", np.tile(p, (3, 1)), 3, k, "mean", "1 GiB")


def test_cli_psd_integrate_writes_integrated_db_rows(tmp_path, capsys):
    base = str(tmp_path / "rec")
    assert cli.main(["synth", base, "--frames", "40", "--nfft", "4096"]) == 0
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", "8", "--detector", "max", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["integrated_rows"] == 5 and report["integrate_k"] == 8
    from sdr_iq_visualizer_amd import sigmf_io
    samples, _ = sigmf_io.read_sigmf(base + ".sigmf-meta")
    ref = pkg.integrated_db(np.asarray(samples, dtype=np.complex64), 4096, 8, detector="max")
    with np.load(out) as z:
        assert same_bits(z["integrated_db"], ref)
        assert "power_db" in z and "welch_pxx" not in z
    assert cli.main(["psd", base + ".sigmf-meta", "--out", out]) == 0
    with np.load(out) as z:
        assert sorted(z.files) == ["freqs", "power_db"]


def test_refusals_on_a_device():
    lib = _ffi.lib()
    with SpectrumPlan(64, precision="double") as p64, DevBuf(1024) as d:
        st = lib.sdrk_exec_device_integrated(p64.handle, d.p, 1, 1, 64, 0, 0, 1.0, d.p, None)
        assert st == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        with pytest.raises(ValueError):
            p64.integrate(np.zeros(64, np.complex64), 1)
    with SpectrumPlan(64) as p, DevBuf(1024) as d:
        for args in ((0, 1, 64, 0, 0), (1, 0, 64, 0, 0), (1, 1, 0, 0, 0), (1, 1, 64, 3, 0), (1, 1, 64, 0, 2)):
            g, k, stride, det, form = args
            assert lib.sdrk_exec_device_integrated(p.handle, d.p, g, k, stride, det, form, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
            assert lib.sdrk_exec_host_integrated(p.handle, d.p, g, k, stride, det, form, 1.0, d.p) == _ffi.SDRK_ERR_INVALID
        ms = p.exec_device_integrated_timed_each(d.p.value, 1, 1, d.p.value + 512, launches=3)
        assert len(ms) == 3 and all(v > 0 for v in ms)


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8 (24 resident workgroups): other split factors, more groups than the grid at every size — in a child
    process, as the plans read the variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "amplitude_bound or k_4096 or in_db or bit_identical or repeated or across_chunks or larger_than_the_staging"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

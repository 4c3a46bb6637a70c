"""Spectral kurtosis on the GPU: per group of K frames the mean power (plane 0) and SK = (K+1)/(K-1) (K S2/S1^2 - 1) (plane 1)
from sdrk_exec_device_sk* / sdrk_exec_host_sk*, against float64 numpy on the same samples (tests.gpu_helpers.ref_power, fold32 /
ref64 behind the filter bank, then S1, S2 and SK in float64) — never against the library.

The bound on plane 1 is derived, not tuned: first-order propagation of the project's amplitude bar and of plain float32
summation through the estimator.  Per group and bin, with a_f = sqrt(p_f), S_g the group's largest reference amplitude,
d = REL_TOL * S_g, u = 2^-24 and c = (K+1)/(K-1):

    E1  = sum_f (2 a_f d + d^2) + K u S1
    E2  = sum_f (4 a_f^3 d + 6 a_f^2 d^2) + (K+2) u S2
    tol = 2 c (K S2/S1^2) (E2/S2 + 2 E1/S1) + 8 u c (K S2/S1^2 + 1)

(the factor 2 covers the second-order terms; the last term the roundings of the expression itself).  Plane 0:
|sqrt(R_got) - sqrt(R_ref)| <= REL_TOL * S_g + (K u / 2) sqrt(R_ref) — the amplitude bar plus the drift of an uncompensated sum.
Every check prints its worst err/tol."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
from tests.gpu_helpers import (DevBuf, fold32, ref64, ref_power, same_bits_f32 as same_bits, stream16_noise_tone,
                               stream_noise_tone as stream, widen_flat)
from tests.parity import REL_TOL, mag_from_db

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-12
U = 2.0 ** -24
FORMS = ("db", "power")


def hop_of(kind, n):
    return {"packed": n, "half": n // 2, "gapped": n + n // 3 + 1}[kind]


def device_sk(plan, x, groups, k, hop, out="db", scale=1.0, entry="exec_device_sk"):
    """(groups, 2, nfft) float32 from a device entry; x: the stream as that entry reads it."""
    with DevBuf(x.nbytes) as d_in, DevBuf(groups * 2 * plan.nfft * 4) as d_out:
        d_in.put(x)
        d_out.put(np.full((groups, 2, plan.nfft), np.nan, np.float32))
        getattr(plan, entry)(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, out=out, scale=scale)
        plan.sync()
        return d_out.get((groups, 2, plan.nfft), np.float32)


def host_sk(plan, x, k, hop, out="db", scale=1.0, entry="spectral_kurtosis"):
    mean_rows, sk_rows = getattr(plan, entry)(x, k, hop, out, scale)
    assert mean_rows.base is sk_rows.base and mean_rows.base is not None          # two views of one array
    return mean_rows.base


def ref_sk(p, groups, k):
    """float64 (S1, S2, SK, tol, S_g) of the reference powers p (frames, n)."""
    g = p[: groups * k].reshape(groups, k, -1)
    s1, s2 = g.sum(axis=1), (g * g).sum(axis=1)
    c = (k + 1.0) / (k - 1.0)
    ratio = k * s2 / s1 ** 2
    a = np.sqrt(g)
    s_g = a.reshape(groups, -1).max(axis=1)
    d = (REL_TOL * s_g)[:, None, None]
    e1 = (2 * a * d + d * d).sum(axis=1) + k * U * s1
    e2 = (4 * a ** 3 * d + 6 * a * a * d * d).sum(axis=1) + (k + 2) * U * s2
    tol = 2 * c * ratio * (e2 / s2 + 2 * e1 / s1) + 8 * U * c * (ratio + 1)
    return s1, s2, c * (ratio - 1.0), tol, s_g


def check_planes(got, form, scale, p, groups, k, what):
    """Both planes of got (groups, 2, n) against the float64 reference; -> the worst err/tol of plane 1."""
    s1, _, sk, tol, s_g = ref_sk(p, groups, k)
    assert got.shape == (groups, 2, p.shape[1]) and got.dtype == np.float32, (what, got.shape)
    r = s1 / k
    if form == "db":
        a_got, a_ref = mag_from_db(got[:, 0]), np.sqrt(r) + EPS
    else:
        a_got, a_ref = np.sqrt(got[:, 0].astype(np.float64) / scale), np.sqrt(r)
    bound0 = REL_TOL * s_g[:, None] + (k * U / 2) * np.sqrt(r)
    w0 = float((np.abs(a_got - a_ref) / bound0).max())
    w1 = float((np.abs(got[:, 1].astype(np.float64) - sk) / tol).max())
    print(f"{what}: plane 0 err/bound {w0:.2e}, plane 1 err/tol {w1:.2e}")
    assert w0 <= 1.0, (what, "plane 0", w0)
    assert np.all(np.isfinite(got[:, 1])) and w1 <= 1.0, (what, "plane 1", w1)
    return w1


# (n, k, groups, hop, window, shift): noise plus an off-bin tone
CASES = [
    (4096, 2, 5, "packed", None, True),
    (4096, 3, 1000, "half", None, True),          # more groups than the resident grid
    (4096, 64, 1, "packed", "hann", True),        # split into slices: partials and finalize
    (4096, 16, 40, "half", "hann", False),
    (64, 7, 9, "gapped", None, True),
    (1000, 5, 3, "half", "hann", True),           # chirp-z
    (1024, 100, 2, "packed", None, False),
    (65536, 3, 2, "packed", "hann", True),
]
SUBSET_FOR_8_CUS = "sk_parity or known or across_chunks or repeated or int16 or filter_bank"     # (not this test itself)


@pytest.mark.parametrize("n,k,groups,hop_kind,window,shift", CASES)
def test_sk_parity_with_float64_numpy(n, k, groups, hop_kind, window, shift):
    rng = np.random.default_rng(n * 31 + k)
    hop = hop_of(hop_kind, n)
    x = stream(rng, n, groups * k, hop)
    p = ref_power(x, n, groups * k, hop, window, shift)
    what = f"N={n} K={k} G={groups} {hop_kind} {window}"
    with SpectrumPlan(n, window=window, eps=EPS, shift=shift) as plan:
        for form, scale in (("db", 1.0), ("power", 0.25)):
            check_planes(device_sk(plan, x, groups, k, hop, form, scale), form, scale, p, groups, k, f"{what} {form}")
        check_planes(host_sk(plan, x, k, hop), "db", 1.0, p, groups, k, f"{what} host")


# ---- known answers (N = 4096, K = 64): asserted on the reference first ("input:"), then on the result ------------------------
N, K = 4096, 64


def _noise_and_tone(rng, on):
    """K packed frames of unit noise; an on-bin tone 20 dB over the noise's per-bin level in the frames `on` marks."""
    x = (rng.standard_normal(K * N) + 1j * rng.standard_normal(K * N)) / np.sqrt(2)
    tone = 10.0 / np.sqrt(N) * np.exp(2j * np.pi * (500 / N) * np.arange(K * N))
    return (x + tone * np.repeat(on, N)).astype(np.complex64), (500 + N // 2) % N          # (its position in a shifted row)


def _known(x):
    p = ref_power(x, N, K, N, None, True)
    with SpectrumPlan(N, eps=EPS) as plan:
        got = device_sk(plan, x, 1, K, N)
        assert same_bits(got, host_sk(plan, x, K, N))
    return p, ref_sk(p, 1, K), got


def test_known_a_carrier_drives_sk_towards_zero():
    x, b = _noise_and_tone(np.random.default_rng(7), np.ones(K))
    p, (_, _, sk, _, _), got = _known(x)
    assert sk[0, b] < 0.1, ("input:", sk[0, b])
    check_planes(got, "db", 1.0, p, 1, K, "CW")
    assert got[0, 1, b] < 0.1, got[0, 1, b]


def test_known_a_pulsed_carrier_drives_sk_well_above_one():
    x, b = _noise_and_tone(np.random.default_rng(8), (np.arange(K) % 8 == 0).astype(np.float64))
    p, (_, _, sk, _, _), got = _known(x)
    assert sk[0, b] > 4.0, ("input:", sk[0, b])                     # (about 6.5; a 50 % duty cycle would give SK near 1)
    check_planes(got, "db", 1.0, p, 1, K, "pulsed")
    assert got[0, 1, b] > 4.0, got[0, 1, b]


def test_known_zeros_give_sk_zero_and_the_plans_row_of_a_zero_frame():
    x = np.zeros(K * N, np.complex64)
    with SpectrumPlan(N, window="hann", eps=EPS) as plan:
        zero_row = plan.spectrum_db(x[:N])
        for groups, k in ((1, K), (32, 2)):                         # split, and unsplit on every device
            for got in (device_sk(plan, x, groups, k, N), host_sk(plan, x, k, N)):
                assert np.array_equal(got[:, 1].view(np.uint32), np.zeros((groups, N), np.uint32))      # +0.0 exactly
                assert all(same_bits(row, zero_row) for row in got[:, 0])
    with SpectrumPlan(1024, eps=EPS) as plan:                       # the column kernel and its finalize
        got = device_sk(plan, x[: 1024 * K], 1, K, 1024)
        assert np.array_equal(got[:, 1].view(np.uint32), np.zeros((1, 1024), np.uint32))
        assert same_bits(got[0, 0], plan.spectrum_db(x[:1024]))


def test_known_identical_frames_give_sk_zero_within_tol():
    rng = np.random.default_rng(9)
    x = np.tile(stream(rng, N, 1, N), K)
    p = ref_power(x, N, K, N, "hann", True)
    _, _, sk, tol, _ = ref_sk(p, 1, K)
    assert np.all(np.abs(sk) <= tol), ("input:", float(np.abs(sk / tol).max()))
    with SpectrumPlan(N, window="hann", eps=EPS) as plan:
        got = device_sk(plan, x, 1, K, N)
    w = float((np.abs(got[:, 1]) / tol).max())
    print(f"identical frames: |SK|/tol {w:.2e}")
    assert w <= 1.0, w


# ---- bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,groups", [(4096, 101, 12), (1024, 100, 45)])
def test_host_entry_equals_device_entry_across_chunks(n, k, groups):
    """More than two 16 MiB chunks, groups (and, where they are split, slices) straddling them: the carried sums continue, so
    pageable and pinned host arrays give the device entry's bits in both planes."""
    rng = np.random.default_rng(n + k)
    x = stream(rng, n, groups * k, n)
    assert x.nbytes > 2 * (16 << 20) and ((16 << 20) // (n * 8)) % k != 0
    xp = pinned_empty(x.shape, np.complex64)
    xp[:] = x
    with SpectrumPlan(n, window="hann") as plan:
        for form in FORMS:
            dev = device_sk(plan, x, groups, k, n, form, 0.5)
            assert same_bits(host_sk(plan, x, k, n, form, 0.5), dev), (form, "pageable")
            assert same_bits(host_sk(plan, xp, k, n, form, 0.5), dev), (form, "pinned")


def test_repeated_calls_give_identical_bits():
    rng = np.random.default_rng(2)
    for n, k, groups in ((4096, 64, 1), (4096, 7, 900), (1024, 50, 3)):
        x = stream(rng, n, groups * k, n)
        with SpectrumPlan(n, window="hann") as plan:
            a = device_sk(plan, x, groups, k, n)
            assert same_bits(a, device_sk(plan, x, groups, k, n)), n
            assert same_bits(a, host_sk(plan, x, k, n)), (n, "host")


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 5, 40, 4096), (4096, 33, 2, 1001), (1024, 9, 7, 512), (1000, 4, 3, 1000)])
def test_int16_entries_equal_the_complex64_entries_on_the_widened_samples(n, k, groups, hop):
    iq = stream16_noise_tone(n + k, n, groups * k, hop)
    wide = widen_flat(iq)
    with SpectrumPlan(n, window="hann") as plan:
        for form in FORMS:
            want = device_sk(plan, wide, groups, k, hop, form, 2.0)
            assert same_bits(device_sk(plan, iq, groups, k, hop, form, 2.0, "exec_device_sk_ci16"), want), (n, form)
        assert same_bits(host_sk(plan, iq, k, hop, entry="spectral_kurtosis_ci16"), host_sk(plan, wide, k, hop)), n


@pytest.mark.parametrize("n,k,groups,hop_kind", [(1024, 6, 5, "half"), (1000, 3, 4, "packed")])
def test_filter_bank_entries_equal_the_complex64_entry_on_the_packed_folded_frames(n, k, groups, hop_kind):
    taps, hop = 3, hop_of(hop_kind, n)
    rng = np.random.default_rng(n)
    x = stream(rng, taps * n, groups * k, hop)
    h = pfb_prototype(n, taps)
    y = fold32(x, h, n, taps, groups * k, hop).reshape(-1)
    iq = stream16_noise_tone(n, taps * n, groups * k, hop)
    y16 = fold32(widen_flat(iq), h, n, taps, groups * k, hop).reshape(-1)
    with SpectrumPlan(n) as plan:
        plan.set_pfb(h)
        want = device_sk(plan, y, groups, k, n)
        assert same_bits(device_sk(plan, x, groups, k, hop, entry="exec_device_pfb_sk"), want)
        assert same_bits(host_sk(plan, x, k, hop, entry="pfb_spectral_kurtosis"), want)
        want16 = device_sk(plan, y16, groups, k, n)
        assert same_bits(device_sk(plan, iq, groups, k, hop, entry="exec_device_pfb_sk_ci16"), want16)
        assert same_bits(host_sk(plan, iq, k, hop, entry="pfb_spectral_kurtosis_ci16"), want16)


def test_filter_bank_at_4096_staged_route_against_float64():
    """N = 4096 behind the filter bank folds and transforms per frame and reduces the staged spectra; the plain call on the
    packed folded frames keeps the sums inside the transform.  Both hold the float64 bound; whether their bits agree is
    reported, not required."""
    n, taps, k, groups, hop = 4096, 4, 6, 30, 2048
    rng = np.random.default_rng(41)
    x = stream(rng, taps * n, groups * k, hop)
    h = pfb_prototype(n, taps)
    p = np.abs(ref64(x, h, n, taps, groups * k, hop, True)) ** 2
    with SpectrumPlan(n, eps=EPS) as plan:
        plan.set_pfb(h)
        staged = device_sk(plan, x, groups, k, hop, entry="exec_device_pfb_sk")
        check_planes(staged, "db", 1.0, p, groups, k, "PFB N=4096 staged")
        assert same_bits(host_sk(plan, x, k, hop, entry="pfb_spectral_kurtosis"), staged)
        fused = device_sk(plan, fold32(x, h, n, taps, groups * k, hop).reshape(-1), groups, k, n)
        check_planes(fused, "db", 1.0, p, groups, k, "PFB N=4096 folded frames, fused")
        print(f"PFB N=4096: staged and fused bits agree: {same_bits(staged, fused)}")


def test_existing_integrated_rows_are_unchanged_around_an_sk_call():
    rng = np.random.default_rng(5)
    for n, k, groups in ((4096, 16, 3), (4096, 3, 800), (1024, 10, 4)):
        x = stream(rng, n, groups * k, n)
        with SpectrumPlan(n, window="hann") as plan:
            before = {det: plan.integrate(x, k, n, det) for det in ("mean", "max", "min")}
            sk = host_sk(plan, x, k, n)
            for det, rows in before.items():
                assert same_bits(plan.integrate(x, k, n, det), rows), (n, det)
            assert same_bits(host_sk(plan, x, k, n), sk), n


def test_cli_psd_integrate_sk_adds_its_arrays_and_report_fields(tmp_path, capsys):
    base = str(tmp_path / "rec")
    assert cli.main(["synth", base, "--frames", "40", "--nfft", "4096"]) == 0
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", "8", "--sk", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["sk_rows"] == 5 and report["sk_limits"] == list(pkg.sk_limits(8)) and 0.0 <= report["sk_flagged_fraction"] <= 1.0
    from sdr_iq_visualizer_amd import sigmf_io
    samples, _ = sigmf_io.read_sigmf(base + ".sigmf-meta")
    mean_db, sk = pkg.spectral_kurtosis(np.asarray(samples, dtype=np.complex64), 4096, 8)
    with np.load(out) as z:
        assert same_bits(z["sk"], np.ascontiguousarray(sk)) and same_bits(z["sk_mean_db"], np.ascontiguousarray(mean_db))
        assert "integrated_db" in z
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", "8", "--out", out]) == 0
    with np.load(out) as z:
        assert sorted(z.files) == ["freqs", "integrated_db", "power_db"]


def test_refusals_on_a_device():
    lib = _ffi.lib()
    with SpectrumPlan(64, precision="double") as p64, DevBuf(4096) as d:
        for fn in (lib.sdrk_exec_device_sk, lib.sdrk_exec_device_sk_ci16):
            assert fn(p64.handle, d.p, 1, 2, 64, 0, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        with pytest.raises(ValueError):
            p64.spectral_kurtosis(np.zeros(128, np.complex64), 2)
    with SpectrumPlan(64) as p, DevBuf(4096) as d:
        for g, k, stride, form in ((1, 1, 64, 0), (1, 0, 64, 0), (0, 2, 64, 0), (1, 2, 0, 0), (1, 2, 64, 2)):
            for suffix in ("sk", "sk_ci16"):
                assert getattr(lib, f"sdrk_exec_device_{suffix}")(p.handle, d.p, g, k, stride, form, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
                assert lib.sdrk_last_error()
                assert getattr(lib, f"sdrk_exec_host_{suffix}")(p.handle, d.p, g, k, stride, form, 1.0, d.p) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_sk(p.handle, d.p, 1, 1, 64, 0, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
        assert b"k_frames must be >= 2" in lib.sdrk_last_error()
        # a plan without a prototype, for the filter-bank forms; after all the refusals the plan still works
        for suffix in ("pfb_sk", "pfb_sk_ci16"):
            assert getattr(lib, f"sdrk_exec_device_{suffix}")(p.handle, d.p, 1, 2, 64, 0, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID
            assert b"prototype" in lib.sdrk_last_error()
        ms = p.exec_device_sk_timed_each(d.p.value, 1, 2, d.p.value + 2048, launches=3)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        p.set_pfb(pfb_prototype(64, 2))
        for entry in ("exec_device_sk_ci16_timed_each", "exec_device_pfb_sk_timed_each", "exec_device_pfb_sk_ci16_timed_each"):
            ms = getattr(p, entry)(d.p.value, 1, 2, d.p.value + 2048, launches=2)
            assert len(ms) == 2 and all(v > 0 for v in ms), entry
    with SpectrumPlan(64, window="hann") as pw, DevBuf(4096) as d:
        for suffix in ("pfb_sk", "pfb_sk_ci16"):
            assert getattr(lib, f"sdrk_exec_host_{suffix}")(pw.handle, d.p, 1, 2, 64, 0, 1.0, d.p) == _ffi.SDRK_ERR_INVALID
            assert b"SDRK_WINDOW_RECT" in lib.sdrk_last_error()


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8 (24 resident workgroups): other split factors, more groups than the grid at every size — in a child
    process, as the plans read the variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", SUBSET_FOR_8_CUS],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

"""Two-channel cross-spectra on the GPU: per group of K frames the four planes scale*Saa/K, scale*Sbb/K, scale*Sre/K, scale*Sim/K
(A conj B) from sdrk_exec_device_xspec* / sdrk_exec_host_xspec*, against float64 numpy on the same samples (numpy.fft of each
channel, the products and sums in float64) — never against the library.

The bounds are derived, not tuned.  Per group and bin, with a_f = |A_f|, b_f = |B_f|, S_a and S_b each channel's largest
reference amplitude in the group, d_a = REL_TOL * S_a, d_b = REL_TOL * S_b (the project's amplitude bar on each spectrum) and
u = 2^-24:

    planes 2, 3:  tol = 2 [ sum_f (a_f d_b + b_f d_a + d_a d_b) + (K + 2) u sum_f a_f b_f ] scale / K

(first-order propagation of the bar through one product, two roundings per term and K of the plain float32 sum; the factor 2
covers the second-order terms).  Planes 0, 1: the plane-0 bound of tests/test_sk_gpu.py, |sqrt(R_got) - sqrt(R_ref)| <=
REL_TOL * S + (K u / 2) sqrt(R_ref).  Every check prints its worst err/tol.

Measured on the device (profiles/xspec/SUMMARY.md): worst err/tol 2.8e-2 on planes 0 and 1, 6.0e-3 on planes 2 and 3."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import CrossSpectrum, SpectrumPlan
from tests.gpu_helpers import DevBuf, same_bits_f32 as same_bits, window_of
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def hop_of(kind, n):
    return {"packed": n, "half": n // 2, "gapped": n + n // 3 + 1}[kind]


# ---- inputs: 12-bit integers, so that the int16 form sees the same data -----------------------------------------------------
def to16(x0, x1):
    """Two complex streams -> (L, 2, 2) int16 elements, rounded and clipped to 12 bits."""
    out = np.empty((x0.shape[0], 2, 2), np.int16)
    for c, x in enumerate((x0, x1)):
        out[:, c, 0] = np.clip(np.rint(x.real), -2048, 2047)
        out[:, c, 1] = np.clip(np.rint(x.imag), -2048, 2047)
    return out


def noise(rng, L, sigma):
    return (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * (sigma / np.sqrt(2))


def elements16(seed, n, frames, hop):
    """Channel 0: a common component plus its own noise plus an off-bin tone; channel 1: the common component scaled and
    phase-rotated plus its own noise."""
    rng = np.random.default_rng(seed)
    L = (frames - 1) * hop + n
    common = noise(rng, L, 150.0)
    tone = min(150.0 * 10 ** 1.5 / np.sqrt(n), 900.0) * np.exp(2j * np.pi * (0.1234 + 0.37 / n) * np.arange(L))
    return to16(common + noise(rng, L, 100.0) + tone, 0.7 * np.exp(0.9j) * common + noise(rng, L, 100.0))


def widen2(x16):
    """(L, 2, 2) int16 -> (L, 2) complex64, exactly."""
    return np.ascontiguousarray(x16).astype(np.float32).view(np.complex64).reshape(-1, 2)


# ---- the float64 reference and the derived bounds ---------------------------------------------------------------------------
def ref_spectra(x16, n, frames, hop, window, shift):
    """float64 (A, B), each (frames, n) complex128 in the plan's bin order."""
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n)[None, :]
    z = x16.astype(np.float64)
    out = []
    for c in range(2):
        s = np.fft.fft((z[:, c, 0] + 1j * z[:, c, 1])[idx] * window_of(window, n), axis=-1)
        out.append(np.fft.fftshift(s, axes=-1) if shift else s)
    return out


class Ref:
    """The four float64 means (groups, n) per unit scale, and the bounds of the module docstring (per unit scale too)."""

    def __init__(self, A, B, groups, k):
        A, B = (s[: groups * k].reshape(groups, k, -1) for s in (A, B))
        a, b = np.abs(A), np.abs(B)
        c = (A * np.conj(B)).sum(axis=1)
        self.k = k
        self.paa, self.pbb = (a * a).sum(axis=1) / k, (b * b).sum(axis=1) / k
        self.cre, self.cim = c.real / k, c.imag / k
        s_a, s_b = (m.reshape(groups, -1).max(axis=1)[:, None] for m in (a, b))
        d_a, d_b = REL_TOL * s_a[:, None, :], REL_TOL * s_b[:, None, :]
        self.tol_c = 2 * ((a * d_b + b * d_a + d_a * d_b).sum(axis=1) + (k + 2) * U * (a * b).sum(axis=1)) / k
        self.bound_a = REL_TOL * s_a + (k * U / 2) * np.sqrt(self.paa)          # on the amplitude sqrt(R)
        self.bound_b = REL_TOL * s_b + (k * U / 2) * np.sqrt(self.pbb)

    def check(self, got, scale, what):
        """All four planes of got (groups, 4, n); -> the worst err/tol."""
        assert got.shape == (self.paa.shape[0], 4, self.paa.shape[1]) and got.dtype == np.float32, (what, got.shape)
        assert np.all(np.isfinite(got)), what
        g = got.astype(np.float64) / scale
        w = [float((np.abs(np.sqrt(g[:, 0]) - np.sqrt(self.paa)) / self.bound_a).max()),
             float((np.abs(np.sqrt(g[:, 1]) - np.sqrt(self.pbb)) / self.bound_b).max()),
             float((np.abs(g[:, 2] - self.cre) / self.tol_c).max()),
             float((np.abs(g[:, 3] - self.cim) / self.tol_c).max())]
        print(f"{what}: err/tol of planes 0..3 " + " ".join(f"{v:.2e}" for v in w))
        assert max(w) <= 1.0, (what, w)
        return max(w)

    # what the plane bounds allow the derived quantities to move (first order, doubled)
    def power_tols(self):
        return (2 * np.sqrt(self.paa) * self.bound_a + self.bound_a ** 2, 2 * np.sqrt(self.pbb) * self.bound_b + self.bound_b ** 2)

    def coherence(self):
        return (self.cre ** 2 + self.cim ** 2) / (self.paa * self.pbb)

    def coherence_tol(self):
        ta, tb = self.power_tols()
        c2 = self.cre ** 2 + self.cim ** 2
        return 2 * self.coherence() * (2 * (np.abs(self.cre) + np.abs(self.cim)) * self.tol_c / c2 + ta / self.paa + tb / self.pbb)

    def phase(self):
        return np.arctan2(self.cim, self.cre)

    def phase_tol(self):
        return 2 * (np.abs(self.cre) + np.abs(self.cim)) * self.tol_c / (self.cre ** 2 + self.cim ** 2)


def reference(x16, n, groups, k, hop, window, shift):
    A, B = ref_spectra(x16, n, groups * k, hop, window, shift)
    return Ref(A, B, groups, k)


# ---- the entries ------------------------------------------------------------------------------------------------------------
def device_xs(plan, x, groups, k, hop, scale=1.0, entry="exec_device_xspec"):
    """(groups, 4, nfft) float32 from a device entry; x: the element stream as that entry reads it."""
    with DevBuf(x.nbytes) as d_in, DevBuf(groups * 4 * plan.nfft * 4) as d_out:
        d_in.put(x)
        d_out.put(np.full((groups, 4, plan.nfft), np.nan, np.float32))
        getattr(plan, entry)(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, scale=scale)
        plan.sync()
        return d_out.get((groups, 4, plan.nfft), np.float32)


def host_xs(plan, x, k, hop, scale=1.0, entry="cross_spectrum"):
    r = getattr(plan, entry)(x, k, hop, scale)
    assert isinstance(r, CrossSpectrum) and all(v.base is r.paa.base for v in r) and r.paa.base is not None   # views of one array
    return r.paa.base


def wrap(phi):
    return (phi + np.pi) % (2 * np.pi) - np.pi


# (n, k, groups, hop, window, shift): the shapes of tests/test_sk_gpu.py::CASES, the smallest that reach every route
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
SUBSET_FOR_8_CUS = "xspec_parity or known or across_chunks or repeated or int16 or swapped or sk_plane"   # (not this test itself)


@pytest.mark.parametrize("n,k,groups,hop_kind,window,shift", CASES)
def test_xspec_parity_with_float64_numpy(n, k, groups, hop_kind, window, shift):
    hop = hop_of(hop_kind, n)
    x16 = elements16(n * 31 + k, n, groups * k, hop)
    x = widen2(x16)
    ref = reference(x16, n, groups, k, hop, window, shift)
    what = f"N={n} K={k} G={groups} {hop_kind} {window}"
    with SpectrumPlan(n, window=window, shift=shift) as plan:
        for scale in (1.0, 0.25):
            ref.check(device_xs(plan, x, groups, k, hop, scale), scale, f"{what} device scale {scale}")
            ref.check(host_xs(plan, x, k, hop, scale), scale, f"{what} host scale {scale}")


# ---- bit identities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,groups", [(4096, 101, 6), (1024, 100, 22)])
def test_host_entry_equals_device_entry_across_chunks(n, k, groups):
    """At least 2^21 elements, more than two 16 MiB host chunks, groups (and, where they are split, slices) straddling them:
    the carried sums continue, so pageable and pinned host arrays give the device entry's bits in all four planes."""
    x = widen2(elements16(n + k, n, groups * k, n))
    assert x.shape[0] >= 1 << 21 and x.nbytes > 2 * (16 << 20) and ((16 << 20) // (n * 16)) % k != 0
    xp = pinned_empty(x.shape, np.complex64)
    xp[:] = x
    with SpectrumPlan(n, window="hann") as plan:
        dev = device_xs(plan, x, groups, k, n, 0.5)
        assert same_bits(host_xs(plan, x, k, n, 0.5), dev), "pageable"
        assert same_bits(host_xs(plan, xp, k, n, 0.5), dev), "pinned"


def test_repeated_calls_give_identical_bits():
    for n, k, groups in ((4096, 64, 1), (4096, 7, 600), (1024, 50, 3)):
        x = widen2(elements16(n + groups, n, groups * k, n))
        with SpectrumPlan(n, window="hann") as plan:
            a = device_xs(plan, x, groups, k, n)
            assert same_bits(a, device_xs(plan, x, groups, k, n)), n
            assert same_bits(a, host_xs(plan, x, k, n)), (n, "host")


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 5, 40, 4096), (4096, 33, 2, 1001), (1024, 9, 7, 512), (1000, 4, 3, 1000),
                                            (4096, 1, 3, 4096)])
def test_int16_entries_equal_the_complex64_entries_on_the_widened_elements(n, k, groups, hop):
    x16 = elements16(n + k, n, groups * k, hop)
    wide = widen2(x16)
    with SpectrumPlan(n, window="hann") as plan:
        want = device_xs(plan, wide, groups, k, hop, 2.0)
        assert same_bits(device_xs(plan, x16, groups, k, hop, 2.0, "exec_device_xspec_ci16"), want), n
        assert same_bits(host_xs(plan, x16, k, hop, 2.0, "cross_spectrum_ci16"), want), (n, "host")
        assert same_bits(host_xs(plan, x16.reshape(-1, 4), k, hop, 2.0, "cross_spectrum_ci16"), want), (n, "(n, 4)")


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 6, 30, 2048), (4096, 40, 2, 4096), (1024, 9, 7, 1024), (1000, 4, 3, 1000)])
def test_swapped_channels_give_the_exact_conjugate_and_identical_channels_no_imaginary_part(n, k, groups, hop):
    x = widen2(elements16(3 * n + k, n, groups * k, hop))
    with SpectrumPlan(n, window="hann") as plan:
        ab = device_xs(plan, x, groups, k, hop)
        ba = device_xs(plan, np.ascontiguousarray(x[:, ::-1]), groups, k, hop)
        assert same_bits(ba[:, 0], ab[:, 1]) and same_bits(ba[:, 1], ab[:, 0]) and same_bits(ba[:, 2], ab[:, 2])
        assert np.array_equal(ba[:, 3], -ab[:, 3])                            # as values: a zero's sign may differ
        aa = device_xs(plan, np.ascontiguousarray(np.repeat(x[:, :1], 2, axis=1)), groups, k, hop)
        assert np.array_equal(aa[:, 3], np.zeros_like(aa[:, 3]))
        assert same_bits(aa[:, 0], ab[:, 0]) and same_bits(aa[:, 1], ab[:, 0])


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 5, 40, 4096), (4096, 64, 1, 4096), (4096, 3, 700, 2048), (1024, 9, 7, 512),
                                            (1024, 100, 2, 1024)])
def test_auto_planes_equal_the_sk_plane_of_mean_power_on_each_channel(n, k, groups, hop):
    """Planes 0 and 1 carry the bits of plane 0 of exec_device_sk (power form, the same scale) on the de-interleaved channel."""
    x = widen2(elements16(5 * n + k, n, groups * k, hop))
    with SpectrumPlan(n, window="hann") as plan:
        xs = device_xs(plan, x, groups, k, hop, 0.5)
        for c in range(2):
            ch = np.ascontiguousarray(x[:, c])
            with DevBuf(ch.nbytes) as d_in, DevBuf(groups * 2 * n * 4) as d_out:
                d_in.put(ch)
                plan.exec_device_sk(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, out="power", scale=0.5)
                plan.sync()
                sk = d_out.get((groups, 2, n), np.float32)
            assert same_bits(xs[:, c], sk[:, 0]), (n, k, "channel", c)


def test_existing_integrated_rows_are_unchanged_around_a_cross_spectrum_call():
    for n, k, groups in ((4096, 16, 3), (4096, 3, 600), (1024, 10, 4)):
        x = widen2(elements16(7 * n + k, n, groups * k, n))
        ch0 = np.ascontiguousarray(x[:, 0])
        with SpectrumPlan(n, window="hann") as plan:
            before = plan.integrate(ch0, k, n, "mean")
            xs = host_xs(plan, x, k, n)
            assert same_bits(plan.integrate(ch0, k, n, "mean"), before), n
            assert same_bits(host_xs(plan, x, k, n), xs), n


# ---- known answers (N = 4096, K = 16): asserted on the float64 reference first ("input:"), then on the result ----------------
N, K = 4096, 16


def _known(x16, window=None, hop=N):
    ref = reference(x16, N, 1, K, hop, window, True)
    with SpectrumPlan(N, window=window) as plan:
        got = device_xs(plan, widen2(x16), 1, K, hop)
        res = plan.cross_spectrum_ci16(x16, K, hop)
        assert same_bits(res.paa.base, got)
    ref.check(got, 1.0, "known")
    return ref, res


def test_known_a_quarter_turn_between_the_channels_gives_coherence_one_and_phase_minus_half_pi():
    rng = np.random.default_rng(7)
    x0 = noise(rng, K * N, 300.0)
    x16 = to16(x0, x0)
    x16[:, 1, 0], x16[:, 1, 1] = -x16[:, 0, 1], x16[:, 0, 0]                  # channel 1 = i * channel 0, exactly
    ref, res = _known(x16)
    powered = ref.paa > 0
    assert powered.all() and np.abs(ref.coherence() - 1).max() < 1e-12, "input:"
    assert np.abs(ref.phase() + np.pi / 2).max() < 1e-12, "input:"
    w_c = float((np.abs(res.coherence - 1) / ref.coherence_tol()).max())
    w_p = float((np.abs(res.phase + np.pi / 2) / ref.phase_tol()).max())
    print(f"quarter turn: coherence err/tol {w_c:.2e}, phase err/tol {w_p:.2e}")
    assert w_c <= 1.0 and w_p <= 1.0, (w_c, w_p)


def test_known_independent_noise_gives_a_mean_coherence_of_one_over_k():
    rng = np.random.default_rng(8)
    ref, res = _known(to16(noise(rng, K * N, 300.0), noise(rng, K * N, 300.0)))
    m_ref = float(ref.coherence().mean())
    # per bin the coherence of independent Gaussian noise has mean 1/K and a standard deviation below 1/K; N bins average it
    assert abs(m_ref - 1 / K) < 5 / (K * np.sqrt(N)), ("input:", m_ref)
    m_got, slack = float(res.coherence.mean()), float(ref.coherence_tol().mean())
    print(f"independent noise: mean coherence {m_got:.6f}, reference {m_ref:.6f}, 1/K {1 / K:.6f}, allowed {slack:.2e}")
    assert abs(m_got - m_ref) <= slack
    assert abs(m_got - 1 / K) < 5 / (K * np.sqrt(N)) + slack


def test_known_a_delay_of_three_samples_gives_a_phase_ramp():
    """Channel 1 = channel 0 delayed by 3 samples on one continuous stream, Hann: B = A exp(-2 pi i 3 k / N) up to what the
    window's edges see differently, so the phase of A conj(B) follows 2 pi 3 k / N."""
    rng = np.random.default_rng(9)
    L = K * N
    x = noise(rng, L + 3, 300.0)
    ref, res = _known(to16(x[3:], x[:L]), "hann")
    ramp = 2 * np.pi * 3 * (np.arange(N) - N // 2) / N                         # the shifted row: bin k - N/2 at position k
    dev_ref = np.abs(wrap(ref.phase()[0] - ramp))
    # the window sits 3 samples further along channel 1's copy of the signal: w[n + 3] - w[n] is at most 3 pi / N of its peak,
    # which is how far B may be off A exp(-i theta) in relative terms; twice that for the phase of a sum of K such terms
    edge = 2 * 3 * np.pi / N
    assert dev_ref.max() < edge, ("input:", float(dev_ref.max()))
    err = np.abs(wrap(res.phase[0] - ref.phase()[0]))
    w = float((err / ref.phase_tol()[0]).max())
    print(f"delay: reference off the ramp by {dev_ref.max():.2e} rad at most, result off the reference {err.max():.2e} rad, err/tol {w:.2e}")
    assert w <= 1.0, w
    assert np.abs(wrap(res.phase[0] - ramp)).max() < edge + float(ref.phase_tol().max())


# ---- the rest ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device():
    lib = _ffi.lib()
    each = (ctypes.c_float * 2)()
    with SpectrumPlan(64, precision="double") as p64, DevBuf(8192) as d:
        for fn in (lib.sdrk_exec_device_xspec, lib.sdrk_exec_device_xspec_ci16):
            assert fn(p64.handle, d.p, 1, 2, 64, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        for fn in (lib.sdrk_exec_host_xspec, lib.sdrk_exec_host_xspec_ci16):
            assert fn(p64.handle, d.p, 1, 2, 64, 1.0, d.p) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        with pytest.raises(ValueError):
            p64.cross_spectrum(np.zeros((128, 2), np.complex64), 2)
    with SpectrumPlan(64) as p, DevBuf(16384) as d:
        bad = (((1, 0, 64), b"must be >= 1"), ((0, 2, 64), b"must be >= 1"), ((1 << 40, 1 << 40, 64), b"out of range"),
               ((1, 2, 0), b"frame_stride"))
        for suffix in ("xspec", "xspec_ci16"):
            dev, host = getattr(lib, f"sdrk_exec_device_{suffix}"), getattr(lib, f"sdrk_exec_host_{suffix}")
            timed = getattr(lib, f"sdrk_exec_device_{suffix}_timed_each")
            for (g, k, stride), msg in bad:
                assert dev(p.handle, d.p, g, k, stride, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID and msg in lib.sdrk_last_error()
                assert host(p.handle, d.p, g, k, stride, 1.0, d.p) == _ffi.SDRK_ERR_INVALID and msg in lib.sdrk_last_error()
                assert timed(p.handle, d.p, g, k, stride, 1.0, d.p, 2, each) == _ffi.SDRK_ERR_INVALID and msg in lib.sdrk_last_error()
            assert dev(p.handle, None, 1, 2, 64, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert dev(p.handle, d.p, 1, 2, 64, 1.0, None, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert dev(None, d.p, 1, 2, 64, 1.0, d.p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
            assert timed(p.handle, d.p, 1, 2, 64, 1.0, d.p, 0, each) == _ffi.SDRK_ERR_INVALID and b"launches" in lib.sdrk_last_error()
        # after all the refusals the plan still works: 2 frames of 64 elements in (2 KiB), one group of 4 rows out (1 KiB)
        for entry in ("exec_device_xspec_timed_each", "exec_device_xspec_ci16_timed_each"):
            ms = getattr(p, entry)(d.p.value, 1, 2, d.p.value + 8192, launches=3)
            assert len(ms) == 3 and all(v > 0 for v in ms), entry
        p.set_pfb(np.ones(128, np.float32))                                    # a prototype is ignored
        x = widen2(elements16(1, 64, 6, 64))
        with_proto = device_xs(p, x, 3, 2, 64)
    with SpectrumPlan(64) as p:
        assert same_bits(device_xs(p, x, 3, 2, 64), with_proto)


@pytest.mark.parametrize("datatype", ["cf32_le", "ci16_le"])
def test_cli_psd_integrate_cross_adds_its_arrays_and_report_fields(tmp_path, capsys, datatype):
    n, k, groups = 4096, 4, 3
    x16 = elements16(11, n, groups * k, n)
    x = x16 if datatype == "ci16_le" else widen2(x16)
    base, out = str(tmp_path / "two"), str(tmp_path / "rows.npz")
    sigmf_io.write_sigmf(base, x, 1e6, 1e9, datatype=datatype, num_channels=2)
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", str(k), "--cross", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = pkg.cross_spectrum(x[:, 0], x[:, 1], n, k)                     # the module function: stacks the pair, cached plan
    assert report["cross_rows"] == groups and report["wrote"] == [out] and report["samples"] == groups * k * n
    g, b = np.unravel_index(int(np.argmax(want.coherence)), want.coherence.shape)
    assert report["cross_peak_coherence"] == float(want.coherence[g, b]) and report["cross_peak_row"] == g
    assert report["cross_peak_phase_rad"] == float(want.phase[g, b])
    assert report["cross_median_coherence"] == float(np.median(want.coherence)) and 0.0 <= report["cross_median_coherence"] <= 1.0
    with np.load(out) as z:
        assert same_bits(z["cross_paa"], np.ascontiguousarray(want.paa)) and same_bits(z["cross_pbb"], np.ascontiguousarray(want.pbb))
        assert np.array_equal(z["cross"], want.cross) and np.array_equal(z["coherence"], want.coherence)
        assert np.array_equal(z["phase"], want.phase) and "integrated_db" in z
    with SpectrumPlan(n) as plan:                                          # and both are the plan's own call on the elements
        direct = (plan.cross_spectrum_ci16 if datatype == "ci16_le" else plan.cross_spectrum)(x, k)
        assert same_bits(direct.paa.base, want.paa.base)


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8: other split factors, more groups than the grid at every size — in a child process, as the plans read the
    variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", SUBSET_FOR_8_CUS],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

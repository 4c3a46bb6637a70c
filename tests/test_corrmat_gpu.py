"""The correlation matrix of 2..8 channels on the GPU: per group of K frames the C*C planes of sdrk_exec_device_corrmat* /
sdrk_exec_host_corrmat*, against float64 numpy on the same samples (tests/corrmat_helpers.py has the reference and the derived
bounds, per pair those of tests/test_xspec_gpu.py) — never against the library — and the bit identities of include/sdrk.h:
(a) C = 2 is the two-channel call, (b) every pair of any C is the two-channel call on that pair, (c) int16 and 8-bit are the
complex64 form on the widened elements, (d) the host entry is the device entry however it is chunked, (e) permuting the
channels permutes the planes.

Measured on the device (profiles/corrmat/SUMMARY.md): worst err/tol 1.4e-2 on the auto planes, 3.1e-3 on the
pair planes."""
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
from sdr_iq_visualizer_amd.spectrum import CorrelationMatrix, SpectrumPlan, iq8_to_c64, plane_index
from tests.corrmat_helpers import (device_cm, device_xs, elements16, hop_of, host_cm, noise, pair_planes, pair_stream, reference,
                                   to_ci8, to_cu8, widen_c, wrap)
from tests.gpu_helpers import DevBuf, same_bits_f32 as same_bits

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CHUNK_BYTES = 16 << 20          # csrc/plan_internal.h

# (n, k, groups, hop, window, shift, channels)
CASES = [
    (4096, 2, 5, "packed", None, True, 3),
    (4096, 3, 300, "half", None, True, 5),        # more groups than the resident grid of the spectra kernel's frames per chunk
    (4096, 64, 1, "packed", "hann", True, 8),     # split into slices: partials and finalize
    (64, 7, 9, "gapped", None, True, 4),
    (1000, 5, 3, "half", "hann", True, 3),        # chirp-z
    (1024, 100, 2, "packed", None, False, 8),
    (65536, 3, 2, "packed", "hann", True, 2),
]
SUBSET_FOR_8_CUS = "parity or identity or repeated or known"   # (not this test itself)


@pytest.mark.parametrize("n,k,groups,hop_kind,window,shift,channels", CASES)
def test_corrmat_parity_with_float64_numpy(n, k, groups, hop_kind, window, shift, channels):
    hop = hop_of(hop_kind, n)
    x = widen_c(elements16(n * 31 + k, n, groups * k, hop, channels))
    ref = reference(x, n, groups, k, hop, window, shift)
    what = f"N={n} K={k} G={groups} {hop_kind} {window} C={channels}"
    with SpectrumPlan(n, window=window, shift=shift) as plan:
        for scale in (1.0, 0.25):
            ref.check(device_cm(plan, x, groups, k, hop, scale), scale, f"{what} device scale {scale}")
            ref.check(host_cm(plan, x, k, hop, scale), scale, f"{what} host scale {scale}")


# ---- bit identities ---------------------------------------------------------------------------------------------------------
SHAPES_AB = [(4096, 5, 40, 4096), (4096, 64, 1, 4096), (1024, 9, 7, 1024), (1000, 4, 3, 1000)]


@pytest.mark.parametrize("n,k,groups,hop", SHAPES_AB)
def test_identity_a_two_channels_return_the_bits_of_the_two_channel_call(n, k, groups, hop):
    x = widen_c(elements16(n + k, n, groups * k, hop, 2))
    with SpectrumPlan(n, window="hann") as plan:
        assert same_bits(device_cm(plan, x, groups, k, hop, 0.5), device_xs(plan, x, groups, k, hop, 0.5)), n


@pytest.mark.parametrize("channels", [3, 5])
@pytest.mark.parametrize("n,k,groups,hop", SHAPES_AB + [(4096, 3, 700, 2048)])
def test_identity_b_every_pair_returns_the_bits_of_the_two_channel_call_on_that_pair(n, k, groups, hop, channels):
    """(the (4096, 64, 1) shape is split into slices: what pins the cut the two calls share)"""
    x = widen_c(elements16(3 * n + k + channels, n, groups * k, hop, channels))
    with SpectrumPlan(n, window="hann") as plan:
        cm = device_cm(plan, x, groups, k, hop, 2.0)
        for i in range(channels):
            for j in range(i + 1, channels):
                want = device_xs(plan, pair_stream(x, i, j), groups, k, hop, 2.0)
                assert same_bits(pair_planes(cm, channels, i, j), want), (n, i, j)


@pytest.mark.parametrize("channels", [3, 8])
@pytest.mark.parametrize("n,k,groups,hop", [(4096, 5, 7, 4096), (1024, 9, 4, 512), (1000, 4, 3, 1000)])
def test_identity_c_int16_and_8_bit_equal_complex64_on_the_widened_elements(n, k, groups, hop, channels):
    x16 = elements16(5 * n + k + channels, n, groups * k, hop, channels)
    x7 = elements16(6 * n + k + channels, n, groups * k, hop, channels, bits=7)
    cu8 = to_cu8(x7)
    cu8[0, 0], cu8[1, channels - 1], cu8[n - 1, 1] = (0, 255), (255, 0), (0, 0)     # both ends of the byte range
    with SpectrumPlan(n, window="hann") as plan:
        for xi in (x16, to_ci8(x7), cu8):
            wide = widen_c(xi)
            if xi.dtype != np.int16:
                assert np.array_equal(wide, iq8_to_c64(xi))
            want = device_cm(plan, wide, groups, k, hop, 2.0)
            assert same_bits(device_cm(plan, xi, groups, k, hop, 2.0), want), (n, xi.dtype, "device")
            assert same_bits(host_cm(plan, xi, k, hop, 2.0), want), (n, xi.dtype, "host")
            # the stream one sample into the buffer: aligned to a sample of one channel, not to an element
            assert same_bits(device_cm(plan, xi, groups, k, hop, 2.0, offset_samples=1), want), (n, xi.dtype, "offset")
        assert same_bits(device_cm(plan, widen_c(x16), groups, k, hop, 2.0, offset_samples=1),
                         device_cm(plan, widen_c(x16), groups, k, hop, 2.0)), (n, "complex64 offset")


@pytest.mark.parametrize("n", [4096, 1024])
@pytest.mark.parametrize("channels,form", [(3, "c64"), (5, "cu8")])
def test_identity_d_host_entry_equals_device_entry_across_chunks(n, channels, form):
    """K = 101 and more than three 16 MiB host chunks, cut at element boundaries (the chunk size is no multiple of the element),
    groups straddling them: the carried sums continue, so pageable and pinned host arrays give the device entry's bits."""
    k = 101
    elem = channels * (8 if form == "c64" else 2)
    groups = (3 * HOST_CHUNK_BYTES // (n * elem)) // k + 1
    assert HOST_CHUNK_BYTES % elem != 0 and (HOST_CHUNK_BYTES // (n * elem)) % k != 0
    x = elements16(n + channels, n, groups * k, n, channels, bits=7)
    x = widen_c(x) if form == "c64" else to_cu8(x)
    assert x.nbytes > 3 * HOST_CHUNK_BYTES
    xp = pinned_empty(x.shape, x.dtype)
    xp[:] = x
    with SpectrumPlan(n, window="hann") as plan:
        dev = device_cm(plan, x, groups, k, n, 0.5)
        assert same_bits(host_cm(plan, x, k, n, 0.5), dev), "pageable"
        assert same_bits(host_cm(plan, xp, k, n, 0.5), dev), "pinned"


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 6, 30, 2048), (4096, 40, 2, 4096), (1024, 9, 7, 1024)])
def test_identity_e_reversed_channels_permute_the_planes(n, k, groups, hop):
    C = 5
    x = widen_c(elements16(7 * n + k, n, groups * k, hop, C))
    with SpectrumPlan(n, window="hann") as plan:
        fwd = device_cm(plan, x, groups, k, hop)
        rev = device_cm(plan, np.ascontiguousarray(x[:, ::-1]), groups, k, hop)
    for c in range(C):
        assert same_bits(rev[:, c], fwd[:, C - 1 - c]), c
    for i in range(C):
        for j in range(i + 1, C):
            q, r = plane_index(C, i, j), plane_index(C, C - 1 - j, C - 1 - i)      # reversed: (C-1-j, C-1-i), order flipped
            assert same_bits(rev[:, r], fwd[:, q]), (i, j)
            assert np.array_equal(rev[:, r + 1], -fwd[:, q + 1]), (i, j)           # as values: a zero's sign may differ


def test_repeated_calls_give_identical_bits_and_existing_calls_keep_theirs():
    for n, k, groups in ((4096, 64, 1), (4096, 7, 400), (1024, 50, 3)):
        x = widen_c(elements16(n + groups, n, groups * k, n, 4))
        ch0, pair = np.ascontiguousarray(x[:, 0]), pair_stream(x, 0, 1)
        with SpectrumPlan(n, window="hann") as plan:
            rows, xs = plan.integrate(ch0, k, n, "mean"), device_xs(plan, pair, groups, k, n)
            a = device_cm(plan, x, groups, k, n)
            assert same_bits(a, device_cm(plan, x, groups, k, n)), n
            assert same_bits(a, host_cm(plan, x, k, n)), (n, "host")
            assert same_bits(plan.integrate(ch0, k, n, "mean"), rows), (n, "integrate")
            assert same_bits(device_xs(plan, pair, groups, k, n), xs), (n, "xspec")
            assert same_bits(device_cm(plan, x, groups, k, n), a), (n, "after")


# ---- known answers (N = 4096, K = 16): asserted on the float64 reference first ("input:"), then on the result ----------------
N, K = 4096, 16


def _known(x16, window=None):
    xc = widen_c(x16)
    ref = reference(xc, N, 1, K, N, window, True)
    with SpectrumPlan(N, window=window) as plan:
        got = device_cm(plan, xc, 1, K, N)
        assert same_bits(plan.correlate_ci16(x16, K).planes, got)
    ref.check(got, 1.0, "known")
    return ref, CorrelationMatrix(got, x16.shape[1])


def test_known_plane_wave_on_a_uniform_line_gives_the_phase_steps_and_coherence_one():
    """Channel c = s * exp(i c phi) + independent noise, s a tone on bin B.  Tone amplitude 600 and noise sigma 20 per channel:
    in the tone's bin the tone holds N * 600 against noise of rms sqrt(N) * 20, a per-frame SNR of N * 600^2 / 20^2 = 3.7e6
    (65.7 dB); over K frames the phase of a pair is off by at most ~ 1/sqrt(K * SNR) = 1.3e-4 rad rms and the coherence
    1 - O(2/SNR).  The test allows 6 sigma: 8e-4 rad, and 1 - coherence < 1e-5."""
    C, phi, B = 5, 0.7, 517
    rng = np.random.default_rng(21)
    s = 600.0 * np.exp(2j * np.pi * B * np.arange(K * N) / N)
    x16 = np.empty((K * N, C, 2), np.int16)
    for c in range(C):
        x = s * np.exp(1j * c * phi) + noise(rng, K * N, 20.0)
        x16[:, c, 0], x16[:, c, 1] = np.rint(x.real), np.rint(x.imag)
    ref, cm = _known(x16)
    pos = B + N // 2                                                          # the shifted row
    rm = ref.matrix()
    for i in range(C):
        for j in range(i + 1, C):
            want = wrap((i - j) * phi)                                        # A conj(B): channel i's phase minus channel j's
            assert abs(wrap(rm.phase(i, j)[0, pos] - want)) < 8e-4 and 1 - rm.coherence(i, j)[0, pos] < 1e-5, ("input:", i, j)
            slack_p, slack_c = float(ref.phase_tol(i, j)[0, pos]), float(ref.coherence_tol(i, j)[0, pos])
            assert abs(wrap(cm.phase(i, j)[0, pos] - want)) < 8e-4 + slack_p, (i, j)
            assert abs(cm.phase(j, i)[0, pos] + cm.phase(i, j)[0, pos]) < 1e-12, (i, j)
            assert 1 - cm.coherence(i, j)[0, pos] < 1e-5 + slack_c, (i, j)


def test_known_independent_noise_gives_a_mean_coherence_of_one_over_k():
    C = 4
    rng = np.random.default_rng(22)
    x16 = np.empty((K * N, C, 2), np.int16)
    for c in range(C):
        x = noise(rng, K * N, 300.0)
        x16[:, c, 0], x16[:, c, 1] = np.rint(x.real), np.rint(x.imag)
    ref, cm = _known(x16)
    rm = ref.matrix()
    for i in range(C):
        for j in range(i + 1, C):
            # per bin the coherence of independent Gaussian noise has mean 1/K and a standard deviation below 1/K; N bins average it
            m_ref = float(rm.coherence(i, j).mean())
            assert abs(m_ref - 1 / K) < 5 / (K * np.sqrt(N)), ("input:", i, j, m_ref)
            m_got, slack = float(cm.coherence(i, j).mean()), float(ref.coherence_tol(i, j).mean())
            assert abs(m_got - m_ref) <= slack and abs(m_got - 1 / K) < 5 / (K * np.sqrt(N)) + slack, (i, j, m_got)


@pytest.mark.parametrize("n,k,groups", [(4096, 40, 2), (1024, 9, 7)])
def test_known_identical_channels_have_no_imaginary_part(n, k, groups):
    C = 4
    x = np.ascontiguousarray(np.repeat(widen_c(elements16(n + 1, n, groups * k, n, 2))[:, :1], C, axis=1))
    with SpectrumPlan(n, window="hann") as plan:
        cm = device_cm(plan, x, groups, k, n)
    for i in range(C):
        for j in range(i + 1, C):
            q = plane_index(C, i, j)
            assert np.array_equal(cm[:, q + 1], np.zeros_like(cm[:, q + 1])), (i, j)
            # (the autos agree to the bit; the real plane is the same sum with its products rounded on their own, not fused)
            assert same_bits(cm[:, j], cm[:, 0]) and same_bits(cm[:, q], cm[:, C]), (i, j)


# ---- the rest ---------------------------------------------------------------------------------------------------------------
def _entries(lib, suffix):
    """(device, timed, host) of a form as callables of (plan, ptr, channels, groups, k, stride, out, *tail)."""
    fmt = (0,) if suffix == "corrmat_iq8" else ()
    dev, host = getattr(lib, f"sdrk_exec_device_{suffix}"), getattr(lib, f"sdrk_exec_host_{suffix}")
    timed = getattr(lib, f"sdrk_exec_device_{suffix}_timed_each")
    each = (ctypes.c_float * 2)()
    return (lambda p, d, c, g, k, s, o: dev(p, d, *fmt, c, g, k, s, 1.0, o, None),
            lambda p, d, c, g, k, s, o, launches=2: timed(p, d, *fmt, c, g, k, s, 1.0, o, launches, each),
            lambda p, d, c, g, k, s, o: host(p, d, *fmt, c, g, k, s, 1.0, o))


def test_refusals_on_a_device():
    lib = _ffi.lib()
    INVALID = _ffi.SDRK_ERR_INVALID
    with SpectrumPlan(64, precision="double") as p64, DevBuf(8192) as d:
        for suffix in ("corrmat", "corrmat_ci16", "corrmat_iq8"):
            for fn in _entries(lib, suffix):
                assert fn(p64.handle, d.p, 3, 1, 2, 64, d.p) == INVALID and b"float64" in lib.sdrk_last_error(), suffix
        with pytest.raises(ValueError):
            p64.correlate(np.zeros((128, 3), np.complex64), 2)
    with SpectrumPlan(64) as p, DevBuf(65536) as d:
        bad = (((3, 1, 0, 64), b"must be >= 1"), ((3, 0, 2, 64), b"must be >= 1"), ((3, 1 << 40, 1 << 40, 64), b"out of range"),
               ((3, 1, 2, 0), b"frame_stride"), ((1, 1, 2, 64), b"channels"), ((9, 1, 2, 64), b"channels"),
               ((0, 1, 2, 64), b"channels"), ((-3, 1, 2, 64), b"channels"),
               ((3, 1 << 20, 1 << 20, 1 << 30), b"out of range"),              # the element count overflows
               ((8, 1 << 20, 1 << 20, 1 << 20), b"out of range"))              # ... or its byte size does
        for suffix in ("corrmat", "corrmat_ci16", "corrmat_iq8"):
            dev, timed, host = _entries(lib, suffix)
            for (c, g, k, stride), msg in bad:
                for fn in (dev, timed, host):
                    assert fn(p.handle, d.p, c, g, k, stride, d.p) == INVALID and msg in lib.sdrk_last_error(), (suffix, c, g, k)
            assert dev(p.handle, None, 3, 1, 2, 64, d.p) == INVALID and b"NULL" in lib.sdrk_last_error()
            assert dev(p.handle, d.p, 3, 1, 2, 64, None) == INVALID and b"NULL" in lib.sdrk_last_error()
            assert dev(None, d.p, 3, 1, 2, 64, d.p) == INVALID and lib.sdrk_last_error() == b"plan is NULL"
            assert timed(p.handle, d.p, 3, 1, 2, 64, d.p, 0) == INVALID and b"launches" in lib.sdrk_last_error()
        for fmt in (2, -1):
            assert lib.sdrk_exec_device_corrmat_iq8(p.handle, d.p, fmt, 3, 1, 2, 64, 1.0, d.p, None) == INVALID
            assert lib.sdrk_exec_host_corrmat_iq8(p.handle, d.p, fmt, 3, 1, 2, 64, 1.0, d.p) == INVALID
        # after all the refusals the plan still works: 2 frames of 64 three-channel elements in, one group of 9 rows out
        for entry in ("exec_device_corrmat_timed_each", "exec_device_corrmat_ci16_timed_each", "exec_device_corrmat_ci8_timed_each"):
            ms = getattr(p, entry)(d.p.value, 3, 1, 2, d.p.value + 32768, launches=3)
            assert len(ms) == 3 and all(v > 0 for v in ms), entry
        p.set_pfb(np.ones(128, np.float32))                                    # a prototype is ignored
        x = widen_c(elements16(1, 64, 6, 64, 3))
        with_proto = device_cm(p, x, 3, 2, 64)
    with SpectrumPlan(64) as p:
        assert same_bits(device_cm(p, x, 3, 2, 64), with_proto)


def test_cli_psd_integrate_correlate_on_a_three_channel_cu8_recording(tmp_path, capsys):
    n, k, groups, C = 4096, 4, 3, 3
    x = to_cu8(elements16(11, n, groups * k, n, C, bits=7))
    base, out = str(tmp_path / "three"), str(tmp_path / "rows.npz")
    sigmf_io.write_sigmf(base, x, 1e6, 1e9, datatype="cu8", num_channels=C)
    back, meta = sigmf_io.read_sigmf_channels(base)
    assert back.dtype == np.uint8 and np.array_equal(back, x) and meta["num_channels"] == C
    assert cli.main(["psd", base + ".sigmf-meta", "--integrate", str(k), "--correlate", "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = pkg.spectrum.correlation_matrix(x, n, k)                          # the module function, on the cached plan
    assert report["corr_rows"] == groups and report["corr_channels"] == C and report["samples"] == groups * k * n
    assert [p["pair"] for p in report["corr_pairs"]] == [[0, 1], [0, 2], [1, 2]]
    for p in report["corr_pairs"]:
        coh, phase = want.coherence(*p["pair"]), want.phase(*p["pair"])
        g, b = np.unravel_index(int(np.argmax(coh)), coh.shape)
        assert p["peak_coherence"] == float(coh[g, b]) and p["peak_row"] == g and p["peak_phase_rad"] == float(phase[g, b])
        assert p["median_coherence"] == float(np.median(coh)) and 0.0 <= p["median_coherence"] <= 1.0
    with np.load(out) as z:
        assert same_bits(z["corr_planes"], want.planes) and "integrated_db" in z
    with SpectrumPlan(n) as plan:                                            # and both are the complex64 call on the widened elements
        assert same_bits(plan.correlate(widen_c(x), k).planes, want.planes)
        lst = pkg.spectrum.correlation_matrix([np.ascontiguousarray(widen_c(x)[:, c]) for c in range(C)], n, k)
        assert same_bits(lst.planes, want.planes)


@pytest.mark.parametrize("n,k,groups,hop", [(4096, 5, 40, 4096), (4096, 64, 1, 4096), (1024, 9, 7, 512)])
def test_cross_spectrum_ci8_equals_cross_spectrum_on_the_widened_pair(n, k, groups, hop):
    x7 = elements16(n + k, n, groups * k, hop, 2, bits=7)
    with SpectrumPlan(n, window="hann") as plan:
        for x8 in (to_ci8(x7), to_cu8(x7)):
            got, want = plan.cross_spectrum_ci8(x8, k, hop, 0.5), plan.cross_spectrum(widen_c(x8), k, hop, 0.5)
            assert same_bits(got.paa.base, want.paa.base), (n, x8.dtype)


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8: other split factors, more groups than the grid at every size — in a child process, as the plans read the
    variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", SUBSET_FOR_8_CUS],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

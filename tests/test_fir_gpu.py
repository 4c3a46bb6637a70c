"""FIR filtering and channel extraction on the GPU (sdrk_exec_device_fir* / sdrk_exec_host_fir*): overlap-save in blocks of 4096,
tune + filter + decimate in one kernel, against float64 numpy on the same samples — the four lines of include/sdrk.h:

    h_s[t] = h[t] exp(+2 pi i s t / 4096);   v = np.convolve(x, h_s, "valid");   out[m] = v[m D] exp(-2 pi i ((phase0 + s m D) mod 4096) / 4096)

never against the library.

The bound: max |out - ref| <= REL_TOL * ||h||_1 * max|x| with REL_TOL = 1e-5 of tests/parity.py.  ||h||_1 max|x| bounds |v|, and the
errors of both transforms scale with it; a complex64 numpy emulation of the same blocks has its worst case over these shapes at
6.6e-8 of that scale, so the bound has two orders of margin and still catches any wrong twiddle, bin or offset.  Every check
prints its worst err/tol.

Measured on the device (profiles/fir/SUMMARY.md): worst err/tol 8.0e-2 (M = 1), 8e-3 to 3e-2 at the longer filters."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd.spectrum import ChannelStream, SpectrumPlan, channel_taps, fir_filter, pfb_prototype
from tests.gpu_helpers import DevBuf, same_bits, stream16_planted, widen_flat
from tests.parity import REL_TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
GUARD = 64   # complex64 behind the last output, which must stay as they were

# (M, D, s): one tap, two taps, L one step below 4096, decimation alone, and the mixer at growing M up to the tap limit
SHAPES = [(1, 1, 0), (2, 1, 0), (257, 1, 0), (129, 4, 0), (513, 8, 611), (1025, 16, 300), (2049, 64, -1000), (1793, 256, 7)]
SUBSET_FOR_8_CUS = "parity or hundred or chunks or int16 or repeated"   # (not this test itself)


def block_len(m):
    return (4097 - m) // 256 * 256


def lengths(m):
    L = block_len(m)
    return [m, m + L - 1, m + L, 3 * N + 123]


def shifted(h, s):
    return h.astype(np.complex128) * np.exp(2j * np.pi * s * np.arange(h.shape[0]) / N)


def ref_fir(x, h, d, s, phase0=0):
    """float64: the valid convolution, the mixer, every d-th sample."""
    v = np.convolve(x.astype(np.complex128), shifted(h, s), "valid")
    q = (phase0 + s * np.arange(v.shape[0])) % N
    return (v * np.exp(-2j * np.pi * q / N))[::d]


def tol_of(x, h):
    return REL_TOL * float(np.abs(h.astype(np.complex128)).sum()) * float(np.abs(x.astype(np.complex128)).max())


def random_taps(seed, m):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(m) + 1j * rng.standard_normal(m)) / np.sqrt(2 * m)).astype(np.complex64)


def noise(seed, n):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def noise_tone(seed, n, d, s):
    """unit noise plus an off-bin tone inside the passband of channel_taps(d) around bin s"""
    f = (s + 0.3 * 0.4 * N / d) / N
    return (noise(seed, n) + 3.0 * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)


def device_fir(plan, x, d, s, phase0=0, ci16=False):
    """The device entry's output, with the GUARD samples behind it checked to be untouched."""
    n_in = x.shape[0]
    n_out = plan.fir_outputs(n_in, d)
    with DevBuf(x.nbytes) as d_in, DevBuf((n_out + GUARD) * 8) as d_out:
        d_in.put(x)
        d_out.put(np.full(n_out + GUARD, np.nan + 1j * np.nan, np.complex64))
        (plan.exec_device_fir_ci16 if ci16 else plan.exec_device_fir)(d_in.p.value, n_in, d_out.p.value, decim=d, shift_bins=s,
                                                                      phase0=phase0)
        plan.sync()
        got = d_out.get(n_out + GUARD, np.complex64)
    assert np.all(np.isnan(got[n_out:].real)), "stored past n_out"
    return got[:n_out]


def check(got, ref, tol, what):
    assert got.shape == ref.shape and got.dtype == np.complex64, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got.view(np.float32))), what
    w = float(np.abs(got.astype(np.complex128) - ref).max()) / tol
    print(f"{what}: err/tol {w:.2e}")
    assert w <= 1.0, (what, w)
    return w


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d,s", SHAPES)
def test_fir_parity_with_float64_numpy(m, d, s):
    worst = 0.0
    with SpectrumPlan(N) as plan:
        for n_in in lengths(m):
            x16 = stream16_planted(m + n_in, n_in)
            cases = [("noise", noise(m + n_in, n_in), random_taps(m, m), False),
                     ("tone", noise_tone(m + n_in + 1, n_in, d, s), channel_taps(d, m), False),
                     ("int16", x16, channel_taps(d, m), True)]
            for name, x, h, ci16 in cases:
                plan.set_fir(h)
                assert plan.fir_taps == m == _ffi.lib().sdrk_plan_fir_taps(plan.handle)
                xc = widen_flat(x) if ci16 else x
                got = device_fir(plan, x, d, s, ci16=ci16)
                assert got.shape[0] == (n_in - m) // d + 1
                worst = max(worst, check(got, ref_fir(xc, h, d, s), tol_of(xc, h), f"M={m} D={d} s={s} n_in={n_in} {name}"))
    print(f"M={m} D={d} s={s}: worst err/tol {worst:.2e}")


def test_fir_parity_over_a_hundred_blocks_with_a_carried_phase():
    m, d, s, phase0 = 513, 8, 611, 1234
    n_in = 100 * block_len(m) + m - 1
    x, h = noise_tone(5, n_in, d, s), channel_taps(d, m)
    with SpectrumPlan(N) as plan:
        plan.set_fir(h)
        got = device_fir(plan, x, d, s, phase0)
        check(got, ref_fir(x, h, d, s, phase0), tol_of(x, h), "100 blocks")
        assert same_bits(device_fir(plan, x, d, s, phase0 - 3 * N), got)      # the phase is periodic


# ---- bit identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d,s,sample0", [(257, 1, 0, 0), (513, 8, 611, 5), (2049, 64, -1000, 64 * 7 + 63), (2, 4, 3, 2)])
def test_host_entry_equals_device_entry_across_chunks(m, d, s, sample0, monkeypatch):
    """Chunks of 5 blocks, 4 of them: the host entry on (prefix, iq) returns the device entry's bits on prefix || iq from the
    first sample whose stream index is a multiple of D, with a non-zero prefix and with none (zeros)."""
    monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "5")
    n = 18 * block_len(m) + 77
    x, h = noise(m + d, n), random_taps(m + 1, m)
    pre = noise(m + d + 1, m - 1)
    j0 = (-sample0) % d
    with SpectrumPlan(N) as plan:
        plan.set_fir(h)
        for prefix in (pre, None):
            virt = np.concatenate((pre if prefix is not None else np.zeros(m - 1, np.complex64), x))
            dev = device_fir(plan, virt[j0:], d, s, (s * (sample0 + j0)) % N)
            host = plan.fir(x, decim=d, shift_bins=s, prefix=prefix, sample0=sample0)
            assert same_bits(host, dev), (m, d, "prefix" if prefix is not None else "zeros")
            ref = ref_fir(virt, h, 1, s, s * sample0)[j0::d]
            check(host, ref, tol_of(virt, h), f"host M={m} D={d}")
        monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "3")                          # another cut into chunks: the same bits
        assert same_bits(plan.fir(x, decim=d, shift_bins=s, prefix=None, sample0=sample0), host)
        monkeypatch.delenv("SDRK_FIR_CHUNK_BLOCKS")                               # and the shipped chunk size (one chunk here)
        assert same_bits(plan.fir(x, decim=d, shift_bins=s, prefix=None, sample0=sample0), host)


@pytest.mark.parametrize("m,d,s", [(129, 4, 0), (513, 8, 611), (2049, 64, -1000), (1, 1, 5)])
def test_int16_entries_equal_the_complex64_entries_on_the_widened_samples(m, d, s, monkeypatch):
    monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "2")
    n_in = 5 * N + 321
    x16 = stream16_planted(m, n_in)
    wide = widen_flat(x16)
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m, m))
        assert same_bits(device_fir(plan, x16, d, s, 9, ci16=True), device_fir(plan, wide, d, s, 9)), (m, "device")
        pre16 = stream16_planted(m + 1, max(m - 1, 1))[: m - 1]
        a = plan.fir_ci16(x16, decim=d, shift_bins=s, prefix=pre16, sample0=3)
        assert same_bits(a, plan.fir(wide, decim=d, shift_bins=s, prefix=widen_flat(pre16), sample0=3)), (m, "host")


def test_repeated_calls_give_identical_bits():
    for m, d, s in ((257, 1, 0), (1025, 16, 300)):
        x = noise(m, 40 * N)
        with SpectrumPlan(N) as plan:
            plan.set_fir(random_taps(m, m))
            a = device_fir(plan, x, d, s)
            assert same_bits(a, device_fir(plan, x, d, s)), m
            h = plan.fir(x, decim=d, shift_bins=s)
            assert same_bits(h, plan.fir(x, decim=d, shift_bins=s)), (m, "host")
            assert same_bits(fir_filter(x, random_taps(m, m), d, s), h), (m, "module function")


def test_existing_rows_are_unchanged_around_a_fir_call():
    x = noise(3, 8 * N)
    with SpectrumPlan(N) as plan:
        plan.set_pfb(pfb_prototype(N, 4))
        row, pfb_row = plan.spectrum_db(x[:N]), plan.pfb_db(x)
        plan.set_fir(channel_taps(8))
        y = plan.fir(x, decim=8, shift_bins=100)
        assert same_bits(plan.spectrum_db(x[:N]), row) and same_bits(plan.pfb_db(x), pfb_row)
        assert plan.pfb_taps == 4 and plan.fir_taps == 129
        assert same_bits(plan.fir(x, decim=8, shift_bins=100), y)


# ---- known answers --------------------------------------------------------------------------------------------------------------
def test_known_one_tap_returns_the_input_and_a_unit_tap_at_d_delays_it():
    x = noise(11, 3 * N + 5)
    with SpectrumPlan(N) as plan:
        plan.set_fir(np.ones(1, np.complex64))
        check(device_fir(plan, x, 1, 0), x.astype(np.complex128), REL_TOL * float(np.abs(x).max()), "h = [1]")
        for delay in (1, 255, 2048):
            e = np.zeros(delay + 1, np.complex64)
            e[delay] = 1
            plan.set_fir(e)
            got = plan.fir(x)                                                      # zero prefix: lfilter
            want = np.concatenate((np.zeros(delay), x.astype(np.complex128)))[: x.shape[0]]
            check(got, want, REL_TOL * float(np.abs(x).max()), f"h = e_{delay}")


def test_known_a_tone_in_the_passband_comes_out_tuned_and_one_in_the_stopband_is_suppressed():
    d, s, amp, n_in = 8, 611, 1000.0, 6 * N
    h = channel_taps(d)
    m = h.shape[0]
    t = np.arange(n_in)
    tone = (amp * np.exp(2j * np.pi * (s + 0.3) / N * t)).astype(np.complex64)
    hd = h.astype(np.complex128)
    resp = (hd * np.exp(-2j * np.pi * 0.3 / N * np.arange(m))).sum()              # H(0.3 / 4096)
    with SpectrumPlan(N) as plan:
        plan.set_fir(h)
        got = device_fir(plan, tone, d, s)
        i = np.arange(got.shape[0]) * d
        want = amp * resp * np.exp(2j * np.pi * (s + 0.3) / N * (m - 1)) * np.exp(2j * np.pi * 0.3 / N * i)
        tol = tol_of(tone, h)
        check(got, want, tol, "tone at bin 611.3, tuned to 611")
        assert abs(float(np.abs(got).mean()) - amp * abs(resp)) <= tol
        step = np.angle(got[1:] * np.conj(got[:-1]))
        # 0.3 bins of the input rate; two samples each within tol of a phasor of length amp |H| bound the step's error
        assert np.abs(step - 2 * np.pi * 0.3 * d / N).max() <= 2 * np.arcsin(tol / (amp * abs(resp)))
        stop = (amp * np.exp(2j * np.pi * (0.75 / d) * t)).astype(np.complex64)    # beyond 0.6/D
        out = device_fir(plan, stop, d, 0)
        level = float(np.abs(out).max()) / amp
        print(f"stopband tone: {20 * np.log10(level):.1f} dB")
        assert level <= 10 ** (-55 / 20) + tol_of(stop, h) / amp


# ---- streaming ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci16", [False, True])
def test_channel_stream_in_pieces_equals_the_float64_reference_of_the_whole_stream(ci16):
    pieces, d, fs = (1, 4095, 4097, 10000), 16, 2.4e6
    n = sum(pieces)
    x = stream16_planted(21, n) if ci16 else noise_tone(21, n, d, 300)
    xc = widen_flat(x) if ci16 else x
    h = channel_taps(d)
    with ChannelStream(None, h, d, 300.4 * fs / N, fs) as ch:
        assert ch.shift_bins == 300 and ch.tuned_hz == 300 * fs / N and ch.out_rate == fs / d
        out, at, cuts = [], 0, []
        for p in pieces:
            out.append(ch.push(x[at:at + p]))
            at += p
            cuts.append(sum(o.shape[0] for o in out))
        assert ch.sample_index == n
        got = np.concatenate(out)
    full = np.convolve(xc.astype(np.complex128), shifted(h, 300))[:n]               # lfilter: a zero prefix
    ref = (full * np.exp(-2j * np.pi * ((300 * np.arange(n)) % N) / N))[::d]
    tol = tol_of(xc, h)
    check(got, ref, tol, f"ChannelStream in pieces {pieces}")
    for c in cuts[:-1]:                                                           # no phase jump where two pieces meet
        assert np.abs(got[c - 1:c + 1].astype(np.complex128) - ref[c - 1:c + 1]).max() <= tol, c


# ---- the rest -------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device():
    lib = _ffi.lib()
    h = channel_taps(4)
    hp = h.ctypes.data_as(ctypes.c_void_p)
    n_out = ctypes.c_size_t()
    each = (ctypes.c_float * 2)()
    x = noise(1, N)
    with SpectrumPlan(1024) as p, DevBuf(1 << 16) as d:
        assert lib.sdrk_plan_set_fir(p.handle, h.shape[0], hp) == _ffi.SDRK_ERR_UNSUPPORTED and b"4096" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_fir(p.handle, d.p, 1024, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_UNSUPPORTED
        assert lib.sdrk_exec_host_fir(p.handle, None, d.p, 1024, 1, 0, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_UNSUPPORTED
        assert lib.sdrk_plan_fir_taps(p.handle) == 0
        assert p.spectrum_db(x[:1024]).shape == (1024,)                           # a plan that has refused still works
    with SpectrumPlan(N, precision="double") as p64, DevBuf(1 << 16) as d:
        assert lib.sdrk_plan_set_fir(p64.handle, h.shape[0], hp) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_fir(p64.handle, d.p, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_fir_ci16(p64.handle, d.p, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError):
            p64.set_fir(h)
        assert p64.spectrum_db(x.astype(np.complex128)).shape == (N,)
    with SpectrumPlan(N) as p, DevBuf(1 << 16) as d:
        for fn in (lib.sdrk_exec_device_fir, lib.sdrk_exec_device_fir_ci16):
            assert fn(p.handle, d.p, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"no FIR filter" in lib.sdrk_last_error()
        assert lib.sdrk_exec_device_fir_timed_each(p.handle, d.p, N, 1, 0, 0, d.p, 2, each) == _ffi.SDRK_ERR_INVALID
        for fn in (lib.sdrk_exec_host_fir, lib.sdrk_exec_host_fir_ci16):
            assert fn(p.handle, None, d.p, N, 1, 0, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError):
            p.fir(x)
        assert lib.sdrk_plan_set_fir(p.handle, 0, hp) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_plan_set_fir(p.handle, 2050, hp) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_plan_set_fir(p.handle, 4, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
        p.set_fir(h)
        m = h.shape[0]
        for fn in (lib.sdrk_exec_device_fir, lib.sdrk_exec_device_fir_ci16):
            assert fn(p.handle, None, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 1, 0, 0, None, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, m - 1, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"n_in" in lib.sdrk_last_error()
            for decim in (0, 3, 512, -4):
                assert fn(p.handle, d.p, N, decim, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"decim" in lib.sdrk_last_error()
            for s in (-2049, 2048):
                assert fn(p.handle, d.p, N, 1, s, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and b"shift_bins" in lib.sdrk_last_error()
            assert fn(None, d.p, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
        assert lib.sdrk_exec_device_fir_timed_each(p.handle, d.p, N, 1, 0, 0, d.p, 0, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_fir(p.handle, None, d.p, N, 1, 0, 0, d.p, None) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_host_fir(p.handle, None, None, N, 1, 0, 0, d.p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        # after all the refusals the plan still works: 4096 samples in (32 KiB), their outputs behind them
        ms = p.exec_device_fir_timed_each(d.p.value, N, d.p.value + (1 << 15), launches=3, decim=4, shift_bins=-5)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        check(p.fir(x, decim=4), ref_fir(np.concatenate((np.zeros(m - 1), x)), h, 4, 0), tol_of(x, h), "after the refusals")


def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8: several blocks per workgroup at every size, so the loads in flight across iterations are covered — in a
    child process, as the plans read the variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", SUBSET_FOR_8_CUS],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

"""Polyphase filter bank spectra on the GPU (sdrk_plan_set_pfb, sdrk_exec_*_pfb): T blocks of nfft samples folded under a
prototype of T*nfft float32 coefficients in front of the plan's transform.

The fold is defined per real component in float32, every product and every sum rounded, taps ascending — what numpy computes
on float32 arrays — so the first check is in bits: numpy's fold handed to the EXISTING entry points of the same rectangular
plan must give the rows the new entry points give for the raw stream.  The second is the project's amplitude bar against
float64 numpy on the same complex64 samples (tests/parity.REL_TOL): per frame

    max_k | |Y_got[k]| - |Y_ref[k]| |  <=  1e-5 * max_k |Y_ref[k]|

(a float32 restatement in numpy — rounded fold, float32 FFT — stays at 1.2-1.4e-7 of the frame peak for (N, T, hop) =
(4096, 4, 4096), (4096, 8, 1024), (1024, 3, 1500), (64, 16, 64): the fold adds nothing visible to the transform's own error).
Inputs are 12-bit integer-valued noise (synth.py) plus an integer-rounded tone."""
import ctypes
import json

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.hostmem import pinned_empty
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype
from tests.gpu_helpers import DevBuf, fold32, held_during, prototype, ref64, same_bits, stream_synth_tone as stream
from tests.parity import REL_TOL, mag_from_db

pytestmark = pytest.mark.gpu

EPS = 1e-12
N4K = 4096


def device_rows(plan, x, frames, hop, pfb):
    with DevBuf(x.nbytes) as d_in, DevBuf(frames * plan.nfft * 4) as d_out:
        d_in.put(x)
        if pfb:
            plan.exec_device_pfb(d_in.p.value, frames, d_out.p.value, frame_stride=hop)
        else:
            plan.exec_device(d_in.p.value, frames, d_out.p.value, frame_stride=hop)
        plan.sync()
        return d_out.get((frames, plan.nfft), np.float32)


def check_case(n, taps, frames, hop, shift, proto, seed=1):
    x = stream(seed, (frames - 1) * hop + taps * n)
    h = prototype(proto, n, taps, seed + 7)
    what = f"N={n} T={taps} frames={frames} hop={hop} shift={shift} {proto}"
    with SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        assert plan.set_pfb(h) == taps
        got_db = device_rows(plan, x, frames, hop, pfb=True)
        got_fft = plan.pfb_fft(x, hop)
        y = fold32(x, h, n, taps, frames, hop)
        want_db = device_rows(plan, y, frames, n, pfb=False)      # the existing packed entry point on numpy's fold
        want_fft = plan.fft(y)
    assert got_fft.shape == (frames, n)
    db_same, fft_same = same_bits(got_db, want_db), same_bits(got_fft, want_fft.reshape(frames, n))
    Y = ref64(x, h, n, taps, frames, hop, shift)
    peak = np.abs(Y).max(axis=-1)
    err_db = (np.abs(mag_from_db(got_db) - (np.abs(Y) + EPS)).max(axis=-1) / peak).max()
    err_fft = (np.abs(np.abs(got_fft.astype(np.complex128)) - np.abs(Y)).max(axis=-1) / peak).max()
    print(f"{what}: dB rows identical {db_same}, spectra identical {fft_same}, amplitude error {err_db:.2e} (dB rows) "
          f"{err_fft:.2e} (spectra) of the frame peak")
    assert db_same, what
    assert fft_same, what
    assert err_db <= REL_TOL and err_fft <= REL_TOL, (what, err_db, err_fft)


G3 = N4K + N4K // 3 + 1
# (taps, frames, hop, shift, prototype): every T x every frame count, every hop with every T, both shifts, both prototypes;
# 1700 frames exceed the 768-workgroup grid, so the persistent loop and its prefetch across frames run
CASES_4096 = [
    (1, 1, N4K, True, "random"), (1, 7, N4K // 4, False, "default"), (1, 1700, G3, True, "default"), (1, 1700, 1, False, "random"),
    (2, 1, 1, False, "default"), (2, 7, G3, True, "random"), (2, 1700, N4K, True, "random"), (2, 1700, N4K // 4, False, "default"),
    (4, 1, N4K // 4, True, "default"), (4, 7, N4K, False, "random"), (4, 1700, N4K, True, "default"), (4, 1700, 1, True, "random"),
    (4, 1700, N4K // 4, False, "random"), (4, 1700, G3, False, "default"),
    (5, 1, G3, False, "random"), (5, 7, 1, True, "default"), (5, 1700, N4K // 4, True, "random"), (5, 1700, N4K, False, "default"),
]


@pytest.mark.parametrize("taps,frames,hop,shift,proto", CASES_4096)
def test_n4096_same_bits_as_the_existing_transform_and_float64_bound(taps, frames, hop, shift, proto):
    check_case(N4K, taps, frames, hop, shift, proto, seed=taps * 100 + frames)


# (n, taps, frames, hop, shift, prototype): the route through plan-owned staging — a short length, chirp-z, single-pass lengths
# on either side of 4096, the two-pass lengths
CASES_GENERIC = [
    (64, 16, 9, 64, True, "default"), (64, 3, 5, 1, False, "random"), (64, 1, 4, 100, True, "random"),
    (1000, 3, 7, 1500, True, "default"), (1000, 2, 3, 250, False, "random"),
    (1024, 3, 9, 1500, True, "random"), (1024, 8, 6, 256, False, "default"),
    (8192, 2, 5, 8192, True, "default"), (8192, 4, 3, 2731, False, "random"),
    (65536, 3, 5, 65536 // 2, True, "default"), (1 << 20, 2, 2, (1 << 20) + 12345, True, "random"),
]


@pytest.mark.parametrize("n,taps,frames,hop,shift,proto", CASES_GENERIC)
def test_other_lengths_same_bits_and_float64_bound(n, taps, frames, hop, shift, proto):
    check_case(n, taps, frames, hop, shift, proto, seed=n % 1000 + taps)


@pytest.mark.parametrize("assign", ["0", "1", "2"])
def test_n4096_rows_do_not_depend_on_the_frame_assignment(assign, monkeypatch):
    """SDRK_PFB_ASSIGN picks how the persistent workgroups share the frames (grid-stride, per-XCD ranges, runs per workgroup);
    it is read when the prototype is set.  Every choice gives the bits of numpy's fold through the existing entry point."""
    monkeypatch.setenv("SDRK_PFB_ASSIGN", assign)
    for frames, hop in ((1700, N4K), (13, N4K // 4), (769, G3)):
        x = stream(3, (frames - 1) * hop + 4 * N4K)
        h = prototype("random", N4K, 4, 11)
        with SpectrumPlan(N4K, eps=EPS) as plan:
            plan.set_pfb(h)
            got = device_rows(plan, x, frames, hop, pfb=True)
            want = device_rows(plan, fold32(x, h, N4K, 4, frames, hop), frames, N4K, pfb=False)
        assert same_bits(got, want), (assign, frames, hop)


@pytest.mark.parametrize("frames,hop", [(3000, N4K), (6000, N4K // 2)])
def test_host_entry_returns_the_device_entrys_bits_in_bounded_memory(frames, hop):
    """~98 MB of input at T = 4 through the chunked numpy boundary, overlap across every chunk boundary, from a pageable and
    from a pinned array; the staging the plan holds afterwards is capped as in the integrate tests (192 MiB)."""
    taps = 4
    L = (frames - 1) * hop + taps * N4K
    x = np.tile(stream(5, 64 * N4K + 1), L // (64 * N4K + 1) + 1)[:L]
    h = pfb_prototype(N4K, taps)
    with SpectrumPlan(N4K, eps=EPS) as plan:
        plan.set_pfb(h)
        dev = device_rows(plan, x, frames, hop, pfb=True)
        host, held = held_during(lambda: plan.pfb_db(x, hop), lambda: plan.pfb_db(x[: taps * N4K]))
        print(f"frames={frames} hop={hop}: device memory taken by the host call {held / 2**20:.1f} MiB")
        assert held <= 192 << 20, held
        assert same_bits(host, dev)
        xp = pinned_empty(x.shape, np.complex64)
        xp[...] = x
        out = pinned_empty((frames, N4K), np.float32)
        assert plan.pfb_db(xp, hop, out=out) is out
        assert same_bits(out, dev)
        assert same_bits(plan.pfb_fft(x[: 40 * hop + taps * N4K], hop)[:3], plan.fft(fold32(x, h, N4K, taps, 3, hop)))
    assert same_bits(dev[[0, frames - 1]], _reference_rows(x, h, N4K, taps, frames, hop)[[0, 1]])


def _reference_rows(x, h, n, taps, frames, hop):
    """first and last frame: numpy's fold through the existing entry point"""
    y = np.concatenate([fold32(x, h, n, taps, 1, hop), fold32(x[(frames - 1) * hop:], h, n, taps, 1, hop)])
    with SpectrumPlan(n, eps=EPS) as plan:
        return plan.spectrum_db(y)


def test_host_entry_through_staging_of_more_than_64_mib():
    """N = 1024: 9000 folded frames are 70 MiB of complex64 — two chunks of the plan's staging on the device entry, and the
    chunked boundary in front of it on the host entry."""
    n, taps, frames, hop = 1024, 3, 9000, 512
    x = stream(9, (frames - 1) * hop + taps * n)
    h = pfb_prototype(n, taps)
    with SpectrumPlan(n, eps=EPS) as plan:
        plan.set_pfb(h)
        dev = device_rows(plan, x, frames, hop, pfb=True)
        want = device_rows(plan, fold32(x, h, n, taps, frames, hop), frames, n, pfb=False)
        host = plan.pfb_db(x, hop)
    assert same_bits(dev, want)
    assert same_bits(host, dev)


def test_filter_bank_confines_a_tone_between_two_bins_better_than_the_hann_window():
    """The reason for the feature.  A tone exactly half-way between two bins, amplitude 100 over unit-variance noise (40 dB):
    the share of the row's power outside +-2 bins of the tone is smaller for the PFB row (T = 4, default prototype) than for
    the plan's Hann row on the same samples.  Both shares are computed in float64 numpy first; asserted are the ordering and
    that each GPU share is within 1 dB of its float64 value."""
    n, taps, k0 = N4K, 4, 700
    rng = np.random.default_rng(42)
    L = taps * n
    x = ((rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(2)
         + 100.0 * np.exp(2j * np.pi * ((k0 + 0.5) / n) * np.arange(L))).astype(np.complex64)
    h = pfb_prototype(n, taps)
    outside = np.abs(np.arange(n) - (k0 + 0.5)) > 2.0               # unshifted bin order

    def share(power):
        return float(power[outside].sum() / power.sum())

    ref_pfb = share(np.abs(ref64(x, h, n, taps, 1, n, False)[0]) ** 2)
    ref_hann = share(np.abs(np.fft.fft(x[:n].astype(np.complex128) * np.hanning(n))) ** 2)
    with SpectrumPlan(n, eps=EPS, shift=False) as plan, SpectrumPlan(n, window="hann", eps=EPS, shift=False) as hann:
        plan.set_pfb(h)
        got_pfb = share(mag_from_db(plan.pfb_db(x)[0]) ** 2)
        got_hann = share(mag_from_db(hann.spectrum_db(x[:n])) ** 2)
    print(f"power outside +-2 bins of the tone: PFB {10 * np.log10(got_pfb):.2f} dB (float64 {10 * np.log10(ref_pfb):.2f}), "
          f"Hann {10 * np.log10(got_hann):.2f} dB (float64 {10 * np.log10(ref_hann):.2f})")
    assert ref_pfb < ref_hann
    assert got_pfb < got_hann
    assert abs(10 * np.log10(got_pfb / ref_pfb)) <= 1.0
    assert abs(10 * np.log10(got_hann / ref_hann)) <= 1.0


def test_refusals_return_invalid_with_a_message():
    lib = _ffi.lib()
    n = 256
    h = pfb_prototype(n, 2)
    hp = h.ctypes.data_as(ctypes.c_void_p)
    x = stream(1, 4 * n)
    out = np.empty((2, n), np.float32)
    outc = np.empty((2, n), np.complex64)
    xp, op, ocp = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, out, outc))
    ms = (ctypes.c_float * 2)()

    def refused(status):
        assert status == _ffi.SDRK_ERR_INVALID, status
        assert lib.sdrk_last_error(), "no message"

    def every_exec(handle, iq=xp, frames=2, rows=op, rows_c=ocp):
        refused(lib.sdrk_exec_device_pfb(handle, iq, frames, n, rows, None))
        refused(lib.sdrk_exec_device_pfb_timed_each(handle, iq, frames, n, rows, 2, ms))
        refused(lib.sdrk_exec_host_pfb(handle, iq, frames, n, rows))
        refused(lib.sdrk_exec_fft_host_pfb(handle, iq, frames, n, rows_c))

    with SpectrumPlan(n, window="hann") as windowed, SpectrumPlan(n, precision="double") as f64, SpectrumPlan(n) as plan:
        for bad in (windowed, f64):
            refused(lib.sdrk_plan_set_pfb(bad.handle, 2, hp))
            every_exec(bad.handle)
            assert lib.sdrk_plan_pfb_taps(bad.handle) == 0
        every_exec(plan.handle)                                   # no prototype set
        refused(lib.sdrk_plan_set_pfb(plan.handle, 0, hp))
        refused(lib.sdrk_plan_set_pfb(plan.handle, 33, hp))
        refused(lib.sdrk_plan_set_pfb(plan.handle, 2, None))
        refused(lib.sdrk_plan_set_pfb(None, 2, hp))
        refused(lib.sdrk_plan_pfb_taps(None))
        assert lib.sdrk_plan_pfb_taps(plan.handle) == 0
        assert lib.sdrk_plan_set_pfb(plan.handle, 2, hp) == 0 and lib.sdrk_plan_pfb_taps(plan.handle) == 2
        every_exec(None)
        every_exec(plan.handle, iq=None)
        every_exec(plan.handle, rows=None, rows_c=None)
        every_exec(plan.handle, frames=0)
        refused(lib.sdrk_exec_device_pfb_timed_each(plan.handle, xp, 2, n, op, 0, ms))
        refused(lib.sdrk_exec_device_pfb_timed_each(plan.handle, xp, 2, n, op, 2, None))
        refused(lib.sdrk_exec_host_pfb(plan.handle, xp, 2, 0, op))
        # the refused plan still works
        assert lib.sdrk_exec_host_pfb(plan.handle, xp, 2, n, op) == 0
        y = fold32(x, h, n, 2, 2, n)
        assert same_bits(out, plan.spectrum_db(y))
        # Python-side refusals of the same plans
        with pytest.raises(ValueError):
            windowed.set_pfb(h)
        with pytest.raises(ValueError):
            f64.set_pfb(h)


def test_ordinary_entry_points_are_unchanged_and_a_second_prototype_takes_effect():
    n = N4K
    x = stream(21, 12 * n)
    with SpectrumPlan(n, eps=EPS) as plan:
        rows0 = plan.spectrum_db(x.reshape(12, n))
        stft0 = plan.stft_db(x, n // 2)
        h4 = prototype("random", n, 4, 1)
        plan.set_pfb(h4)
        assert same_bits(plan.spectrum_db(x.reshape(12, n)), rows0)
        assert same_bits(plan.stft_db(x, n // 2), stft0)
        a = plan.pfb_db(x, n)
        assert a.shape == (plan.pfb_frames(x.size, n), n) == (9, n)
        assert same_bits(a, plan.spectrum_db(fold32(x, h4, n, 4, 9, n)))
        h2 = prototype("random", n, 2, 2)
        assert plan.set_pfb(h2) == 2
        b = plan.pfb_db(x, n)
        assert b.shape == (11, n)
        assert same_bits(b, plan.spectrum_db(fold32(x, h2, n, 2, 11, n)))
        assert same_bits(plan.spectrum_db(x.reshape(12, n)), rows0)
    assert same_bits(spectrum.pfb_db(x, n, 2, prototype=h2, eps=EPS), b)


def test_cli_psd_pfb_reproduces_pfb_db(tmp_path, capsys):
    n, taps = 1024, 4
    x = stream(31, 9 * n + 17)
    _, meta = sigmf_io.write_sigmf(str(tmp_path / "rec"), x, 1e6, 2.4e9)
    out = str(tmp_path / "rows.npz")
    assert cli.main(["psd", meta, "--nfft", str(n), "--pfb", str(taps), "--out", out]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    rows = np.load(out)["pfb_db"]
    assert report["pfb_taps"] == taps and report["pfb_rows"] == rows.shape[0] == 6
    assert same_bits(rows, spectrum.pfb_db(x, n, taps))
    with SpectrumPlan(n) as plan:
        assert same_bits(rows, plan.spectrum_db(fold32(x, pfb_prototype(n, taps), n, taps, 6, n)))

"""GPU (-m gpu): the kernels that carry every frame length other than 4096 — fft_lds.hip (16 ... 16384), fft_small.hip (2, 4, 8
and the catch-all), fft_tiled2.hip / fft_fused64k.hip (2^15 ... 2^22) — against float64 numpy on the samples the device was
given.

A. The whole operator one input position at a time (impulse basis) and one output bin at a time (tone basis), to bars derived
   from the number format (tests/basis_helpers.py), not tuned.
B. Long calls: more groups than the persistent grid, with a ragged last group, on the full device and with the grids of an
   8-CU device; the host entries in both of their forms.
C. Frame addressing: overlapped, gapped and odd hops from a skewed base, and both sides of the 2 GiB rule of launch_fft_lds.

Lines that start with BASIS, LONG, HOPS and SPAN carry the measured figures (pytest -s); profiles/generic_sizes/SUMMARY.md has
those of one MI355X."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_ref
from tests import basis_helpers as bh
from tests.gpu_helpers import REPO, DevBuf, same_bits
from tests.parity import assert_complex_parity, assert_db_parity, assert_db_parity_deep, peak_rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import sdr_iq_visualizer_amd as p
    assert p.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return p


def _plan(n, **kw):
    from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
    return SpectrumPlan(n, **kw)


def _num_cus(pkg):
    """The CU count the plans size their grids by: the device's, or a smaller SDRK_NUM_CUS (sdrk_plan.hip)."""
    cus = int(re.search(r"(\d+) CUs", pkg.device_info(0)).group(1))
    env = os.environ.get("SDRK_NUM_CUS", "")
    return int(env) if env.isdigit() and 1 <= int(env) < cus else cus


# =====================================================================================================================
# A. the two bases
# =====================================================================================================================
def _fft(n, **kw):
    def run(x):
        with _plan(n, **kw) as plan:
            return plan.fft(x)
    return run


def _db(n, **kw):
    def run(x):
        with _plan(n, **kw) as plan:
            return plan.spectrum_db(x)
    return run


SETTINGS = ("rect shift c64", "custom c64", "custom db")


def _setting(which, n, pos, route="", **kw):
    """One of: rectangular, shifted, complex; custom window, unshifted, complex; custom window, unshifted, dB."""
    w = bh.custom_window(n)
    if which == "rect shift c64":
        return bh.check_impulse_basis(_fft(n, shift=True, **kw), n, pos, shift=True, what=f"{route} rect shift")
    if which == "custom c64":
        return bh.check_impulse_basis(_fft(n, window=w, shift=False, **kw), n, pos, window=w, what=f"{route} custom")
    return bh.check_impulse_basis(_db(n, window=w, shift=False, **kw), n, pos, window=w, db=True, what=f"{route} custom")


def _three_settings(n, pos, sub, route="", **kw):
    """The first setting on `pos`, the other two on `sub`."""
    for which in SETTINGS:
        _setting(which, n, pos if which == SETTINGS[0] else sub, route, **kw)


@pytest.mark.parametrize("n", [1 << a for a in range(1, 13)])
def test_impulse_basis_every_position_up_to_4096(pkg, n):
    """All N frames a_j delta[n - j] in one call (N = 4096: 128 MiB of spectra, through the plan's default route); the other
    settings on the full basis up to 1024 and on 256 positions above."""
    _three_settings(n, np.arange(n), bh.positions(n, n if n <= 1024 else 256))


@pytest.mark.parametrize("n", [8192, 16384])
def test_impulse_basis_sampled_positions_8192_16384(pkg, n):
    pos = bh.positions(n, 128, powers=True)
    _three_settings(n, pos, pos)


def _tile_edges(n):
    """A - 1, A, A + 1 of the length's A x M split (fft_tiled2_split)."""
    lg = n.bit_length() - 1
    a = 1 << (9 if lg == 20 else max(7, lg // 2))
    return (a - 1, a, a + 1)


def _large_positions(n):
    return bh.positions(n, 8 if n >= 1 << 21 else 24, extra=_tile_edges(n))


@pytest.mark.parametrize("which", SETTINGS)
@pytest.mark.parametrize("n", [1 << a for a in range(15, 23)])
def test_impulse_basis_two_pass_lengths(pkg, n, which):
    """2^15 ... 2^22 through the two tiled launches (65536: the tiled form by option): 24 positions (8 at 2^21 and 2^22) with
    the edges of the first column tile among them."""
    _setting(which, n, _large_positions(n), route="tiled", **({"fused64k": False} if n == 65536 else {}))


def test_impulse_basis_fused_65536_in_a_512_frame_call(pkg):
    """The persistent N = 65536 kernel: 512 frames, impulses in the sampled positions on scattered frames and zeros elsewhere;
    the zero frames return exact zeros (complex) and one and the same eps floor (dB)."""
    n = 65536
    pos, amp, w = _large_positions(n), bh.amplitudes(n), bh.custom_window(n)
    at = np.sort(np.random.default_rng(65536).choice(512, len(pos), replace=False))
    at[0], at[-1] = 0, 511
    x = np.zeros((512, n), np.complex64)
    x[at] = bh.impulse_frames(n, pos, amp)
    zero = np.ones(512, bool)
    zero[at] = False
    with _plan(n, fused64k=True, shift=True) as plan:
        got = plan.fft(x)
        status = plan.fused_status()
        assert status["launches"] >= 1 and not status["fallen_back"]
    r = bh.impulse_complex_err(got[at], n, pos, amp, None, True)
    print(f"BASIS impulse N={n} fused rect shift c64 frames=512 err/tol={r:.3f}")
    assert r <= 1.0 and not got[zero].any()
    del got
    with _plan(n, fused64k=True, window=w, shift=False) as plan:
        got = plan.fft(x)
        rows = plan.spectrum_db(x)
    r = bh.impulse_complex_err(got[at], n, pos, amp, w, False)
    print(f"BASIS impulse N={n} fused custom c64 frames=512 err/tol={r:.3f}")
    assert r <= 1.0 and not got[zero].any()
    r = bh.impulse_db_err(rows[at], n, pos, amp, w)
    print(f"BASIS impulse N={n} fused custom db frames=512 err/tol={r:.3f}")
    assert r <= 1.0
    floor = rows[zero]
    assert np.all(floor == floor[0, 0]) and abs(float(floor[0, 0]) + 240.0) < 1e-4
    # (the host entries above cut the call into chunks of 32 frames; device resident, all 512 frames are ONE persistent launch)
    with DevBuf(x.nbytes) as d_in, DevBuf(512 * n * 4) as d_out, _plan(n, fused64k=True, window=w, shift=False) as plan:
        d_in.put(x)
        d_out.put(np.full((512, n), np.nan, np.float32))
        plan.exec_device(d_in.p.value, 512, d_out.p.value)
        plan.sync()
        assert plan.fused_status() == {"launches": 1, "fallen_back": False}
        rows = d_out.get((512, n), np.float32)
    r = bh.impulse_db_err(rows[at], n, pos, amp, w)
    print(f"BASIS impulse N={n} fused custom db frames=512 (one launch) err/tol={r:.3f}")
    assert r <= 1.0
    assert np.all(rows[zero] == floor[0, 0])


def _tone_count(n):
    return n if n <= 1024 else (128 if n <= 1 << 19 else (24 if n == 1 << 20 else (8 if n == 1 << 21 else 4)))


@pytest.mark.parametrize("n", [1 << a for a in range(1, 23)])
def test_tone_basis(pkg, n):
    """Frame k = exp(+2 pi i k n / N) rounded to complex64: the dynamic range the impulses cannot give.  Every k up to 1024,
    128 sampled k up to 2^19; above that the float64 reference of 128 frames takes more than the few seconds a case may, so
    24 k at 2^20, 8 at 2^21 and 4 at 2^22."""
    kw = {"fused64k": False} if n == 65536 else {}
    bh.check_tone_basis(_fft(n, shift=False, **kw), n, bh.positions(n, _tone_count(n), extra=_tile_edges(n) if 1 << 15 <= n <= 1 << 20 else ()),
                        what="tiled" if n >= 1 << 15 else "")


def test_tone_basis_fused_65536(pkg):
    bh.check_tone_basis(_fft(65536, shift=False, fused64k=True), 65536, bh.positions(65536, 128, extra=_tile_edges(65536)), what="fused")


# =====================================================================================================================
# B. long calls
# =====================================================================================================================
SEED = 2718


def _stream(start, count, seed=SEED):
    """Samples [start, start + count) of the stream the device generator writes as consecutive 4096-sample blocks:
    complex64, regenerating only the blocks that hold them."""
    from sdr_iq_visualizer_amd import synth
    b0, b1 = start // 4096, (start + count - 1) // 4096
    return synth.synth_iq(seed, b0, b1 - b0 + 1, 4096).reshape(-1)[start - b0 * 4096: start - b0 * 4096 + count]


def _filled(n_samples, ci16=False, seed=SEED):
    """A device buffer of whole 4096-sample blocks that hold n_samples of the stream (int16 pairs with ci16)."""
    from sdr_iq_visualizer_amd import _ffi
    gen = (n_samples + 4095) // 4096
    buf = DevBuf(gen * 4096 * (4 if ci16 else 8))
    fill = _ffi.lib().sdrk_synth_fill_ci16 if ci16 else _ffi.lib().sdrk_synth_fill
    try:
        _ffi.check(fill(0, seed, 0, gen, 4096, buf.p, None))
    except Exception:
        buf.__exit__()
        raise
    return buf


def _window64(window, n):
    """The plan's float32 window, in float64."""
    return None if window is None else np.hanning(n).astype(np.float32).astype(np.float64)


def _oracle_rows(starts, n, window):
    x = np.stack([_stream(int(s), n) for s in starts]).astype(np.complex128)
    return cpu_ref.spectrum_db(x, window=_window64(window, n))


def _check_rows(got, ref, what):
    assert_db_parity(got, ref, what=what)
    deep = assert_db_parity_deep(got, ref, what=what)
    return float(peak_rel_err(got, ref).max()), deep


def _device_rows(n, frames, hop, window, picks, skew=0, ci16=False):
    """Rows `picks` of one device-resident call of `frames` frames, `hop` apart, from sample `skew` of the stream."""
    with _filled(skew + (frames - 1) * hop + n, ci16) as d_in, DevBuf(frames * n * 4) as d_out:
        d_out.put(np.full((frames, n), np.nan, np.float32))             # a row the call does not write stays NaN
        with _plan(n, window=window) as plan:
            run = plan.exec_device_ci16 if ci16 else plan.exec_device
            run(d_in.p.value + skew * (4 if ci16 else 8), frames, d_out.p.value, frame_stride=hop)
            plan.sync()
        return np.stack([d_out.get((n,), np.float32, offset=int(r) * n * 4) for r in picks])


ZERO_COPY_MAX_BYTES = 32 << 20      # plan_internal.h
HOST_CHUNK_BYTES = 16 << 20


def _host_spectra(x, n, frames, hop, window, picks):
    """(rows `picks` of the complex epilogue, frames per launch).  The library has no device entry with complex output, so
    the call goes through sdrk_exec_fft_host.  With caller arrays in pinned memory and at most 32 MiB of input that entry
    makes ONE launch on the whole call (exec_host, sdrk_host_pipeline.hip); a longer call it cuts into chunks of about 16 MiB,
    which is half a grid of the full device.  So the complex epilogue makes a second and third trip of the persistent loop
    where the whole call fits 32 MiB: with the grids of an 8-CU device."""
    from sdr_iq_visualizer_amd import _ffi, hostmem
    assert x.shape == ((frames - 1) * hop + n,) and hop >= n
    single = x.nbytes <= ZERO_COPY_MAX_BYTES
    if single:
        xin, out = hostmem.pinned_empty(x.shape, np.complex64), hostmem.pinned_empty((frames, n), np.complex64)
        xin[:] = x
        assert hostmem.is_pinned(xin) and hostmem.is_pinned(out)
        per_launch = frames
    else:
        xin, out = np.ascontiguousarray(x), np.empty((frames, n), np.complex64)
        per_launch = max(1, min(HOST_CHUNK_BYTES // (hop * 8), HOST_CHUNK_BYTES // (n * 8), frames))
    out[:] = np.nan
    with _plan(n, window=window, shift=True) as plan:
        _ffi.check(_ffi.lib().sdrk_exec_fft_host(plan.handle, xin.ctypes.data_as(ctypes.c_void_p), frames, hop,
                                                 out.ctypes.data_as(ctypes.c_void_p)))
    return np.array(out[picks]), per_launch


def _check_spectra(stream, n, frames, hop, window, picks, grid_frames, what):
    got, per_launch = _host_spectra(stream, n, frames, hop, window, picks)
    # whenever the call is one launch it is longer than two grids; with SDRK_NUM_CUS=8 every case is one launch
    assert per_launch > 2 * grid_frames or stream.nbytes > ZERO_COPY_MAX_BYTES, (per_launch, grid_frames)
    assert per_launch == frames or os.environ.get("SDRK_NUM_CUS") != "8", (per_launch, frames)
    x = np.stack([_stream(int(r) * hop, n) for r in picks]).astype(np.complex128)
    ref = cpu_ref.fft(x, window=_window64(window, n), shift=True)
    assert_complex_parity(got, ref, what=what)
    rel = float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
    print(f"LONG spectra {what} frames/launch={per_launch} ({per_launch / grid_frames:.2f} grids) peak-rel={rel:.2e}")


WELCH_SPECTRA_BYTES = 256 << 20     # sdrk_welch_psd_host: spectra of one launch


def _check_welch(stream, n, frames, hop, window, grid_frames, what):
    """The complex epilogue in ONE launch of all the frames on the full device too: sdrk_welch_psd_host uploads the stream,
    makes one EPI_COMPLEX launch per 256 MiB of spectra and sums |X|^2 over the frames (Kahan).  A sum does not see a row in
    the wrong place; it sees a group that is lost, stale or computed twice: with G groups a lost one moves it by 1 / G of its
    value, one taken for another by the scatter of |X|^2 over G — about 4e-5 at N = 16 (2049 groups of 256 frames) and more at
    every other length, against the suite's 1e-5 of the largest bin."""
    assert frames * n * 8 <= WELCH_SPECTRA_BYTES and frames > 2 * grid_frames
    with _plan(n, window=window, shift=True) as plan:
        got = plan.welch_psd(stream, 1.0, hop)
    w = np.ones(n) if window is None else _window64(window, n)
    view = np.lib.stride_tricks.as_strided(stream, (frames, n), (hop * 8, 8), writeable=False)
    acc = np.zeros(n)
    for lo in range(0, frames, max(1, (1 << 20) // n)):
        acc += (np.abs(np.fft.fft(view[lo:lo + max(1, (1 << 20) // n)].astype(np.complex128) * w, axis=-1)) ** 2).sum(axis=0)
    ref = np.fft.fftshift(acc) / (frames * (float(n) if window is None else float(np.sum(np.hanning(n) ** 2))))
    rel = float(np.abs(got - ref).max() / ref.max())
    print(f"LONG welch {what} frames/launch={frames} ({frames / grid_frames:.2f} grids) peak-rel={rel:.2e}")
    assert rel <= 1e-5, f"{what}: Welch sum of the spectra at {rel:.2e} of its largest bin"


# (n, hop - n, int16 input): staged and direct forms of the short frames, the non-prefetching int16 form at 512, one
# workgroup per frame above 4096
LONG_CASES = [(16, 0, False), (16, 1, False), (128, 0, False), (128, 1, False), (256, 0, False), (512, 0, False),
              (512, 0, True), (2048, 0, False), (8192, 0, False), (16384, 0, False)]


@pytest.mark.parametrize("n,gap,ci16", LONG_CASES)
def test_long_call_two_grid_wraps_and_a_ragged_group(pkg, n, gap, ci16):
    """2 grid F + F + 1 frames, device resident: the persistent loop of fft_lds_kernel makes three trips, the last with one
    full and one one-frame group.  First and last frame, both sides of each wrap, the last group and 16 random frames
    against the oracle; Hann and rectangular; dB rows from the device entry (one launch of all the frames), spectra through
    the host entry (_host_spectra: one launch where the call fits 32 MiB, which is the 8-CU run), and the Welch sum of the
    spectra (_check_welch: one launch of all the frames on any device)."""
    grid, f = bh.lds_grid(n, _num_cus(pkg)), bh.lds_frames_per_group(n)
    frames, hop = bh.long_call_frames(grid, f), n + gap
    assert frames > 2 * grid * f + f
    picks = bh.pick_rows(frames, grid, f, seed=n)
    stream = None if ci16 else np.ascontiguousarray(_stream(0, (frames - 1) * hop + n))
    for window in ("hann", None):
        what = f"N={n} hop={hop} {'ci16' if ci16 else 'c64'} {window or 'rect'} grid={grid} frames={frames}"
        rel, deep = _check_rows(_device_rows(n, frames, hop, window, picks, ci16=ci16), _oracle_rows(picks * hop, n, window), what)
        print(f"LONG rows {what} peak-rel={rel:.2e} deep-dB={deep:.2e}")
        if ci16:
            continue
        _check_spectra(stream, n, frames, hop, window, picks, grid * f, what)
        _check_welch(stream, n, frames, hop, window, grid * f, what)


def test_long_call_fft_small_n8(pkg):
    """N = 8 through fft_small (one frame per workgroup): 2 max_blocks + 3 frames."""
    n, grid = 8, bh.small_grid(8, _num_cus(pkg))
    frames = 2 * grid + 3
    assert frames > 2 * grid
    picks = bh.pick_rows(frames, grid, 1, seed=n)
    stream = np.ascontiguousarray(_stream(0, frames * n))
    for window in ("hann", None):
        what = f"N={n} hop={n} c64 {window or 'rect'} grid={grid} frames={frames}"
        rel, deep = _check_rows(_device_rows(n, frames, n, window, picks), _oracle_rows(picks * n, n, window), what)
        print(f"LONG rows {what} peak-rel={rel:.2e} deep-dB={deep:.2e}")
        _check_spectra(stream, n, frames, n, window, picks, grid, what)
        _check_welch(stream, n, frames, n, window, grid, what)


@pytest.mark.parametrize("n", [1 << 15, 1 << 18, 1 << 20])
def test_long_call_two_pass_lengths_at_5_frames(pkg, n):
    """Five frames of a two-pass length; with the grids of an 8-CU device that is more tiles than workgroups."""
    picks = np.arange(5)
    rel, deep = _check_rows(_device_rows(n, 5, n, "hann", picks), _oracle_rows(picks * n, n, "hann"), f"N={n}")
    print(f"LONG rows N={n} hop={n} c64 hann cus={_num_cus(pkg)} frames=5 peak-rel={rel:.2e} deep-dB={deep:.2e}")


def test_long_calls_with_the_grids_of_an_8_cu_device():
    """The long calls above with SDRK_NUM_CUS=8 (32 workgroups, a few hundred frames per case) — in a child process, as the
    plans read the variable when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", "test_long_call_"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    print("\n".join(line.lstrip(".").replace("LONG", "LONG 8-CU") for line in r.stdout.splitlines() if line.lstrip(".").startswith("LONG")))
    assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])


@pytest.mark.parametrize("n,frames", [(64, 70001), (64, 30011), (16384, 600)])
def test_host_entries_against_oracle_and_device_entry(pkg, n, frames):
    """pkg.spectrum_db on packed frames: N = 64 above 32 MiB of input (DMA form) and below it (zero-copy form), N = 16384 with
    600 frames.  Sampled rows against the oracle, every row against the device entry bit for bit."""
    x = _stream(0, frames * n).reshape(frames, n)
    got = pkg.spectrum_db(x, window="hann")
    picks = bh.pick_rows(frames, bh.lds_grid(n, _num_cus(pkg)), bh.lds_frames_per_group(n), seed=frames)
    rel, deep = _check_rows(got[picks], _oracle_rows(picks * n, n, "hann"), f"host N={n} frames={frames}")
    print(f"LONG host rows N={n} frames={frames} peak-rel={rel:.2e} deep-dB={deep:.2e}")
    with DevBuf(x.nbytes) as d_in, DevBuf(frames * n * 4) as d_out:
        d_in.put(x)
        with _plan(n, window="hann") as plan:
            plan.exec_device(d_in.p.value, frames, d_out.p.value)
            plan.sync()
        assert same_bits(got, d_out.get((frames, n), np.float32))


# =====================================================================================================================
# C. frame addressing
# =====================================================================================================================
@pytest.mark.parametrize("n", [16, 64, 128, 256, 1024, 8192])
def test_hops_from_a_skewed_base(pkg, n):
    """37 frames at hops N/4, N/2 + 1, N - 1, N, N + 7 and 3 N from a base pointer one sample into the stream (8-byte, not
    16-byte aligned); every row against the oracle.  N <= 128 at hop N takes the staged form, at the other hops the direct."""
    frames, skew = 37, 1
    picks = np.arange(frames)
    for hop in (n // 4, n // 2 + 1, n - 1, n, n + 7, 3 * n):
        for window in ("hann", None):
            what = f"N={n} hop={hop} {window or 'rect'} skew={skew}"
            rel, deep = _check_rows(_device_rows(n, frames, hop, window, picks, skew=skew), _oracle_rows(skew + picks * hop, n, window), what)
            print(f"HOPS {what} peak-rel={rel:.2e} deep-dB={deep:.2e}")


@pytest.mark.parametrize("n,frames,hop,ci16", [
    (16, 259, (1 << 20) - 1, False),        # (256 hop + 16) 8 B < 2 GiB: fft_lds_kernel, lane offsets up to 2.139e9
    (16, 259, 1 << 20, False),              # >= 2 GiB: the pointer-addressed catch-all
    (256, 19, (1 << 25) - 17, True),        # (16 hop + 256) 4 B < 2 GiB: the int16-reading fft_lds_kernel
    (256, 19, (1 << 25) - 16, True),        # >= 2 GiB: widened into staging, then the complex64 kernels
])
def test_both_sides_of_the_2_gib_group_span(pkg, n, frames, hop, ci16):
    """A group of frames shares one buffer descriptor with 32-bit lane offsets; launch_fft_lds / fft_lds_ci16_supports send a
    group that spans 2 GiB or more elsewhere.  One full group and three frames more on each side of the rule, in one device
    allocation of about 2.2 GiB filled by the device generator; every row against the oracle."""
    span = ((4096 // n) * hop + n) * (4 if ci16 else 8)
    assert (span < 1 << 31) == (hop % 2 == 1)
    picks = np.arange(frames)
    what = f"N={n} hop={hop} {'ci16' if ci16 else 'c64'} group span {span / 2 ** 31:.6f} of 2 GiB"
    rel, deep = _check_rows(_device_rows(n, frames, hop, "hann", picks, ci16=ci16), _oracle_rows(picks * hop, n, "hann"), what)
    print(f"SPAN {what} peak-rel={rel:.2e} deep-dB={deep:.2e}")

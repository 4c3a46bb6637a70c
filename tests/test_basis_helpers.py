"""CPU: the checkers of tests/basis_helpers.py see what they are for.  Stand-in transforms written in numpy float32 take the
place of the kernels: honest ones pass the derived bars with room, subtly wrong ones are rejected — and the suite's older
statement (five white-noise frames to 1e-5 of the peak) accepts two of the wrong ones, which is the gap the bases close.
The row picks of the long calls are tried the same way on a model of the persistent loop."""
import numpy as np
import pytest

from tests import basis_helpers as bh
from tests.parity import assert_complex_parity


# ---- stand-ins -------------------------------------------------------------------------------------------------------
def _windowed(x, window):
    return x if window is None else (x * np.asarray(window, np.float32)[None, :]).astype(np.complex64)


def numpy32(window=None, shift=False, db=False, mutate=None):
    """numpy's single-precision FFT of the complex64 frames (window product in float32)."""
    def run(x):
        assert x.dtype == np.complex64
        w = window
        if mutate == "window_neighbour":                   # sample 100 gets the coefficient of sample 101
            w = np.array(window, np.float32)
            w[100] = w[101]
        if mutate == "swap_iq":                            # I and Q swapped on sample 37
            x = x.copy()
            x[:, 37] = x[:, 37].imag + 1j * x[:, 37].real
        X = np.fft.fft(_windowed(x, w), axis=-1).astype(np.complex64)
        if mutate == "swap_bins":
            X[:, [5, 6]] = X[:, [6, 5]]
        if shift:
            X = np.fft.fftshift(X, axes=-1)
        return (20 * np.log10(np.abs(X) + np.float32(bh.EPS))).astype(np.float32) if db else X
    return run


def stockham32(window=None, shift=False, wrong_index=None, table=None):
    """Radix-2 Stockham autosort in float32 with a table rounded once from float64: the shape of fft_small.hip.
    wrong_index = (stage, butterfly): that butterfly reads the next table entry."""
    def run(x):
        n = x.shape[1]
        log2n, half = int(np.log2(n)), n // 2
        tw = bh.twiddle_table(n).astype(np.complex64) if table is None else table
        a = _windowed(x, window)
        i = np.arange(half)
        for s in range(log2n):
            ns = 1 << s
            k = i & (ns - 1)
            idx = k << (log2n - 1 - s)
            if wrong_index is not None and wrong_index[0] == s:
                idx[wrong_index[1]] += 1
            t1 = a[:, half:] * tw[idx][None, :]
            u0 = a[:, :half]
            j = ((i - k) << 1) + k
            b = np.empty_like(a)
            b[:, j] = u0 + t1
            b[:, j + ns] = u0 - t1
            a = b
        assert a.dtype == np.complex64
        return np.roll(a, half, axis=1) if shift else a
    return run


# ---- honest stand-ins pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8, 16, 64, 256, 1024, 4096])
@pytest.mark.parametrize("make", [numpy32, stockham32], ids=["numpy32", "stockham32"])
def test_honest_transforms_pass_both_bases(make, n):
    count = n if n <= 1024 else 256
    pos = bh.positions(n, count)
    w = bh.custom_window(n)
    r = [bh.check_impulse_basis(make(shift=True), n, pos, shift=True, what="rect shift"),
         bh.check_impulse_basis(make(window=w), n, pos, window=w, what="custom")]
    l2, off = bh.check_tone_basis(make(), n, bh.positions(n, min(count, 128)), what="rect")
    assert max(r) < 0.5 and l2 < 0.5 and off < 0.5           # float32 done right sits far inside the bars
    if make is numpy32:
        bh.check_impulse_basis(make(window=w, db=True), n, pos, window=w, db=True, what="custom")


def test_the_bars_are_the_derived_ones():
    assert bh.tol(16384) == 112 * 2.0 ** -24 and bh.tol(2) == 2.0 ** -21
    assert bh.complex_bar(1024, True) == 81 * 2.0 ** -24
    assert bh.db_bar(1024, False) == pytest.approx(8.69 * 81 * 2.0 ** -24 + 1e-6, rel=1e-12)


def test_positions_cover_the_edges_the_issue_names():
    p = bh.positions(2048, 256)
    assert len(p) == 256 and set(range(32)) <= set(p) and set(range(2048 - 32, 2048)) <= set(p)
    assert set(range(1024 - 16, 1024 + 16)) <= set(p)
    q = bh.positions(16384, 128, powers=True)
    assert {0, 1, 2, 3, 4, 5, 255, 256, 257, 8191, 8192, 8193, 16383} <= set(q) and len(q) > 128
    t = bh.positions(1 << 20, 24, extra=(511, 512, 513))
    assert len(t) == 24 and {0, (1 << 20) - 1, 1 << 19, 511, 512, 513} <= set(t)
    assert np.array_equal(bh.positions(64, 256), np.arange(64))
    assert np.array_equal(t, bh.positions(1 << 20, 24, extra=(511, 512, 513)))       # seeded


def test_impulse_reference_is_the_float64_fft():
    n = 64
    pos, amp, w = bh.positions(n, n), bh.amplitudes(n), bh.custom_window(n)
    x = bh.impulse_frames(n, pos, amp).astype(np.complex128) * w.astype(np.float64)
    assert np.abs(bh.impulse_ref(n, pos, amp, w, False) - np.fft.fft(x, axis=-1)).max() < 1e-13
    assert np.abs(bh.impulse_ref(n, pos, amp, w, True) - np.fft.fftshift(np.fft.fft(x, axis=-1), axes=-1)).max() < 1e-13
    assert np.all((np.abs(amp) >= 0.5) & (np.abs(amp) <= 2.0)) and amp.dtype == np.complex64


# ---- mutated stand-ins are rejected; the white-noise check accepts two of them -------------------------------------------
def _white_noise_check_accepts(transform, n):
    rng = np.random.default_rng(n)
    x = ((rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))) * 3.0).astype(np.complex64)
    assert_complex_parity(transform(x), np.fft.fft(x.astype(np.complex128), axis=-1), what="white noise")


def test_one_wrong_twiddle_index_in_the_first_stage_at_16384():
    """Butterfly i0 of stage 0 reads W^1 for W^0: its operand is off by 2 pi / 16384 = 3.8e-4, which is 57 bars on the frame
    whose impulse feeds it and about 1e-6 of the peak of a white-noise frame.  The sampled basis sees the sampled input
    positions only, so the butterfly is taken among them here; the full bases (N <= 4096) have no such restriction."""
    n = 16384
    pos = bh.positions(n, 128, powers=True)
    j = int(pos[pos >= n // 2][7])
    bad = stockham32(wrong_index=(0, j - n // 2))
    _white_noise_check_accepts(bad, n)                       # the gap
    with pytest.raises(AssertionError, match="impulse basis"):
        bh.check_impulse_basis(bad, n, pos)
    bh.check_impulse_basis(stockham32(), n, pos)
    # any butterfly, full basis
    with pytest.raises(AssertionError, match="impulse basis"):
        bh.check_impulse_basis(stockham32(wrong_index=(0, 333)), 1024, bh.positions(1024, 1024))


def test_one_table_entry_off_by_2e_5_at_16384():
    """An odd entry is read by one butterfly of the last stage: 2e-5 of that operand, three bars on every frame that reaches
    it, under 1e-5 of a white-noise peak."""
    n = 16384
    table = bh.twiddle_table(n).astype(np.complex64)
    table[4097] += np.float32(2e-5)
    bad = stockham32(table=table)
    _white_noise_check_accepts(bad, n)                       # the gap
    with pytest.raises(AssertionError, match="impulse basis"):
        bh.check_impulse_basis(bad, n, bh.positions(n, 128, powers=True))


@pytest.mark.parametrize("mutation", ["window_neighbour", "swap_iq", "swap_bins"])
def test_moved_window_coefficient_swapped_iq_exchanged_bins(mutation):
    n = 256
    pos, w = bh.positions(n, n), bh.custom_window(n)
    with pytest.raises(AssertionError, match="impulse basis"):
        bh.check_impulse_basis(numpy32(window=w, mutate=mutation), n, pos, window=w)
    # (the dB row of an impulse is flat at |w[j] a_j|: of the three only the window coefficient shows there)
    if mutation == "window_neighbour":
        with pytest.raises(AssertionError, match="impulse basis"):
            bh.check_impulse_basis(numpy32(window=w, db=True, mutate=mutation), n, pos, window=w, db=True)
    if mutation == "swap_bins":
        with pytest.raises(AssertionError, match="tone basis"):
            bh.check_tone_basis(numpy32(mutate=mutation), n, np.arange(n))


# ---- the row picks of the long calls, on a model of the persistent loop ---------------------------------------------------
def _persistent_loop(n_frames, grid, f, fault=None):
    """Row r holds the number of the frame it was computed from, -1 where nothing was written."""
    out = np.full(n_frames, -1, np.int64)
    n_groups = -(-n_frames // f)
    for g in range(n_groups):
        src = g
        if fault == "next_trip_into_this_group" and g + grid < n_groups:
            src = g + grid                                   # the prefetched group lands in the current rows
        if fault == "stale_after_wrap" and g >= grid:
            src = g - grid                                   # the prefetch was never picked up
        if fault == "drops_ragged_group" and (g + 1) * f > n_frames:
            continue
        if fault == "grid_one_short" and g % grid == grid - 1:
            continue
        rows = np.arange(g * f, min((g + 1) * f, n_frames))
        out[rows] = src * f + (rows - g * f)
    return out


@pytest.mark.parametrize("n,num_cus", [(16, 256), (128, 256), (512, 8), (2048, 256), (8192, 8), (16384, 256)])
def test_row_picks_catch_a_wrong_persistent_loop(n, num_cus):
    grid, f = bh.lds_grid(n, num_cus), bh.lds_frames_per_group(n)
    frames = bh.long_call_frames(grid, f)
    picks = bh.pick_rows(frames, grid, f)
    assert len(picks) <= 2 * f + 32 and picks[0] == 0 and picks[-1] == frames - 1
    assert np.array_equal(_persistent_loop(frames, grid, f)[picks], picks)
    faults = ("next_trip_into_this_group", "stale_after_wrap", "grid_one_short") + (("drops_ragged_group",) if f > 1 else ())
    for fault in faults:                                     # (one frame per workgroup: no group is ragged)
        assert not np.array_equal(_persistent_loop(frames, grid, f, fault)[picks], picks), fault


def test_grids_are_the_launchers():
    """launch_lds_n: per_cu = min(160 KiB / LDS, 2048 / WG, 4); launch_fft_small: min(160 KiB / max(LDS, 8 KiB), 8)."""
    assert [bh.lds_grid(n, 256) for n in (16, 128, 256, 512, 2048, 8192, 16384)] == [1024, 1024, 1024, 1024, 1024, 512, 256]
    assert [bh.lds_frames_per_group(n) for n in (16, 128, 512, 2048, 8192)] == [256, 32, 8, 2, 1]
    assert bh.small_grid(8, 256) == 2048 and bh.small_grid(4096, 8) == 16
    assert bh.long_call_frames(1024, 256) == 524545

"""What test_generic_sizes_gpu (the kernels) and test_basis_helpers (numpy stand-ins) share: the two bases that describe a
linear transform completely, their float64 references and derived bars, and the frame counts and row picks of the long
calls.  A plain module; nothing here touches the GPU.

The bars.  u = 2^-24.  Frame j of the impulse basis is a_j * delta[n - j]: along its single non-zero path every addition has
an exact zero operand, so only the twiddle products (and the window product) round.  Higham's per-level constant for a
twiddle correctly rounded to float32 is mu + gamma_4 (sqrt 2 + mu) < 8 u, a radix-16 pass counts as four levels (32 u also
covers its depth-4 twiddle product tree), hence

    tol(N) = 8 log2(N) u      per complex entry, relative to |w[j] a_j|     (+ u for the window product)

and for the dB rows |delta dB| <= 8.69 (tol + u) + 1e-6.  The tone basis (frame k = exp(+2 pi i k n / N) rounded to
complex64) is held to Higham's statement itself, ||got - ref||_2 <= tol(N) ||ref||_2 per frame, and its largest off-peak bin
to tol(N) of the peak.  None of these figures comes from a measurement of the code under test.
"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-12
SLAB = 512                      # rows of a reference built at a time, at most (and at most 2^22 entries)


def _slab(n):
    return max(1, min(SLAB, (1 << 22) // n))


def tol(n):
    return 8.0 * np.log2(n) * U


def complex_bar(n, windowed):
    return tol(n) + (U if windowed else 0.0)


def db_bar(n, windowed):
    return 8.69 * (complex_bar(n, windowed) + U) + 1e-6


# ---- inputs --------------------------------------------------------------------------------------------------------
def amplitudes(n, seed=1):
    """a_j, complex64 (n,): magnitude in [0.5, 2], seeded random phase — a swapped I/Q, a lost sign or a moved window
    coefficient changes the value, not only the phase."""
    rng = np.random.default_rng([seed, n])
    return (rng.uniform(0.5, 2.0, n) * np.exp(2j * np.pi * rng.random(n))).astype(np.complex64)


def custom_window(n, seed=2):
    return (0.25 + 0.75 * np.random.default_rng([seed, n]).random(n)).astype(np.float32)


def twiddle_table(n):
    """T[m] = exp(-2 pi i m / n), float64."""
    return np.exp(-2j * np.pi * np.arange(n) / n)


def _lookup(t, idx):
    """t[idx] for a twiddle table t; a long table is read as the product of two short ones that stay in the cache
    (W^(2048 hi + lo) = W^(2048 hi) W^lo, one more rounding of 1e-16)."""
    if len(t) <= 1 << 16:
        return t[idx]
    return t[::2048][idx >> 11] * t[:2048][idx & 2047]


def positions(n, count, seed=3, extra=(), powers=False):
    """`count` input positions of an n-point frame (all of them when count >= n): the first and last count/8, count/8
    around n/2, `extra` (tile edges), with `powers` every 2^a and 2^a +- 1, the rest seeded random.  Sorted, unique."""
    if count >= n:
        return np.arange(n)
    e = max(count // 8, 1)
    must = set(range(e)) | set(range(n - e, n)) | set(range(n // 2 - e // 2, n // 2 + (e + 1) // 2))
    must |= {int(p) for p in extra if 0 <= int(p) < n}
    rng = np.random.default_rng([seed, n])
    while len(must) < count:
        must.add(int(rng.integers(0, n)))
    if powers:                                  # on top of the count
        for a in range(int(np.log2(n)) + 1):
            must |= {p for p in ((1 << a) - 1, 1 << a, (1 << a) + 1) if 0 <= p < n}
    return np.array(sorted(must))


def impulse_frames(n, pos, amp):
    """complex64 (len(pos), n): frame i is amp[pos[i]] at sample pos[i], zeros elsewhere."""
    x = np.zeros((len(pos), n), np.complex64)
    x[np.arange(len(pos)), pos] = amp[pos]
    return x


def tone_frames(n, ks):
    """complex64 (len(ks), n): frame i is exp(+2 pi i ks[i] m / n), from the float64 table, rounded once."""
    t = np.conj(twiddle_table(n))
    m, ks = np.arange(n, dtype=np.int64), np.asarray(ks, np.int64)
    x = np.empty((len(ks), n), np.complex64)
    for lo in range(0, len(ks), _slab(n)):
        x[lo:lo + _slab(n)] = _lookup(t, (ks[lo:lo + _slab(n), None] * m[None, :]) & (n - 1))
    return x


# ---- checkers: each returns its worst err / bar, prints it, and asserts it is <= 1 ----------------------------------------
def _worst(d):
    """The largest entry; a NaN counts as infinite."""
    return float(np.where(np.isnan(d), np.inf, d).max())


def _scale(n, pos, amp, window):
    w = np.ones(n) if window is None else np.asarray(window, np.float64)
    return w[pos] * amp[pos].astype(np.complex128)


def impulse_ref(n, pos, amp, window, shift, table=None):
    """complex128 (len(pos), n): w[j] a_j T[(j k) mod n], rolled by n/2 when `shift`.  A table lookup, no FFT."""
    t = twiddle_table(n) if table is None else table
    k = np.arange(n, dtype=np.int64) + (n // 2 if shift else 0)
    idx = (np.asarray(pos, np.int64)[:, None] * k[None, :]) & (n - 1)
    return _scale(n, pos, amp, window)[:, None] * _lookup(t, idx)


def impulse_complex_err(got, n, pos, amp, window=None, shift=False):
    """max over entries of |got - ref| / |w[j] a_j|, divided by the bar; the reference is built a slab of rows at a time."""
    got = np.asarray(got)
    assert got.shape == (len(pos), n) and got.dtype == np.complex64, (got.shape, got.dtype)
    t, bar, worst = twiddle_table(n), complex_bar(n, window is not None), 0.0
    mag = np.abs(_scale(n, pos, amp, window))
    for lo in range(0, len(pos), _slab(n)):
        hi = lo + _slab(n)
        d = np.abs(got[lo:hi] - impulse_ref(n, pos[lo:hi], amp, window, shift, t)).max(axis=1) / mag[lo:hi]
        worst = max(worst, _worst(d) / bar)
    return worst


def impulse_db_err(got, n, pos, amp, window=None, eps=EPS):
    """max |got - 20 log10(|w[j] a_j| + eps)| over every bin, divided by the bar."""
    got = np.asarray(got)
    assert got.shape == (len(pos), n) and got.dtype == np.float32, (got.shape, got.dtype)
    ref = 20.0 * np.log10(np.abs(_scale(n, pos, amp, window)) + eps)
    d = np.abs(got.astype(np.float64) - ref[:, None])
    return _worst(d) / db_bar(n, window is not None)


def tone_err(got, frames, ks):
    """(worst ||got - ref||_2 / ||ref||_2, worst off-peak |got| / peak), each divided by tol(n); ref = float64 FFT of the
    rounded samples."""
    got, n = np.asarray(got), frames.shape[1]
    assert got.shape == frames.shape and got.dtype == np.complex64, (got.shape, got.dtype)
    l2 = off = 0.0
    ks = np.asarray(ks)
    for lo in range(0, len(ks), _slab(n)):
        hi = lo + _slab(n)
        g = got[lo:hi].astype(np.complex128)
        ref = np.fft.fft(frames[lo:hi].astype(np.complex128), axis=-1)
        l2 = max(l2, _worst(np.linalg.norm(g - ref, axis=1) / np.linalg.norm(ref, axis=1)))
        a = np.abs(g)
        rows = np.arange(a.shape[0])
        peak = a[rows, ks[lo:hi] % n].copy()
        a[rows, ks[lo:hi] % n] = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            off = max(off, _worst(a.max(axis=1) / peak))
    return l2 / tol(n), off / tol(n)


def check_impulse_basis(transform, n, pos, *, window=None, shift=False, db=False, what=""):
    """transform(frames complex64 (P, n)) -> complex64 spectra (or float32 dB rows with `db`) of a plan with this window and
    shift.  One call with all the frames; prints and returns the worst err / bar, which must not exceed 1."""
    amp = amplitudes(n)
    got = transform(impulse_frames(n, pos, amp))
    r = impulse_db_err(got, n, pos, amp, window) if db else impulse_complex_err(got, n, pos, amp, window, shift)
    print(f"BASIS impulse N={n} {what} {'db' if db else 'c64'} frames={len(pos)} err/tol={r:.3f}")
    assert r <= 1.0, f"N={n} {what}: impulse basis at {r:.3f} of its bar"
    return r


def check_tone_basis(transform, n, ks, what=""):
    frames = tone_frames(n, ks)
    l2, off = tone_err(transform(frames), frames, ks)
    print(f"BASIS tone N={n} {what} frames={len(ks)} l2/tol={l2:.3f} offpeak/tol={off:.3f}")
    assert l2 <= 1.0 and off <= 1.0, f"N={n} {what}: tone basis at {l2:.3f} (l2) and {off:.3f} (off-peak) of tol(N)"
    return l2, off


# ---- the long calls: the grid as the launchers size it, the frame count, the rows read back -------------------------------
def lds_frames_per_group(n):
    """LdsCfg::F: 4096 / N frames share a 256-thread workgroup below 4096, one frame per workgroup above."""
    return 4096 // n if n < 4096 else 1


def lds_grid(n, num_cus):
    """The grid cap of launch_lds_n: num_cus * per_cu workgroups."""
    t = n // 16
    wg = max(t, 256)
    lds_bytes = (wg // t) * (n + n // 16) * 8
    return num_cus * max(1, min(160 * 1024 // lds_bytes, 2048 // wg, 4))


def small_grid(n, num_cus):
    """The grid cap of launch_fft_small (one frame per workgroup)."""
    return num_cus * min(160 * 1024 // max(2 * n * 8, 8192), 8)


def long_call_frames(grid, f):
    """Two full trips of the persistent loop, one more full group and a last group of one frame."""
    return 2 * grid * f + f + 1


def pick_rows(n_frames, grid, f, seed=0, n_random=16):
    """First and last frame, both sides of each grid wrap, the whole last group, n_random seeded frames."""
    picks = {0, n_frames - 1}
    for wrap in range(grid * f, n_frames, grid * f):
        picks |= {wrap - 1, wrap}
    picks |= set(range(((n_frames - 1) // f) * f, n_frames))
    picks |= {int(v) for v in np.random.default_rng([seed, n_frames]).integers(0, n_frames, n_random)}
    return np.array(sorted(p for p in picks if 0 <= p < n_frames))

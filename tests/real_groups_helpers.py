"""What the tests of the integrated real-input mode share (test_real_groups_gpu.py, test_real_groups_host.py and the snippets
they run in child processes): the input streams of the amplitude-bound cases, the float64 reference powers, the float32 replay
of the compensated mean, and a numpy stand-in of SpectrumPlan.rintegrate.  A plain module, no GPU needed."""
import numpy as np

K4096_HOP = 64          # the K = 4096 case: 4096 frames of 8192 samples, 64 apart


def bound_stream(n, frames, seed):
    """(frames, 2 n) float32: unit noise plus an off-bin tone 26 dB above it in amplitude, as test_real_gpu's staged cases."""
    length = 2 * n
    rng = np.random.default_rng(seed)
    t = np.arange(frames * length).reshape(frames, length)
    x = rng.standard_normal((frames, length)) + 20 * np.cos(2 * np.pi * (0.1234 * length + 0.3) * t / length)
    return np.ascontiguousarray(x.astype(np.float32))


def k4096_stream():
    """Flat float32: a strong tone in weak noise, long enough for 4096 frames of 8192 at K4096_HOP — per bin 4096 nearly
    equal powers, the case in which plain float32 summation drifts."""
    n = 8192 + 4095 * K4096_HOP
    rng = np.random.default_rng(4096)
    x = 100.0 * np.cos(2 * np.pi * (611.3 / 8192) * np.arange(n) + 0.3) + 0.01 * rng.standard_normal(n)
    return x.astype(np.float32)


def frames_of(x, length, frames, hop):
    """(frames, length): frame f of the flat stream x covers [f hop, f hop + length)."""
    return x[(np.arange(frames) * hop)[:, None] + np.arange(length)[None, :]]


def window64(window, length):
    if window is None:
        return np.ones(length)
    if isinstance(window, str):
        assert window == "hann"
        return np.hanning(length)
    return np.asarray(window, dtype=np.float64)


def ref_power(frames, window, chunk=512):
    """float64 |rfft(w x_f)|^2 of (frames, length) real frames: (frames, length // 2 + 1)."""
    w = window64(window, frames.shape[1])
    out = np.empty((frames.shape[0], frames.shape[1] // 2 + 1))
    for i in range(0, frames.shape[0], chunk):
        out[i:i + chunk] = np.abs(np.fft.rfft(frames[i:i + chunk].astype(np.float64) * w, axis=-1)) ** 2
    return out


def kahan_mean32(p, groups, k):
    """The MEAN detector replayed in float32 on per-frame powers p (groups * k, bins): int_accumulate's compensated sum in
    frame order, then (acc - cmp) * float32(1 / k).  numpy's float32 operations round once each and fuse nothing."""
    assert p.dtype == np.float32
    g = p.reshape(groups, k, -1)
    acc = np.zeros((groups, g.shape[2]), np.float32)
    cmp = np.zeros_like(acc)
    for f in range(k):
        y = g[:, f] - cmp
        t = acc + y
        cmp = (t - acc) - y
        acc = t
    return (acc - cmp) * (np.float32(1.0) / np.float32(k))


def numpy_rintegrate(nfft, window):
    """A stand-in of SpectrumPlan.rintegrate in float64 numpy, for tests that monkeypatch the plan call away: the same
    arguments, float32 rows."""
    def rintegrate(self, x, k, hop=None, detector="mean", out="db", scale=1.0):
        length = 2 * nfft
        hop = length if hop is None else int(hop)
        frames = (1 + (x.shape[0] - length) // hop) // int(k) * int(k)
        p = ref_power(frames_of(np.asarray(x, dtype=np.float64), length, frames, hop), window).reshape(-1, int(k), nfft + 1)
        r = {"mean": p.mean(axis=1), "max": p.max(axis=1), "min": p.min(axis=1)}[detector]
        return (scale * r if out == "power" else 20 * np.log10(np.sqrt(r) + 1e-12)).astype(np.float32)
    return rintegrate

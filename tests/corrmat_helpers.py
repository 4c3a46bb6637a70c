"""What the correlation-matrix tests (test_corrmat_gpu.py) share: the 12-bit integer test signals, from ONE generator so that the
complex64, int16 and 8-bit forms see the same data; the float64 numpy reference (numpy.fft of each channel, products and sums in
float64 — never the library) and the bounds of tests/test_xspec_gpu.py's docstring applied per pair; the entries.  A plain module,
imported by name.

The bounds are derived, not tuned.  Per group, bin and channel pair (i, j), with a_f = |X_i,f|, b_f = |X_j,f|, S_i and S_j each
channel's largest reference amplitude in the group, d_i = REL_TOL * S_i (the project's amplitude bar on each spectrum, tests/
parity.py) and u = 2^-24:

    re_ij, im_ij:  tol = 2 [ sum_f (a_f d_j + b_f d_i + d_i d_j) + (K + 2) u sum_f a_f b_f ] scale / K
    auto c:        |sqrt(R_got) - sqrt(R_ref)| <= REL_TOL * S_c + (K u / 2) sqrt(R_ref)

Every check prints its worst err/tol."""
import numpy as np

from sdr_iq_visualizer_amd.spectrum import CorrelationMatrix, plane_index
from tests.gpu_helpers import DevBuf, window_of
from tests.parity import REL_TOL

U = 2.0 ** -24


def hop_of(kind, n):
    return {"packed": n, "half": n // 2, "gapped": n + n // 3 + 1}[kind]


def noise(rng, L, sigma):
    return (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * (sigma / np.sqrt(2))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def elements16(seed, n, frames, hop, channels, bits=12):
    """(L, C, 2) int16 elements, rounded and clipped to `bits` bits (12; the 8-bit cases: 7, with everything scaled to fit).
    Channel c: a common component with a gain and phase of its own, plus the channel's own noise, plus an off-bin tone."""
    rng = np.random.default_rng(seed)
    L = (frames - 1) * hop + n
    amp = 2.0 ** (bits - 12)
    common = noise(rng, L, 150.0 * amp)
    out = np.empty((L, channels, 2), np.int16)
    lim = 2 ** (bits - 1)
    for c in range(channels):
        tone = amp * min(150.0 * 10 ** 1.5 / np.sqrt(n), 900.0) * np.exp(2j * np.pi * ((0.1234 + 0.05 * c) + 0.37 / n) * np.arange(L))
        x = (1.0 - 0.08 * c) * np.exp(0.9j * c) * common + noise(rng, L, 100.0 * amp) + tone
        out[:, c, 0] = np.clip(np.rint(x.real), -lim, lim - 1)
        out[:, c, 1] = np.clip(np.rint(x.imag), -lim, lim - 1)
    return out


def to_ci8(x16):
    """7-bit int16 elements -> int8 elements (exact)."""
    assert x16.min() >= -128 and x16.max() <= 127
    return x16.astype(np.int8)


def to_cu8(x16):
    """7-bit int16 elements v -> uint8 bytes v + 128, which the library widens to v + 0.5."""
    assert x16.min() >= -128 and x16.max() <= 127
    return (x16 + 128).astype(np.uint8)


def widen_c(x):
    """(L, C, 2) int16 / int8 / uint8 -> (L, C) complex64, exactly as the library widens (cu8: byte - 127.5)."""
    f = np.ascontiguousarray(x).astype(np.float32)
    if x.dtype == np.uint8:
        f -= np.float32(127.5)
    return f.view(np.complex64).reshape(x.shape[0], x.shape[1])


def pair_stream(x, i, j):
    """The two-channel element stream built from channels i and j of an (L, C) or (L, C, 2) stream."""
    return np.ascontiguousarray(x[:, [i, j]])


# ---- the float64 reference and the derived bounds ---------------------------------------------------------------------------
def ref_spectra(xc, n, frames, hop, window, shift):
    """float64 spectra (C, frames, n) complex128 in the plan's bin order, of an (L, C) complex stream."""
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n)[None, :]
    z = xc.astype(np.complex128)
    s = np.fft.fft(z.T[:, idx] * window_of(window, n), axis=-1)
    return np.fft.fftshift(s, axes=-1) if shift else s


class Ref:
    """The float64 means of every plane (groups, C*C, n) per unit scale, and the bounds of the module docstring."""

    def __init__(self, X, groups, k):
        C = X.shape[0]
        X = X[:, : groups * k].reshape(C, groups, k, -1)
        a = np.abs(X)
        self.C, self.k = C, k
        self.mean = np.empty((groups, C * C, X.shape[-1]))
        self.tol = np.empty_like(self.mean)          # autos: on the amplitude sqrt(R); pairs: on the plane's value
        s = a.reshape(C, groups, -1).max(axis=2)[:, :, None]          # (C, groups, 1)
        d = REL_TOL * s
        for c in range(C):
            self.mean[:, c] = (a[c] ** 2).sum(axis=1) / k
            self.tol[:, c] = d[c] + (k * U / 2) * np.sqrt(self.mean[:, c])
        for i in range(C):
            for j in range(i + 1, C):
                q = plane_index(C, i, j)
                z = (X[i] * np.conj(X[j])).sum(axis=1) / k
                self.mean[:, q], self.mean[:, q + 1] = z.real, z.imag
                di, dj = d[i][:, None, :], d[j][:, None, :]
                t = 2 * ((a[i] * dj + a[j] * di + di * dj).sum(axis=1) + (k + 2) * U * (a[i] * a[j]).sum(axis=1)) / k
                self.tol[:, q] = self.tol[:, q + 1] = t

    def check(self, got, scale, what):
        """Every plane of got (groups, C*C, n); -> (worst err/tol of the autos, of the pair planes)."""
        assert got.shape == self.mean.shape and got.dtype == np.float32, (what, got.shape)
        assert np.all(np.isfinite(got)), what
        g = got.astype(np.float64) / scale
        C = self.C
        w_auto = float((np.abs(np.sqrt(g[:, :C]) - np.sqrt(self.mean[:, :C])) / self.tol[:, :C]).max())
        w_pair = float((np.abs(g[:, C:] - self.mean[:, C:]) / self.tol[:, C:]).max())
        print(f"{what}: worst err/tol autos {w_auto:.2e}, pairs {w_pair:.2e}")
        assert w_auto <= 1.0 and w_pair <= 1.0, (what, w_auto, w_pair)
        return w_auto, w_pair

    def matrix(self):
        return CorrelationMatrix(self.mean, self.C)

    def pair_tol(self, i, j):
        return self.tol[:, plane_index(self.C, i, j)]

    def coherence_tol(self, i, j):
        """What the plane bounds allow the coherence of (i, j) to move (first order, doubled)."""
        m = self.mean
        q = plane_index(self.C, i, j)
        pa, pb, cre, cim, t = m[:, i], m[:, j], m[:, q], m[:, q + 1], self.tol[:, q]
        ta = 2 * np.sqrt(pa) * self.tol[:, i] + self.tol[:, i] ** 2
        tb = 2 * np.sqrt(pb) * self.tol[:, j] + self.tol[:, j] ** 2
        c2 = cre ** 2 + cim ** 2
        return 2 * (c2 / (pa * pb)) * (2 * (np.abs(cre) + np.abs(cim)) * t / c2 + ta / pa + tb / pb)

    def phase_tol(self, i, j):
        q = plane_index(self.C, i, j)
        cre, cim = self.mean[:, q], self.mean[:, q + 1]
        return 2 * (np.abs(cre) + np.abs(cim)) * self.tol[:, q] / (cre ** 2 + cim ** 2)


def reference(xc, n, groups, k, hop, window, shift):
    return Ref(ref_spectra(xc, n, groups * k, hop, window, shift), groups, k)


# ---- the entries ------------------------------------------------------------------------------------------------------------
_DEVICE = {np.dtype(np.complex64): ("exec_device_corrmat", {}), np.dtype(np.int16): ("exec_device_corrmat_ci16", {}),
           np.dtype(np.int8): ("exec_device_corrmat_ci8", {"unsigned": False}),
           np.dtype(np.uint8): ("exec_device_corrmat_ci8", {"unsigned": True})}
_HOST = {np.dtype(np.complex64): "correlate", np.dtype(np.int16): "correlate_ci16", np.dtype(np.int8): "correlate_ci8",
         np.dtype(np.uint8): "correlate_ci8"}


def device_cm(plan, x, groups, k, hop, scale=1.0, offset_samples=0):
    """(groups, C*C, nfft) float32 from the device entry of x's format; x: (L, C) complex64 or (L, C, 2) integers.  With
    offset_samples the stream starts that many samples of one channel into the device buffer: aligned to a sample only."""
    C = x.shape[1]
    entry, kw = _DEVICE[x.dtype]
    off = offset_samples * (x.nbytes // (x.shape[0] * C))
    with DevBuf(x.nbytes + off) as d_in, DevBuf(groups * C * C * plan.nfft * 4) as d_out:
        flat = np.zeros(x.nbytes + off, np.uint8)
        flat[off:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        d_in.put(flat)
        d_out.put(np.full((groups, C * C, plan.nfft), np.nan, np.float32))
        getattr(plan, entry)(d_in.p.value + off, C, groups, k, d_out.p.value, frame_stride=hop, scale=scale, **kw)
        plan.sync()
        return d_out.get((groups, C * C, plan.nfft), np.float32)


def host_cm(plan, x, k, hop, scale=1.0):
    r = getattr(plan, _HOST[x.dtype])(x, k, hop, scale)
    assert isinstance(r, CorrelationMatrix) and r.channels == x.shape[1]
    return r.planes


def device_xs(plan, x2, groups, k, hop, scale=1.0):
    """(groups, 4, nfft) float32 from the existing two-channel device entry on (L, 2) complex64 elements."""
    with DevBuf(x2.nbytes) as d_in, DevBuf(groups * 4 * plan.nfft * 4) as d_out:
        d_in.put(x2)
        plan.exec_device_xspec(d_in.p.value, groups, k, d_out.p.value, frame_stride=hop, scale=scale)
        plan.sync()
        return d_out.get((groups, 4, plan.nfft), np.float32)


def pair_planes(cm, C, i, j):
    """The four planes (i, j, re_ij, im_ij) of a (groups, C*C, nfft) result, in the two-channel layout."""
    q = plane_index(C, i, j)
    return np.ascontiguousarray(cm[:, [i, j, q, q + 1]])


def wrap(phi):
    return (phi + np.pi) % (2 * np.pi) - np.pi

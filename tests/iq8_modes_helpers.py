"""What the GPU tests of the 8-bit filter-bank and spectral-kurtosis entry points (test_iq8_modes_gpu.py) and the snippets they
run in child processes share: the 8-bit stream (first sample at byte 2 of its buffer) and its widened form resident on the
device with an output buffer that ends in a canary row, the N = 4096 cases that run twice (in the test process, and in a
child with SDRK_NUM_CUS=8), and the float64 reference of the two spectral-kurtosis planes with its tolerances.  The yardstick
of every bit comparison is the existing complex64 entry of the same plan on widen8(x).  A plain module, imported by name
(tests.iq8_modes_helpers); the byte streams and the widening are tests.ci8_helpers'."""
import numpy as np

from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.ci8_helpers import DTYPES, stream8, widen8  # noqa: F401  (re-exported to the snippets)
from tests.gpu_helpers import DETECTORS, EPS, FORMS, DevBuf, prototype, same_bits, same_bits_f32
from tests.parity import REL_TOL, mag_from_db

N4K = 4096
G3 = N4K + N4K // 3 + 1          # an odd, gapped hop (test_pfb_ci16_gpu.py's)
SCALE = 0.37
U = 2.0 ** -24
CANARY = 0x7FC0DEAD              # a NaN pattern no row holds

# (taps, frames, hop, shift, prototype)
PER_FRAME_4096 = [
    (1, 1, N4K, True, "default"),
    (2, 7, G3, False, "random"),            # fewer than 8 frames: empty per-XCD ranges
    (4, 1700, N4K, True, "random"),         # more frames than the 768 workgroups: the persistent loop, prefetch across frames
    (4, 1700, 1, False, "default"),         # 2-byte-aligned starts, odd sample offsets
    (5, 769, N4K // 4, True, "default"),
    (32, 3, N4K, False, "random"),          # the tap limit
]
# (taps, k, groups, hop, shift, prototype)
INTEGRATED_4096 = [
    (1, 1, 9, N4K, True, "default"),
    (2, 3, 5, G3, False, "random"),
    (4, 2, 800, N4K, True, "random"),       # more units than workgroups
    (4, 16, 40, N4K // 4, False, "default"),
    (4, 1700, 1, N4K, True, "default"),     # slices, partials, finalize
    (5, 100, 2, 1, False, "random"),
    (32, 2, 3, N4K, True, "random"),
]
# (k, groups, hop)
SK_4096 = [(5, 40, N4K), (33, 2, 1001), (2, 800, N4K), (1700, 1, N4K)]


class Dev8:
    """An 8-bit stream whose first sample sits at byte 2 of its device buffer, its widened form beside it, and an output
    buffer that holds max_rows rows of row_floats float32 + one canary row (fewer, longer rows too)."""

    OFFSET = 2

    def __init__(self, iq, max_rows, row_floats):
        self.unsigned = iq.dtype == np.uint8
        self.d8, self.d64 = DevBuf(iq.nbytes + self.OFFSET), DevBuf(iq.nbytes * 4)
        self.out = DevBuf((max_rows + 1) * row_floats * 4)
        self.d8.put(np.concatenate([np.zeros(self.OFFSET, np.uint8), iq.reshape(-1).view(np.uint8)]))
        self.d64.put(widen8(iq))
        self.p8, self.p64 = self.d8.p.value + self.OFFSET, self.d64.p.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in (self.d8, self.d64, self.out):
            d.__exit__()

    def run(self, plan, rows, row_floats, call):
        """call(out pointer) -> the `rows` rows of row_floats float32 it wrote; nothing may be written behind them."""
        self.out.put(np.full((rows + 1, row_floats), CANARY, np.uint32))
        call(self.out.p.value)
        plan.sync()
        got = self.out.get((rows + 1, row_floats), np.uint32)
        assert np.all(got[rows] == CANARY), "a row was written past the last one"
        return got[:rows].view(np.float32)

    # the 8-bit entry and its complex64 yardstick, pair by pair
    def pfb(self, plan, frames, hop):
        n = plan.nfft
        return (self.run(plan, frames, n, lambda o: plan.exec_device_pfb_ci8(self.p8, frames, o, unsigned=self.unsigned, frame_stride=hop)),
                self.run(plan, frames, n, lambda o: plan.exec_device_pfb(self.p64, frames, o, frame_stride=hop)))

    def pfb_int(self, plan, groups, k, hop, det, form):
        kw = dict(frame_stride=hop, detector=det, out=form, scale=SCALE)
        n = plan.nfft
        return (self.run(plan, groups, n, lambda o: plan.exec_device_pfb_integrated_ci8(self.p8, groups, k, o, unsigned=self.unsigned, **kw)),
                self.run(plan, groups, n, lambda o: plan.exec_device_pfb_integrated(self.p64, groups, k, o, **kw)))

    def sk(self, plan, groups, k, hop, form, pfb=False):
        kw = dict(frame_stride=hop, out=form, scale=SCALE)
        new, old = (plan.exec_device_pfb_sk_ci8, plan.exec_device_pfb_sk) if pfb else (plan.exec_device_sk_ci8, plan.exec_device_sk)
        n2 = 2 * plan.nfft      # (per group the mean-power row, then the SK row)
        return (self.run(plan, groups, n2, lambda o: new(self.p8, groups, k, o, unsigned=self.unsigned, **kw)),
                self.run(plan, groups, n2, lambda o: old(self.p64, groups, k, o, **kw)))


def case_per_frame(dtype, n, taps, frames, hop, shift, proto, seed=1, spectra=True):
    """dB rows of the device entry and (through the host entry, which alone returns them) the spectra, in bits."""
    iq = stream8(seed + frames, (frames - 1) * hop + taps * n, dtype)
    with Dev8(iq, frames, n) as d, SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        assert plan.set_pfb(prototype(proto, n, taps, seed + 7)) == taps
        got, want = d.pfb(plan, frames, hop)
        assert same_bits_f32(got, want), (dtype, n, taps, frames, hop, shift, int(np.sum(got != want)))
        assert np.all(np.isfinite(got)) and got.std() > 0
        if spectra:
            got_fft = plan.pfb_fft_ci8(iq, hop)
            assert got_fft.shape == (frames, n) and same_bits(got_fft, plan.pfb_fft(widen8(iq), hop)), (dtype, n, taps, frames, hop, "spectra")


def case_integrated(dtype, n, taps, k, groups, hop, shift, proto, seed=2):
    """Every detector and both forms of the integrated filter bank, in bits."""
    iq = stream8(seed + k, (groups * k - 1) * hop + taps * n, dtype)
    with Dev8(iq, groups, n) as d, SpectrumPlan(n, eps=EPS, shift=shift) as plan:
        plan.set_pfb(prototype(proto, n, taps, seed + 3))
        for det in DETECTORS:
            for form in FORMS:
                got, want = d.pfb_int(plan, groups, k, hop, det, form)
                assert same_bits_f32(got, want), (dtype, n, taps, k, groups, hop, det, form)
                assert np.all(np.isfinite(got)) and got.std() > 0


def case_sk(dtype, n, k, groups, hop, windows=("hann", None), seed=3):
    """Both planes, both forms, with and without a window, in bits."""
    iq = stream8(seed + k, (groups * k - 1) * hop + n, dtype)
    with Dev8(iq, groups, 2 * n) as d:
        for window in windows:
            with SpectrumPlan(n, window=window, eps=EPS, shift=window is None) as plan:
                for form in FORMS:
                    got, want = d.sk(plan, groups, k, hop, form)
                    assert same_bits_f32(got, want), (dtype, n, k, groups, hop, window, form)
                    planes = got.reshape(groups, 2, n)
                    assert np.all(np.isfinite(planes)) and planes[:, 0].std() > 0 and planes[:, 1].std() > 0


def case_pfb_sk(dtype, n, taps, k, groups, hop, seed=4):
    iq = stream8(seed + k, (groups * k - 1) * hop + taps * n, dtype)
    with Dev8(iq, groups, 2 * n) as d, SpectrumPlan(n, eps=EPS) as plan:
        plan.set_pfb(prototype("default", n, taps, seed))
        for form in FORMS:
            got, want = d.sk(plan, groups, k, hop, form, pfb=True)
            assert same_bits_f32(got, want), (dtype, n, taps, k, groups, hop, form)
            assert np.all(np.isfinite(got))
        host = plan.pfb_spectral_kurtosis_ci8(iq, k, hop, "power", SCALE)
        assert same_bits_f32(host[0].base.reshape(groups, 2 * n), got), (dtype, n, taps, k, groups, hop, "host")


def cases_4096(dtype):
    """Sections 1 to 3 (the N = 4096 kernels) for one byte type; the host spectra once, not per case."""
    for i, (taps, frames, hop, shift, proto) in enumerate(PER_FRAME_4096):
        case_per_frame(dtype, N4K, taps, frames, hop, shift, proto, spectra=i == 1)
    for c in INTEGRATED_4096:
        case_integrated(dtype, N4K, *c)
    for c in SK_4096:
        case_sk(dtype, N4K, *c)


# ---- the float64 reference of the two planes (the bounds of test_sk_gpu.py, restated: no test module imports another) ------
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

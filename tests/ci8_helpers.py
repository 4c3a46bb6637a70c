"""What the 8-bit GPU tests (test_ci8_gpu.py) and the snippets they run in child processes share: byte-pair streams over the
whole range with the edge bytes planted, the numpy widening that is the yardstick's input, the stream and its widened form
resident on the device, and the bodies of the N = 4096 cases that run twice (in the test process, and in a child with
SDRK_NUM_CUS=8).  A plain module, imported by name (tests.ci8_helpers)."""
import numpy as np

from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import DETECTORS, FORMS, DevBuf, same_bits, same_bits_f32

DTYPES = (np.int8, np.uint8)
EDGE_BYTES = np.array([0, 127, 128, 255], np.uint8)        # int8: 0, 127, -128, -1; uint8: 0, 127, 128, 255


def stream8(seed, n_samples, dtype):
    """(n_samples, 2) int8 / uint8 over the full byte range; 0, 127, 128 (-128) and 255 (-1) planted at both ends and scattered."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n_samples, 2), dtype=np.int64).astype(np.uint8)
    flat = b.reshape(-1)
    m = min(4, flat.size)
    flat[:m] = EDGE_BYTES[:m]
    flat[flat.size - m:] = EDGE_BYTES[:m][::-1]
    if flat.size > 64:
        at = rng.integers(0, flat.size, size=flat.size // 16)
        flat[at] = EDGE_BYTES[rng.integers(0, 4, size=at.shape[0])]
    return b.view(dtype)


def widen8(x):
    """(..., 2) int8 / uint8 -> (...) complex64 by the contract: I + iQ, or (I - 127.5) + i(Q - 127.5); exact in float32."""
    f = np.ascontiguousarray(x).astype(np.float32)
    if x.dtype == np.uint8:
        f -= np.float32(127.5)
    assert x.dtype in DTYPES and not np.any(np.signbit(f) & (f == 0))          # no -0.0 in the yardstick's input either
    return f.view(np.complex64)[..., 0]


class Pair8:
    """An 8-bit stream (first sample at byte `offset` of its buffer) and its widened form resident on the device, and an output
    buffer of max_rows rows + one canary row."""

    def __init__(self, iq, max_rows, nfft, offset=0):
        self.unsigned = iq.dtype == np.uint8
        self.d8, self.d64 = DevBuf(iq.nbytes + offset), DevBuf(iq.nbytes * 4)
        self.out = DevBuf((max_rows + 1) * nfft * 4)
        self.d8.put(np.concatenate([np.zeros(offset, np.uint8), iq.reshape(-1).view(np.uint8)]))
        self.d64.put(widen8(iq))
        self.p8 = self.d8.p.value + offset
        self.nfft = nfft

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in (self.d8, self.d64, self.out):
            d.__exit__()

    def _read(self, rows):
        got = self.out.get((rows + 1, self.nfft), np.uint32)
        assert np.all(got[rows] == 0x7FC0DEAD), "a row was written past the last one"
        return got[:rows].view(np.float32)

    def _canary(self, rows):
        self.out.put(np.full((rows + 1, self.nfft), 0x7FC0DEAD, np.uint32))    # (a NaN pattern no row holds)

    def rows8(self, plan, frames, stride):
        self._canary(frames)
        plan.exec_device_ci8(self.p8, frames, self.out.p.value, unsigned=self.unsigned, frame_stride=stride)
        plan.sync()
        return self._read(frames)

    def rows64(self, plan, frames, stride):
        self._canary(frames)
        plan.exec_device(self.d64.p.value, frames, self.out.p.value, frame_stride=stride)
        plan.sync()
        return self._read(frames)

    def int8(self, plan, groups, k, hop, det, form="db", scale=1.0):
        self._canary(groups)
        plan.exec_device_integrated_ci8(self.p8, groups, k, self.out.p.value, unsigned=self.unsigned, frame_stride=hop,
                                        detector=det, out=form, scale=scale)
        plan.sync()
        return self._read(groups)

    def int64(self, plan, groups, k, hop, det, form="db", scale=1.0):
        self._canary(groups)
        plan.exec_device_integrated(self.d64.p.value, groups, k, self.out.p.value, frame_stride=hop, detector=det, out=form,
                                    scale=scale)
        plan.sync()
        return self._read(groups)


PLANS_4096 = (("hann", True), (None, True), ("hann", False), (None, False))
STRIDES_4096 = (4096, 2048, 1, 4097, 5000)


def case_4096_per_frame(dtype, frames, offset=0):
    """Rows of the N = 4096 kernel at every stride, window and shift, against exec_device on the widened samples; spectra
    (packed frames: the host entry) against fft.  Nothing past the last row."""
    n = 4096
    iq = stream8(7 * frames + offset, (frames - 1) * max(STRIDES_4096) + n, dtype)
    with Pair8(iq, frames, n, offset) as d:
        for window, shift in PLANS_4096:
            with SpectrumPlan(n, window=window, shift=shift, max_batch=1024) as plan:
                for stride in STRIDES_4096:
                    got, ref = d.rows8(plan, frames, stride), d.rows64(plan, frames, stride)
                    assert same_bits_f32(got, ref), (dtype, frames, window, shift, stride, int(np.sum(got != ref)))
                    assert np.all(np.isfinite(got))
                x = np.ascontiguousarray(iq[: min(frames, 40) * n].reshape(-1, n, 2))
                assert same_bits(plan.fft_ci8(x), plan.fft(widen8(x))), (dtype, frames, window, shift, "spectra")
                assert same_bits(plan.spectrum_db_ci8(x), plan.spectrum_db(widen8(x))), (dtype, frames, window, shift, "host rows")


def case_4096_integrated(dtype, k, groups, windows=("hann", None)):
    """The reducing N = 4096 kernel against the complex64 integrated entry: every detector and form, hop N and N/2."""
    n = 4096
    iq = stream8(100 * k + groups, (groups * k - 1) * n + n, dtype)
    with Pair8(iq, groups, n) as d:
        for window in windows:
            with SpectrumPlan(n, window=window) as plan:
                for hop in (n, n // 2):
                    for det in DETECTORS:
                        for form in FORMS:
                            got = d.int8(plan, groups, k, hop, det, form, 0.5)
                            assert same_bits_f32(got, d.int64(plan, groups, k, hop, det, form, 0.5)), (dtype, k, groups, window, hop, det, form)
                            assert np.all(np.isfinite(got)) and got.std() > 0

"""What the GPU tests of the int16, PFB and integrated corners (test_ci16_gpu, test_integrate_gpu, test_integrate_ci16_gpu,
test_pfb_gpu, test_pfb_integrate_gpu, test_pfb_ci16_gpu) share: device buffers, bit comparisons, input streams, the numpy
references, and the child-process runner.  A plain module: the tests and the snippets they run in child processes import it by
name (tests.gpu_helpers); no test module imports another.

same_bits is test_ci16_gpu's; test_pfb_gpu's copy was the same comparison without the contiguity step (it raised where this
one answers).  Where the former copies of a helper differed otherwise, each behaviour has a name of its own here:
same_bits / same_bits_u32 / same_bits_f32, widen / widen_flat, stream_noise_tone / stream_synth_tone,
stream16_noise_tone / stream16_planted."""
import ctypes
import os
import subprocess
import sys

import numpy as np

from sdr_iq_visualizer_amd import _ffi, synth
from sdr_iq_visualizer_amd.spectrum import pfb_prototype
from tests.parity import REL_TOL, mag_from_db

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-12
DETECTORS = ("mean", "max", "min")
FORMS = ("db", "power")

PLANTED = np.array([[-32768, 32767], [32767, -32768], [-1, 0], [0, -1], [-32768, -32768], [32767, 32767], [-1, 1], [1, -1],
                    [0, 0], [-2, 255], [255, -256], [-256, 256]], dtype=np.int16)


class DevBuf:
    """Device memory on GPU 0 (at least 8 bytes of it), freed on leaving the `with`; get() reads from a byte offset."""
    def __init__(self, nbytes):
        self.p = ctypes.c_void_p()
        _ffi.check(_ffi.lib().sdrk_dev_alloc(0, max(int(nbytes), 8), ctypes.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _ffi.lib().sdrk_dev_free(0, self.p)

    def get(self, shape, dtype, offset=0):
        a = np.empty(shape, dtype)
        _ffi.check(_ffi.lib().sdrk_memcpy_d2h(0, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.p.value + offset), a.nbytes))
        return a

    def put(self, a):
        a = np.ascontiguousarray(a)
        _ffi.check(_ffi.lib().sdrk_memcpy_h2d(0, self.p, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))


# ---- bit comparisons --------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal as bit patterns (array_equal on the values would call two NaNs different and -0.0 / 0.0 the same)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_u32(a, b):
    """Equal shapes and 32-bit words; the dtypes are not compared."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_bits_f32(a, b):
    """Equal as bit patterns, and both float32."""
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- int16 pairs -> complex64, exactly ------------------------------------------------------------------------------------
def widen(x):
    """(..., 2) int16 -> (...) complex64: keeps the leading shape."""
    return (x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)).astype(np.complex64)


def widen_flat(iq):
    """(n, 2) int16 -> (n,) complex64, exactly."""
    return np.ascontiguousarray(iq).astype(np.float32).view(np.complex64).reshape(-1)


class Pair:
    """The int16 stream and its widened form resident on the device, and one output buffer: both device entries of a plan."""

    def __init__(self, iq, max_rows, nfft):
        self.d16, self.d64, self.out = DevBuf(iq.nbytes), DevBuf(iq.nbytes * 2), DevBuf(max_rows * nfft * 4)
        self.d16.put(iq)
        self.d64.put(widen_flat(iq))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in (self.d16, self.d64, self.out):
            d.__exit__()

    def ci16(self, plan, groups, k, hop, det, form="db", scale=1.0):
        self.out.put(np.full((groups, plan.nfft), np.nan, np.float32))       # (the complex64 call's rows are not left there)
        plan.exec_device_integrated_ci16(self.d16.p.value, groups, k, self.out.p.value, frame_stride=hop, detector=det,
                                         out=form, scale=scale)
        plan.sync()
        return self.out.get((groups, plan.nfft), np.float32)

    def c64(self, plan, groups, k, hop, det, form="db", scale=1.0):
        plan.exec_device_integrated(self.d64.p.value, groups, k, self.out.p.value, frame_stride=hop, detector=det, out=form,
                                    scale=scale)
        plan.sync()
        return self.out.get((groups, plan.nfft), np.float32)


# ---- input streams ---------------------------------------------------------------------------------------------------
def stream_noise_tone(rng, n, frames, hop, tone_db=30.0, noise=1.0):
    """Complex64 noise plus a tone `tone_db` above the noise's per-bin level (an off-bin frequency)."""
    L = (frames - 1) * hop + n
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * (noise / np.sqrt(2))
    amp = noise * 10 ** (tone_db / 20) / np.sqrt(n)
    x += amp * np.exp(2j * np.pi * (0.1234 + 0.37 / n) * np.arange(L))
    return x.astype(np.complex64)


def stream_synth_tone(seed, n_samples, tone_bin_of_4096=611.3):
    """complex64: synth.py's 12-bit integer noise plus a tone of amplitude 700, rounded to integers."""
    x = synth.synth_iq(seed, 0, 1, n_samples)[0].astype(np.complex128)
    t = 700.0 * np.exp(2j * np.pi * (tone_bin_of_4096 / 4096.0) * np.arange(n_samples))
    return (x + np.round(t.real) + 1j * np.round(t.imag)).astype(np.complex64)


def stream16_noise_tone(seed, n, frames, hop, tone_db=30.0):
    """(L, 2) int16: 12-bit noise plus an off-bin tone `tone_db` above the noise's per-bin level, L = the span of the frames."""
    rng = np.random.default_rng(seed)
    L = (frames - 1) * hop + n
    noise = 200.0
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * (noise / np.sqrt(2))
    amp = min(noise * 10 ** (tone_db / 20) / np.sqrt(n), 1200.0)
    x += amp * np.exp(2j * np.pi * (0.1234 + 0.37 / n) * np.arange(L))
    out = np.empty((L, 2), np.int16)
    out[:, 0] = np.clip(np.rint(x.real), -2048, 2047)
    out[:, 1] = np.clip(np.rint(x.imag), -2048, 2047)
    return out


def stream16_planted(seed, n_samples):
    """int16 (n_samples, 2) over the full range; the planted pairs at the start, at the end and scattered."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(n_samples, 2), dtype=np.int64).astype(np.int16)
    m = min(len(PLANTED), n_samples)
    x[:m] = PLANTED[:m]
    x[n_samples - m:] = PLANTED[:m][::-1]
    if n_samples > 4 * len(PLANTED):
        at = rng.integers(0, n_samples, size=n_samples // 16)
        x[at] = PLANTED[rng.integers(0, len(PLANTED), size=at.shape[0])]
    return x


def prototype(kind, n, taps, seed):
    if kind == "default":
        return pfb_prototype(n, taps)
    return np.random.default_rng(seed).standard_normal(taps * n).astype(np.float32)


# ---- references -------------------------------------------------------------------------------------------------------
def window_of(kind, n):
    return np.hanning(n) if kind == "hann" else np.ones(n)


def ref_power(x, n, frames, hop, window, shift):
    """float64 |fft(w x_f)|^2, shape (frames, n), in the plan's bin order."""
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n)[None, :]
    p = np.abs(np.fft.fft(x[idx].astype(np.complex128) * window_of(window, n), axis=-1)) ** 2
    return np.fft.fftshift(p, axes=-1) if shift else p


def ref_reduced(p, groups, k, detector):
    g = p[: groups * k].reshape(groups, k, -1)
    return {"mean": g.mean(axis=1), "max": g.max(axis=1), "min": g.min(axis=1)}[detector]


def check_amplitude(got, out_form, p, groups, k, detector, what):
    r = ref_reduced(p, groups, k, detector)
    s_g = np.sqrt(p[: groups * k].reshape(groups, -1).max(axis=1))
    if out_form == "db":
        a_got, a_ref = mag_from_db(got), np.sqrt(r) + EPS
    else:
        a_got, a_ref = np.sqrt(got.astype(np.float64)), np.sqrt(r)
    err = np.abs(a_got - a_ref).max(axis=1) / s_g
    print(f"{what}: amplitude error {err.max():.2e} of S_g")
    assert np.all(err <= REL_TOL), (what, float(err.max()))


def fold32(x, h, n, taps, frames, hop):
    """numpy's float32 fold, on float32 pairs (complex-times-real in numpy has zero-sign quirks): complex64 (frames, n)."""
    xr = x.view(np.float32).reshape(-1, 2)
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n)[None, :]
    acc = xr[idx] * h[:n][None, :, None]
    for t in range(1, taps):
        acc = acc + xr[idx + t * n] * h[t * n:(t + 1) * n][None, :, None]
    assert acc.dtype == np.float32
    return np.ascontiguousarray(acc).view(np.complex64)[..., 0]


def ref64(x, h, n, taps, frames, hop, shift):
    """float64 fold and FFT of the same complex64 samples: complex128 (frames, n) in the plan's bin order."""
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n)[None, :]
    xd, hd = x.astype(np.complex128), h.astype(np.float64)
    y = np.zeros((frames, n), dtype=np.complex128)
    for t in range(taps):
        y += xd[idx + t * n] * hd[t * n:(t + 1) * n][None, :]
    Y = np.fft.fft(y, axis=-1)
    return np.fft.fftshift(Y, axes=-1) if shift else Y


# ---- measuring and child processes -------------------------------------------------------------------------------------
def held_during(call, warm):
    """(call()'s result, the device memory it left held), after warm() has run."""
    free0, free1, total = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    warm()                                                  # (first call: the runtime's own allocations)
    _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free0), ctypes.byref(total)))
    res = call()
    _ffi.check(_ffi.lib().sdrk_dev_mem_info(0, ctypes.byref(free1), ctypes.byref(total)))
    return res, int(free0.value) - int(free1.value)


def run_child(code, marker, **env):
    """Run `code` in a fresh interpreter at the repository root; it must exit 0 and print `marker`."""
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=REPO, **env))
    assert r.returncode == 0 and marker in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])

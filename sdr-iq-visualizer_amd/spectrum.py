"""numpy-in / numpy-out spectrum functions backed by the gfx950 kernels.

This module is the host-side mirror of the reference's hot path.  The reference
has no function boundary there — it is three inline expressions in the SDR
reader thread — so the functions below *are* the boundary a maintainer would
call from those lines:

    app/sdr/streamer.py:119  fft_data = np.fft.fftshift(np.fft.fft(samples))
    app/sdr/streamer.py:120  freqs = np.fft.fftshift(np.fft.fftfreq(len(samples), 1/self.sample_rate)) + self.center_freq
    app/sdr/streamer.py:121  power_db = 20 * np.log10(np.abs(fft_data) + 1e-12)
    app/sdr/streamer.py:123-130  plot_data = {...}

Defaults reproduce the reference exactly: rectangular window, un-normalised
forward DFT, fftshift, additive floor 1e-12 on |X|.  Contract: complex64 in,
float32 out by default (complex128 input is down-cast; the reference would then
compute in float64 — documented difference, well inside the 1e-5 parity bar).

``precision="double"`` (a plan option and a keyword of the module functions) is
the reference's own arithmetic: complex128 in, float64 ``power_db`` out (complex128
from ``fft_c128``), powers of two 2 ... 2^22, on the float64 kernels of
csrc/fft_f64.hip.  ``precision="auto"`` picks by the input's dtype as numpy's FFT
does — complex64 / float32 / float16 single, everything else (complex128, float64,
integers) double — so the reference's complex128 samples get float64 rows.

``*_ci16`` (plan methods and module functions) take what the radio produces before pyadi-iio widens it, and what SigMF
calls ``ci16_le``: a C-contiguous int16 array whose last axis holds (I, Q).  ``x = float32(I) + 1j*float32(Q)`` exactly, then
the float32 path — the result has the same bits as the complex64 call on the widened samples, from half the input bytes.
No scale is applied (fold 1/32768 into a custom window, or add a constant to the dB rows).

``*_ci8`` take the 8-bit pairs of SigMF ``ci8`` (int8: ``x = I + 1j*Q``) and ``cu8`` (uint8: ``x = (I - 127.5) + 1j*(Q - 127.5)``)
the same way — the array's dtype is the format — for per-frame rows / spectra, integrated spectra, the polyphase filter bank
(``pfb_*_ci8``) and spectral kurtosis (``spectral_kurtosis_ci8``, ``pfb_spectral_kurtosis_ci8``): the bits of the complex64
call on ``iq8_to_c64(iq)``, from a quarter of the input bytes.

``rspectrum_db`` / ``rfft`` / ``rfreq_axis`` (and ``SpectrumPlan.set_real_window`` / ``rspectrum_db`` / ``rfft`` / ``rstft_db`` /
``exec_device_real``; integrated over k frames: ``rintegrated_db`` / ``rwelch_psd``, ``SpectrumPlan.rintegrate`` /
``exec_device_real_integrated``) take REAL sample streams — float32, int16, int8 or uint8 (``v - 127.5``), SigMF ``rf32_le`` / ``ri16_le`` /
``ri8`` / ``ru8``; the dtype is the format, float64 is refused — in frames of ``2*nfft`` samples and return one-sided rows of
``nfft + 1`` bins from 0 to fs/2 (``np.fft.rfft``'s order, never shifted), from a transform of half the frame length.

``pfb_*`` (``SpectrumPlan.set_pfb`` / ``pfb_db`` / ``pfb_fft`` / ``pfb_integrate`` and the module functions ``pfb_db`` and
``pfb_integrated_db``) put a polyphase filter bank front end before the transform: a prototype filter of ``T*nfft`` float32 coefficients (``pfb_prototype``: a windowed
sinc) weights ``T*nfft`` consecutive samples, the ``T`` blocks are summed into ``nfft`` samples (float32, products and sums
rounded one by one as numpy does on float32 arrays) and that frame is transformed, so that the bins are nearly rectangular
channels instead of a window's main lobe and side lobes.  float32 plans with the rectangular window only.

``spectral_kurtosis*`` (plan methods and module functions) return, per group of ``k`` frames, the mean power AND the spectral
kurtosis estimator ``SK = (k+1)/(k-1) * (k*S2/S1^2 - 1)`` of Nita & Gary from the sums ``S1`` of the power and ``S2`` of its
square, both accumulated inside the transform: 1 for Gaussian noise at any level, towards 0 on a carrier, well above 1 on
pulsed interference (``sk_limits`` gives the usual thresholds).  ``detector="sk"`` is not a detector: the calls are their own.

All arithmetic on samples happens on the GPU through ``libsdrk.so``; nothing in
this module computes a spectrum with numpy, and every entry point raises if the
library or a device is missing.
"""
from __future__ import annotations

import hashlib
import threading
import time
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _ffi
from ._ffi import byref, c_float, c_int, c_size_t, c_void_p, check, lib

WindowArg = Union[None, str, np.ndarray, Sequence[float]]


PRECISIONS = ("single", "double")


def resolve_precision(precision: str, samples=None) -> str:
    """``"single"`` / ``"double"`` as given; ``"auto"``: what numpy's FFT computes in for the input's dtype (complex64 for
    complex64, float32 and float16 input; complex128 for everything else, integers included)."""
    if precision in PRECISIONS:
        return precision
    if precision != "auto":
        raise ValueError(f"precision must be 'single', 'double' or 'auto', got {precision!r}")
    dt = np.asarray(samples).dtype if not hasattr(samples, "dtype") else np.dtype(samples.dtype)
    single = dt == np.complex64 or (dt.kind == "f" and dt.itemsize <= 4)
    return "single" if single else "double"


def _check_double_nfft(nfft: int) -> None:
    """float64 plans: powers of two 2 ... 2^22 (no chirp-z in double), checked before any device call."""
    if nfft < 2 or nfft > (1 << _ffi.MAX_LOG2_NFFT) or nfft & (nfft - 1):
        raise ValueError(f"nfft={nfft}: precision='double' supports powers of two 2..2^{_ffi.MAX_LOG2_NFFT} only")


def _window_spec(window: WindowArg, nfft: int, dtype=np.float32):
    """-> (kind, array of `dtype` or None, cache key)."""
    if window is None:
        return _ffi.WINDOW_RECT, None, "rect"
    if isinstance(window, str):
        name = window.lower()
        if name in ("rect", "rectangular", "boxcar", "none"):
            return _ffi.WINDOW_RECT, None, "rect"
        if name in ("hann", "hanning"):
            return _ffi.WINDOW_HANN, None, "hann"
        raise ValueError(f"unknown window {window!r} (use None, 'hann' or an array of nfft floats)")
    w = np.ascontiguousarray(np.asarray(window, dtype=dtype))
    if w.ndim != 1 or w.shape[0] != nfft:
        raise ValueError(f"window must have shape ({nfft},), got {w.shape}")
    return _ffi.WINDOW_CUSTOM, w, ("custom" if w.dtype == np.float32 else "custom64", w.tobytes())


def _as_c64(a) -> np.ndarray:
    """complex64, C-contiguous view or copy of `a` (down-casts complex128)."""
    arr = np.asarray(a)
    if arr.dtype != np.complex64:
        arr = arr.astype(np.complex64)
    return np.ascontiguousarray(arr)


def _as_c128(a) -> np.ndarray:
    """complex128, C-contiguous view or copy of `a`."""
    arr = np.asarray(a)
    if arr.dtype != np.complex128:
        arr = arr.astype(np.complex128)
    return np.ascontiguousarray(arr)


def _as_ci16(a, nfft: Optional[int] = None, stream: bool = False) -> np.ndarray:
    """Check an int16 I,Q array (no copy, no conversion): C-contiguous int16, last axis of length 2; ``(nfft, 2)`` or
    ``(B, nfft, 2)`` for frames, ``(n_samples, 2)`` for a stream.  Anything else is a ValueError, before any device call."""
    if not isinstance(a, np.ndarray) or a.dtype != np.int16:
        raise ValueError(f"ci16 input must be a numpy int16 array of (I, Q) pairs, got "
                         f"{getattr(a, 'dtype', type(a).__name__)}")
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError(f"ci16 input must have a last axis of length 2 (I, Q), got shape {a.shape}")
    if not a.flags.c_contiguous:
        raise ValueError("ci16 input must be C-contiguous (interleaved I, Q)")
    if stream:
        if a.ndim != 2:
            raise ValueError(f"ci16 stream must have shape (n_samples, 2), got {a.shape}")
    elif a.ndim > 3 or (nfft is not None and a.shape[-2] != nfft):
        want = "(N, 2) or (B, N, 2)" if nfft is None else f"({nfft}, 2) or (B, {nfft}, 2)"
        raise ValueError(f"ci16 frames must have shape {want}, got {a.shape}")
    return a


IQ8_SIGNED, IQ8_UNSIGNED = 0, 1      # SDRK_IQ8_SIGNED / SDRK_IQ8_UNSIGNED (include/sdrk.h)


def _as_ci8(a, nfft: Optional[int] = None, stream: bool = False) -> np.ndarray:
    """Check an 8-bit I,Q array (no copy, no conversion): C-contiguous int8 (SigMF ci8, signed) or uint8 (cu8, unsigned),
    last axis of length 2; shapes as ``_as_ci16``.  The dtype is the format.  Anything else is a ValueError, before any
    device call."""
    if not isinstance(a, np.ndarray) or a.dtype not in (np.int8, np.uint8):
        raise ValueError(f"8-bit I,Q input must be a numpy int8 (ci8) or uint8 (cu8) array of (I, Q) pairs, got "
                         f"{getattr(a, 'dtype', type(a).__name__)}")
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError(f"8-bit I,Q input must have a last axis of length 2 (I, Q), got shape {a.shape}")
    if not a.flags.c_contiguous:
        raise ValueError("8-bit I,Q input must be C-contiguous (interleaved I, Q)")
    if stream:
        if a.ndim != 2:
            raise ValueError(f"8-bit I,Q stream must have shape (n_samples, 2), got {a.shape}")
    elif a.ndim > 3 or (nfft is not None and a.shape[-2] != nfft):
        want = "(N, 2) or (B, N, 2)" if nfft is None else f"({nfft}, 2) or (B, {nfft}, 2)"
        raise ValueError(f"8-bit I,Q frames must have shape {want}, got {a.shape}")
    return a


_REAL_FORMATS = {np.dtype(np.float32): _ffi.REAL_F32, np.dtype(np.int16): _ffi.REAL_S16, np.dtype(np.int8): _ffi.REAL_S8,
                 np.dtype(np.uint8): _ffi.REAL_U8}
REAL_FORMAT_NAMES = {"f32": _ffi.REAL_F32, "s16": _ffi.REAL_S16, "s8": _ffi.REAL_S8, "u8": _ffi.REAL_U8}


def _as_real(a, frame_len: int, stream: bool = False) -> np.ndarray:
    """Check a real-sampled array (no copy, no conversion): C-contiguous float32, int16, int8 or uint8 — the dtype is the
    format (SigMF rf32_le / ri16_le / ri8 / ru8); ``(frames, frame_len)`` or a flat stream.  float64 is refused, not
    narrowed.  Anything else is a ValueError, before any device call."""
    if not isinstance(a, np.ndarray) or a.dtype not in _REAL_FORMATS:
        raise ValueError(f"real-sampled input must be a numpy float32, int16, int8 or uint8 array, got "
                         f"{getattr(a, 'dtype', type(a).__name__)}")
    if not a.flags.c_contiguous:
        raise ValueError("real-sampled input must be C-contiguous")
    if stream:
        if a.ndim != 1:
            raise ValueError(f"a real-sampled stream must have shape (n_samples,), got {a.shape}")
    elif a.ndim == 1:
        if a.shape[0] == 0 or a.shape[0] % frame_len:
            raise ValueError(f"a flat real-sampled array must hold whole frames of {frame_len} samples, got {a.shape[0]}")
    elif a.ndim != 2 or a.shape[1] != frame_len:
        raise ValueError(f"real-sampled frames must have shape (frames, {frame_len}) or be flat, got {a.shape}")
    return a


def _real_format(a: np.ndarray) -> int:
    """The C format code (SDRK_REAL_*) of a checked real-sampled array."""
    return _REAL_FORMATS[a.dtype]


def _real_window(window: WindowArg, frame_len: int) -> Optional[np.ndarray]:
    """The real window of ``frame_len`` float32 coefficients a ``WindowArg`` names, None for rectangular."""
    kind, w, _ = _window_spec(window, frame_len)
    if kind == _ffi.WINDOW_HANN:
        return np.hanning(frame_len).astype(np.float32)
    return w


def _real_hop(hop: Optional[int], frame_len: int) -> int:
    """The hop of an integrated real-input call in real samples: even and positive, by default the frame length."""
    hop = int(frame_len) if hop is None else int(hop)
    if hop < 2 or hop % 2:
        raise ValueError(f"hop must be a positive even number of real samples, got {hop}")
    return hop


def _iq8_format(a: np.ndarray) -> int:
    """The C format code of a checked 8-bit array: int8 is signed, uint8 unsigned."""
    return IQ8_SIGNED if a.dtype == np.int8 else IQ8_UNSIGNED


def iq8_to_c64(a) -> np.ndarray:
    """What the 8-bit entry points compute on, as complex64: ``I + 1j*Q`` for int8 pairs, ``(I - 127.5) + 1j*(Q - 127.5)`` for
    uint8 pairs (127.5: the mid-scale of 0...255); exact in float32."""
    x = _as_ci8(np.ascontiguousarray(a))
    f = x.astype(np.float32) - (np.float32(0.0) if x.dtype == np.int8 else np.float32(127.5))
    return np.ascontiguousarray(f).view(np.complex64)[..., 0]


def _as_iq2_c64(iq2) -> np.ndarray:
    """Two-channel complex64 elements ``(n, 2)``, C-contiguous (a view where ``iq2`` already is that).  A pair ``(a, b)`` of
    equal-length 1-D arrays is stacked into one: that is a copy of both."""
    if isinstance(iq2, (tuple, list)) and len(iq2) == 2:
        a, b = (np.asarray(c) for c in iq2)
        if a.ndim != 1 or a.shape != b.shape:
            raise ValueError(f"a channel pair must be two 1-D arrays of equal length, got shapes {a.shape} and {b.shape}")
        return np.stack([a.astype(np.complex64, copy=False), b.astype(np.complex64, copy=False)], axis=1)
    x = np.asarray(iq2)
    if x.ndim != 2 or x.shape[1] != 2 or not np.issubdtype(x.dtype, np.complexfloating):
        raise ValueError(f"two-channel input must be a complex (n, 2) array or a pair (a, b), got shape {x.shape} {x.dtype}")
    return _as_c64(x)


def _as_iq2_ci16(iq2) -> np.ndarray:
    """Two-channel int16 elements ``(n, 2, 2)`` (channel, then I,Q) or ``(n, 4)``: checked, never converted.  A pair
    ``(a, b)`` of ``(n, 2)`` int16 arrays of equal length is stacked into one: that is a copy of both."""
    if isinstance(iq2, (tuple, list)) and len(iq2) == 2:
        a, b = (np.asarray(c) for c in iq2)
        if a.dtype != np.int16 or b.dtype != np.int16 or a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
            raise ValueError(f"a channel pair must be two (n, 2) int16 arrays of equal length, got {a.shape} {a.dtype} and "
                             f"{b.shape} {b.dtype}")
        return np.stack([a, b], axis=1)
    if not isinstance(iq2, np.ndarray) or iq2.dtype != np.int16:
        raise ValueError(f"two-channel ci16 input must be a numpy int16 array, got {getattr(iq2, 'dtype', type(iq2).__name__)}")
    if not ((iq2.ndim == 3 and iq2.shape[1:] == (2, 2)) or (iq2.ndim == 2 and iq2.shape[1] == 4)):
        raise ValueError(f"two-channel ci16 input must have shape (n, 2, 2) or (n, 4) (I0 Q0 I1 Q1), got {iq2.shape}")
    if not iq2.flags.c_contiguous:
        raise ValueError("two-channel ci16 input must be C-contiguous (interleaved I0 Q0 I1 Q1)")
    return iq2


class CrossSpectrum(NamedTuple):
    """What ``SpectrumPlan.cross_spectrum`` returns: four ``(groups, nfft)`` float32 views of one array, per group of ``k``
    frames and bin ``scale/k`` times the sums of ``|A|^2``, ``|B|^2``, ``Re(A conj B)`` and ``Im(A conj B)``."""
    paa: np.ndarray
    pbb: np.ndarray
    cre: np.ndarray
    cim: np.ndarray

    @property
    def cross(self) -> np.ndarray:
        """The averaged cross-spectrum ``<A conj(B)>`` as complex64 (a new array)."""
        c = np.empty(self.cre.shape, dtype=np.complex64)
        c.real, c.imag = self.cre, self.cim
        return c

    @property
    def coherence(self) -> np.ndarray:
        """Magnitude-squared coherence ``|C|^2 / (Paa * Pbb)`` in float64: 1 where the channels carry one signal, about
        ``1/k`` on independent noise.  0 where the denominator is 0 (a dead bin), never NaN."""
        cre, cim = self.cre.astype(np.float64), self.cim.astype(np.float64)
        den = self.paa.astype(np.float64) * self.pbb.astype(np.float64)
        ok = np.isfinite(den) & (den > 0)
        coh = np.zeros(den.shape, dtype=np.float64)
        np.divide(cre * cre + cim * cim, den, out=coh, where=ok)
        return np.where(np.isfinite(coh), coh, 0.0)

    @property
    def phase(self) -> np.ndarray:
        """The phase of the cross-spectrum in radians, ``atan2(cim, cre)`` in float64: channel 0's phase minus channel 1's."""
        return np.arctan2(self.cim.astype(np.float64), self.cre.astype(np.float64))


CORRMAT_MIN_CHANNELS, CORRMAT_MAX_CHANNELS = 2, 8      # sdrk.h: channels of a correlation-matrix call


def _corrmat_channels(c: int) -> int:
    if not CORRMAT_MIN_CHANNELS <= int(c) <= CORRMAT_MAX_CHANNELS:
        raise ValueError(f"a correlation matrix takes {CORRMAT_MIN_CHANNELS}..{CORRMAT_MAX_CHANNELS} channels, got {int(c)}")
    return int(c)


def _as_iqc_c64(iq) -> np.ndarray:
    """C-channel complex64 elements ``(n, C)``, C-contiguous (a view where ``iq`` already is that), C in 2..8."""
    x = np.asarray(iq)
    if x.ndim != 2 or not np.issubdtype(x.dtype, np.complexfloating):
        raise ValueError(f"multi-channel input must be a complex (n, C) array, got shape {x.shape} {x.dtype}")
    _corrmat_channels(x.shape[1])
    return _as_c64(x)


def _as_iqc_int(iq, dtypes, name: str) -> np.ndarray:
    """C-channel integer elements ``(n, C, 2)`` (channel, then I,Q) of one of ``dtypes``: checked, never converted."""
    if not isinstance(iq, np.ndarray) or iq.dtype not in dtypes:
        raise ValueError(f"multi-channel {name} input must be a numpy {' or '.join(np.dtype(d).name for d in dtypes)} array, got "
                         f"{getattr(iq, 'dtype', type(iq).__name__)}")
    if iq.ndim != 3 or iq.shape[2] != 2:
        raise ValueError(f"multi-channel {name} input must have shape (n, C, 2) (channel, then I, Q), got {iq.shape}")
    _corrmat_channels(iq.shape[1])
    if not iq.flags.c_contiguous:
        raise ValueError(f"multi-channel {name} input must be C-contiguous (I0 Q0 I1 Q1 ... per element)")
    return iq


def plane_index(channels: int, i: int, j: int) -> int:
    """Where a correlation matrix of ``channels`` channels keeps ``(i, j)`` among its ``channels**2`` planes: the auto power
    of channel ``i`` for ``i == j``, else the REAL plane of the pair ``(min, max)`` — its imaginary plane is the next one.
    The autos come first, then the pairs (0,1), (0,2), ..., (0,C-1), (1,2), ..., (C-2,C-1), two planes each."""
    c = _corrmat_channels(channels)
    i, j = int(i), int(j)
    if not (0 <= i < c and 0 <= j < c):
        raise ValueError(f"channels ({i}, {j}) are not both in 0..{c - 1}")
    if i == j:
        return i
    a, b = min(i, j), max(i, j)
    return c + 2 * (a * c - a * (a + 1) // 2 + (b - a - 1))


class CorrelationMatrix:
    """What ``SpectrumPlan.correlate`` returns: one ``(groups, C*C, nfft)`` float32 array, per group of ``k`` frames and bin
    ``scale/k`` times the sums of ``|X_c|^2`` (planes ``0..C-1``) and of ``Re`` and ``Im`` of ``X_i conj(X_j)`` for the pairs
    ``i < j`` (``plane_index``).  The members derive the rest; direction-finding estimators are numpy on ``matrix()``."""

    def __init__(self, planes: np.ndarray, channels: int):
        c = _corrmat_channels(channels)
        planes = np.asarray(planes)
        if planes.ndim != 3 or planes.shape[1] != c * c:
            raise ValueError(f"{c} channels take planes of shape (groups, {c * c}, nfft), got {planes.shape}")
        self.planes = planes
        self.channels = c

    def auto(self, c: int) -> np.ndarray:
        """The averaged power ``<|X_c|^2>`` of channel ``c``: a ``(groups, nfft)`` float32 view."""
        return self.planes[:, plane_index(self.channels, c, c)]

    def cross(self, i: int, j: int) -> np.ndarray:
        """The averaged cross-spectrum ``<X_i conj(X_j)>`` as complex64 (a new array): the conjugate of ``cross(j, i)`` for
        ``i > j``, the auto power for ``i == j``."""
        q = plane_index(self.channels, i, j)
        z = np.empty(self.planes[:, q].shape, dtype=np.complex64)
        if i == j:
            z.real, z.imag = self.planes[:, q], 0.0
        else:
            z.real = self.planes[:, q]
            z.imag = self.planes[:, q + 1] if i < j else -self.planes[:, q + 1]
        return z

    def matrix(self) -> np.ndarray:
        """The Hermitian matrix per group and bin: ``(groups, nfft, C, C)`` complex64 (a new array)."""
        c = self.channels
        m = np.empty((self.planes.shape[0], self.planes.shape[2], c, c), dtype=np.complex64)
        for i in range(c):
            for j in range(c):
                m[:, :, i, j] = self.cross(i, j)
        return m

    def coherence(self, i: int, j: int) -> np.ndarray:
        """Magnitude-squared coherence ``|R_ij|^2 / (R_ii R_jj)`` in float64: 1 where the two channels carry one signal, about
        ``1/k`` on independent noise.  0 where the denominator is 0 (a dead bin), never NaN."""
        z = self.cross(i, j).astype(np.complex128)
        den = self.auto(i).astype(np.float64) * self.auto(j).astype(np.float64)
        ok = np.isfinite(den) & (den > 0)
        coh = np.zeros(den.shape, dtype=np.float64)
        np.divide(z.real * z.real + z.imag * z.imag, den, out=coh, where=ok)
        return np.where(np.isfinite(coh), coh, 0.0)

    def phase(self, i: int, j: int) -> np.ndarray:
        """The phase of ``<X_i conj(X_j)>`` in radians in float64: channel ``i``'s phase minus channel ``j``'s."""
        z = self.cross(i, j)
        return np.arctan2(z.imag.astype(np.float64), z.real.astype(np.float64))


PFB_MAX_TAPS = 32                 # sdrk.h: taps of a prototype filter


def pfb_prototype(nfft: int, taps: int, window: WindowArg = "hann") -> np.ndarray:
    """The default prototype filter of a polyphase filter bank with ``nfft`` channels and ``taps`` blocks: float32
    ``sinc((m - (T*N - 1)/2) / N) * window(T*N)[m]`` for ``m < T*N``, computed in float64 and rounded once.  ``window``:
    ``"hann"`` (``numpy.hanning``), ``"hamming"``, ``"blackman"``, ``None`` / ``"rect"``, or ``T*N`` coefficients."""
    nfft, taps = int(nfft), int(taps)
    if nfft < 2:
        raise ValueError(f"nfft must be >= 2, got {nfft}")
    if not 1 <= taps <= PFB_MAX_TAPS:
        raise ValueError(f"taps must be in 1..{PFB_MAX_TAPS}, got {taps}")
    n = taps * nfft
    if window is None or (isinstance(window, str) and window.lower() in ("rect", "rectangular", "boxcar", "none")):
        w = np.ones(n, dtype=np.float64)
    elif isinstance(window, str):
        makers = {"hann": np.hanning, "hanning": np.hanning, "hamming": np.hamming, "blackman": np.blackman}
        if window.lower() not in makers:
            raise ValueError(f"unknown window {window!r} (use 'hann', 'hamming', 'blackman', None or an array of taps*nfft floats)")
        w = makers[window.lower()](n)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f"window must have shape ({n},), got {w.shape}")
    m = np.arange(n, dtype=np.float64)
    return (np.sinc((m - (n - 1) / 2.0) / nfft) * w).astype(np.float32)


FIR_MAX_TAPS = 2049               # sdrk.h: taps of a FIR filter (overlap-save in blocks of 4096)
FIR_MAX_DECIM = 256
FIR_BLOCK = 4096
FIR_BANK_MAX_CHANNELS = 64        # sdrk.h: channels of one channel-bank call
BEAM_MAX_CHANNELS = 8             # sdrk.h: coherent channels of one beamformer call


def channel_taps(decim: int, ntaps: Optional[int] = None, window: WindowArg = "hann") -> np.ndarray:
    """The default low-pass of a channel extraction that decimates by ``decim``: complex64 windowed sinc with cutoff
    ``0.4/decim`` cycles per sample and unit DC gain, ``sinc(0.8 (t - (M - 1)/2) / decim) * window(M + 2)[t + 1]`` normalised to sum 1,
    computed in float64 and rounded once.  ``ntaps`` defaults to ``min(16*decim + 1, 2049)``.  ``window``: ``"hann"``
    (``numpy.hanning``), ``"hamming"``, ``"blackman"``, ``None`` / ``"rect"``, or ``ntaps`` coefficients.
    With the default length the stopband from ``0.6/decim`` on lies below -55 dB under Hann and below -75 dB under Blackman
    for ``decim`` up to 128; at ``decim = 256`` the 2049-tap limit leaves -43 dB (Hann)."""
    decim = int(decim)
    if decim < 1 or decim > FIR_MAX_DECIM or decim & (decim - 1):
        raise ValueError(f"decim must be a power of two in 1..{FIR_MAX_DECIM}, got {decim}")
    return _lowpass_taps(decim, ntaps, window)


def ddc_taps(decim: int, ntaps: Optional[int] = None, window: WindowArg = "hann") -> np.ndarray:
    """``channel_taps`` for the digital down-converter: the same low-pass (cutoff ``0.4/decim``, unit DC gain, default length
    ``min(16*decim + 1, 2049)``) for ANY integer ``decim`` in 1..256; for a power of two it is ``channel_taps(decim, ...)``."""
    return _lowpass_taps(_ddc_decim(decim), ntaps, window)


def _lowpass_taps(decim: int, ntaps: Optional[int], window: WindowArg) -> np.ndarray:
    m = min(16 * decim + 1, FIR_MAX_TAPS) if ntaps is None else int(ntaps)
    if not 1 <= m <= FIR_MAX_TAPS:
        raise ValueError(f"ntaps must be in 1..{FIR_MAX_TAPS}, got {m}")
    if window is None or (isinstance(window, str) and window.lower() in ("rect", "rectangular", "boxcar", "none")):
        w = np.ones(m, dtype=np.float64)
    elif isinstance(window, str):
        makers = {"hann": np.hanning, "hanning": np.hanning, "hamming": np.hamming, "blackman": np.blackman}
        if window.lower() not in makers:
            raise ValueError(f"unknown window {window!r} (use 'hann', 'hamming', 'blackman', None or an array of ntaps floats)")
        w = makers[window.lower()](m + 2)[1:-1]              # (without the two zero end points: every tap works)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.shape != (m,):
            raise ValueError(f"window must have shape ({m},), got {w.shape}")
    t = np.arange(m, dtype=np.float64) - (m - 1) / 2.0
    h = np.sinc(0.8 * t / decim) * w
    return (h / h.sum()).astype(np.complex64)


def _fir_args(decim, shift_bins):
    decim, shift_bins = int(decim), int(shift_bins)
    if decim < 1 or decim > FIR_MAX_DECIM or decim & (decim - 1):
        raise ValueError(f"decim must be a power of two in 1..{FIR_MAX_DECIM}, got {decim}")
    if not -FIR_BLOCK // 2 <= shift_bins < FIR_BLOCK // 2:
        raise ValueError(f"shift_bins must be in {-FIR_BLOCK // 2}..{FIR_BLOCK // 2 - 1}, got {shift_bins}")
    return decim, shift_bins


def _bank_shifts(shift_bins):
    """The tuning offsets of a channel-bank call as a ctypes int array: 1..64 of them, each a whole bin in -2048..2047."""
    shifts = [int(v) for v in np.asarray(shift_bins).reshape(-1)]
    if not 1 <= len(shifts) <= FIR_BANK_MAX_CHANNELS:
        raise ValueError(f"a channel bank takes 1..{FIR_BANK_MAX_CHANNELS} shift_bins, got {len(shifts)}")
    for v in shifts:
        _fir_args(1, v)
    return (c_int * len(shifts))(*shifts)


def _ddc_decim(decim) -> int:
    decim = int(decim)
    if decim < 1 or decim > FIR_MAX_DECIM:
        raise ValueError(f"decim must be in 1..{FIR_MAX_DECIM}, got {decim}")
    return decim


def _ddc_word(word) -> int:
    """A frequency word as the C call takes it: any int, taken mod 2^32 (so -1 is the word just below zero)."""
    return int(word) & 0xFFFFFFFF


def _ddc_words(freq_words):
    """The frequency words of a DDC bank call as a ctypes uint32 array: 1..64 of them."""
    words = [_ddc_word(v) for v in np.asarray(freq_words, dtype=object).reshape(-1)]
    if not 1 <= len(words) <= FIR_BANK_MAX_CHANNELS:
        raise ValueError(f"a DDC bank takes 1..{FIR_BANK_MAX_CHANNELS} frequency words, got {len(words)}")
    return (_ffi.c_uint32 * len(words))(*words)


def freq_word(offset_hz: float, sample_rate: float) -> int:
    """The 32-bit frequency word of the digital down-converter nearest to ``offset_hz`` at ``sample_rate``:
    ``round(offset_hz / sample_rate * 2^32) mod 2^32`` (steps of ``sample_rate / 2^32``); offsets beyond half the sample rate
    wrap around, as the frequencies of a sampled signal do."""
    fs = float(sample_rate)
    if not fs > 0:
        raise ValueError("sample_rate must be positive")
    from fractions import Fraction
    return int(round(Fraction(float(offset_hz)) / Fraction(fs) * (1 << 32))) & 0xFFFFFFFF


def freq_word_hz(word: int, sample_rate: float) -> float:
    """The frequency a word tunes to: ``int32(word) / 2^32 * sample_rate``, in -sample_rate/2 .. sample_rate/2."""
    w = _ddc_word(word)
    return (w - (1 << 32) if w >= 1 << 31 else w) / float(1 << 32) * float(sample_rate)



class _Mode(NamedTuple):
    """One corner of sample format x front end, and the C entry points that serve it (include/sdrk.h)."""
    ci16: bool                  # int16 I,Q pairs in (else complex64)
    pfb: bool                   # frames folded from taps * nfft samples by the plan's polyphase filter bank
    host_db: str                # per frame: host arrays, dB rows
    host_fft: str               # ... complex spectra
    device: str                 # ... device pointers
    timed_each: str             # ... timed launches
    int_host: str               # one row per k frames: host arrays
    int_device: str             # ... device pointers
    int_timed_each: str         # ... timed launches
    sk_host: str                # mean power and spectral kurtosis per k frames: host arrays
    sk_device: str              # ... device pointers
    sk_timed_each: str          # ... timed launches
    iq8: bool = False           # 8-bit I,Q pairs in: the entry points take the format right after the input pointer

    def stream(self, iq) -> np.ndarray:
        """One contiguous stream as the entry points read it: ``(n,)`` complex64, or checked ``(n, 2)`` int16 / int8 / uint8."""
        if self.iq8:
            return _as_ci8(iq, stream=True)
        return _as_ci16(iq, stream=True) if self.ci16 else _as_c64(iq).reshape(-1)

    def entry(self, name: str, fmt: Optional[int] = None):
        """The C entry point ``name``; of an 8-bit mode, with the format ``fmt`` bound in behind the input pointer."""
        fn = getattr(lib(), name)
        if not self.iq8:
            return fn
        return lambda handle, iq, *rest: fn(handle, iq, c_int(int(fmt)), *rest)


class _Integ(NamedTuple):
    """What a call that returns one row per ``k`` frames adds to the per-frame one."""
    k: int
    detector: str
    out: str
    scale: float
    sk: bool = False            # the spectral-kurtosis call: two planes per group, k >= 2, no detector argument


_C64 = _Mode(False, False, "sdrk_exec_host", "sdrk_exec_fft_host", "sdrk_exec_device", "sdrk_exec_device_timed_each",
             "sdrk_exec_host_integrated", "sdrk_exec_device_integrated", "sdrk_exec_device_integrated_timed_each",
             "sdrk_exec_host_sk", "sdrk_exec_device_sk", "sdrk_exec_device_sk_timed_each")
_CI16 = _Mode(True, False, "sdrk_exec_host_ci16", "sdrk_exec_fft_host_ci16", "sdrk_exec_device_ci16",
              "sdrk_exec_device_ci16_timed_each", "sdrk_exec_host_integrated_ci16", "sdrk_exec_device_integrated_ci16",
              "sdrk_exec_device_integrated_ci16_timed_each",
              "sdrk_exec_host_sk_ci16", "sdrk_exec_device_sk_ci16", "sdrk_exec_device_sk_ci16_timed_each")
_CI8 = _Mode(False, False, "sdrk_exec_host_ci8", "sdrk_exec_fft_host_ci8", "sdrk_exec_device_ci8",
             "sdrk_exec_device_ci8_timed_each", "sdrk_exec_host_integrated_ci8", "sdrk_exec_device_integrated_ci8",
             "sdrk_exec_device_integrated_ci8_timed_each",
             "sdrk_exec_host_kurtosis_iq8", "sdrk_exec_device_kurtosis_iq8", "sdrk_exec_device_kurtosis_iq8_timed_each", iq8=True)
_PFB = _Mode(False, True, "sdrk_exec_host_pfb", "sdrk_exec_fft_host_pfb", "sdrk_exec_device_pfb",
             "sdrk_exec_device_pfb_timed_each", "sdrk_exec_host_pfb_integrated", "sdrk_exec_device_pfb_integrated",
             "sdrk_exec_device_pfb_integrated_timed_each",
             "sdrk_exec_host_pfb_sk", "sdrk_exec_device_pfb_sk", "sdrk_exec_device_pfb_sk_timed_each")
_PFB_CI16 = _Mode(True, True, "sdrk_exec_host_pfb_ci16", "sdrk_exec_fft_host_pfb_ci16", "sdrk_exec_device_pfb_ci16",
                  "sdrk_exec_device_pfb_ci16_timed_each", "sdrk_exec_host_pfb_integrated_ci16",
                  "sdrk_exec_device_pfb_integrated_ci16", "sdrk_exec_device_pfb_integrated_ci16_timed_each",
                  "sdrk_exec_host_pfb_sk_ci16", "sdrk_exec_device_pfb_sk_ci16", "sdrk_exec_device_pfb_sk_ci16_timed_each")
_PFB_CI8 = _Mode(False, True, "sdrk_exec_host_pfb_iq8", "sdrk_exec_fft_host_pfb_iq8", "sdrk_exec_device_pfb_iq8",
                 "sdrk_exec_device_pfb_iq8_timed_each", "sdrk_exec_host_pfb_integrated_iq8",
                 "sdrk_exec_device_pfb_integrated_iq8", "sdrk_exec_device_pfb_integrated_iq8_timed_each",
                 "sdrk_exec_host_pfb_kurtosis_iq8", "sdrk_exec_device_pfb_kurtosis_iq8",
                 "sdrk_exec_device_pfb_kurtosis_iq8_timed_each", iq8=True)


class SpectrumPlan:
    """A compiled plan for one (nfft, window, eps, shift, device, precision) combination.

    Thin owner of an ``sdrk_plan``; methods take and return numpy arrays.  A plan
    is used by one thread at a time (an internal lock enforces it); create one
    plan per device to drive several GPUs from several threads.

    ``precision="double"``: complex128 in, float64 rows (complex128 from ``fft``) out, powers of two only; Welch and the
    ``fused64k`` / ``overlap_passes`` / ``tune_staging`` options are float32-only.
    """

    def __init__(self, nfft: int, *, window: WindowArg = None, eps: float = 1e-12,
                 shift: bool = True, device: int = 0, max_batch: int = 1 << 30, fused64k: Optional[bool] = None,
                 overlap_passes: bool = False, tune_staging: bool = False, precision: str = "single"):
        nfft = int(nfft)
        if precision not in PRECISIONS:
            raise ValueError(f"plan precision must be 'single' or 'double', got {precision!r}")
        self.precision = precision
        self._double = precision == "double"
        if self._double:
            _check_double_nfft(nfft)
            if fused64k is not None or overlap_passes or tune_staging:
                raise ValueError("fused64k, overlap_passes and tune_staging are options of float32 plans only")
        pow2 = nfft >= 2 and not (nfft & (nfft - 1))
        if nfft < 2 or nfft > (1 << _ffi.MAX_LOG2_NFFT) or (not pow2 and nfft > (1 << (_ffi.MAX_LOG2_NFFT - 1))):
            raise ValueError(
                f"nfft={nfft}: frames must have 2..2^{_ffi.MAX_LOG2_NFFT} samples (powers of two) or "
                f"2..2^{_ffi.MAX_LOG2_NFFT - 1} (other lengths, via Bluestein)")
        kind, warr, self._wkey = _window_spec(window, nfft, np.float64 if self._double else np.float32)
        _ffi.require_device(device)
        self.nfft = nfft
        self.eps = float(eps)
        self.shift = bool(shift)
        self.device = int(device)
        self._lock = threading.Lock()
        self.pfb_taps = 0                              # taps of the prototype filter set by set_pfb() (0: none)
        self.fir_taps = 0                              # taps of the FIR filter set by set_fir() (0: none)
        self.beam_channels = 0                         # channels of the beam filters set by set_beam() (0: none)
        self.beam_taps = 0                             # ... and their taps per channel
        self.last_placement: Optional[dict] = None     # report of the last tune_scratch() on this plan
        self._handle = c_void_p()
        wptr = warr.ctypes.data_as(c_void_p) if warr is not None else None
        # fused64k (nfft = 65536 only): None = the library's default (the single persistent launch for calls
        # of 512 frames or more, the two tiled launches below that), True = the persistent launch for every call, False = never
        # (sdrk.h SDRK_PLAN_FUSED64K / SDRK_PLAN_TILED64K).  An explicit plan option, so the path is visible in the API.
        self.fused64k = None if fused64k is None else bool(fused64k)
        # overlap_passes: the two passes of a large frame on two streams (slower, kept for A/B)
        self.overlap_passes = bool(overlap_passes)
        # tune_staging: the numpy boundary's device staging placed at creation (sdrk.h SDRK_PLAN_TUNE_STAGING; measured:
        # no effect at the shipped chunk size)
        self.tune_staging = bool(tune_staging)
        if self._double:
            check(lib().sdrk_plan_create_f64(self.device, nfft, c_size_t(int(max_batch)), kind, wptr,
                                             _ffi.c_double(self.eps), int(self.shift), byref(self._handle)))
            return
        flags = ((_ffi.PLAN_FUSED64K if self.fused64k else 0) |
                 (_ffi.PLAN_TILED64K if self.fused64k is False and nfft == 65536 else 0) |
                 (_ffi.PLAN_OVERLAP_PASSES if self.overlap_passes else 0) |
                 (_ffi.PLAN_TUNE_STAGING if self.tune_staging else 0))
        check(lib().sdrk_plan_create_ex(self.device, nfft, c_size_t(int(max_batch)), kind, wptr,
                                        c_float(self.eps), int(self.shift), flags, byref(self._handle)))

    # -- lifetime ---------------------------------------------------------------
    def close(self) -> None:
        h, self._handle = self._handle, c_void_p()
        if h:
            lib().sdrk_plan_destroy(h)

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> c_void_p:
        if not self._handle:
            raise RuntimeError("plan is closed")
        return self._handle

    # -- host arrays ------------------------------------------------------------
    def _run_host(self, fn, iq: np.ndarray, n_frames: int, stride: int, out: np.ndarray) -> None:
        """One C call for the whole batch: libsdrk cuts it into pinned, pipelined chunks itself."""
        with self._lock:
            check(fn(self.handle, iq.ctypes.data_as(c_void_p), c_size_t(n_frames), c_size_t(stride),
                     out.ctypes.data_as(c_void_p)))

    def _float32_only(self, what: str) -> None:
        if self._double:
            raise ValueError(f"{what} is not available on a precision='double' plan")

    def _as_input(self, a) -> np.ndarray:
        return _as_c128(a) if self._double else _as_c64(a)

    def _frames(self, samples):
        x = self._as_input(samples)
        if x.ndim == 1:
            if x.shape[0] != self.nfft:
                raise ValueError(f"frame has {x.shape[0]} samples, plan nfft is {self.nfft}")
            return x.reshape(1, -1), True
        if x.ndim != 2 or x.shape[1] != self.nfft:
            raise ValueError(f"expected shape ({self.nfft},) or (B, {self.nfft}), got {x.shape}")
        return x, False

    @staticmethod
    def _out_array(out, shape, dtype) -> np.ndarray:
        """A caller-provided result array (reused across calls: no page faults on fresh memory, no munmap of
        the previous result — at 256 MiB those cost as much as the transfer) or a new one."""
        if out is None:
            return np.empty(shape, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {np.dtype(dtype).name} array of shape {tuple(shape)}")
        return out

    @property
    def _row_dtype(self):
        return np.float64 if self._double else np.float32

    def _exec_host_fn(self):
        return lib().sdrk_exec_host_f64 if self._double else lib().sdrk_exec_host

    def spectrum_db(self, samples, out: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 (float64 on a double plan) ``20*log10(|fftshift(fft(w*x))| + eps)`` for one frame or a batch; ``out``
        (same shape as ``samples``, of the row dtype) receives the rows in place when given."""
        x, one = self._frames(samples)
        res = self._out_array(out, x.shape[1:] if one else x.shape, self._row_dtype)
        if x.shape[0]:
            self._run_host(self._exec_host_fn(), x, x.shape[0], self.nfft, res)
        return res

    def fft(self, samples) -> np.ndarray:
        """complex64 (complex128 on a double plan) spectrum ``fft(w*x)`` (fftshifted if the plan shifts), no log."""
        x, one = self._frames(samples)
        out = np.empty(x.shape, dtype=np.complex128 if self._double else np.complex64)
        if x.shape[0]:
            self._run_host(lib().sdrk_exec_fft_host_f64 if self._double else lib().sdrk_exec_fft_host, x, x.shape[0],
                           self.nfft, out)
        return out[0] if one else out

    def stft_db(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Rows of a spectrogram over one contiguous stream: row r covers samples
        ``[r*hop, r*hop + nfft)``; ``rows = 1 + (len(iq) - nfft) // hop`` (0 if the
        stream is shorter than one frame).  Frames are cut on the device from the
        single uploaded stream; overlapped samples are not duplicated on the host."""
        x = self._as_input(iq).reshape(-1)
        hop = self.nfft if hop is None else int(hop)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        rows = 0 if x.shape[0] < self.nfft else 1 + (x.shape[0] - self.nfft) // hop
        out = self._out_array(out, (rows, self.nfft), self._row_dtype)
        if rows:
            self._run_host(self._exec_host_fn(), x, rows, hop, out)
        return out

    # -- the shared bodies of the modes of _Mode: each public method below is a call into one of these ------------------
    def _ready(self, m: _Mode, what: str, integrated: bool = False) -> int:
        """The readiness check of mode ``m`` -> the samples a frame spans: ``nfft``, or ``taps * nfft`` behind the filter
        bank.  ``what`` names the caller to the user of a double plan (the filter bank names itself)."""
        if not m.pfb:
            self._float32_only(what)
            return self.nfft
        span = self._pfb_ready()
        if integrated and self._wkey != "rect":
            raise ValueError("the polyphase filter bank needs a plan with the rectangular window: the prototype is the window")
        return span

    def _n_frames(self, span: int, n_samples: int, hop: Optional[int]) -> int:
        """Full frames of ``span`` samples, ``hop`` apart (default ``nfft``), in a stream of ``n_samples``."""
        hop = self.nfft if hop is None else int(hop)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        return 0 if int(n_samples) < span else 1 + (int(n_samples) - span) // hop

    def _n_groups(self, span: int, n_samples: int, k: int, hop: Optional[int], min_k: int = 1) -> int:
        """Whole groups of ``k`` among those frames."""
        if int(k) < min_k:
            raise ValueError(f"k must be >= {min_k}")
        return self._n_frames(span, n_samples, hop) // int(k)

    def _host_rows(self, m: _Mode, iq, hop: Optional[int], out: Optional[np.ndarray] = None, *, spectra: bool = False,
                   what: str = "") -> np.ndarray:
        """Per-frame rows over one contiguous stream: float32 dB rows (into ``out`` when given), or complex64 ``spectra``."""
        span = self._ready(m, what)
        x = m.stream(iq)
        rows = self._n_frames(span, x.shape[0], hop)
        shape = (rows, self.nfft)
        res = np.empty(shape, dtype=np.complex64) if spectra else self._out_array(out, shape, np.float32)
        if rows:
            fn = m.entry(m.host_fft if spectra else m.host_db, _iq8_format(x) if m.iq8 else None)
            self._run_host(fn, x, rows, self.nfft if hop is None else int(hop), res)
        return res

    def _host_integrated(self, m: _Mode, iq, hop: Optional[int], i: _Integ, *, what: str = "") -> np.ndarray:
        """One float32 row per ``i.k`` frames of one contiguous stream, ``(groups, nfft)``; the spectral-kurtosis call: two,
        ``(groups, 2, nfft)``."""
        span = self._ready(m, what, integrated=True)
        codes = self._int_codes(i.detector, i.out, i.sk)
        x = m.stream(iq)
        groups = self._n_groups(span, x.shape[0], i.k, hop, 2 if i.sk else 1)
        res = np.empty((groups, 2, self.nfft) if i.sk else (groups, self.nfft), dtype=np.float32)
        if groups:
            with self._lock:
                check(m.entry(m.sk_host if i.sk else m.int_host, _iq8_format(x) if m.iq8 else None)(
                    self.handle, x.ctypes.data_as(c_void_p), c_size_t(groups), c_size_t(int(i.k)),
                    c_size_t(self.nfft if hop is None else int(hop)), *codes, c_float(i.scale), res.ctypes.data_as(c_void_p)))
        return res

    def _device_args(self, m: _Mode, d_iq: int, n: int, d_out: int, frame_stride: Optional[int], i: Optional[_Integ],
                     what: str) -> list:
        """The C arguments of a device call of mode ``m`` between the plan and the stream (or the launch count), behind its
        checks; ``i``: the parameters of a call that returns one row per ``i.k`` frames."""
        self._ready(m, what, i is not None)
        stride = self.nfft if frame_stride is None else int(frame_stride)
        if i is None:
            return [c_void_p(d_iq), c_size_t(n), c_size_t(stride), c_void_p(d_out)]
        codes = self._int_codes(i.detector, i.out, i.sk)
        if int(i.k) < 1 or int(n) < 1:
            raise ValueError("k and n_groups must be >= 1")
        if i.sk and int(i.k) < 2:
            raise ValueError("k must be >= 2: the spectral-kurtosis estimator divides by k - 1")
        if stride < 1:
            raise ValueError("frame_stride must be >= 1")
        return [c_void_p(d_iq), c_size_t(n), c_size_t(int(i.k)), c_size_t(stride), *codes, c_float(i.scale), c_void_p(d_out)]

    def _exec_device(self, m: _Mode, d_iq: int, n: int, d_out: int, frame_stride: Optional[int], stream: int,
                     i: Optional[_Integ] = None, *, what: str = "", fmt: Optional[int] = None) -> None:
        args = self._device_args(m, d_iq, n, d_out, frame_stride, i, what)
        with self._lock:
            fn = m.device if i is None else (m.sk_device if i.sk else m.int_device)
            check(m.entry(fn, fmt)(self.handle, *args, c_void_p(stream) if stream else None))

    def _exec_device_timed_each(self, m: _Mode, d_iq: int, n: int, d_out: int, launches: int, frame_stride: Optional[int],
                                i: Optional[_Integ] = None, *, what: str = "", fmt: Optional[int] = None) -> list:
        args = self._device_args(m, d_iq, n, d_out, frame_stride, i, what)
        ms = (c_float * int(launches))()
        with self._lock:
            fn = m.timed_each if i is None else (m.sk_timed_each if i.sk else m.int_timed_each)
            check(m.entry(fn, fmt)(self.handle, *args, int(launches), ms))
        return [float(v) for v in ms]

    # -- int16 I,Q input (float32 plans; same bits as the complex64 calls on the widened samples) --------------
    def _frames_ci16(self, iq):
        x = _as_ci16(iq, self.nfft)
        self._float32_only("ci16 input")
        return (x.reshape(1, self.nfft, 2), True) if x.ndim == 2 else (x, False)

    def spectrum_db_ci16(self, iq, out: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 rows of int16 I,Q frames ``(nfft, 2)`` or ``(B, nfft, 2)``: bit-identical to ``spectrum_db`` on
        ``float32(I) + 1j*float32(Q)``."""
        x, one = self._frames_ci16(iq)
        res = self._out_array(out, (self.nfft,) if one else x.shape[:2], np.float32)
        if x.shape[0]:
            self._run_host(lib().sdrk_exec_host_ci16, x, x.shape[0], self.nfft, res)
        return res

    def fft_ci16(self, iq) -> np.ndarray:
        """complex64 spectrum of int16 I,Q frames: bit-identical to ``fft`` on the widened samples."""
        x, one = self._frames_ci16(iq)
        out = np.empty(x.shape[:2], dtype=np.complex64)
        if x.shape[0]:
            self._run_host(lib().sdrk_exec_fft_host_ci16, x, x.shape[0], self.nfft, out)
        return out[0] if one else out

    def stft_db_ci16(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Spectrogram rows over one contiguous int16 I,Q stream ``(n_samples, 2)``; rows as ``stft_db``."""
        return self._host_rows(_CI16, iq, hop, out, what="ci16 input")

    def exec_device_ci16(self, d_iq: int, n_frames: int, d_out: int, *, frame_stride: Optional[int] = None,
                         stream: int = 0) -> None:
        """Device pointers: int16 I,Q in (4 bytes per sample) / float32 rows out, asynchronous on ``stream`` (0: the
        plan's stream); any number of frames."""
        self._exec_device(_CI16, d_iq, n_frames, d_out, frame_stride, stream, what="ci16 input")

    def exec_device_ci16_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                                    frame_stride: Optional[int] = None) -> list:
        """``exec_device_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_CI16, d_iq, n_frames, d_out, launches, frame_stride, what="ci16 input")

    def exec_device_ci16_timed(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                               frame_stride: Optional[int] = None) -> float:
        """The same, all launches together (the sum of the per-launch times)."""
        return float(sum(self.exec_device_ci16_timed_each(d_iq, n_frames, d_out, launches, frame_stride=frame_stride)))

    # -- 8-bit I,Q input, SigMF ci8 (int8) / cu8 (uint8): the array's dtype is the format; float32 plans; the same bits as
    #    the complex64 calls on iq8_to_c64 of the samples --------------------------------------------------------------
    def _frames_ci8(self, iq):
        x = _as_ci8(iq, self.nfft)
        self._float32_only("8-bit I,Q input")
        return (x.reshape(1, self.nfft, 2), True) if x.ndim == 2 else (x, False)

    def spectrum_db_ci8(self, iq, out: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 rows of 8-bit I,Q frames ``(nfft, 2)`` or ``(B, nfft, 2)``, int8 (ci8) or uint8 (cu8): bit-identical to
        ``spectrum_db`` on ``iq8_to_c64(iq)``."""
        x, one = self._frames_ci8(iq)
        res = self._out_array(out, (self.nfft,) if one else x.shape[:2], np.float32)
        if x.shape[0]:
            self._run_host(_CI8.entry(_CI8.host_db, _iq8_format(x)), x, x.shape[0], self.nfft, res)
        return res

    def fft_ci8(self, iq) -> np.ndarray:
        """complex64 spectrum of 8-bit I,Q frames: bit-identical to ``fft`` on the widened samples."""
        x, one = self._frames_ci8(iq)
        out = np.empty(x.shape[:2], dtype=np.complex64)
        if x.shape[0]:
            self._run_host(_CI8.entry(_CI8.host_fft, _iq8_format(x)), x, x.shape[0], self.nfft, out)
        return out[0] if one else out

    def stft_db_ci8(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Spectrogram rows over one contiguous 8-bit I,Q stream ``(n_samples, 2)``; rows as ``stft_db``."""
        return self._host_rows(_CI8, iq, hop, out, what="8-bit I,Q input")

    def exec_device_ci8(self, d_iq: int, n_frames: int, d_out: int, *, unsigned: bool = False,
                        frame_stride: Optional[int] = None, stream: int = 0) -> None:
        """Device pointers: 8-bit I,Q in (2 bytes per sample; ``unsigned``: cu8, else ci8) / float32 rows out, asynchronous
        on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_CI8, d_iq, n_frames, d_out, frame_stride, stream, what="8-bit I,Q input",
                          fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_ci8_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *, unsigned: bool = False,
                                   frame_stride: Optional[int] = None) -> list:
        """``exec_device_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_CI8, d_iq, n_frames, d_out, launches, frame_stride, what="8-bit I,Q input",
                                            fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    # -- real-sampled input (SigMF rf32_le / ri16_le / ri8 / ru8): frames of 2 * nfft real samples, one-sided rows of
    #    nfft + 1 bins from 0 to fs / 2 in ascending order; the array's dtype is the format; float32 power-of-two plans.  The
    #    plan's own window and shift play no part: the mode has its window (set_real_window), rectangular until one is set --
    def set_real_window(self, window: WindowArg) -> None:
        """The real window of the ``r*`` calls: None / ``"rect"``, ``"hann"`` or ``2 * nfft`` coefficients (copied)."""
        self._float32_only("real-sampled input")
        w = _real_window(window, 2 * self.nfft)
        with self._lock:
            if w is None:
                check(lib().sdrk_plan_set_real_window(self.handle, None, c_size_t(0)))
            else:
                check(lib().sdrk_plan_set_real_window(self.handle, w.ctypes.data_as(c_void_p), c_size_t(w.shape[0])))

    def _frames_real(self, x):
        self._float32_only("real-sampled input")
        x = _as_real(x, 2 * self.nfft)
        one = x.ndim == 1 and x.shape[0] == 2 * self.nfft
        return x.reshape(-1, 2 * self.nfft), one

    def _run_host_real(self, fn, x: np.ndarray, n_frames: int, stride: int, out: np.ndarray) -> None:
        with self._lock:
            check(fn(self.handle, x.ctypes.data_as(c_void_p), _real_format(x), c_size_t(n_frames), c_size_t(stride),
                     out.ctypes.data_as(c_void_p)))

    def rspectrum_db(self, x, out: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 rows ``20*log10(|rfft(w*x)| + eps)`` of real frames ``(frames, 2*nfft)`` (or flat: one frame gives one
        row), ``nfft + 1`` bins each.  float32, int16, int8 or uint8 (``v - 127.5``) samples."""
        x, one = self._frames_real(x)
        res = self._out_array(out, (self.nfft + 1,) if one else (x.shape[0], self.nfft + 1), np.float32)
        self._run_host_real(lib().sdrk_exec_host_real, x, x.shape[0], 2 * self.nfft, res)
        return res

    def rfft(self, x) -> np.ndarray:
        """complex64 ``np.fft.rfft(w*x, axis=-1)`` of real frames, shapes and dtypes as ``rspectrum_db``."""
        x, one = self._frames_real(x)
        res = np.empty((x.shape[0], self.nfft + 1), dtype=np.complex64)
        self._run_host_real(lib().sdrk_exec_fft_host_real, x, x.shape[0], 2 * self.nfft, res)
        return res[0] if one else res

    def rstft_db(self, x, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Spectrogram rows over one flat real-sampled stream: ``1 + (len - 2*nfft) // hop`` rows of ``nfft + 1`` bins;
        ``hop`` in real samples, even (default ``2*nfft``)."""
        self._float32_only("real-sampled input")
        x = _as_real(x, 2 * self.nfft, stream=True)
        length = 2 * self.nfft
        hop = length if hop is None else int(hop)
        if hop < 2 or hop % 2:
            raise ValueError(f"hop must be a positive even number of real samples, got {hop}")
        if x.shape[0] < length:
            raise ValueError(f"the stream has {x.shape[0]} samples, fewer than one frame of {length}")
        rows = 1 + (x.shape[0] - length) // hop
        res = self._out_array(out, (rows, self.nfft + 1), np.float32)
        self._run_host_real(lib().sdrk_exec_host_real, x, rows, hop, res)
        return res

    def _device_real_args(self, d_x: int, n_frames: int, d_out: int, fmt, out: str, frame_stride: Optional[int],
                          out_stride: Optional[int]) -> list:
        self._float32_only("real-sampled input")
        if isinstance(fmt, str):
            if fmt not in REAL_FORMAT_NAMES:
                raise ValueError(f"fmt must be one of {sorted(REAL_FORMAT_NAMES)} or an SDRK_REAL_* code, got {fmt!r}")
            fmt = REAL_FORMAT_NAMES[fmt]
        if out not in ("db", "complex"):
            raise ValueError(f"out must be 'db' or 'complex', got {out!r}")
        stride = 2 * self.nfft if frame_stride is None else int(frame_stride)
        return [c_void_p(d_x), int(fmt), c_size_t(int(n_frames)), c_size_t(stride),
                _ffi.REAL_OUT_DB if out == "db" else _ffi.REAL_OUT_COMPLEX, c_void_p(d_out),
                c_size_t(0 if out_stride is None else int(out_stride))]

    def exec_device_real(self, d_x: int, n_frames: int, d_out: int, *, fmt, out: str = "db",
                         frame_stride: Optional[int] = None, out_stride: Optional[int] = None, stream: int = 0) -> None:
        """Device pointers: real samples in (``fmt``: ``"f32"``, ``"s16"``, ``"s8"``, ``"u8"``), rows of ``nfft + 1`` float32
        dB values (``out="db"``) or complex64 (``"complex"``) out, asynchronous on ``stream`` (0: the plan's stream).
        ``frame_stride`` in real samples (even; default ``2*nfft``), ``out_stride`` in output elements (default packed)."""
        args = self._device_real_args(d_x, n_frames, d_out, fmt, out, frame_stride, out_stride)
        with self._lock:
            check(lib().sdrk_exec_device_real(self.handle, *args, c_void_p(stream) if stream else None))

    def exec_device_real_timed_each(self, d_x: int, n_frames: int, d_out: int, launches: int = 1, *, fmt, out: str = "db",
                                    frame_stride: Optional[int] = None, out_stride: Optional[int] = None) -> list:
        """``exec_device_real`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_real_args(d_x, n_frames, d_out, fmt, out, frame_stride, out_stride)
        ms = (c_float * int(launches))()
        with self._lock:
            check(lib().sdrk_exec_device_real_timed_each(self.handle, *args, int(launches), ms))
        return [float(v) for v in ms]

    # ... integrated: one row of nfft + 1 bins per k consecutive real frames, the reduction inside the transform
    def _real_hop(self, hop: Optional[int]) -> int:
        return _real_hop(hop, 2 * self.nfft)

    def rintegrated_groups(self, n_samples: int, k: int, hop: Optional[int] = None) -> int:
        """Rows ``rintegrate`` returns for a real-sampled stream of ``n_samples``: the ``1 + (n - 2*nfft)//hop`` full frames
        in whole groups of ``k``; trailing frames that do not fill a group are dropped."""
        return self._n_groups(2 * self.nfft, n_samples, k, self._real_hop(hop))

    def rintegrate(self, x, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                   scale: float = 1.0) -> np.ndarray:
        """One float32 row per ``k`` consecutive frames of one flat real-sampled stream, ``(groups, nfft + 1)``: per bin
        from 0 to fs/2 the mean (``detector="mean"``), maximum or minimum over the group's frames of ``|rfft(w*x_f)|^2``,
        returned as ``20*log10(sqrt(R) + eps)`` (``out="db"``) or ``scale * R`` (``out="power"``).  Frame f covers samples
        ``[f*hop, f*hop + 2*nfft)``; ``hop`` in real samples, even (default ``2*nfft``).  float32, int16, int8 or uint8
        (``v - 127.5``) samples; the reduction runs inside the transform on the GPU, the stream goes through in chunks."""
        self._float32_only("real-sampled input")
        x = _as_real(x, 2 * self.nfft, stream=True)
        hop = self._real_hop(hop)
        codes = self._int_codes(detector, out)
        groups = self._n_groups(2 * self.nfft, x.shape[0], k, hop)
        if groups < 1:
            raise ValueError(f"the stream has {x.shape[0]} samples, fewer than one group of {int(k)} frames of {2 * self.nfft}")
        res = np.empty((groups, self.nfft + 1), dtype=np.float32)
        with self._lock:
            check(lib().sdrk_exec_host_real_integrated(self.handle, x.ctypes.data_as(c_void_p), _real_format(x), c_size_t(groups),
                                                       c_size_t(int(k)), c_size_t(hop), *codes, c_float(float(scale)),
                                                       res.ctypes.data_as(c_void_p)))
        return res

    def _device_real_integrated_args(self, d_x: int, n_groups: int, k: int, d_out: int, fmt, frame_stride: Optional[int],
                                     detector: str, out: str, scale: float) -> list:
        self._float32_only("real-sampled input")
        if isinstance(fmt, str):
            if fmt not in REAL_FORMAT_NAMES:
                raise ValueError(f"fmt must be one of {sorted(REAL_FORMAT_NAMES)} or an SDRK_REAL_* code, got {fmt!r}")
            fmt = REAL_FORMAT_NAMES[fmt]
        codes = self._int_codes(detector, out)
        if int(k) < 1 or int(n_groups) < 1:
            raise ValueError("n_groups and k must be >= 1")
        return [c_void_p(d_x), int(fmt), c_size_t(int(n_groups)), c_size_t(int(k)), c_size_t(self._real_hop(frame_stride)), *codes,
                c_float(float(scale)), c_void_p(d_out)]

    def exec_device_real_integrated(self, d_x: int, n_groups: int, k: int, d_out: int, *, fmt,
                                    frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                    scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: real samples in (``fmt``: ``"f32"``, ``"s16"``, ``"s8"``, ``"u8"``), ``n_groups`` packed float32
        rows of ``nfft + 1`` bins out (one per ``k`` frames), asynchronous on ``stream`` (0: the plan's stream).
        ``frame_stride`` in real samples (even; default ``2*nfft``)."""
        args = self._device_real_integrated_args(d_x, n_groups, k, d_out, fmt, frame_stride, detector, out, scale)
        with self._lock:
            check(lib().sdrk_exec_device_real_integrated(self.handle, *args, c_void_p(stream) if stream else None))

    def exec_device_real_integrated_timed_each(self, d_x: int, n_groups: int, k: int, d_out: int, launches: int = 1, *, fmt,
                                               frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                               scale: float = 1.0) -> list:
        """``exec_device_real_integrated`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_real_integrated_args(d_x, n_groups, k, d_out, fmt, frame_stride, detector, out, scale)
        ms = (c_float * int(launches))()
        with self._lock:
            check(lib().sdrk_exec_device_real_integrated_timed_each(self.handle, *args, int(launches), ms))
        return [float(v) for v in ms]

    def welch_psd(self, iq, sample_rate: float, hop: Optional[int] = None) -> np.ndarray:
        """Averaged periodogram of one contiguous stream, float32 ``(nfft,)``:
        ``mean_r |fft(w * x_r)|^2 / (sample_rate * sum(w^2))`` over the
        ``1 + (len - nfft)//hop`` full segments — matplotlib's ``mlab.psd`` (no detrend,
        two-sided; in fftshift order when the plan shifts), which is what the reference's
        offline script plots (scripts/process_sigmf_data.py:188-189).  The per-segment
        transforms and the averaging both run on the GPU."""
        self._float32_only("welch_psd")
        x = _as_c64(iq).reshape(-1)
        hop = self.nfft if hop is None else int(hop)
        if hop < 1:
            raise ValueError("hop must be >= 1")
        if x.shape[0] < self.nfft:
            raise ValueError(f"stream of {x.shape[0]} samples is shorter than one {self.nfft}-sample segment")
        rows = 1 + (x.shape[0] - self.nfft) // hop
        if self._wkey == "rect":
            wss = float(self.nfft)
        elif self._wkey == "hann":
            wss = float(np.sum(np.hanning(self.nfft) ** 2))
        else:
            wss = float(np.sum(np.frombuffer(self._wkey[1], dtype=np.float32).astype(np.float64) ** 2))
        scale = 1.0 / (rows * float(sample_rate) * wss)
        out = np.empty(self.nfft, dtype=np.float32)
        with self._lock:
            check(lib().sdrk_welch_psd_host(self.handle, x.ctypes.data_as(c_void_p), c_size_t(rows), c_size_t(hop),
                                            c_float(scale), out.ctypes.data_as(c_void_p)))
        return out

    # -- integrated spectra: one row per k frames (float32 plans) ---------------------------------------------
    @staticmethod
    def _int_codes(detector: str, out: str, sk: bool = False):
        """The C codes between the stride and the scale: (detector, out_form), or for a spectral-kurtosis call (out_form,)."""
        if out not in _ffi.INT_OUT_FORMS:
            raise ValueError(f"out must be one of {sorted(_ffi.INT_OUT_FORMS)}, got {out!r}")
        if sk:
            return (_ffi.INT_OUT_FORMS[out],)
        if detector not in _ffi.DETECTORS:
            raise ValueError(f"detector must be one of {sorted(_ffi.DETECTORS)}, got {detector!r}")
        return _ffi.DETECTORS[detector], _ffi.INT_OUT_FORMS[out]

    def integrated_groups(self, n_samples: int, k: int, hop: Optional[int] = None) -> int:
        """Rows ``integrate`` returns for a stream of ``n_samples``: the ``1 + (n - nfft)//hop`` full frames in whole
        groups of ``k``; trailing frames that do not fill a group are dropped (as ``mlab.psd`` drops a partial segment)."""
        return self._n_groups(self.nfft, n_samples, k, hop)

    def integrate(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                  scale: float = 1.0) -> np.ndarray:
        """One float32 row per ``k`` consecutive frames of one contiguous stream, ``(groups, nfft)``: per bin the mean
        (``detector="mean"``), maximum or minimum over the group's frames of ``|fft(w*x_f)|^2``, returned as
        ``20*log10(sqrt(R) + eps)`` (``out="db"``) or ``scale * R`` (``out="power"``).  Frame f covers samples
        ``[f*hop, f*hop + nfft)``.  The reduction runs inside the transform on the GPU; the stream goes through in
        chunks, in device memory that does not depend on its length."""
        return self._host_integrated(_C64, iq, hop, _Integ(k, detector, out, scale), what="integrate")

    def exec_device_integrated(self, d_iq: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                               detector: str = "mean", out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: complex64 in, ``n_groups`` float32 rows out (one per ``k`` frames), asynchronous on
        ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_C64, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale), what="integrate")

    def exec_device_integrated_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                          frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                          scale: float = 1.0) -> list:
        """``exec_device_integrated`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_C64, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale), what="integrate")

    # ... from int16 I,Q: the bits of the three above on the widened samples, from half the input bytes
    def integrate_ci16(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                       scale: float = 1.0) -> np.ndarray:
        """``integrate`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: bit-identical to ``integrate`` on
        ``float32(I) + 1j*float32(Q)``; no scale is applied to the samples.  At nfft = 4096 the int16 samples are read
        inside the reducing transform."""
        return self._host_integrated(_CI16, iq, hop, _Integ(k, detector, out, scale), what="integrate_ci16")

    def exec_device_integrated_ci16(self, d_iq: int, n_groups: int, k: int, d_out: int, *,
                                    frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                    scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: int16 I,Q in (4 bytes per sample, frame starts 4-byte aligned), ``n_groups`` float32 rows out,
        asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_CI16, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale),
                          what="integrate_ci16")

    def exec_device_integrated_ci16_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                               frame_stride: Optional[int] = None, detector: str = "mean",
                                               out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_integrated_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_CI16, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale), what="integrate_ci16")

    # ... from 8-bit I,Q (int8: ci8, uint8: cu8): the bits of the complex64 three on the widened samples, from a quarter of
    # the input bytes
    def integrate_ci8(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                      scale: float = 1.0) -> np.ndarray:
        """``integrate`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)``, int8 or uint8: bit-identical to
        ``integrate`` on ``iq8_to_c64(iq)``; no scale is applied to the samples.  At nfft = 4096 the bytes are read inside
        the reducing transform."""
        return self._host_integrated(_CI8, iq, hop, _Integ(k, detector, out, scale), what="integrate_ci8")

    def exec_device_integrated_ci8(self, d_iq: int, n_groups: int, k: int, d_out: int, *, unsigned: bool = False,
                                   frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                   scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: 8-bit I,Q in (2 bytes per sample; ``unsigned``: cu8, else ci8), ``n_groups`` float32 rows out,
        asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_CI8, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale),
                          what="integrate_ci8", fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_integrated_ci8_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                              unsigned: bool = False, frame_stride: Optional[int] = None,
                                              detector: str = "mean", out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_integrated_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_CI8, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale), what="integrate_ci8",
                                            fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    # -- polyphase filter bank: T blocks folded under a prototype in front of the transform (float32, rectangular plans) ----
    def set_pfb(self, h) -> int:
        """Set the prototype filter: ``taps*nfft`` float32 coefficients (``pfb_prototype`` makes the usual windowed sinc);
        ``taps`` follows from the length and is returned.  May be called again with another prototype or another ``taps``."""
        self._float32_only("the polyphase filter bank")
        if self._wkey != "rect":
            raise ValueError("the polyphase filter bank needs a plan with the rectangular window: the prototype is the window")
        c = np.ascontiguousarray(np.asarray(h, dtype=np.float32))
        if c.ndim != 1 or c.shape[0] == 0 or c.shape[0] % self.nfft:
            raise ValueError(f"prototype must be a 1-D array of taps*{self.nfft} coefficients, got shape {c.shape}")
        taps = c.shape[0] // self.nfft
        if taps > PFB_MAX_TAPS:
            raise ValueError(f"prototype has {taps} taps, at most {PFB_MAX_TAPS} are supported")
        with self._lock:
            check(lib().sdrk_plan_set_pfb(self.handle, taps, c.ctypes.data_as(c_void_p)))
            self.pfb_taps = taps
        return taps

    def _pfb_ready(self) -> int:
        self._float32_only("the polyphase filter bank")
        if self.pfb_taps < 1:
            raise ValueError("no prototype filter set: call set_pfb() first")
        return self.pfb_taps * self.nfft

    def pfb_frames(self, n_samples: int, hop: Optional[int] = None) -> int:
        """Rows ``pfb_db`` returns for a stream of ``n_samples``: frame r covers samples ``[r*hop, r*hop + taps*nfft)``,
        so ``1 + (n_samples - taps*nfft) // hop`` (0 if the stream is shorter than one span)."""
        return self._n_frames(self._pfb_ready(), n_samples, hop)

    def pfb_db(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """float32 dB rows ``(pfb_frames, nfft)`` of the polyphase filter bank over one contiguous complex64 stream: the
        plan's ``spectrum_db`` of the folded frames ``sum_t h[t*nfft + n] * x[r*hop + t*nfft + n]``, bit for bit what
        numpy's float32 fold followed by ``spectrum_db`` gives; the fold runs inside the transform on the GPU."""
        return self._host_rows(_PFB, iq, hop, out)

    def pfb_fft(self, iq, hop: Optional[int] = None) -> np.ndarray:
        """complex64 spectra ``(pfb_frames, nfft)`` of the folded frames (fftshifted if the plan shifts), no log."""
        return self._host_rows(_PFB, iq, hop, spectra=True)

    def exec_device_pfb(self, d_iq: int, n_frames: int, d_out: int, *, frame_stride: Optional[int] = None,
                        stream: int = 0) -> None:
        """Device pointers: the raw complex64 stream in (``(n_frames-1)*frame_stride + taps*nfft`` samples) / float32 rows
        out, asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_PFB, d_iq, n_frames, d_out, frame_stride, stream)

    def exec_device_pfb_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                                   frame_stride: Optional[int] = None) -> list:
        """``exec_device_pfb`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB, d_iq, n_frames, d_out, launches, frame_stride)

    # ... integrated: one row per k folded frames (the spectrometer form of the filter bank)
    def pfb_integrated_groups(self, n_samples: int, k: int, hop: Optional[int] = None) -> int:
        """Rows ``pfb_integrate`` returns for a stream of ``n_samples``: the ``pfb_frames`` full frames in whole groups of
        ``k``; trailing frames that do not fill a group are dropped."""
        return self._n_groups(self._pfb_ready(), n_samples, k, hop)

    def pfb_integrate(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                      scale: float = 1.0) -> np.ndarray:
        """One float32 row per ``k`` consecutive polyphase-filter-bank frames of one contiguous complex64 stream,
        ``(groups, nfft)``: per bin the mean, maximum or minimum over the group of ``|fft(y_f)|^2`` with ``y_f`` the folded
        frame of ``pfb_db``, as ``20*log10(sqrt(R) + eps)`` (``out="db"``) or ``scale * R`` (``out="power"``) — bit for bit
        ``integrate`` on the packed folded frames.  Fold, transform and reduction run in one kernel at nfft = 4096; the
        stream goes through in chunks, in device memory that does not depend on its length."""
        return self._host_integrated(_PFB, iq, hop, _Integ(k, detector, out, scale))

    def exec_device_pfb_integrated(self, d_iq: int, n_groups: int, k: int, d_out: int, *,
                                   frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                   scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: the raw complex64 stream in (``(n_groups*k - 1)*frame_stride + taps*nfft`` samples),
        ``n_groups`` float32 rows out, asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_PFB, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale))

    def exec_device_pfb_integrated_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                              frame_stride: Optional[int] = None, detector: str = "mean",
                                              out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_pfb_integrated`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale))

    # ... from int16 I,Q: the bits of the seven above on the widened samples, from half the input bytes
    def pfb_db_ci16(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``pfb_db`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: bit-identical to ``pfb_db`` on
        ``float32(I) + 1j*float32(Q)``; no scale is applied to the samples.  The int16 samples are read by the folding
        kernel itself (4 bytes per sample over the link and from device memory)."""
        return self._host_rows(_PFB_CI16, iq, hop, out)

    def pfb_fft_ci16(self, iq, hop: Optional[int] = None) -> np.ndarray:
        """``pfb_fft`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples."""
        return self._host_rows(_PFB_CI16, iq, hop, spectra=True)

    def exec_device_pfb_ci16(self, d_iq: int, n_frames: int, d_out: int, *, frame_stride: Optional[int] = None,
                             stream: int = 0) -> None:
        """Device pointers: the raw int16 I,Q stream in (``(n_frames-1)*frame_stride + taps*nfft`` samples of 4 bytes, frame
        starts 4-byte aligned) / float32 rows out, asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_PFB_CI16, d_iq, n_frames, d_out, frame_stride, stream)

    def exec_device_pfb_ci16_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                                        frame_stride: Optional[int] = None) -> list:
        """``exec_device_pfb_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB_CI16, d_iq, n_frames, d_out, launches, frame_stride)

    def pfb_integrate_ci16(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                           scale: float = 1.0) -> np.ndarray:
        """``pfb_integrate`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: bit-identical to ``pfb_integrate`` on
        ``float32(I) + 1j*float32(Q)``.  At nfft = 4096 the int16 samples are read inside the folding, reducing transform."""
        return self._host_integrated(_PFB_CI16, iq, hop, _Integ(k, detector, out, scale))

    def exec_device_pfb_integrated_ci16(self, d_iq: int, n_groups: int, k: int, d_out: int, *,
                                        frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                        scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: the raw int16 I,Q stream in (``(n_groups*k - 1)*frame_stride + taps*nfft`` samples of 4 bytes),
        ``n_groups`` float32 rows out, asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device(_PFB_CI16, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale))

    def exec_device_pfb_integrated_ci16_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                                   frame_stride: Optional[int] = None, detector: str = "mean",
                                                   out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_pfb_integrated_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB_CI16, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale))

    # ... from 8-bit I,Q (int8: ci8, uint8: cu8): the bits of the seven on ``iq8_to_c64`` of the samples, from a quarter of the bytes
    def pfb_db_ci8(self, iq, hop: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``pfb_db`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 or uint8: bit-identical to ``pfb_db`` on
        ``iq8_to_c64(iq)``; no scale is applied to the samples.  The bytes are read by the folding kernel itself (2 bytes per
        sample over the link and from device memory)."""
        return self._host_rows(_PFB_CI8, iq, hop, out)

    def pfb_fft_ci8(self, iq, hop: Optional[int] = None) -> np.ndarray:
        """``pfb_fft`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples."""
        return self._host_rows(_PFB_CI8, iq, hop, spectra=True)

    def exec_device_pfb_ci8(self, d_iq: int, n_frames: int, d_out: int, *, unsigned: bool = False,
                            frame_stride: Optional[int] = None, stream: int = 0) -> None:
        """Device pointers: the raw 8-bit I,Q stream in (``(n_frames-1)*frame_stride + taps*nfft`` samples of 2 bytes;
        ``unsigned``: cu8, else ci8; frame starts 2-byte aligned) / float32 rows out, asynchronous on ``stream`` (0: the
        plan's stream); any number of frames."""
        self._exec_device(_PFB_CI8, d_iq, n_frames, d_out, frame_stride, stream, fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_pfb_ci8_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                                       unsigned: bool = False, frame_stride: Optional[int] = None) -> list:
        """``exec_device_pfb_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB_CI8, d_iq, n_frames, d_out, launches, frame_stride,
                                            fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def pfb_integrate_ci8(self, iq, k: int, hop: Optional[int] = None, detector: str = "mean", out: str = "db",
                          scale: float = 1.0) -> np.ndarray:
        """``pfb_integrate`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 or uint8: bit-identical to
        ``pfb_integrate`` on ``iq8_to_c64(iq)``.  At nfft = 4096 the bytes are read inside the folding, reducing transform."""
        return self._host_integrated(_PFB_CI8, iq, hop, _Integ(k, detector, out, scale))

    def exec_device_pfb_integrated_ci8(self, d_iq: int, n_groups: int, k: int, d_out: int, *, unsigned: bool = False,
                                       frame_stride: Optional[int] = None, detector: str = "mean", out: str = "db",
                                       scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: the raw 8-bit I,Q stream in (``(n_groups*k - 1)*frame_stride + taps*nfft`` samples of 2 bytes;
        ``unsigned``: cu8, else ci8), ``n_groups`` float32 rows out, asynchronous on ``stream`` (0: the plan's stream)."""
        self._exec_device(_PFB_CI8, d_iq, n_groups, d_out, frame_stride, stream, _Integ(k, detector, out, scale),
                          fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_pfb_integrated_ci8_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                                  unsigned: bool = False, frame_stride: Optional[int] = None,
                                                  detector: str = "mean", out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_pfb_integrated_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_timed_each(_PFB_CI8, d_iq, n_groups, d_out, launches, frame_stride,
                                            _Integ(k, detector, out, scale), fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    # -- spectral kurtosis: mean power and SK per k frames, both sums kept inside the transform (float32 plans) ----------
    def _host_sk(self, m: _Mode, iq, k: int, hop: Optional[int], out: str, scale: float, what: str = ""):
        planes = self._host_integrated(m, iq, hop, _Integ(k, "mean", out, scale, True), what=what)
        return planes[:, 0], planes[:, 1]

    def spectral_kurtosis(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``(mean_rows, sk_rows)``: two ``(groups, nfft)`` float32 views of one array, one row each per ``k >= 2``
        consecutive frames of one contiguous stream (frames and groups as for ``integrate``).  ``mean_rows`` is the group's
        mean power ``S1/k`` as ``20*log10(sqrt(R) + eps)`` (``out="db"``) or ``scale * R`` (``out="power"``); ``sk_rows`` is
        the spectral kurtosis estimator ``(k+1)/(k-1) * (k*S2/S1^2 - 1)`` with ``S1 = sum p``, ``S2 = sum p^2`` over the
        group's ``p = |fft(w*x_f)|^2``: 1 for Gaussian noise, towards 0 on a carrier, well above 1 on pulsed interference;
        0 on a bin without power.  The sums are plain float32 sums kept inside the transform: ``mean_rows`` is not the
        compensated mean of ``integrate`` (relative error up to ``k * 2^-24`` on near-constant bins)."""
        return self._host_sk(_C64, iq, k, hop, out, scale, "spectral_kurtosis")

    def spectral_kurtosis_ci16(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``spectral_kurtosis`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: bit-identical to it on
        ``float32(I) + 1j*float32(Q)``, from half the input bytes."""
        return self._host_sk(_CI16, iq, k, hop, out, scale, "spectral_kurtosis_ci16")

    def spectral_kurtosis_ci8(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``spectral_kurtosis`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 (ci8) or uint8 (cu8):
        bit-identical to it on ``iq8_to_c64(iq)``, from a quarter of the input bytes."""
        return self._host_sk(_CI8, iq, k, hop, out, scale, "spectral_kurtosis_ci8")

    def pfb_spectral_kurtosis(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``spectral_kurtosis`` of the polyphase-filter-bank frames of ``pfb_db`` (``set_pfb`` first; rectangular float32
        plans): fold and transform per frame, the sums down the columns of the staged spectra at every nfft."""
        return self._host_sk(_PFB, iq, k, hop, out, scale)

    def pfb_spectral_kurtosis_ci16(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``pfb_spectral_kurtosis`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same bits as on the
        widened samples."""
        return self._host_sk(_PFB_CI16, iq, k, hop, out, scale)

    def pfb_spectral_kurtosis_ci8(self, iq, k: int, hop: Optional[int] = None, out: str = "db", scale: float = 1.0):
        """``pfb_spectral_kurtosis`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 or uint8: the same bits as
        on ``iq8_to_c64(iq)``."""
        return self._host_sk(_PFB_CI8, iq, k, hop, out, scale)

    def _exec_device_sk(self, m: _Mode, what: str, d_iq: int, n_groups: int, k: int, d_out: int, frame_stride, out: str,
                        scale: float, stream: int = 0, launches: Optional[int] = None, fmt: Optional[int] = None):
        i = _Integ(k, "mean", out, scale, True)
        if launches is None:
            return self._exec_device(m, d_iq, n_groups, d_out, frame_stride, stream, i, what=what, fmt=fmt)
        return self._exec_device_timed_each(m, d_iq, n_groups, d_out, launches, frame_stride, i, what=what, fmt=fmt)

    def exec_device_sk(self, d_iq: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                       out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: complex64 in, ``n_groups * 2 * nfft`` float32 out (per group the mean-power row, then the SK
        row), asynchronous on ``stream`` (0: the plan's stream); any number of frames."""
        self._exec_device_sk(_C64, "spectral_kurtosis", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream)

    def exec_device_sk_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                  frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_sk`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_C64, "spectral_kurtosis", d_iq, n_groups, k, d_out, frame_stride, out, scale,
                                    launches=launches)

    def exec_device_sk_ci16(self, d_iq: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                            out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_sk`` from int16 I,Q (4 bytes per sample, frame starts 4-byte aligned)."""
        self._exec_device_sk(_CI16, "spectral_kurtosis_ci16", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream)

    def exec_device_sk_ci16_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                       frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_sk_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_CI16, "spectral_kurtosis_ci16", d_iq, n_groups, k, d_out, frame_stride, out, scale,
                                    launches=launches)

    def exec_device_pfb_sk(self, d_iq: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                           out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_sk`` behind the filter bank: the raw complex64 stream in
        (``(n_groups*k - 1)*frame_stride + taps*nfft`` samples)."""
        self._exec_device_sk(_PFB, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream)

    def exec_device_pfb_sk_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                      frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_pfb_sk`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_PFB, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, launches=launches)

    def exec_device_pfb_sk_ci16(self, d_iq: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                                out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_pfb_sk`` from the raw int16 I,Q stream (4 bytes per sample)."""
        self._exec_device_sk(_PFB_CI16, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream)

    def exec_device_pfb_sk_ci16_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                           frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0) -> list:
        """``exec_device_pfb_sk_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_PFB_CI16, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, launches=launches)

    def exec_device_sk_ci8(self, d_iq: int, n_groups: int, k: int, d_out: int, *, unsigned: bool = False,
                           frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_sk`` from 8-bit I,Q (2 bytes per sample; ``unsigned``: cu8, else ci8; frame starts 2-byte aligned)."""
        self._exec_device_sk(_CI8, "spectral_kurtosis_ci8", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream,
                             fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_sk_ci8_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                      unsigned: bool = False, frame_stride: Optional[int] = None, out: str = "db",
                                      scale: float = 1.0) -> list:
        """``exec_device_sk_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_CI8, "spectral_kurtosis_ci8", d_iq, n_groups, k, d_out, frame_stride, out, scale,
                                    launches=launches, fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_pfb_sk_ci8(self, d_iq: int, n_groups: int, k: int, d_out: int, *, unsigned: bool = False,
                               frame_stride: Optional[int] = None, out: str = "db", scale: float = 1.0,
                               stream: int = 0) -> None:
        """``exec_device_pfb_sk`` from the raw 8-bit I,Q stream (2 bytes per sample; ``unsigned``: cu8, else ci8)."""
        self._exec_device_sk(_PFB_CI8, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, stream,
                             fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    def exec_device_pfb_sk_ci8_timed_each(self, d_iq: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                          unsigned: bool = False, frame_stride: Optional[int] = None, out: str = "db",
                                          scale: float = 1.0) -> list:
        """``exec_device_pfb_sk_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_sk(_PFB_CI8, "", d_iq, n_groups, k, d_out, frame_stride, out, scale, launches=launches,
                                    fmt=IQ8_UNSIGNED if unsigned else IQ8_SIGNED)

    # -- two-channel cross-spectra: auto and cross power per k frames, four sums kept inside the transform (float32 plans) --
    def _host_xspec(self, x: np.ndarray, ci16: bool, k: int, hop: Optional[int], scale: float, what: str) -> CrossSpectrum:
        self._float32_only(what)
        groups = self._n_groups(self.nfft, x.shape[0], k, hop)
        res = np.empty((groups, 4, self.nfft), dtype=np.float32)
        if groups:
            fn = getattr(lib(), "sdrk_exec_host_xspec_ci16" if ci16 else "sdrk_exec_host_xspec")
            with self._lock:
                check(fn(self.handle, x.ctypes.data_as(c_void_p), c_size_t(groups), c_size_t(int(k)),
                         c_size_t(self.nfft if hop is None else int(hop)), c_float(scale), res.ctypes.data_as(c_void_p)))
        return CrossSpectrum(res[:, 0], res[:, 1], res[:, 2], res[:, 3])

    def cross_spectrum(self, iq2, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CrossSpectrum:
        """Auto and cross power of two coherent channels per ``k >= 1`` consecutive frames of one contiguous two-channel
        stream: a ``CrossSpectrum`` of four ``(groups, nfft)`` float32 views of one array, ``scale/k`` times the sums over
        the group of ``|A|^2``, ``|B|^2``, ``Re(A conj B)``, ``Im(A conj B)`` with ``A = fft(w*x0_f)``, ``B = fft(w*x1_f)``;
        its ``.cross``, ``.coherence`` and ``.phase`` derive the rest.  ``iq2`` is an ``(n, 2)`` complex array (element ``n``
        = sample ``n`` of channel 0, then of channel 1: used as it is when complex64 and C-contiguous) or a pair ``(a, b)``
        of equal-length arrays, which is stacked first — a copy of both.  Frames start every ``hop`` elements (default
        ``nfft``).  The sums are plain float32 sums kept inside the transform, as for ``spectral_kurtosis``."""
        return self._host_xspec(_as_iq2_c64(iq2), False, k, hop, scale, "cross_spectrum")

    def cross_spectrum_ci16(self, iq2, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CrossSpectrum:
        """``cross_spectrum`` over int16 elements, ``(n, 2, 2)`` or ``(n, 4)`` int16 (``I0 Q0 I1 Q1``; or a pair of
        ``(n, 2)`` int16 arrays, stacked first — a copy): bit-identical to it on the widened elements, from half the bytes."""
        return self._host_xspec(_as_iq2_ci16(iq2), True, k, hop, scale, "cross_spectrum_ci16")

    def _xspec_device_args(self, what: str, d_iq2: int, n_groups: int, k: int, d_out: int, frame_stride, scale: float) -> list:
        self._float32_only(what)
        stride = self.nfft if frame_stride is None else int(frame_stride)
        if int(k) < 1 or int(n_groups) < 1:
            raise ValueError("k and n_groups must be >= 1")
        if stride < 1:
            raise ValueError("frame_stride must be >= 1")
        return [c_void_p(d_iq2), c_size_t(int(n_groups)), c_size_t(int(k)), c_size_t(stride), c_float(scale), c_void_p(d_out)]

    def _exec_device_xspec(self, sym: str, d_iq2: int, n_groups: int, k: int, d_out: int, frame_stride, scale: float,
                           stream: int = 0, launches: Optional[int] = None):
        args = self._xspec_device_args(sym, d_iq2, n_groups, k, d_out, frame_stride, scale)
        with self._lock:
            if launches is None:
                return check(getattr(lib(), sym)(self.handle, *args, c_void_p(stream) if stream else None))
            ms = (c_float * int(launches))()
            check(getattr(lib(), sym + "_timed_each")(self.handle, *args, int(launches), ms))
        return [float(v) for v in ms]

    def exec_device_xspec(self, d_iq2: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                          scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: complex64 elements in (16 bytes each; ``frame_stride`` counts elements), ``n_groups * 4 * nfft``
        float32 out (per group the four planes of ``cross_spectrum``), asynchronous on ``stream`` (0: the plan's stream)."""
        self._exec_device_xspec("sdrk_exec_device_xspec", d_iq2, n_groups, k, d_out, frame_stride, scale, stream)

    def exec_device_xspec_timed_each(self, d_iq2: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                     frame_stride: Optional[int] = None, scale: float = 1.0) -> list:
        """``exec_device_xspec`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_xspec("sdrk_exec_device_xspec", d_iq2, n_groups, k, d_out, frame_stride, scale,
                                       launches=launches)

    def exec_device_xspec_ci16(self, d_iq2: int, n_groups: int, k: int, d_out: int, *, frame_stride: Optional[int] = None,
                               scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_xspec`` from int16 elements (8 bytes each)."""
        self._exec_device_xspec("sdrk_exec_device_xspec_ci16", d_iq2, n_groups, k, d_out, frame_stride, scale, stream)

    def exec_device_xspec_ci16_timed_each(self, d_iq2: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                          frame_stride: Optional[int] = None, scale: float = 1.0) -> list:
        """``exec_device_xspec_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_xspec("sdrk_exec_device_xspec_ci16", d_iq2, n_groups, k, d_out, frame_stride, scale,
                                       launches=launches)

    # -- correlation matrix of 2..8 channels per k frames: every channel transformed once, C*C sums per bin (float32 plans) --
    _CORRMAT_SYMS = {"c64": "corrmat", "ci16": "corrmat_ci16", "ci8": "corrmat_iq8"}

    def _host_corrmat(self, x: np.ndarray, form: str, k: int, hop: Optional[int], scale: float, what: str) -> np.ndarray:
        self._float32_only(what)
        c = int(x.shape[1])
        groups = self._n_groups(self.nfft, x.shape[0], k, hop)
        res = np.empty((groups, c * c, self.nfft), dtype=np.float32)
        if groups:
            fn = getattr(lib(), "sdrk_exec_host_" + self._CORRMAT_SYMS[form])
            fmt = [c_int(_iq8_format(x))] if form == "ci8" else []
            with self._lock:
                check(fn(self.handle, x.ctypes.data_as(c_void_p), *fmt, c_int(c), c_size_t(groups), c_size_t(int(k)),
                         c_size_t(self.nfft if hop is None else int(hop)), c_float(scale), res.ctypes.data_as(c_void_p)))
        return res

    def correlate(self, iq, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CorrelationMatrix:
        """The correlation matrix of ``C`` = 2..8 coherent channels per ``k >= 1`` consecutive frames of one contiguous
        ``C``-channel stream: a ``CorrelationMatrix`` over one ``(groups, C*C, nfft)`` float32 array.  ``iq`` is an ``(n, C)``
        complex array (element ``n`` = sample ``n`` of channel 0, 1, ... ``C-1``: used as it is when complex64 and
        C-contiguous).  Frames start every ``hop`` elements (default ``nfft``).  Every channel is transformed once per frame;
        each pair's planes are the bits ``cross_spectrum`` gives for that pair."""
        x = _as_iqc_c64(iq)
        return CorrelationMatrix(self._host_corrmat(x, "c64", k, hop, scale, "correlate"), x.shape[1])

    def correlate_ci16(self, iq, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CorrelationMatrix:
        """``correlate`` over int16 elements, ``(n, C, 2)`` int16 (channel, then I, Q): bit-identical to it on the widened
        elements, from half the bytes."""
        x = _as_iqc_int(iq, (np.int16,), "ci16")
        return CorrelationMatrix(self._host_corrmat(x, "ci16", k, hop, scale, "correlate_ci16"), x.shape[1])

    def correlate_ci8(self, iq, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CorrelationMatrix:
        """``correlate`` over 8-bit elements, ``(n, C, 2)`` int8 (ci8) or uint8 (cu8: ``byte - 127.5``); the dtype is the
        format.  Bit-identical to ``correlate`` on ``iq8_to_c64`` of the elements, from a quarter of the bytes."""
        x = _as_iqc_int(iq, (np.int8, np.uint8), "8-bit")
        return CorrelationMatrix(self._host_corrmat(x, "ci8", k, hop, scale, "correlate_ci8"), x.shape[1])

    def cross_spectrum_ci8(self, iq8, k: int, hop: Optional[int] = None, scale: float = 1.0) -> CrossSpectrum:
        """``cross_spectrum`` over 8-bit elements, ``(n, 2, 2)`` int8 or uint8: served by the correlation-matrix call at two
        channels, whose four planes are the two-channel layout; bit-identical to ``cross_spectrum`` on the widened pair."""
        x = _as_iqc_int(iq8, (np.int8, np.uint8), "8-bit")
        if x.shape[1] != 2:
            raise ValueError(f"cross_spectrum_ci8 takes two channels, (n, 2, 2), got {x.shape}")
        res = self._host_corrmat(x, "ci8", k, hop, scale, "cross_spectrum_ci8")
        return CrossSpectrum(res[:, 0], res[:, 1], res[:, 2], res[:, 3])

    def _exec_device_corrmat(self, form: str, d_iq: int, channels: int, n_groups: int, k: int, d_out: int, frame_stride,
                             scale: float, stream: int = 0, launches: Optional[int] = None, unsigned: bool = False):
        sym = "sdrk_exec_device_" + self._CORRMAT_SYMS[form]
        args = self._xspec_device_args(sym, d_iq, n_groups, k, d_out, frame_stride, scale)
        fmt = [c_int(IQ8_UNSIGNED if unsigned else IQ8_SIGNED)] if form == "ci8" else []
        args = [args[0], *fmt, c_int(_corrmat_channels(channels)), *args[1:]]
        with self._lock:
            if launches is None:
                return check(getattr(lib(), sym)(self.handle, *args, c_void_p(stream) if stream else None))
            ms = (c_float * int(launches))()
            check(getattr(lib(), sym + "_timed_each")(self.handle, *args, int(launches), ms))
        return [float(v) for v in ms]

    def exec_device_corrmat(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int, *,
                            frame_stride: Optional[int] = None, scale: float = 1.0, stream: int = 0) -> None:
        """Device pointers: complex64 elements of ``channels`` samples in (``frame_stride`` counts elements; aligned to a
        sample), ``n_groups * channels**2 * nfft`` float32 out, asynchronous on ``stream`` (0: the plan's stream)."""
        self._exec_device_corrmat("c64", d_iq, channels, n_groups, k, d_out, frame_stride, scale, stream)

    def exec_device_corrmat_timed_each(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int, launches: int = 1, *,
                                       frame_stride: Optional[int] = None, scale: float = 1.0) -> list:
        """``exec_device_corrmat`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_corrmat("c64", d_iq, channels, n_groups, k, d_out, frame_stride, scale, launches=launches)

    def exec_device_corrmat_ci16(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int, *,
                                 frame_stride: Optional[int] = None, scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_corrmat`` from int16 elements (``4 * channels`` bytes each)."""
        self._exec_device_corrmat("ci16", d_iq, channels, n_groups, k, d_out, frame_stride, scale, stream)

    def exec_device_corrmat_ci16_timed_each(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int,
                                            launches: int = 1, *, frame_stride: Optional[int] = None,
                                            scale: float = 1.0) -> list:
        """``exec_device_corrmat_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_corrmat("ci16", d_iq, channels, n_groups, k, d_out, frame_stride, scale, launches=launches)

    def exec_device_corrmat_ci8(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int, *, unsigned: bool = False,
                                frame_stride: Optional[int] = None, scale: float = 1.0, stream: int = 0) -> None:
        """``exec_device_corrmat`` from 8-bit elements (``2 * channels`` bytes each; ``unsigned``: cu8, else ci8)."""
        self._exec_device_corrmat("ci8", d_iq, channels, n_groups, k, d_out, frame_stride, scale, stream, unsigned=unsigned)

    def exec_device_corrmat_ci8_timed_each(self, d_iq: int, channels: int, n_groups: int, k: int, d_out: int,
                                           launches: int = 1, *, unsigned: bool = False, frame_stride: Optional[int] = None,
                                           scale: float = 1.0) -> list:
        """``exec_device_corrmat_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._exec_device_corrmat("ci8", d_iq, channels, n_groups, k, d_out, frame_stride, scale, launches=launches,
                                         unsigned=unsigned)

    # -- FIR filtering and channel extraction: tune, filter, decimate (float32 plans with nfft = 4096) -----------------------
    def set_fir(self, taps) -> int:
        """Set the FIR filter: 1..2049 complex taps (``channel_taps`` makes the usual low-pass); returns their number.  The plan
        keeps the filter's 4096-point frequency response; may be called again, and leaves a PFB prototype alone."""
        self._float32_only("FIR filtering")
        h = _as_c64(taps)
        if h.ndim != 1 or not 1 <= h.shape[0] <= FIR_MAX_TAPS:
            raise ValueError(f"taps must be a 1-D array of 1..{FIR_MAX_TAPS} coefficients, got shape {h.shape}")
        with self._lock:
            check(lib().sdrk_plan_set_fir(self.handle, int(h.shape[0]), h.ctypes.data_as(c_void_p)))
            self.fir_taps = int(h.shape[0])
        return self.fir_taps

    def _fir_ready(self) -> int:
        self._float32_only("FIR filtering")
        if self.fir_taps < 1:
            raise ValueError("no FIR filter set: call set_fir() first")
        return self.fir_taps

    def _host_fir(self, sym: str, x: np.ndarray, n: int, prefix, decim: int, shift_bins: int, sample0: int) -> np.ndarray:
        decim, shift_bins = _fir_args(decim, shift_bins)
        if int(sample0) < 0:
            raise ValueError("sample0 must be >= 0")
        out = np.empty((n + decim - 1) // decim, dtype=np.complex64)
        n_out = c_size_t(0)
        with self._lock:
            check(getattr(lib(), sym)(self.handle, prefix.ctypes.data_as(c_void_p) if prefix is not None else None,
                                      x.ctypes.data_as(c_void_p), c_size_t(n), decim, shift_bins, _ffi.c_uint64(int(sample0)),
                                      out.ctypes.data_as(c_void_p), byref(n_out)))
        return out[: n_out.value]

    def fir(self, iq, *, decim: int = 1, shift_bins: int = 0, prefix=None, sample0: int = 0) -> np.ndarray:
        """Tune, filter and decimate one piece of a complex64 stream: with ``h`` the taps set by ``set_fir`` (``M`` of them),
        ``y[j] = sum_t h[t] exp(2 pi i s t / 4096) v[j + M - 1 - t]`` over ``v = prefix || iq`` (``prefix``: the ``M - 1``
        samples before ``iq``, default zeros: ``lfilter``), times ``exp(-2 pi i s (sample0 + j) / 4096)``, and of those the
        samples whose stream index ``sample0 + j`` is a multiple of ``decim``.  Overlap-save on the GPU in one kernel."""
        m = self._fir_ready()
        x = _as_c64(iq).reshape(-1)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_c64(prefix).reshape(-1)
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return self._host_fir("sdrk_exec_host_fir", x, x.shape[0], pre, decim, shift_bins, sample0)

    def fir_ci16(self, iq, *, decim: int = 1, shift_bins: int = 0, prefix=None, sample0: int = 0) -> np.ndarray:
        """``fir`` on interleaved int16 I,Q of shape ``(n, 2)`` (``prefix``: ``(M - 1, 2)`` int16): the bits of ``fir`` on the
        widened samples, at 4 bytes per sample over the link and from device memory."""
        m = self._fir_ready()
        x = _as_ci16(iq, stream=True)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_ci16(prefix, stream=True)
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return self._host_fir("sdrk_exec_host_fir_ci16", x, x.shape[0], pre, decim, shift_bins, sample0)

    def fir_outputs(self, n_in: int, decim: int = 1) -> int:
        """Samples ``exec_device_fir`` writes for ``n_in`` input samples: ``(n_in - M)//decim + 1``."""
        m = self._fir_ready()
        if int(n_in) < m:
            raise ValueError(f"n_in={n_in}: a valid convolution needs at least the {m} taps")
        return (int(n_in) - m) // int(decim) + 1

    def _device_fir_args(self, d_in: int, n_in: int, decim: int, shift_bins: int, phase0: int, d_out: int) -> list:
        self._fir_ready()
        decim, shift_bins = _fir_args(decim, shift_bins)
        return [self.handle, c_void_p(d_in), c_size_t(int(n_in)), decim, shift_bins, int(phase0) & (FIR_BLOCK - 1), c_void_p(d_out)]

    def exec_device_fir(self, d_in: int, n_in: int, d_out: int, *, decim: int = 1, shift_bins: int = 0, phase0: int = 0,
                        stream: int = 0) -> None:
        """Device pointers, "valid" form: ``n_in`` complex64 samples in, ``fir_outputs(n_in, decim)`` complex64 out,
        ``out[m] = v[m decim] W4096^(phase0 + s m decim)``; asynchronous on ``stream`` (0: the plan's stream)."""
        args = self._device_fir_args(d_in, n_in, decim, shift_bins, phase0, d_out)
        check(lib().sdrk_exec_device_fir(*args, c_void_p(stream) if stream else None))

    def exec_device_fir_ci16(self, d_in: int, n_in: int, d_out: int, *, decim: int = 1, shift_bins: int = 0, phase0: int = 0,
                             stream: int = 0) -> None:
        """``exec_device_fir`` on int16 I,Q input (4 bytes per sample)."""
        args = self._device_fir_args(d_in, n_in, decim, shift_bins, phase0, d_out)
        check(lib().sdrk_exec_device_fir_ci16(*args, c_void_p(stream) if stream else None))

    def exec_device_fir_timed_each(self, d_in: int, n_in: int, d_out: int, launches: int = 1, *, decim: int = 1,
                                   shift_bins: int = 0, phase0: int = 0) -> list:
        """``exec_device_fir`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_fir_args(d_in, n_in, decim, shift_bins, phase0, d_out)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_fir_timed_each(*args, int(launches), each))
        return list(each)

    # -- channel bank: C tuned channels from one pass over the input (the filter of set_fir) ---------------------------------
    def _host_fir_bank(self, sym: str, x: np.ndarray, prefix, shift_bins, decim: int, sample0: int) -> np.ndarray:
        decim, _ = _fir_args(decim, 0)
        shifts = _bank_shifts(shift_bins)
        if int(sample0) < 0:
            raise ValueError("sample0 must be >= 0")
        n = int(x.shape[0])
        stride = (n + decim - 1) // decim
        out = np.empty((len(shifts), stride), dtype=np.complex64)
        n_out = c_size_t(0)
        with self._lock:
            check(getattr(lib(), sym)(self.handle, prefix.ctypes.data_as(c_void_p) if prefix is not None else None,
                                      x.ctypes.data_as(c_void_p), c_size_t(n), decim, len(shifts), shifts,
                                      _ffi.c_uint64(int(sample0)), out.ctypes.data_as(c_void_p), c_size_t(stride), byref(n_out)))
        return np.ascontiguousarray(out[:, : n_out.value])

    def fir_bank(self, iq, shift_bins, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``fir`` for ``C = len(shift_bins)`` channels at once (1..64, duplicates allowed), from ONE pass over ``iq``: row
        ``c`` of the ``(C, n_out)`` complex64 result carries the bits of ``fir(iq, decim=decim, shift_bins=shift_bins[c],
        prefix=prefix, sample0=sample0)``.  The input is read once and every block transformed once; only the channel-dependent
        half (rotated filter, inverse transform, mixer, decimated store) runs per channel."""
        m = self._fir_ready()
        x = _as_c64(iq).reshape(-1)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_c64(prefix).reshape(-1)
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return self._host_fir_bank("sdrk_exec_host_chanbank", x, pre, shift_bins, decim, sample0)

    def fir_bank_ci16(self, iq, shift_bins, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``fir_bank`` on interleaved int16 I,Q of shape ``(n, 2)`` (``prefix``: ``(M - 1, 2)`` int16): the bits of
        ``fir_bank`` on the widened samples."""
        m = self._fir_ready()
        x = _as_ci16(iq, stream=True)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_ci16(prefix, stream=True)
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return self._host_fir_bank("sdrk_exec_host_chanbank_ci16", x, pre, shift_bins, decim, sample0)

    def _device_fir_bank_args(self, d_in: int, n_in: int, d_out: int, shift_bins, decim: int, phase0, out_stride) -> list:
        decim, _ = _fir_args(decim, 0)
        shifts = _bank_shifts(shift_bins)
        n_out = self.fir_outputs(n_in, decim)
        stride = n_out if out_stride is None else int(out_stride)
        if stride < n_out:
            raise ValueError(f"out_stride={stride}: a plane holds the {n_out} outputs of a channel")
        phases = None
        if phase0 is not None:
            ph = [int(v) & (FIR_BLOCK - 1) for v in np.asarray(phase0).reshape(-1)]
            if len(ph) != len(shifts):
                raise ValueError(f"phase0 must hold one value per channel ({len(shifts)}), got {len(ph)}")
            phases = (c_int * len(ph))(*ph)
        return [c_void_p(d_in), c_size_t(int(n_in)), decim, len(shifts), shifts, phases, c_void_p(d_out), c_size_t(stride)]

    def exec_device_fir_bank(self, d_in: int, n_in: int, d_out: int, shift_bins, *, decim: int = 1, phase0=None,
                             out_stride: Optional[int] = None, stream: int = 0) -> None:
        """Device pointers: ``exec_device_fir`` for ``len(shift_bins)`` channels from one pass.  Plane ``c`` starts at
        ``d_out + 8 * c * out_stride`` (default: packed, ``fir_outputs(n_in, decim)`` apart) and carries the bits of
        ``exec_device_fir(..., shift_bins=shift_bins[c], phase0=phase0[c])`` (``phase0``: one value per channel, default zeros);
        asynchronous on ``stream`` (0: the plan's stream)."""
        args = self._device_fir_bank_args(d_in, n_in, d_out, shift_bins, decim, phase0, out_stride)
        check(lib().sdrk_exec_device_chanbank(self.handle, *args, c_void_p(stream) if stream else None))

    def exec_device_fir_bank_ci16(self, d_in: int, n_in: int, d_out: int, shift_bins, *, decim: int = 1, phase0=None,
                                  out_stride: Optional[int] = None, stream: int = 0) -> None:
        """``exec_device_fir_bank`` on int16 I,Q input (4 bytes per sample)."""
        args = self._device_fir_bank_args(d_in, n_in, d_out, shift_bins, decim, phase0, out_stride)
        check(lib().sdrk_exec_device_chanbank_ci16(self.handle, *args, c_void_p(stream) if stream else None))

    def exec_device_fir_bank_timed_each(self, d_in: int, n_in: int, d_out: int, shift_bins, launches: int = 1, *, decim: int = 1,
                                        phase0=None, out_stride: Optional[int] = None) -> list:
        """``exec_device_fir_bank`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_fir_bank_args(d_in, n_in, d_out, shift_bins, decim, phase0, out_stride)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_chanbank_timed_each(self.handle, *args, int(launches), each))
        return list(each)

    # -- filter-and-sum beamformer: C coherent channels in, one down-converted channel out ---------------------------------
    def set_beam(self, taps) -> int:
        """Set the beam filters: ``(C, M)`` complex taps, one row per channel, C in 1..8 and M in 1..2049 (``beam_taps`` makes
        them from weights and a shared low-pass); returns C.  Row ``c`` becomes what ``set_fir`` makes of it.  May be called
        again; leaves the FIR filter and a PFB prototype alone."""
        self._float32_only("beamforming")
        h = _as_c64(taps)
        if h.ndim != 2 or not 1 <= h.shape[0] <= BEAM_MAX_CHANNELS or not 1 <= h.shape[1] <= FIR_MAX_TAPS:
            raise ValueError(f"beam taps must have shape (C, M) with C in 1..{BEAM_MAX_CHANNELS} and M in 1..{FIR_MAX_TAPS}, "
                             f"got shape {h.shape}")
        with self._lock:
            check(lib().sdrk_plan_set_beam(self.handle, int(h.shape[0]), int(h.shape[1]), h.ctypes.data_as(c_void_p)))
            self.beam_channels, self.beam_taps = int(h.shape[0]), int(h.shape[1])
        return self.beam_channels

    def _beam_ready(self) -> int:
        self._float32_only("beamforming")
        if self.beam_channels < 1:
            raise ValueError("no beam filters set: call set_beam(taps) first")
        return self.beam_taps

    def _beam_input(self, iq, prefix, kind: str):
        """``iq`` and ``prefix`` as the arrays the C entry of ``kind`` ("", "_ci16", "_ci8") takes: ``(n, C)`` complex64 or
        ``(n, C, 2)`` integers with the plan's C, checked and (integers) never converted."""
        m, c = self._beam_ready(), self.beam_channels

        def one(a, what):
            if kind == "":
                x = np.asarray(a)
                if x.ndim != 2 or not np.issubdtype(x.dtype, np.complexfloating):
                    raise ValueError(f"beam {what} must be a complex (n, C) array, got shape {x.shape} {x.dtype}")
                x = _as_c64(x)
            else:
                dtypes, name = ((np.int16,), "int16") if kind == "_ci16" else ((np.int8, np.uint8), "int8 or uint8")
                if not isinstance(a, np.ndarray) or a.dtype not in dtypes:
                    raise ValueError(f"beam {what} must be a numpy {name} array, got {getattr(a, 'dtype', type(a).__name__)}")
                if a.ndim != 3 or a.shape[2] != 2:
                    raise ValueError(f"beam {what} must have shape (n, C, 2) (channel, then I, Q), got {a.shape}")
                if not a.flags.c_contiguous:
                    raise ValueError(f"beam {what} must be C-contiguous (I0 Q0 I1 Q1 ... per element)")
                x = a
            if x.shape[1] != c:
                raise ValueError(f"beam {what} has {x.shape[1]} channels, the plan's beam filters have {c}")
            return x

        x = one(iq, "input")
        pre = None
        if prefix is not None and m > 1:
            pre = one(prefix, "prefix")
            if pre.dtype != x.dtype:
                raise ValueError(f"beam prefix must have the dtype of iq ({x.dtype}), got {pre.dtype}")
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} elements before iq, got {pre.shape[0]}")
        return x, pre

    def beam(self, iq, freq_word: int = 0, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """Filter-and-sum beamformer on ``(n, C)`` complex64 elements (one sample of each of the plan's C channels): every
        channel filtered by its own row of ``set_beam``'s taps, the sum tuned by ``freq_word`` and decimated by ``decim`` as
        ``ddc`` does it, in one pass.  With C = 1 the bits of ``ddc`` with that row as the FIR filter."""
        x, pre = self._beam_input(iq, prefix, "")
        return self._host_ddc("sdrk_exec_host_beam", x, pre, freq_word, decim, sample0)

    def beam_ci16(self, iq, freq_word: int = 0, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``beam`` on int16 elements of shape ``(n, C, 2)``: the bits of ``beam`` on the widened elements."""
        x, pre = self._beam_input(iq, prefix, "_ci16")
        return self._host_ddc("sdrk_exec_host_beam_ci16", x, pre, freq_word, decim, sample0)

    def beam_ci8(self, iq, freq_word: int = 0, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``beam`` on 8-bit elements of shape ``(n, C, 2)``, int8 (ci8) or uint8 (cu8) — the dtype is the format: the bits of
        ``beam`` on ``iq8_to_c64(iq)``; without a prefix a uint8 stream starts from M - 1 elements of byte 128."""
        x, pre = self._beam_input(iq, prefix, "_ci8")
        return self._host_ddc("sdrk_exec_host_beam_iq8", x, pre, freq_word, decim, sample0, fmt=_iq8_format(x))

    def beam_outputs(self, n_in: int, decim: int = 1, index0: int = 0) -> int:
        """Samples ``exec_device_beam`` writes for ``n_in`` input elements (``sdrk_ddc_outputs`` with the beam's taps)."""
        m = self._beam_ready()
        if int(n_in) < m:
            raise ValueError(f"n_in={n_in}: a valid convolution needs at least the {m} taps")
        if int(index0) < 0:
            raise ValueError("index0 must be >= 0")
        return int(lib().sdrk_ddc_outputs(c_size_t(int(n_in)), m, _ddc_decim(decim), _ffi.c_uint64(int(index0))))

    def _device_beam_args(self, d_in: int, n_in: int, freq_word: int, decim: int, index0: int, d_out: int, unsigned=None) -> list:
        self.beam_outputs(n_in, decim, index0)
        fmt = [] if unsigned is None else [c_int(IQ8_UNSIGNED if unsigned else IQ8_SIGNED)]
        return [self.handle, c_void_p(d_in), *fmt, c_size_t(int(n_in)), _ffi.c_uint32(_ddc_word(freq_word)), _ddc_decim(decim),
                _ffi.c_uint64(int(index0)), c_void_p(d_out)]

    def exec_device_beam(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, *, decim: int = 1, index0: int = 0,
                         stream: int = 0) -> None:
        """Device pointers, "valid" form: ``n_in`` elements of C complex64 samples in, ``beam_outputs(n_in, decim, index0)``
        complex64 out; asynchronous on ``stream`` (0: the plan's stream)."""
        args = self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out)
        check(lib().sdrk_exec_device_beam(*args, c_void_p(stream) if stream else None))

    def exec_device_beam_ci16(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, *, decim: int = 1, index0: int = 0,
                              stream: int = 0) -> None:
        """``exec_device_beam`` on int16 elements (4 bytes per sample)."""
        args = self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out)
        check(lib().sdrk_exec_device_beam_ci16(*args, c_void_p(stream) if stream else None))

    def exec_device_beam_ci8(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, *, unsigned: bool = False, decim: int = 1,
                             index0: int = 0, stream: int = 0) -> None:
        """``exec_device_beam`` on 8-bit elements (2 bytes per sample; ``unsigned``: cu8, else ci8)."""
        args = self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out, unsigned)
        check(lib().sdrk_exec_device_beam_iq8(*args, c_void_p(stream) if stream else None))

    def _beam_timed(self, sym: str, args: list, launches: int) -> list:
        each = (c_float * max(int(launches), 1))()
        check(getattr(lib(), sym)(*args, int(launches), each))
        return list(each)

    def exec_device_beam_timed_each(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, launches: int = 1, *,
                                    decim: int = 1, index0: int = 0) -> list:
        """``exec_device_beam`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._beam_timed("sdrk_exec_device_beam_timed_each",
                                self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out), launches)

    def exec_device_beam_ci16_timed_each(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, launches: int = 1, *,
                                         decim: int = 1, index0: int = 0) -> list:
        """``exec_device_beam_ci16`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._beam_timed("sdrk_exec_device_beam_ci16_timed_each",
                                self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out), launches)

    def exec_device_beam_ci8_timed_each(self, d_in: int, n_in: int, d_out: int, freq_word: int = 0, launches: int = 1, *,
                                        unsigned: bool = False, decim: int = 1, index0: int = 0) -> list:
        """``exec_device_beam_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        return self._beam_timed("sdrk_exec_device_beam_iq8_timed_each",
                                self._device_beam_args(d_in, n_in, freq_word, decim, index0, d_out, unsigned), launches)

    # -- digital down-converter: the two calls above tuned by a 32-bit frequency word, decimated by any integer 1..256 ------
    def _ddc_input(self, iq, prefix, ci16: bool):
        m = self._fir_ready()
        x = _as_ci16(iq, stream=True) if ci16 else _as_c64(iq).reshape(-1)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_ci16(prefix, stream=True) if ci16 else _as_c64(prefix).reshape(-1)
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return x, pre

    def _ddc_input_ci8(self, iq, prefix):
        m = self._fir_ready()
        x = _as_ci8(iq, stream=True)
        pre = None
        if prefix is not None and m > 1:
            pre = _as_ci8(prefix, stream=True)
            if pre.dtype != x.dtype:
                raise ValueError(f"8-bit I,Q prefix must have the dtype of iq ({x.dtype}), got {pre.dtype}")
            if pre.shape[0] != m - 1:
                raise ValueError(f"prefix must hold the {m - 1} samples before iq, got {pre.shape[0]}")
        return x, pre

    def _host_ddc(self, sym: str, x: np.ndarray, prefix, word, decim: int, sample0: int, fmt: Optional[int] = None) -> np.ndarray:
        decim, word = _ddc_decim(decim), _ddc_word(word)
        if int(sample0) < 0:
            raise ValueError("sample0 must be >= 0")
        n = int(x.shape[0])
        out = np.empty((n + decim - 1) // decim, dtype=np.complex64)
        n_out = c_size_t(0)
        samples = [x.ctypes.data_as(c_void_p)] if fmt is None else [x.ctypes.data_as(c_void_p), c_int(fmt)]   # (8-bit: the format)
        with self._lock:
            check(getattr(lib(), sym)(self.handle, prefix.ctypes.data_as(c_void_p) if prefix is not None else None,
                                      *samples, c_size_t(n), _ffi.c_uint32(word), decim,
                                      _ffi.c_uint64(int(sample0)), out.ctypes.data_as(c_void_p), byref(n_out)))
        return out[: n_out.value]

    def ddc(self, iq, freq_word: int, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """Tune, filter and decimate one piece of a complex64 stream as a digital down-converter does: ``fir`` with the tuning
        given as a 32-bit frequency word (``int32(freq_word) / 2^32`` cycles per sample: ``spectrum.freq_word`` makes one from
        hertz) and ``decim`` ANY integer in 1..256.  The filter is centred on the nearest bin of 4096, the signal at the tuned
        frequency lands at DC exactly, and of the outputs those whose stream index ``sample0 + j`` is a multiple of ``decim``
        are returned — none, if the piece holds none."""
        x, pre = self._ddc_input(iq, prefix, False)
        return self._host_ddc("sdrk_exec_host_ddc", x, pre, freq_word, decim, sample0)

    def ddc_ci16(self, iq, freq_word: int, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``ddc`` on interleaved int16 I,Q of shape ``(n, 2)`` (``prefix``: ``(M - 1, 2)`` int16): the bits of ``ddc`` on the
        widened samples."""
        x, pre = self._ddc_input(iq, prefix, True)
        return self._host_ddc("sdrk_exec_host_ddc_ci16", x, pre, freq_word, decim, sample0)

    def _host_ddc_bank(self, sym: str, x: np.ndarray, prefix, freq_words, decim: int, sample0: int,
                       fmt: Optional[int] = None) -> np.ndarray:
        decim, words = _ddc_decim(decim), _ddc_words(freq_words)
        if int(sample0) < 0:
            raise ValueError("sample0 must be >= 0")
        n = int(x.shape[0])
        stride = (n + decim - 1) // decim
        out = np.empty((len(words), stride), dtype=np.complex64)
        n_out = c_size_t(0)
        samples = [x.ctypes.data_as(c_void_p)] if fmt is None else [x.ctypes.data_as(c_void_p), c_int(fmt)]   # (8-bit: the format)
        with self._lock:
            check(getattr(lib(), sym)(self.handle, prefix.ctypes.data_as(c_void_p) if prefix is not None else None,
                                      *samples, c_size_t(n), len(words), words, decim,
                                      _ffi.c_uint64(int(sample0)), out.ctypes.data_as(c_void_p), c_size_t(stride), byref(n_out)))
        return np.ascontiguousarray(out[:, : n_out.value])

    def ddc_bank(self, iq, freq_words, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``ddc`` for ``C = len(freq_words)`` channels at once (1..64, duplicates allowed), from ONE pass over ``iq``: row ``c``
        of the ``(C, n_out)`` complex64 result carries the bits of ``ddc(iq, freq_words[c], decim=decim, prefix=prefix,
        sample0=sample0)``."""
        x, pre = self._ddc_input(iq, prefix, False)
        return self._host_ddc_bank("sdrk_exec_host_ddcbank", x, pre, freq_words, decim, sample0)

    def ddc_bank_ci16(self, iq, freq_words, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``ddc_bank`` on interleaved int16 I,Q of shape ``(n, 2)``: the bits of ``ddc_bank`` on the widened samples."""
        x, pre = self._ddc_input(iq, prefix, True)
        return self._host_ddc_bank("sdrk_exec_host_ddcbank_ci16", x, pre, freq_words, decim, sample0)

    def ddc_ci8(self, iq, freq_word: int, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``ddc`` on interleaved 8-bit I,Q of shape ``(n, 2)``, int8 (SigMF ci8) or uint8 (cu8) — the dtype is the format —
        read as they are, 2 bytes per sample: the bits of ``ddc`` on ``iq8_to_c64(iq)``.  ``prefix``: ``(M - 1, 2)`` of the same
        dtype; None means bytes of 0 for int8 and of 128 for uint8 (the mid-scale byte: ``+0.5 + 0.5j``; no uint8 byte is zero)."""
        x, pre = self._ddc_input_ci8(iq, prefix)
        return self._host_ddc("sdrk_exec_host_downconv_iq8", x, pre, freq_word, decim, sample0, fmt=_iq8_format(x))

    def ddc_bank_ci8(self, iq, freq_words, *, decim: int = 1, prefix=None, sample0: int = 0) -> np.ndarray:
        """``ddc_bank`` on interleaved 8-bit I,Q of shape ``(n, 2)`` (int8 or uint8, as ``ddc_ci8``): the bits of ``ddc_bank`` on
        the widened samples."""
        x, pre = self._ddc_input_ci8(iq, prefix)
        return self._host_ddc_bank("sdrk_exec_host_downconvbank_iq8", x, pre, freq_words, decim, sample0, fmt=_iq8_format(x))

    def ddc_outputs(self, n_in: int, decim: int = 1, index0: int = 0) -> int:
        """Samples ``exec_device_ddc`` writes for ``n_in`` input samples whose first valid output has stream index ``index0``:
        the ``i`` in ``0 .. n_in - M`` with ``(index0 + i) % decim == 0`` (``sdrk_ddc_outputs``)."""
        m = self._fir_ready()
        if int(n_in) < m:
            raise ValueError(f"n_in={n_in}: a valid convolution needs at least the {m} taps")
        if int(index0) < 0:
            raise ValueError("index0 must be >= 0")
        return int(lib().sdrk_ddc_outputs(c_size_t(int(n_in)), m, _ddc_decim(decim), _ffi.c_uint64(int(index0))))

    def _device_ddc_args(self, d_in: int, n_in: int, freq_word: int, decim: int, index0: int, d_out: int) -> list:
        self.ddc_outputs(n_in, decim, index0)
        return [self.handle, c_void_p(d_in), c_size_t(int(n_in)), _ffi.c_uint32(_ddc_word(freq_word)), _ddc_decim(decim),
                _ffi.c_uint64(int(index0)), c_void_p(d_out)]

    def exec_device_ddc(self, d_in: int, n_in: int, d_out: int, freq_word: int, *, decim: int = 1, index0: int = 0,
                        stream: int = 0) -> None:
        """Device pointers, "valid" form: ``n_in`` complex64 samples in, ``ddc_outputs(n_in, decim, index0)`` complex64 out;
        asynchronous on ``stream`` (0: the plan's stream)."""
        args = self._device_ddc_args(d_in, n_in, freq_word, decim, index0, d_out)
        check(lib().sdrk_exec_device_ddc(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_ci16(self, d_in: int, n_in: int, d_out: int, freq_word: int, *, decim: int = 1, index0: int = 0,
                             stream: int = 0) -> None:
        """``exec_device_ddc`` on int16 I,Q input (4 bytes per sample)."""
        args = self._device_ddc_args(d_in, n_in, freq_word, decim, index0, d_out)
        check(lib().sdrk_exec_device_ddc_ci16(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_timed_each(self, d_in: int, n_in: int, d_out: int, freq_word: int, launches: int = 1, *, decim: int = 1,
                                   index0: int = 0) -> list:
        """``exec_device_ddc`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_ddc_args(d_in, n_in, freq_word, decim, index0, d_out)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_ddc_timed_each(*args, int(launches), each))
        return list(each)

    def _device_ddc_ci8_args(self, args: list, unsigned: bool) -> list:
        """The argument list of a device call with the 8-bit format behind the input pointer."""
        return [*args[:2], c_int(IQ8_UNSIGNED if unsigned else IQ8_SIGNED), *args[2:]]

    def exec_device_ddc_ci8(self, d_in: int, n_in: int, d_out: int, freq_word: int, *, unsigned: bool = False, decim: int = 1,
                            index0: int = 0, stream: int = 0) -> None:
        """``exec_device_ddc`` on 8-bit I,Q input (2 bytes per sample; ``unsigned``: cu8, else ci8)."""
        args = self._device_ddc_ci8_args(self._device_ddc_args(d_in, n_in, freq_word, decim, index0, d_out), unsigned)
        check(lib().sdrk_exec_device_downconv_iq8(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_ci8_timed_each(self, d_in: int, n_in: int, d_out: int, freq_word: int, launches: int = 1, *,
                                       unsigned: bool = False, decim: int = 1, index0: int = 0) -> list:
        """``exec_device_ddc_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_ddc_ci8_args(self._device_ddc_args(d_in, n_in, freq_word, decim, index0, d_out), unsigned)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_downconv_iq8_timed_each(*args, int(launches), each))
        return list(each)

    def _device_ddc_bank_args(self, d_in: int, n_in: int, d_out: int, freq_words, decim: int, index0: int, out_stride) -> list:
        words = _ddc_words(freq_words)
        n_out = self.ddc_outputs(n_in, decim, index0)
        stride = n_out if out_stride is None else int(out_stride)
        if stride < n_out:
            raise ValueError(f"out_stride={stride}: a plane holds the {n_out} outputs of a channel")
        return [self.handle, c_void_p(d_in), c_size_t(int(n_in)), len(words), words, _ddc_decim(decim), _ffi.c_uint64(int(index0)),
                c_void_p(d_out), c_size_t(stride)]

    def exec_device_ddc_bank(self, d_in: int, n_in: int, d_out: int, freq_words, *, decim: int = 1, index0: int = 0,
                             out_stride: Optional[int] = None, stream: int = 0) -> None:
        """Device pointers: ``exec_device_ddc`` for ``len(freq_words)`` channels from one pass.  Plane ``c`` starts at
        ``d_out + 8 * c * out_stride`` (default: packed, ``ddc_outputs(n_in, decim, index0)`` apart) and carries the bits of
        ``exec_device_ddc(..., freq_words[c])``; asynchronous on ``stream`` (0: the plan's stream)."""
        args = self._device_ddc_bank_args(d_in, n_in, d_out, freq_words, decim, index0, out_stride)
        check(lib().sdrk_exec_device_ddcbank(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_bank_ci16(self, d_in: int, n_in: int, d_out: int, freq_words, *, decim: int = 1, index0: int = 0,
                                  out_stride: Optional[int] = None, stream: int = 0) -> None:
        """``exec_device_ddc_bank`` on int16 I,Q input (4 bytes per sample)."""
        args = self._device_ddc_bank_args(d_in, n_in, d_out, freq_words, decim, index0, out_stride)
        check(lib().sdrk_exec_device_ddcbank_ci16(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_bank_timed_each(self, d_in: int, n_in: int, d_out: int, freq_words, launches: int = 1, *, decim: int = 1,
                                        index0: int = 0, out_stride: Optional[int] = None) -> list:
        """``exec_device_ddc_bank`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_ddc_bank_args(d_in, n_in, d_out, freq_words, decim, index0, out_stride)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_ddcbank_timed_each(*args, int(launches), each))
        return list(each)

    def exec_device_ddc_bank_ci8(self, d_in: int, n_in: int, d_out: int, freq_words, *, unsigned: bool = False, decim: int = 1,
                                 index0: int = 0, out_stride: Optional[int] = None, stream: int = 0) -> None:
        """``exec_device_ddc_bank`` on 8-bit I,Q input (2 bytes per sample; ``unsigned``: cu8, else ci8)."""
        args = self._device_ddc_ci8_args(self._device_ddc_bank_args(d_in, n_in, d_out, freq_words, decim, index0, out_stride), unsigned)
        check(lib().sdrk_exec_device_downconvbank_iq8(*args, c_void_p(stream) if stream else None))

    def exec_device_ddc_bank_ci8_timed_each(self, d_in: int, n_in: int, d_out: int, freq_words, launches: int = 1, *,
                                            unsigned: bool = False, decim: int = 1, index0: int = 0,
                                            out_stride: Optional[int] = None) -> list:
        """``exec_device_ddc_bank_ci8`` ``launches`` times on the plan's stream; the milliseconds of each."""
        args = self._device_ddc_ci8_args(self._device_ddc_bank_args(d_in, n_in, d_out, freq_words, decim, index0, out_stride), unsigned)
        each = (c_float * int(launches))()
        check(lib().sdrk_exec_device_downconvbank_iq8_timed_each(*args, int(launches), each))
        return list(each)

    def window_power(self) -> float:
        """``sum(w^2)`` of the plan's window (float64)."""
        if self._wkey == "rect":
            return float(self.nfft)
        if self._wkey == "hann":
            return float(np.sum(np.hanning(self.nfft) ** 2))
        return float(np.sum(np.frombuffer(self._wkey[1], dtype=np.float32).astype(np.float64) ** 2))

    def _welch_streamed(self, m: _Mode, what: str, iq, sample_rate: float, hop: Optional[int]) -> np.ndarray:
        self._float32_only(what)
        x = m.stream(iq)
        rows = self._n_frames(self.nfft, x.shape[0], hop)
        if not rows:
            raise ValueError(f"stream of {x.shape[0]} samples is shorter than one {self.nfft}-sample segment")
        scale = 1.0 / (float(sample_rate) * self.window_power())
        return self._host_integrated(m, x, hop, _Integ(rows, "mean", "power", scale), what=what)[0]

    def welch_psd_streamed(self, iq, sample_rate: float, hop: Optional[int] = None) -> np.ndarray:
        """``welch_psd`` through the integrated path: one group of all full segments, mean, linear power.  No
        ``max_batch`` limit, and the stream is not staged whole on the device."""
        return self._welch_streamed(_C64, "welch_psd_streamed", iq, sample_rate, hop)

    def welch_psd_streamed_ci16(self, iq, sample_rate: float, hop: Optional[int] = None) -> np.ndarray:
        """``welch_psd_streamed`` over an int16 I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples (in
        units of the integer samples: no scale is applied to them)."""
        return self._welch_streamed(_CI16, "welch_psd_streamed_ci16", iq, sample_rate, hop)

    def welch_psd_streamed_ci8(self, iq, sample_rate: float, hop: Optional[int] = None) -> np.ndarray:
        """``welch_psd_streamed`` over an 8-bit I,Q stream ``(n_samples, 2)``, int8 or uint8: the same bits as on the widened
        samples (in units of the integer samples: no scale is applied to them)."""
        return self._welch_streamed(_CI8, "welch_psd_streamed_ci8", iq, sample_rate, hop)

    # -- device pointers (bench / pipelines that keep data resident) -------------
    def exec_device(self, d_iq: int, n_frames: int, d_out: int, *, frame_stride: Optional[int] = None,
                    stream: int = 0) -> None:
        """Device pointers: complex64 in / float32 rows out (complex128 / float64 on a double plan), asynchronous on
        ``stream`` (0: the plan's stream)."""
        stride = self.nfft if frame_stride is None else int(frame_stride)
        fn = lib().sdrk_exec_device_f64 if self._double else lib().sdrk_exec_device
        with self._lock:
            check(fn(self.handle, c_void_p(d_iq), c_size_t(n_frames), c_size_t(stride),
                                         c_void_p(d_out), c_void_p(stream) if stream else None))

    def tune_scratch(self, d_iq: int, n_frames: int, d_out: int, candidates: int = 6, *,
                     frame_stride: Optional[int] = None):
        """Large-frame plans: try ``candidates`` placements of the two-pass scratch on this workload and keep the
        fastest (``sdrk_plan_tune_scratch``).  Returns ``(probe_ms, chosen)``; ``d_out`` is overwritten."""
        self._float32_only("tune_scratch")
        stride = self.nfft if frame_stride is None else int(frame_stride)
        ms, chosen = (c_float * int(candidates))(), c_int(0)
        with self._lock:
            check(lib().sdrk_plan_tune_scratch(self.handle, c_void_p(d_iq), c_size_t(n_frames), c_size_t(stride),
                                               c_void_p(d_out), int(candidates), ms, byref(chosen)))
            self.last_placement = placement_report()
        return [float(v) for v in ms], int(chosen.value)

    def exec_device_timed_each(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                               frame_stride: Optional[int] = None) -> list:
        """Like ``exec_device_timed`` but returns the milliseconds of each launch (events between
        consecutive launches on the plan's stream)."""
        stride = self.nfft if frame_stride is None else int(frame_stride)
        ms = (c_float * int(launches))()
        fn = lib().sdrk_exec_device_f64_timed_each if self._double else lib().sdrk_exec_device_timed_each
        with self._lock:
            check(fn(self.handle, c_void_p(d_iq), c_size_t(n_frames),
                                                    c_size_t(stride), c_void_p(d_out), int(launches), ms))
        return [float(v) for v in ms]

    def exec_device_timed(self, d_iq: int, n_frames: int, d_out: int, launches: int = 1, *,
                          frame_stride: Optional[int] = None) -> float:
        """Run `launches` back-to-back transforms on the plan's stream; milliseconds
        between HIP events recorded on that stream (all launches together)."""
        self._float32_only("exec_device_timed (use exec_device_timed_each)")
        stride = self.nfft if frame_stride is None else int(frame_stride)
        ms = c_float(0.0)
        with self._lock:
            check(lib().sdrk_exec_device_timed(self.handle, c_void_p(d_iq), c_size_t(n_frames),
                                               c_size_t(stride), c_void_p(d_out), int(launches), byref(ms)))
        return float(ms.value)

    def sync(self) -> None:
        check(lib().sdrk_plan_sync(self.handle))

    def fused_status(self) -> dict:
        """``nfft = 65536`` plans: ``{"launches": persistent launches made so far, "fallen_back": a launch reported a failed
        hand-over and the plan now takes the two tiled launches}`` (``sdrk_plan_fused_status``); zeros for other plans."""
        n, fb = _ffi.c_uint32(0), c_int(0)
        check(lib().sdrk_plan_fused_status(self.handle, byref(n), byref(fb)))
        return {"launches": int(n.value), "fallen_back": bool(fb.value)}

    def staging_probe(self) -> list:
        """Probe times (ms) of the staging candidates of a ``tune_staging=True`` plan, three per chunk slot; ``[]``
        when nothing was tuned."""
        ms, n = (c_float * 16)(), c_int(0)
        check(lib().sdrk_plan_staging_probe(self.handle, ms, 16, byref(n)))
        return [float(ms[i]) for i in range(min(int(n.value), 16))]


def placement_report() -> dict:
    """What the last placement probe on this thread did (``sdrk_placement_report``): the warm-up, candidate 0 as first timed
    and as timed again after the last candidate, the kept candidate's time (ms); ``gain_vs_retimed_first`` is what the kept
    candidate saves against candidate 0 measured WARM — the honest figure (a first timing taken before the shader clock had
    ramped up would credit the ramp to the placement)."""
    warm, n, first, again, kept = c_float(0), c_int(0), c_float(0), c_float(0), c_float(0)
    tried = int(lib().sdrk_placement_report(byref(warm), byref(n), byref(first), byref(again), byref(kept)))
    rec = {"candidates_tried": tried, "warmup_ms": round(float(warm.value), 2), "warmup_launches": int(n.value),
           "first_ms": round(float(first.value), 4), "retimed_first_ms": round(float(again.value), 4),
           "chosen_ms": round(float(kept.value), 4)}
    rec["gain_vs_retimed_first"] = (round(1.0 - kept.value / again.value, 4) if again.value > 0 and kept.value > 0 else None)
    return rec


# ---- plan cache for the function API -------------------------------------------
_plans: dict = {}
_plans_lock = threading.Lock()


def _cached_plan(nfft: int, window: WindowArg, eps: float, shift: bool, device: int,
                 precision: str = "single") -> SpectrumPlan:
    if precision == "double":
        _check_double_nfft(int(nfft))
    _, _, wkey = _window_spec(window, nfft, np.float64 if precision == "double" else np.float32)
    key = (int(device), int(nfft), wkey, float(eps), bool(shift), precision)
    plan = _plans.get(key)                      # (dict.get is atomic; the lock is only for creation)
    if plan is not None:
        return plan
    with _plans_lock:
        plan = _plans.get(key)
        if plan is None:
            plan = SpectrumPlan(nfft, window=window, eps=eps, shift=shift, device=device, precision=precision)
            _plans[key] = plan
        return plan


def clear_plan_cache() -> None:
    with _plans_lock:
        for p in list(_plans.values()) + list(_real_plans.values()):
            p.close()
        _plans.clear()
        _real_plans.clear()


def _nfft_of(samples) -> int:
    shape = np.shape(samples)
    if len(shape) not in (1, 2):
        raise ValueError(f"expected a frame (N,) or a batch (B, N), got shape {shape}")
    return int(shape[-1])


def _no_sharding(precision: str, devices) -> None:
    if precision == "double" and devices is not None:
        raise ValueError("devices=[...] (multi-GPU sharding) is float32 only; use device= with precision='double'")


def spectrum_db(samples, *, window: WindowArg = None, eps: float = 1e-12, shift: bool = True,
                device: int = 0, devices: Optional[Sequence[int]] = None,
                out: Optional[np.ndarray] = None, pin="auto", precision: str = "single") -> np.ndarray:
    """Power spectrum in dB of one frame ``(N,)`` or a batch ``(B, N)`` of complex IQ.

    Equivalent to ``20*np.log10(np.abs(np.fft.fftshift(np.fft.fft(samples*window, axis=-1),
    axes=-1)) + eps)`` in float32 — with the defaults, exactly the reference's
    ``power_db`` (app/sdr/streamer.py:119,121).  ``devices=[0,1,...]`` splits a
    batch into contiguous frame ranges, one per GPU (no collectives; see
    sharding.py).  ``out``: a float32 array of the result's shape to fill instead of
    allocating (large batches: reusing it saves the page faults and the munmap of a
    fresh result per call).  ``pin`` (with ``devices``): how pageable arrays reach several GPUs — ``"auto"`` stages
    them until reuse has paid for page-locking them (sharding.spectrum_db_sharded, hostmem.plan_pinning).
    ``precision``: ``"single"`` (complex64 -> float32), ``"double"`` (complex128 -> float64, the reference's dtypes) or
    ``"auto"`` (by the input's dtype, as numpy's FFT decides).
    """
    nfft = _nfft_of(samples)
    precision = resolve_precision(precision, samples)
    _no_sharding(precision, devices)
    if precision == "double":
        return _cached_plan(nfft, window, eps, shift, device, "double").spectrum_db(samples, out=out)
    if devices is not None and len(devices) > 1 and np.ndim(samples) == 2:
        from .sharding import spectrum_db_sharded
        return spectrum_db_sharded(samples, devices, window=window, eps=eps, shift=shift, out=out, pin=pin)
    if devices is not None and len(devices) == 1:
        device = devices[0]
    return _cached_plan(nfft, window, eps, shift, device).spectrum_db(samples, out=out)


def fft_c64(samples, *, window: WindowArg = None, shift: bool = False, device: int = 0) -> np.ndarray:
    """complex64 ``np.fft.fft(samples*window, axis=-1)`` (streamer.py:119 without the
    log), optionally fftshifted."""
    nfft = _nfft_of(samples)
    return _cached_plan(nfft, window, 1e-12, shift, device).fft(samples)


def spectrum_db_ci16(iq, *, window: WindowArg = None, eps: float = 1e-12, shift: bool = True, device: int = 0,
                     out: Optional[np.ndarray] = None) -> np.ndarray:
    """``spectrum_db`` for int16 I,Q frames ``(N, 2)`` or ``(B, N, 2)`` as the radio delivers them (the AD936x behind
    app/sdr/streamer.py:114; SigMF ``ci16_le``): float32 rows with exactly the bits of
    ``spectrum_db((iq[..., 0] + 1j*iq[..., 1]).astype(complex64))``, from half the input bytes.  No scaling to full scale;
    one device (no ``devices=[...]``)."""
    x = _as_ci16(iq)
    return _cached_plan(int(x.shape[-2]), window, eps, shift, device).spectrum_db_ci16(x, out=out)


def fft_ci16(iq, *, window: WindowArg = None, shift: bool = False, device: int = 0) -> np.ndarray:
    """``fft_c64`` for int16 I,Q frames ``(N, 2)`` or ``(B, N, 2)``: the same bits as on the widened samples."""
    x = _as_ci16(iq)
    return _cached_plan(int(x.shape[-2]), window, 1e-12, shift, device).fft_ci16(x)


def stft_db_ci16(iq, nfft: int, hop: Optional[int] = None, window: WindowArg = None, *, eps: float = 1e-12,
                 shift: bool = True, device: int = 0) -> np.ndarray:
    """``stft_db`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same rows, bit for bit."""
    x = _as_ci16(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).stft_db_ci16(x, hop)


def spectrum_db_ci8(iq, *, window: WindowArg = None, eps: float = 1e-12, shift: bool = True, device: int = 0,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
    """``spectrum_db`` for 8-bit I,Q frames ``(N, 2)`` or ``(B, N, 2)``: int8 (SigMF ``ci8``, a HackRF) or uint8 (``cu8``, an
    RTL-SDR; mid-scale 127.5) — the dtype is the format.  float32 rows with exactly the bits of
    ``spectrum_db(iq8_to_c64(iq))``, from a quarter of the input bytes.  No scaling to full scale; one device."""
    x = _as_ci8(iq)
    return _cached_plan(int(x.shape[-2]), window, eps, shift, device).spectrum_db_ci8(x, out=out)


def fft_ci8(iq, *, window: WindowArg = None, shift: bool = False, device: int = 0) -> np.ndarray:
    """``fft_c64`` for 8-bit I,Q frames ``(N, 2)`` or ``(B, N, 2)``: the same bits as on the widened samples."""
    x = _as_ci8(iq)
    return _cached_plan(int(x.shape[-2]), window, 1e-12, shift, device).fft_ci8(x)


def stft_db_ci8(iq, nfft: int, hop: Optional[int] = None, window: WindowArg = None, *, eps: float = 1e-12,
                shift: bool = True, device: int = 0) -> np.ndarray:
    """``stft_db`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)``: the same rows, bit for bit."""
    x = _as_ci8(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).stft_db_ci8(x, hop)


def integrated_db_ci8(iq, nfft: int, k: int, hop: Optional[int] = None, detector: str = "mean", window: WindowArg = None,
                      eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """``integrated_db`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)``: the same rows, bit for bit, as on
    ``iq8_to_c64(iq)``, from a quarter of the input bytes."""
    x = _as_ci8(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).integrate_ci8(x, k, hop, detector, "db")


def welch_psd_streamed_ci8(iq, nfft: int, sample_rate: float, hop: Optional[int] = None, window: WindowArg = "hann",
                           shift: bool = True, device: int = 0) -> np.ndarray:
    """``welch_psd_streamed`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples."""
    x = _as_ci8(iq, stream=True)
    return _cached_plan(int(nfft), window, 1e-12, shift, device).welch_psd_streamed_ci8(x, sample_rate, hop)


def fft_c128(samples, *, window: WindowArg = None, shift: bool = False, device: int = 0) -> np.ndarray:
    """complex128 ``np.fft.fft(samples*window, axis=-1)`` computed in double (streamer.py:119 in the reference's own
    dtype), optionally fftshifted; powers of two 2 ... 2^22."""
    nfft = _nfft_of(samples)
    return _cached_plan(nfft, window, 1e-12, shift, device, "double").fft(samples)


_real_plans: dict = {}


def _cached_real_plan(nfft_real: int, window: WindowArg, eps: float, device: int) -> SpectrumPlan:
    """A plan of ``nfft_real // 2`` with the real window set: its own cache, since the real window is state of the plan."""
    nfft_real = int(nfft_real)
    if nfft_real < 32 or nfft_real & (nfft_real - 1):
        raise ValueError(f"nfft_real={nfft_real}: real frames are powers of two 32 ... 2^21 samples long")
    w = _real_window(window, nfft_real)
    key = (int(device), nfft_real, None if w is None else w.tobytes(), float(eps))
    with _plans_lock:
        plan = _real_plans.get(key)
        if plan is None:
            plan = SpectrumPlan(nfft_real // 2, eps=eps, shift=False, device=device)
            if w is not None:
                plan.set_real_window(w)
            if len(_real_plans) >= 8:
                for p in _real_plans.values():
                    p.close()
                _real_plans.clear()
            _real_plans[key] = plan
        return plan


def rspectrum_db(x, nfft_real: int, window: WindowArg = None, *, eps: float = 1e-12, device: int = 0,
                 out: Optional[np.ndarray] = None) -> np.ndarray:
    """One-sided power spectrum in dB of real-sampled frames ``(frames, nfft_real)`` (or flat): float32
    ``20*log10(|np.fft.rfft(x*window, axis=-1)| + eps)``, ``nfft_real // 2 + 1`` bins from 0 to fs/2.  ``x`` is float32,
    int16, int8 or uint8 (``v - 127.5``) — SigMF rf32_le / ri16_le / ri8 / ru8 — read as it is; ``window``: None, ``"hann"``
    or ``nfft_real`` coefficients."""
    x = _as_real(x, int(nfft_real))
    return _cached_real_plan(nfft_real, window, eps, device).rspectrum_db(x, out=out)


def rfft(x, nfft_real: int, window: WindowArg = None, *, device: int = 0) -> np.ndarray:
    """complex64 ``np.fft.rfft(x*window, axis=-1)`` of real-sampled frames; shapes and dtypes as ``rspectrum_db``."""
    x = _as_real(x, int(nfft_real))
    return _cached_real_plan(nfft_real, window, 1e-12, device).rfft(x)


def rintegrated_db(x, nfft_real: int, k: int, hop: Optional[int] = None, detector: str = "mean", window: WindowArg = None,
                   eps: float = 1e-12, device: int = 0) -> np.ndarray:
    """dB rows of a one-sided spectrogram whose time axis is reduced on the device: one row of ``nfft_real // 2 + 1`` bins per
    ``k`` frames of the flat real-sampled stream ``x``, the mean / max / min power per bin (``SpectrumPlan.rintegrate``)."""
    x = _as_real(x, int(nfft_real), stream=True)
    hop = _real_hop(hop, int(nfft_real))
    if int(k) < 1:
        raise ValueError("k must be >= 1")
    return _cached_real_plan(nfft_real, window, eps, device).rintegrate(x, k, hop, detector, "db")


def rwelch_psd(x, nfft_real: int, sample_rate: float, hop: Optional[int] = None, window: WindowArg = "hann", *,
               device: int = 0) -> np.ndarray:
    """Linear one-sided PSD (power per Hz) of one flat real-sampled stream as ``matplotlib.mlab.psd`` computes it for real
    input (no detrend): float32 ``(nfft_real // 2 + 1,)``, the mean over all ``1 + (len - nfft_real)//hop`` full segments of
    ``|rfft(w*x_r)|^2 / (sample_rate * sum(w^2))`` with the interior bins ``1 ... nfft_real/2 - 1`` doubled.  Transforms and
    averaging run inside one kernel pass on the device; the doubling is done here on the returned row."""
    n = int(nfft_real)
    x = _as_real(x, n, stream=True)
    hop = _real_hop(hop, n)
    plan = _cached_real_plan(n, window, 1e-12, device)
    rows = plan.rintegrated_groups(x.shape[0], 1, hop)
    if rows < 1:
        raise ValueError(f"stream of {x.shape[0]} samples is shorter than one {n}-sample segment")
    w = _real_window(window, n)
    wss = float(n) if w is None else float(np.sum(w.astype(np.float64) ** 2))
    row = plan.rintegrate(x, rows, hop, "mean", "power", 1.0 / (float(sample_rate) * wss))[0]
    row[1:n // 2] *= np.float32(2.0)
    return row


def rfreq_axis(nfft_real: int, sample_rate: float, center_freq: float = 0.0) -> np.ndarray:
    """float64 frequency axis in Hz of the one-sided rows: bin k of ``nfft_real // 2 + 1`` at ``k * sample_rate / nfft_real
    + center_freq`` — ``np.fft.rfftfreq(nfft_real, 1/sample_rate) + center_freq`` with the same float operations."""
    n = int(nfft_real)
    if n < 2 or n % 2:
        raise ValueError("nfft_real must be even and >= 2")
    val = 1.0 / (n * (1 / sample_rate))
    return np.arange(0, n // 2 + 1, dtype=int) * val + center_freq


def freq_axis(n: int, sample_rate: float, center_freq: float = 0.0) -> np.ndarray:
    """float64 frequency axis in Hz, bit-identical to the reference's
    ``np.fft.fftshift(np.fft.fftfreq(n, 1/sample_rate)) + center_freq``
    (app/sdr/streamer.py:120): the same float operations in the same order —
    ``val = 1/(n*d)`` with ``d = 1/sample_rate``, integer bin index times ``val``,
    plus ``center_freq`` — on the already-shifted index range.  Host-side; it is
    O(n) float64 arithmetic with no kernel."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    key = (n, sample_rate, center_freq)
    cached = _freq_cache.get(key)
    if cached is None:
        d = 1 / sample_rate
        val = 1.0 / (n * d)
        k = np.arange(-(n // 2), (n - 1) // 2 + 1, dtype=int)
        cached = k * val + center_freq
        if len(_freq_cache) >= 8:               # the live app has one (n, fs, fc); keep a few
            _freq_cache.clear()
        _freq_cache[key] = cached
    return cached.copy()                        # a fresh array per call, like the reference's expression


_freq_cache: dict = {}


def process_frame(samples, sample_rate: float, center_freq: float, *, window: WindowArg = None,
                  eps: float = 1e-12, device: int = 0, precision: str = "single") -> dict:
    """One reader-loop iteration of the reference (app/sdr/streamer.py:119-130):
    returns the ``plot_data`` dict with exactly its keys — ``time``, ``samples``
    (the caller's array, same object), ``freqs``, ``power_db``, ``sample_rate``,
    ``center_freq`` — which is what ``update_graphs`` reads
    (app/dashboard/callbacks.py:110-115).  ``precision="auto"`` gives the reference's float64 ``power_db`` for its
    complex128 samples."""
    power_db = spectrum_db(samples, window=window, eps=eps, shift=True, device=device, precision=precision)
    freqs = freq_axis(len(samples), sample_rate, center_freq)
    return {
        "time": time.time(),
        "samples": samples,
        "freqs": freqs,
        "power_db": power_db,
        "sample_rate": sample_rate,
        "center_freq": center_freq,
    }


def welch_psd(iq, nfft: int, sample_rate: float, hop: Optional[int] = None, window: WindowArg = "hann", *,
              shift: bool = True, device: int = 0) -> np.ndarray:
    """Linear two-sided PSD (power per Hz) as ``matplotlib.mlab.psd`` computes it for the
    reference's offline plots (scripts/process_sigmf_data.py:188-189: NFFT=1024, Hann,
    noverlap=0).  Returns float32 ``(nfft,)`` in fftshift order (use ``freq_axis`` for x)."""
    return _cached_plan(int(nfft), window, 1e-12, shift, device).welch_psd(iq, sample_rate, hop)


def integrated_db(iq, nfft: int, k: int, hop: Optional[int] = None, detector: str = "mean", window: WindowArg = None,
                  eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """dB rows of a spectrogram whose time axis is reduced on the device: one row per ``k`` frames of ``iq``, the
    mean / max / min power per bin (``SpectrumPlan.integrate``)."""
    return _cached_plan(int(nfft), window, eps, shift, device).integrate(iq, k, hop, detector, "db")


def welch_psd_streamed(iq, nfft: int, sample_rate: float, hop: Optional[int] = None, window: WindowArg = "hann",
                       shift: bool = True, device: int = 0) -> np.ndarray:
    """``welch_psd`` for streams of any length: the averaging runs inside the transform, chunk by chunk."""
    return _cached_plan(int(nfft), window, 1e-12, shift, device).welch_psd_streamed(iq, sample_rate, hop)


def integrated_db_ci16(iq, nfft: int, k: int, hop: Optional[int] = None, detector: str = "mean", window: WindowArg = None,
                       eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """``integrated_db`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same rows, bit for bit, as on
    ``float32(I) + 1j*float32(Q)``, from half the input bytes."""
    x = _as_ci16(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).integrate_ci16(x, k, hop, detector, "db")


def welch_psd_streamed_ci16(iq, nfft: int, sample_rate: float, hop: Optional[int] = None, window: WindowArg = "hann",
                            shift: bool = True, device: int = 0) -> np.ndarray:
    """``welch_psd_streamed`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples."""
    x = _as_ci16(iq, stream=True)
    return _cached_plan(int(nfft), window, 1e-12, shift, device).welch_psd_streamed_ci16(x, sample_rate, hop)


def _cached_pfb_plan(nfft: int, taps: int, prototype, eps: float, shift: bool, device: int) -> "SpectrumPlan":
    h = pfb_prototype(nfft, taps) if prototype is None else np.ascontiguousarray(np.asarray(prototype, dtype=np.float32))
    if h.shape != (taps * nfft,):
        raise ValueError(f"prototype must have shape ({taps * nfft},), got {h.shape}")
    key = (int(device), nfft, ("pfb", hashlib.sha1(h.tobytes()).digest()), float(eps), bool(shift), "single")
    plan = _plans.get(key)
    if plan is None:
        with _plans_lock:
            plan = _plans.get(key)
            if plan is None:
                plan = SpectrumPlan(nfft, eps=eps, shift=shift, device=device)
                plan.set_pfb(h)
                _plans[key] = plan
    return plan


def _pfb_integrated_db(m: _Mode, iq, nfft, taps, k, hop, detector, prototype, eps, shift, device) -> np.ndarray:
    """The arguments are checked before a plan is made for the prototype."""
    x = m.stream(iq) if m.ci16 or m.iq8 else iq
    if int(k) < 1:
        raise ValueError("k must be >= 1")
    if hop is not None and int(hop) < 1:
        raise ValueError("hop must be >= 1")
    SpectrumPlan._int_codes(detector, "db")
    plan = _cached_pfb_plan(int(nfft), int(taps), prototype, eps, shift, device)
    return plan._host_integrated(m, x, hop, _Integ(k, detector, "db", 1.0))


def pfb_db(iq, nfft: int, taps: int, hop: Optional[int] = None, prototype=None, *, eps: float = 1e-12, shift: bool = True,
           device: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
    """Polyphase-filter-bank dB rows ``(rows, nfft)`` over one contiguous complex64 stream: ``taps`` blocks of ``nfft``
    samples folded under ``prototype`` (``taps*nfft`` float32 coefficients; default ``pfb_prototype(nfft, taps)``) in front
    of the transform, one row per ``hop`` samples (default ``nfft``); ``rows = 1 + (len(iq) - taps*nfft) // hop``.  A plan is
    cached per prototype (``SpectrumPlan.set_pfb`` / ``pfb_db`` for explicit plans)."""
    return _cached_pfb_plan(int(nfft), int(taps), prototype, eps, shift, device).pfb_db(iq, hop, out=out)


def pfb_integrated_db(iq, nfft: int, taps: int, k: int, hop: Optional[int] = None, detector: str = "mean", prototype=None, *,
                      eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """dB rows of a polyphase-filter-bank spectrometer: one row per ``k`` folded frames of ``iq``, the mean / max / min
    power per bin (``SpectrumPlan.pfb_integrate``); prototype and plan cache as for ``pfb_db``."""
    return _pfb_integrated_db(_PFB, iq, nfft, taps, k, hop, detector, prototype, eps, shift, device)


def pfb_db_ci16(iq, nfft: int, taps: int, hop: Optional[int] = None, prototype=None, *, eps: float = 1e-12,
                shift: bool = True, device: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``pfb_db`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same rows, bit for bit, as on
    ``float32(I) + 1j*float32(Q)``, from half the input bytes; prototype and plan cache as for ``pfb_db``."""
    x = _as_ci16(iq, stream=True)
    return _cached_pfb_plan(int(nfft), int(taps), prototype, eps, shift, device).pfb_db_ci16(x, hop, out=out)


def pfb_integrated_db_ci16(iq, nfft: int, taps: int, k: int, hop: Optional[int] = None, detector: str = "mean",
                           prototype=None, *, eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """``pfb_integrated_db`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same rows, bit for bit, as on the
    widened samples, from half the input bytes."""
    return _pfb_integrated_db(_PFB_CI16, iq, nfft, taps, k, hop, detector, prototype, eps, shift, device)


def pfb_db_ci8(iq, nfft: int, taps: int, hop: Optional[int] = None, prototype=None, *, eps: float = 1e-12,
               shift: bool = True, device: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``pfb_db`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 (ci8) or uint8 (cu8): the same rows, bit for
    bit, as on ``iq8_to_c64(iq)``, from a quarter of the input bytes; prototype and plan cache as for ``pfb_db``."""
    x = _as_ci8(iq, stream=True)
    return _cached_pfb_plan(int(nfft), int(taps), prototype, eps, shift, device).pfb_db_ci8(x, hop, out=out)


def pfb_integrated_db_ci8(iq, nfft: int, taps: int, k: int, hop: Optional[int] = None, detector: str = "mean",
                          prototype=None, *, eps: float = 1e-12, shift: bool = True, device: int = 0) -> np.ndarray:
    """``pfb_integrated_db`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 or uint8: the same rows, bit for
    bit, as on ``iq8_to_c64(iq)``, from a quarter of the input bytes."""
    return _pfb_integrated_db(_PFB_CI8, iq, nfft, taps, k, hop, detector, prototype, eps, shift, device)


def sk_limits(k: int, sigmas: float = 3.0):
    """``(lo, hi) = 1 -/+ sigmas * sqrt(4k^2 / ((k-1)(k+2)(k+3)))``: the band around 1 in which the spectral kurtosis of
    Gaussian noise over ``k`` frames lies (its standard deviation, Nita & Gary); bins outside are flagged as interference."""
    k = int(k)
    if k < 2:
        raise ValueError("k must be >= 2")
    sd = float(np.sqrt(4.0 * k * k / ((k - 1.0) * (k + 2.0) * (k + 3.0))))
    return 1.0 - float(sigmas) * sd, 1.0 + float(sigmas) * sd


def spectral_kurtosis(iq, nfft: int, k: int, hop: Optional[int] = None, window: WindowArg = None, *, out: str = "db",
                      scale: float = 1.0, eps: float = 1e-12, shift: bool = True, device: int = 0):
    """``(mean_rows, sk_rows)`` per ``k >= 2`` frames of ``iq``: the mean power and the spectral kurtosis estimator per bin,
    both accumulated on the device in one pass (``SpectrumPlan.spectral_kurtosis``)."""
    return _cached_plan(int(nfft), window, eps, shift, device).spectral_kurtosis(iq, k, hop, out, scale)


def spectral_kurtosis_ci16(iq, nfft: int, k: int, hop: Optional[int] = None, window: WindowArg = None, *, out: str = "db",
                           scale: float = 1.0, eps: float = 1e-12, shift: bool = True, device: int = 0):
    """``spectral_kurtosis`` over one contiguous int16 I,Q stream ``(n_samples, 2)``: the same bits as on the widened samples."""
    x = _as_ci16(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).spectral_kurtosis_ci16(x, k, hop, out, scale)


def spectral_kurtosis_ci8(iq, nfft: int, k: int, hop: Optional[int] = None, window: WindowArg = None, *, out: str = "db",
                          scale: float = 1.0, eps: float = 1e-12, shift: bool = True, device: int = 0):
    """``spectral_kurtosis`` over one contiguous 8-bit I,Q stream ``(n_samples, 2)`` int8 (ci8) or uint8 (cu8): the same bits
    as on ``iq8_to_c64(iq)``."""
    x = _as_ci8(iq, stream=True)
    return _cached_plan(int(nfft), window, eps, shift, device).spectral_kurtosis_ci8(x, k, hop, out, scale)


def pfb_spectral_kurtosis(iq, nfft: int, taps: int, k: int, hop: Optional[int] = None, prototype=None, *, out: str = "db",
                          scale: float = 1.0, eps: float = 1e-12, shift: bool = True, device: int = 0):
    """``spectral_kurtosis`` of the polyphase-filter-bank frames of ``pfb_db`` (complex64, or ``(n_samples, 2)`` int16 I,Q or
    int8 / uint8 I,Q); prototype and plan cache as for ``pfb_db``.  The arguments are checked before a plan is made for the
    prototype."""
    dt = iq.dtype if isinstance(iq, np.ndarray) else None
    m = _PFB_CI16 if dt == np.int16 else _PFB_CI8 if dt in (np.int8, np.uint8) else _PFB
    x = iq if m is _PFB else m.stream(iq)
    if int(k) < 2:
        raise ValueError("k must be >= 2")
    if hop is not None and int(hop) < 1:
        raise ValueError("hop must be >= 1")
    SpectrumPlan._int_codes("mean", out, True)
    plan = _cached_pfb_plan(int(nfft), int(taps), prototype, eps, shift, device)
    return plan._host_sk(m, x, k, hop, out, scale)


def cross_spectrum(a, b, nfft: int, k: int, hop: Optional[int] = None, window: WindowArg = None, *, scale: float = 1.0,
                   shift: bool = True, device: int = 0) -> CrossSpectrum:
    """The ``CrossSpectrum`` of two coherent channels per ``k`` frames of ``nfft`` samples, accumulated on the device in one
    pass (``SpectrumPlan.cross_spectrum``).  ``a`` and ``b`` are equal-length complex arrays, or two ``(n, 2)`` int16 I,Q
    arrays (the int16 form: the same bits from half the bytes); they are stacked into one element stream, a copy of both."""
    plan = _cached_plan(int(nfft), window, 1e-12, shift, device)
    if isinstance(a, np.ndarray) and a.dtype == np.int16:
        return plan.cross_spectrum_ci16((a, b), k, hop, scale)
    return plan.cross_spectrum((a, b), k, hop, scale)


def correlation_matrix(x, nfft: int, k: int, hop: Optional[int] = None, window: WindowArg = None, scale: float = 1.0, *,
                       shift: bool = True, device: int = 0) -> CorrelationMatrix:
    """The ``CorrelationMatrix`` of ``C`` = 2..8 coherent channels per ``k`` frames of ``nfft`` samples, accumulated on the
    device with every channel transformed once (``SpectrumPlan.correlate``).  ``x`` is an ``(n, C)`` complex array, an
    ``(n, C, 2)`` int16, int8 or uint8 array (the integer forms: the same bits from fewer bytes), or a list of ``C``
    equal-length per-channel arrays, which is stacked into one element stream — a copy of all of them."""
    if isinstance(x, (tuple, list)):
        chans = [np.asarray(c) for c in x]
        if not chans or any(c.shape != chans[0].shape or c.dtype != chans[0].dtype for c in chans):
            raise ValueError("a channel list must hold arrays of one shape and dtype")
        x = np.stack(chans, axis=1)
    plan = _cached_plan(int(nfft), window, 1e-12, shift, device)
    if isinstance(x, np.ndarray) and x.dtype == np.int16:
        return plan.correlate_ci16(x, k, hop, scale)
    if isinstance(x, np.ndarray) and x.dtype in (np.int8, np.uint8):
        return plan.correlate_ci8(x, k, hop, scale)
    return plan.correlate(x, k, hop, scale)


def stft_db(iq, nfft: int, hop: Optional[int] = None, window: WindowArg = None, *, eps: float = 1e-12,
            shift: bool = True, device: int = 0, devices: Optional[Sequence[int]] = None,
            precision: str = "single") -> np.ndarray:
    """Spectrogram rows ``(rows, nfft)`` float32 over one contiguous IQ stream (the
    waterfall of BASELINE.json config 3: nfft=65536, hop=nfft//2).  ``devices=[...]`` splits the
    rows into contiguous ranges, one per GPU, each reading its samples plus an ``nfft-hop`` halo.
    ``precision="double"`` (or ``"auto"`` on complex128 input): float64 rows from complex128 samples, one device."""
    precision = resolve_precision(precision, iq)
    _no_sharding(precision, devices)
    if precision == "double":
        return _cached_plan(int(nfft), window, eps, shift, device, "double").stft_db(iq, hop)
    if devices is not None and len(devices) > 1:
        from .sharding import stft_db_sharded
        return stft_db_sharded(iq, int(nfft), int(nfft if hop is None else hop), devices, window=window, eps=eps,
                               shift=shift)
    if devices is not None and len(devices) == 1:
        device = devices[0]
    return _cached_plan(int(nfft), window, eps, shift, device).stft_db(iq, hop)


def _cached_fir_plan(taps, device: int) -> "SpectrumPlan":
    h = _as_c64(taps)
    key = (int(device), FIR_BLOCK, ("fir", hashlib.sha1(h.tobytes()).digest()), 1e-12, True, "single")
    plan = _plans.get(key)
    if plan is None:
        with _plans_lock:
            plan = _plans.get(key)
            if plan is None:
                plan = SpectrumPlan(FIR_BLOCK, device=device)
                plan.set_fir(h)
                _plans[key] = plan
    return plan


def fir_filter(iq, taps, decim: int = 1, shift_bins: int = 0, *, device: int = 0) -> np.ndarray:
    """``SpectrumPlan.fir`` on a cached plan that holds ``taps``: ``lfilter(taps, 1, iq)`` of the band centred on bin
    ``shift_bins`` of 4096, moved to DC, every ``decim``-th sample.  int16 ``(n, 2)`` input takes the int16 entry."""
    _fir_args(decim, shift_bins)
    plan = _cached_fir_plan(taps, device)
    if isinstance(iq, np.ndarray) and iq.dtype == np.int16:
        return plan.fir_ci16(iq, decim=decim, shift_bins=shift_bins)
    return plan.fir(iq, decim=decim, shift_bins=shift_bins)


def fir_bank(iq, taps, shift_bins, decim: int = 1, *, device: int = 0) -> np.ndarray:
    """``SpectrumPlan.fir_bank`` on a cached plan that holds ``taps``: ``fir_filter(iq, taps, decim, shift_bins[c])`` for every
    channel ``c`` from one pass over ``iq``, as a ``(C, n_out)`` array.  int16 ``(n, 2)`` input takes the int16 entry."""
    _fir_args(decim, 0)
    _bank_shifts(shift_bins)
    plan = _cached_fir_plan(taps, device)
    if isinstance(iq, np.ndarray) and iq.dtype == np.int16:
        return plan.fir_bank_ci16(iq, shift_bins, decim=decim)
    return plan.fir_bank(iq, shift_bins, decim=decim)


def ddc(iq, taps, offset_hz: float, sample_rate: float, decim: int = 1, *, device: int = 0) -> np.ndarray:
    """``SpectrumPlan.ddc`` on a cached plan that holds ``taps``: the band around ``offset_hz`` (to the nearest frequency word,
    ``freq_word(offset_hz, sample_rate)``) moved to DC, low-passed by ``taps`` and decimated by any integer ``decim`` in 1..256.
    int16 ``(n, 2)`` input takes the int16 entry."""
    _ddc_decim(decim)
    word = freq_word(offset_hz, sample_rate)
    plan = _cached_fir_plan(taps, device)
    if isinstance(iq, np.ndarray) and iq.dtype == np.int16:
        return plan.ddc_ci16(iq, word, decim=decim)
    return plan.ddc(iq, word, decim=decim)


def ddc_bank(iq, taps, offsets_hz, sample_rate: float, decim: int = 1, *, device: int = 0) -> np.ndarray:
    """``SpectrumPlan.ddc_bank`` on a cached plan that holds ``taps``: ``ddc(iq, taps, offsets_hz[c], sample_rate, decim)`` for
    every channel ``c`` from one pass over ``iq``, as a ``(C, n_out)`` array.  int16 ``(n, 2)`` input takes the int16 entry."""
    _ddc_decim(decim)
    words = [freq_word(f, sample_rate) for f in np.asarray(offsets_hz, dtype=np.float64).reshape(-1)]
    _ddc_words(words)
    plan = _cached_fir_plan(taps, device)
    if isinstance(iq, np.ndarray) and iq.dtype == np.int16:
        return plan.ddc_bank_ci16(iq, words, decim=decim)
    return plan.ddc_bank(iq, words, decim=decim)


def ddc_ci8(iq, taps, offset_hz: float, sample_rate: float, decim: int = 1, *, device: int = 0) -> np.ndarray:
    """``ddc`` on interleaved 8-bit I,Q of shape ``(n, 2)``, int8 (SigMF ci8) or uint8 (cu8), read as they are (2 bytes per
    sample): ``SpectrumPlan.ddc_ci8`` on a cached plan that holds ``taps``; the bits of ``ddc`` on ``iq8_to_c64(iq)`` — for uint8
    with the stream before ``iq`` taken as bytes of 128 (``+0.5 + 0.5j``), the nearest a cu8 stream comes to silence."""
    _ddc_decim(decim)
    word = freq_word(offset_hz, sample_rate)
    x = _as_ci8(iq, stream=True)
    return _cached_fir_plan(taps, device).ddc_ci8(x, word, decim=decim)


def ddc_bank_ci8(iq, taps, offsets_hz, sample_rate: float, decim: int = 1, *, device: int = 0) -> np.ndarray:
    """``ddc_bank`` on interleaved 8-bit I,Q of shape ``(n, 2)`` (int8 or uint8, as ``ddc_ci8``): row ``c`` carries the bits of
    ``ddc_ci8(iq, taps, offsets_hz[c], sample_rate, decim)``."""
    _ddc_decim(decim)
    words = [freq_word(f, sample_rate) for f in np.asarray(offsets_hz, dtype=np.float64).reshape(-1)]
    _ddc_words(words)
    x = _as_ci8(iq, stream=True)
    return _cached_fir_plan(taps, device).ddc_bank_ci8(x, words, decim=decim)


_NARROW = (np.int16, np.int8, np.uint8)


def _stream_piece(who: str, iq, tail) -> np.ndarray:
    """A piece pushed into a stream as the array its plan call takes: complex64, or int16 / int8 / uint8 ``(n, 2)`` as they
    are; one kind throughout a stream (``tail``: the samples kept so far, None before the first)."""
    if isinstance(iq, np.ndarray) and iq.dtype in _NARROW:
        x = _as_ci16(iq, stream=True) if iq.dtype == np.int16 else _as_ci8(iq, stream=True)
    else:
        x = _as_c64(iq).reshape(-1)
    if tail is not None and tail.dtype != x.dtype:
        raise ValueError(f"a {who} takes complex, int16, int8 or uint8 pieces, not both: one kind throughout "
                         f"(so far {tail.dtype}, now {x.dtype})")
    return x


def _stream_tail(tail, x: np.ndarray, keep: int):
    """The last ``keep`` samples of tail || x.  Before the first piece the tail is silence: zeros, and for uint8 the mid-scale
    byte 128 (no cu8 byte widens to zero; the C entries take a NULL prefix the same way)."""
    if not keep:
        return tail
    if tail is None:
        tail = np.zeros(keep, np.complex64) if x.dtype == np.complex64 else np.full((keep, 2), 128 if x.dtype == np.uint8 else 0, x.dtype)
    return np.ascontiguousarray(np.concatenate((tail, x))[-keep:])


def _bin_word(shift_bins: int) -> int:
    """The frequency word of a whole bin: with a power-of-two decimation and a stream index that is a multiple of it, the DDC call
    then returns the bits of the FIR call."""
    return ((int(shift_bins) % FIR_BLOCK) << 20) & 0xFFFFFFFF


class ChannelStream:
    """One channel out of a stream that arrives in pieces: tuned to ``offset_hz`` from the centre, low-passed by ``taps``,
    decimated by ``decim``.  The offset is rounded to a whole bin of ``sample_rate/4096`` (``shift_bins``; ``tuned_hz`` is the
    frequency actually tuned).  ``push(iq)`` takes pieces of any length (complex64, or int16 / int8 / uint8 ``(n, 2)``, one kind
    throughout; 8-bit pieces are read as they are by the 8-bit down-converter call with the bin's frequency word, which cuts its
    blocks from the piece's first sample where the FIR call cuts them from the first kept one: the FIR call's bits for a piece
    that starts on a multiple of ``decim``, its error bound otherwise) and returns the complex64 output samples they complete; the last ``M - 1`` input samples and the stream index are kept between calls,
    so filter and mixer run on as over one stream.  ``plan``: a float32 ``SpectrumPlan(4096)`` to use (its FIR filter is
    replaced), or None for one of the stream's own."""

    def __init__(self, plan, taps, decim: int, offset_hz: float, sample_rate: float, *, device: int = 0):
        self.decim, _ = _fir_args(decim, 0)
        self.sample_rate = float(sample_rate)
        if not self.sample_rate > 0:
            raise ValueError("sample_rate must be positive")
        bin_hz = self.sample_rate / FIR_BLOCK
        self.shift_bins = int(np.rint(float(offset_hz) / bin_hz))
        _fir_args(self.decim, self.shift_bins)           # an offset beyond the band: ValueError
        self.tuned_hz = self.shift_bins * bin_hz
        self.out_rate = self.sample_rate / self.decim
        self._own = plan is None
        self.plan = SpectrumPlan(FIR_BLOCK, device=device) if plan is None else plan
        self.ntaps = int(self.plan.set_fir(taps))
        self.sample_index = 0                              # stream index of the next input sample
        self._tail = None                                  # the last M - 1 input samples (None: none yet = zeros)

    def push(self, iq) -> np.ndarray:
        x = _stream_piece("ChannelStream", iq, self._tail)
        n = int(x.shape[0])
        if n == 0:
            return np.empty(0, dtype=np.complex64)
        if x.dtype.itemsize == 1:
            out = self.plan.ddc_ci8(x, _bin_word(self.shift_bins), decim=self.decim, prefix=self._tail, sample0=self.sample_index)
        else:
            run = self.plan.fir_ci16 if x.dtype == np.int16 else self.plan.fir
            out = run(x, decim=self.decim, shift_bins=self.shift_bins, prefix=self._tail, sample0=self.sample_index)
        self._tail = _stream_tail(self._tail, x, self.ntaps - 1)
        self.sample_index += n
        return out

    def close(self) -> None:
        if self._own:
            self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ChannelBankStream:
    """``C`` channels out of a stream that arrives in pieces, from one pass over each piece: ``ChannelStream`` for every offset
    of ``offsets_hz`` (1..64 of them, each rounded to a whole bin of ``sample_rate/4096``), with one filter, one decimation and
    ONE kept tail for all channels.  ``push(iq)`` returns the ``(C, n)`` complex64 samples the piece completes; row ``c`` carries
    the bits of a ``ChannelStream`` tuned to ``offsets_hz[c]`` that was pushed the same pieces.  ``shift_bins``, ``tuned_hz``:
    one entry per channel."""

    def __init__(self, plan, taps, decim: int, offsets_hz, sample_rate: float, *, device: int = 0):
        self.decim, _ = _fir_args(decim, 0)
        self.sample_rate = float(sample_rate)
        if not self.sample_rate > 0:
            raise ValueError("sample_rate must be positive")
        bin_hz = self.sample_rate / FIR_BLOCK
        self.shift_bins = [int(np.rint(float(f) / bin_hz)) for f in np.asarray(offsets_hz, dtype=np.float64).reshape(-1)]
        _bank_shifts(self.shift_bins)                      # too few, too many, an offset beyond the band: ValueError
        self.tuned_hz = [s * bin_hz for s in self.shift_bins]
        self.out_rate = self.sample_rate / self.decim
        self._own = plan is None
        self.plan = SpectrumPlan(FIR_BLOCK, device=device) if plan is None else plan
        self.ntaps = int(self.plan.set_fir(taps))
        self.sample_index = 0                              # stream index of the next input sample
        self._tail = None                                  # the last M - 1 input samples (None: none yet = zeros)

    def push(self, iq) -> np.ndarray:
        x = _stream_piece("ChannelBankStream", iq, self._tail)
        n = int(x.shape[0])
        if n == 0:
            return np.empty((len(self.shift_bins), 0), dtype=np.complex64)
        if x.dtype.itemsize == 1:                          # (8-bit pieces: the down-converter call with the bins' words)
            out = self.plan.ddc_bank_ci8(x, [_bin_word(s) for s in self.shift_bins], decim=self.decim, prefix=self._tail,
                                         sample0=self.sample_index)
        else:
            run = self.plan.fir_bank_ci16 if x.dtype == np.int16 else self.plan.fir_bank
            out = run(x, self.shift_bins, decim=self.decim, prefix=self._tail, sample0=self.sample_index)
        self._tail = _stream_tail(self._tail, x, self.ntaps - 1)
        self.sample_index += n
        return out

    def close(self) -> None:
        if self._own:
            self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _DdcStreamBase:
    """What DdcStream and DdcBankStream share: the plan, the filter, the M - 1 kept samples and the stream index."""

    def __init__(self, plan, taps, decim: int, sample_rate: float, device: int):
        self.decim = _ddc_decim(decim)
        self.sample_rate = float(sample_rate)
        if not self.sample_rate > 0:
            raise ValueError("sample_rate must be positive")
        self.out_rate = self.sample_rate / self.decim
        self._own = plan is None
        self.plan = SpectrumPlan(FIR_BLOCK, device=device) if plan is None else plan
        self.ntaps = int(self._set_filter(taps))
        self.sample_index = 0                              # stream index of the next input sample
        self._tail = None                                  # the last M - 1 input samples (None: none yet = zeros)

    def _set_filter(self, taps) -> int:
        """Hand the plan its filter; the taps per channel."""
        return self.plan.set_fir(taps)

    def _piece(self, iq) -> np.ndarray:
        return _stream_piece(type(self).__name__, iq, self._tail)

    def _run(self, x: np.ndarray, bank: bool):
        """The plan call of a piece's kind."""
        kind = "" if x.dtype == np.complex64 else "_ci16" if x.dtype == np.int16 else "_ci8"
        return getattr(self.plan, ("ddc_bank" if bank else "ddc") + kind)

    def _advance(self, x: np.ndarray) -> None:
        self._tail = _stream_tail(self._tail, x, self.ntaps - 1)
        self.sample_index += int(x.shape[0])

    def close(self) -> None:
        if self._own:
            self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DdcStream(_DdcStreamBase):
    """``ChannelStream`` as a digital down-converter: tuned to ``offset_hz`` to the nearest 32-bit frequency word (``freq_word``;
    ``tuned_hz`` is that word's frequency, within ``sample_rate / 2^33`` of the request) and decimated by ANY integer ``decim``
    in 1..256.  ``push(iq)`` takes pieces of any length (complex64, or int16 / int8 / uint8 ``(n, 2)``, one kind throughout;
    8-bit pieces are read as they are, and a uint8 stream starts from M - 1 pairs of byte 128) and returns the output
    samples whose stream index is a multiple of ``decim`` — however many fall into the piece, none included."""

    def __init__(self, plan, taps, decim: int, offset_hz: float, sample_rate: float, *, device: int = 0):
        word = freq_word(offset_hz, sample_rate)           # (checks the rate before a plan is made)
        super().__init__(plan, taps, decim, sample_rate, device)
        self.freq_word = word
        self.tuned_hz = freq_word_hz(word, self.sample_rate)

    def push(self, iq) -> np.ndarray:
        x = self._piece(iq)
        if x.shape[0] == 0:
            return np.empty(0, dtype=np.complex64)
        out = self._run(x, False)(x, self.freq_word, decim=self.decim, prefix=self._tail, sample0=self.sample_index)
        self._advance(x)
        return out


class DdcBankStream(_DdcStreamBase):
    """``C`` digital down-converters on one stream that arrives in pieces, from one pass over each piece: a ``DdcStream`` for every
    offset of ``offsets_hz`` (1..64), with one filter, one decimation and one kept tail.  ``push(iq)`` returns ``(C, n)`` complex64;
    row ``c`` carries the bits of a ``DdcStream`` tuned to ``offsets_hz[c]`` that was pushed the same pieces.  ``freq_words``,
    ``tuned_hz``: one entry per channel."""

    def __init__(self, plan, taps, decim: int, offsets_hz, sample_rate: float, *, device: int = 0):
        words = [freq_word(f, sample_rate) for f in np.asarray(offsets_hz, dtype=np.float64).reshape(-1)]
        _ddc_words(words)                                  # too few or too many: ValueError
        super().__init__(plan, taps, decim, sample_rate, device)
        self.freq_words = words
        self.tuned_hz = [freq_word_hz(w, self.sample_rate) for w in words]

    def push(self, iq) -> np.ndarray:
        x = self._piece(iq)
        if x.shape[0] == 0:
            return np.empty((len(self.freq_words), 0), dtype=np.complex64)
        out = self._run(x, True)(x, self.freq_words, decim=self.decim, prefix=self._tail, sample0=self.sample_index)
        self._advance(x)
        return out


# -- filter-and-sum beamformer ---------------------------------------------------------------------------------------------
def beam_taps(weights, taps) -> np.ndarray:
    """The ``(C, M)`` beam filters of ``C`` complex weights and one shared filter ``taps``: row ``c`` is ``conj(w_c) * taps``,
    the convention ``y = w^H x`` followed by the filter."""
    w = np.asarray(weights, dtype=np.complex128).reshape(-1)
    h = np.asarray(taps, dtype=np.complex128).reshape(-1)
    if not 1 <= w.shape[0] <= BEAM_MAX_CHANNELS:
        raise ValueError(f"weights must hold 1..{BEAM_MAX_CHANNELS} channels, got {w.shape[0]}")
    if not 1 <= h.shape[0] <= FIR_MAX_TAPS:
        raise ValueError(f"taps must hold 1..{FIR_MAX_TAPS} coefficients, got {h.shape[0]}")
    return np.ascontiguousarray((np.conj(w)[:, None] * h[None, :]).astype(np.complex64))


def mvdr_weights(R, steering, loading: float = 0.0) -> np.ndarray:
    """Minimum-variance distortionless-response weights ``R^-1 a / (a^H R^-1 a)`` for one ``(C, C)`` covariance matrix ``R``
    (a bin or a band average of ``CorrelationMatrix.matrix()``) and steering vector ``a``, with ``loading`` added to the
    diagonal: ``w^H a = 1``.  Plain numpy, complex128."""
    r = np.asarray(R, dtype=np.complex128)
    a = np.asarray(steering, dtype=np.complex128).reshape(-1)
    if r.ndim != 2 or r.shape[0] != r.shape[1] or r.shape[0] != a.shape[0]:
        raise ValueError(f"R must be (C, C) and steering (C,), got {r.shape} and {a.shape}")
    if float(loading) < 0:
        raise ValueError("loading must be >= 0")
    ria = np.linalg.solve(r + float(loading) * np.eye(r.shape[0]), a)
    return ria / np.vdot(a, ria)


def _beam_kind(iq) -> str:
    if isinstance(iq, np.ndarray) and iq.dtype in _NARROW:
        return "_ci16" if iq.dtype == np.int16 else "_ci8"
    return ""


def _beam_filters(weights_or_taps, decim: int, taps) -> np.ndarray:
    """``(C, M)`` filters from ``(C, M)`` taps as they are, or from ``(C,)`` weights and ``taps`` (None: ``ddc_taps(decim)``)."""
    w = np.asarray(weights_or_taps)
    if w.ndim == 2:
        if taps is not None:
            raise ValueError("taps goes with (C,) weights; (C, M) filters already hold theirs")
        return _as_c64(w)
    return beam_taps(w, ddc_taps(decim) if taps is None else taps)


def _cached_beam_plan(filters: np.ndarray, device: int) -> "SpectrumPlan":
    key = (int(device), FIR_BLOCK, ("beam", filters.shape, hashlib.sha1(filters.tobytes()).digest()), 1e-12, True, "single")
    plan = _plans.get(key)
    if plan is None:
        with _plans_lock:
            plan = _plans.get(key)
            if plan is None:
                plan = SpectrumPlan(FIR_BLOCK, device=device)
                plan.set_beam(filters)
                _plans[key] = plan
    return plan


def beamform(x, weights_or_taps, offset_hz: float, sample_rate: float, decim: int = 1, *, taps=None, device: int = 0) -> np.ndarray:
    """``SpectrumPlan.beam`` on a cached plan: ``x`` of shape ``(n, C)`` complex, or ``(n, C, 2)`` int16 / int8 / uint8, combined
    with ``(C,)`` weights (``y = w^H x``, then ``taps``, by default ``ddc_taps(decim)``) or ``(C, M)`` per-channel taps, the band
    around ``offset_hz`` moved to DC and decimated by ``decim``."""
    _ddc_decim(decim)
    word = freq_word(offset_hz, sample_rate)
    plan = _cached_beam_plan(_beam_filters(weights_or_taps, decim, taps), device)
    return getattr(plan, "beam" + _beam_kind(x))(x, word, decim=decim)


class BeamStream(_DdcStreamBase):
    """``DdcStream`` behind a filter-and-sum beamformer: pieces of ``(n, C)`` complex64 elements, or ``(n, C, 2)`` int16 / int8 /
    uint8 (one kind throughout), in; the beam's output samples whose stream index is a multiple of ``decim`` out.  ``taps``:
    the ``(C, M)`` beam filters (``beam_taps``).  The last ``M - 1`` elements and the stream index are kept between calls; a
    uint8 stream starts from elements of byte 128."""

    def __init__(self, plan, taps, decim: int, offset_hz: float, sample_rate: float, *, device: int = 0):
        word = freq_word(offset_hz, sample_rate)
        super().__init__(plan, taps, decim, sample_rate, device)
        self.freq_word = word
        self.tuned_hz = freq_word_hz(word, self.sample_rate)

    def _set_filter(self, taps) -> int:
        h = _as_c64(taps)
        self.channels = int(self.plan.set_beam(h))
        return int(h.shape[1])

    def _piece(self, iq) -> np.ndarray:
        x = np.ascontiguousarray(iq) if _beam_kind(iq) else _as_c64(iq)
        if x.ndim != (3 if _beam_kind(iq) else 2) or x.shape[1] != self.channels:
            raise ValueError(f"a BeamStream piece must have shape (n, {self.channels})" + (" + (2,)" if _beam_kind(iq) else "")
                             + f", got {x.shape}")
        if self._tail is not None and self._tail.dtype != x.dtype:
            raise ValueError(f"a BeamStream takes complex, int16, int8 or uint8 pieces, not both: one kind throughout "
                             f"(so far {self._tail.dtype}, now {x.dtype})")
        return x

    def _advance(self, x: np.ndarray) -> None:
        keep = self.ntaps - 1
        if keep:
            tail = self._tail
            if tail is None:
                tail = np.full((keep,) + x.shape[1:], 128 if x.dtype == np.uint8 else 0, x.dtype)
            self._tail = np.ascontiguousarray(np.concatenate((tail, x))[-keep:])
        self.sample_index += int(x.shape[0])

    def push(self, iq) -> np.ndarray:
        x = self._piece(iq)
        if x.shape[0] == 0:
            return np.empty(0, dtype=np.complex64)
        run = getattr(self.plan, "beam" + _beam_kind(x))
        out = run(x, self.freq_word, decim=self.decim, prefix=self._tail, sample0=self.sample_index)
        self._advance(x)
        return out

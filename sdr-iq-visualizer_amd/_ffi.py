"""ctypes binding of the C ABI in ``include/sdrk.h`` (``lib/libsdrk.so``).

This is the only module that touches the shared library.  It declares every
exported symbol with its argument types, turns negative ``sdrk_status`` codes
into Python exceptions, and refuses to go on without the library: there is no
numpy fallback behind the product API (the reference's own producer loop
catches ordinary exceptions at ``app/sdr/streamer.py:157-159``, so raising is
the drop-in-compatible failure mode).

HIP runtime note: the library links ``libamdhip64.so.7``.  A process that also
uses PyTorch must ``import torch`` *before* this module so that both share the
single HIP runtime torch bundles; ``bench.py`` and ``__graft_entry__`` do so.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

SDRK_OK = 0
SDRK_ERR_INVALID = -1
SDRK_ERR_NO_DEVICE = -2
SDRK_ERR_HIP = -3
SDRK_ERR_NOMEM = -4
SDRK_ERR_UNSUPPORTED = -5

WINDOW_RECT = 0
WINDOW_HANN = 1
WINDOW_CUSTOM = 2

MAX_LOG2_NFFT = 22
ABI_VERSION = 500                 # SDRK_VERSION of include/sdrk.h this binding was written against
FEAT_PLANES = 19                  # SDRK_FEAT_* plane numbers of include/sdrk.h
(FEAT_MAX_DB, FEAT_NOISE_FLOOR_DB, FEAT_SNR_DB, FEAT_FLATNESS, FEAT_KURTOSIS, FEAT_THRESHOLD_DB, FEAT_PEAK_SPACING_STD_HZ,
 FEAT_PEAK_DENSITY, FEAT_BANDWIDTH_HZ) = range(9)
FEAT_ARGMAX, FEAT_PEAK_COUNT, FEAT_OCCUPIED_BINS = 11, 12, 13
DETECTORS = {"mean": 0, "max": 1, "min": 2}   # SDRK_DET_*
INT_OUT_FORMS = {"db": 0, "power": 1}         # SDRK_INT_OUT_*
PLAN_FUSED64K = 0x1
PLAN_OVERLAP_PASSES = 0x2
PLAN_TUNE_STAGING = 0x4
PLAN_TILED64K = 0x8

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# SDRK_LIB: developer override (A/B builds made by tools/variant.sh); the product loads lib/libsdrk.so
_LIB_PATH = os.environ.get("SDRK_LIB") or os.path.join(_PKG_DIR, "lib", "libsdrk.so")


class SdrkError(RuntimeError):
    """A call into libsdrk failed (HIP error, no device, out of memory...)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libsdrk status {status}: {message}")
        self.status = status


# (name, restype, argtypes) — must list every symbol include/sdrk.h declares;
# tests/test_abi.py checks this table against the header and the built library.
SYMBOLS = [
    ("sdrk_version", c_int, []),
    ("sdrk_last_error", c_char_p, []),
    ("sdrk_device_count", c_int, []),
    ("sdrk_device_info", c_int, [c_int, c_char_p, c_size_t]),
    ("sdrk_dev_mem_info", c_int, [c_int, POINTER(c_size_t), POINTER(c_size_t)]),
    ("sdrk_dev_alloc", c_int, [c_int, c_size_t, POINTER(c_void_p)]),
    ("sdrk_dev_free", c_int, [c_int, c_void_p]),
    ("sdrk_dev_alloc_stream_pair", c_int, [c_int, c_size_t, c_size_t, c_int, c_void_p, POINTER(c_void_p),
                                           POINTER(c_void_p), POINTER(c_float), POINTER(c_int)]),
    ("sdrk_memcpy_h2d", c_int, [c_int, c_void_p, c_void_p, c_size_t]),
    ("sdrk_memcpy_d2h", c_int, [c_int, c_void_p, c_void_p, c_size_t]),
    ("sdrk_plan_create", c_int,
     [c_int, c_int, c_size_t, c_int, c_void_p, c_float, c_int, POINTER(c_void_p)]),
    ("sdrk_plan_create_ex", c_int,
     [c_int, c_int, c_size_t, c_int, c_void_p, c_float, c_int, c_uint32, POINTER(c_void_p)]),
    ("sdrk_plan_staging_probe", c_int, [c_void_p, POINTER(c_float), c_int, POINTER(c_int)]),
    ("sdrk_plan_fused_status", c_int, [c_void_p, POINTER(c_uint32), POINTER(c_int)]),
    ("sdrk_plan_tune_scratch", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float),
                                       POINTER(c_int)]),
    ("sdrk_placement_report", c_int, [POINTER(c_float), POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    ("sdrk_plan_destroy", c_int, [c_void_p]),
    ("sdrk_plan_nfft", c_int, [c_void_p]),
    ("sdrk_plan_device", c_int, [c_void_p]),
    ("sdrk_exec_host", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_fft_host", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_welch_psd_host", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_float, c_void_p]),
    ("sdrk_plan_sync", c_int, [c_void_p]),
    ("sdrk_exec_device_timed", c_int,
     [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_device_timed_each", c_int,
     [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_stream_ceiling_probe", c_int, [c_int, c_void_p, c_void_p, c_size_t, c_int, POINTER(c_float)]),
    ("sdrk_host_alloc", c_int, [c_size_t, POINTER(c_void_p)]),
    ("sdrk_host_free", c_int, [c_void_p]),
    ("sdrk_host_register", c_int, [c_void_p, c_size_t]),
    ("sdrk_host_unregister", c_int, [c_void_p]),
    ("sdrk_host_is_pinned", c_int, [c_void_p, c_size_t]),
    ("sdrk_copy_probe", c_int, [c_int, c_void_p, c_void_p, c_size_t, c_int, POINTER(c_float)]),
    ("sdrk_host_link_probe", c_int, [c_int, c_size_t, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    ("sdrk_host_threads", c_int, []),
    ("sdrk_synth_fill", c_int, [c_int, c_uint32, c_uint64, c_size_t, c_int, c_void_p, c_void_p]),
    ("sdrk_row_features", c_int, [c_int, c_void_p, c_int, c_size_t, c_int, c_int, c_float, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    ("sdrk_frame_features_device", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, c_float, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("sdrk_frame_features_host", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_float, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("sdrk_row_features_planes", c_int, [c_int, c_void_p, c_int, c_size_t, c_int, c_int, c_float, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p]),
    ("sdrk_frame_features_host_planes", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_float, c_int, c_int,
                                                c_void_p, c_void_p, c_void_p, c_void_p]),
    ("sdrk_row_stats", c_int, [c_int, c_void_p, c_int, c_size_t, c_int, c_int, c_void_p]),
    ("sdrk_row_peaks", c_int, [c_int, c_void_p, c_int, c_size_t, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    ("sdrk_waterfall_create", c_int, [c_int, c_int, c_int, POINTER(c_void_p)]),
    ("sdrk_waterfall_destroy", c_int, [c_void_p]),
    ("sdrk_waterfall_append_rows", c_int, [c_void_p, c_void_p, c_size_t]),
    ("sdrk_waterfall_append_iq", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t]),
    ("sdrk_waterfall_append_iq_device", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t]),
    ("sdrk_waterfall_append_iq_device_async", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t]),
    ("sdrk_waterfall_sync", c_int, [c_void_p, c_void_p]),
    ("sdrk_waterfall_read_decimated_begin", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_size_t)]),
    ("sdrk_waterfall_read_decimated_end", c_int, [c_void_p]),
    ("sdrk_waterfall_rows", c_int, [c_void_p]),
    ("sdrk_waterfall_read", c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("sdrk_waterfall_read_decimated", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_size_t)]),
    ("sdrk_waterfall_maxhold16_rows", c_int, [c_void_p]),
    ("sdrk_waterfall_clear", c_int, [c_void_p]),
    # double precision (the reference's complex128 -> float64, streamer.py:119-121)
    ("sdrk_plan_create_f64", c_int, [c_int, c_int, c_size_t, c_int, c_void_p, c_double, c_int, POINTER(c_void_p)]),
    ("sdrk_plan_precision", c_int, [c_void_p]),
    ("sdrk_exec_host_f64", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_f64", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_f64", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_f64_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    # int16 I,Q input (what the radio delivers, streamer.py:114; SigMF ci16_le) on float32 plans
    ("sdrk_exec_host_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_synth_fill_ci16", c_int, [c_int, c_uint32, c_uint64, c_size_t, c_int, c_void_p, c_void_p]),
    # one row per K frames: mean / max / min of the power inside the transform
    ("sdrk_exec_device_integrated", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                            c_void_p, c_void_p]),
    ("sdrk_exec_device_integrated_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                       c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_integrated", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                          c_void_p]),
    # ... the same from int16 I,Q: the bits of the three above on the widened samples
    ("sdrk_exec_device_integrated_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                 c_void_p, c_void_p]),
    ("sdrk_exec_device_integrated_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                            c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_integrated_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                               c_void_p]),
    # 8-bit I,Q (SigMF ci8 / cu8): per-frame and integrated, the format (SDRK_IQ8_*) right after the input pointer
    ("sdrk_exec_host_ci8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_ci8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_ci8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_ci8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_device_integrated_ci8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                c_void_p, c_void_p]),
    ("sdrk_exec_device_integrated_ci8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                           c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_integrated_ci8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                              c_void_p]),
    # polyphase filter bank: T blocks folded under a prototype of T*nfft coefficients in front of the transform
    ("sdrk_plan_set_pfb", c_int, [c_void_p, c_int, c_void_p]),
    ("sdrk_plan_pfb_taps", c_int, [c_void_p]),
    ("sdrk_exec_device_pfb", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_pfb", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_pfb_integrated", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_integrated_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                           c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_integrated", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                              c_void_p]),
    # ... the seven above from int16 I,Q: the bits of the complex64 forms on the widened samples
    ("sdrk_exec_device_pfb_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_pfb_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_pfb_integrated_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                     c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_integrated_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                                c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_integrated_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                   c_void_p]),
    # spectral kurtosis: per group two planes, the mean power and SK from the sums of p and p^2 (no detector argument)
    ("sdrk_exec_device_sk", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_sk_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_sk", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    ("sdrk_exec_device_sk_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_sk_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_sk_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    ("sdrk_exec_device_pfb_sk", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_sk_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_sk", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    ("sdrk_exec_device_pfb_sk_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_sk_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_sk_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    # two-channel cross-spectra: per group four planes from elements I0 Q0 I1 Q1 (no detector, no out_form)
    ("sdrk_exec_device_xspec", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_xspec_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_xspec", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    ("sdrk_exec_device_xspec_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_xspec_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_xspec_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    # correlation matrix of 2..8 channels: per group channels^2 planes (channels after the samples; iq8: after the format)
    ("sdrk_exec_device_corrmat", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_corrmat_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_corrmat", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    ("sdrk_exec_device_corrmat_ci16", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_corrmat_ci16_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_corrmat_ci16", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    ("sdrk_exec_device_corrmat_iq8", c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_corrmat_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_corrmat_iq8", c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_size_t, c_float, c_void_p]),
    # FIR filtering and channel extraction: overlap-save in blocks of 4096, tune + filter + decimate (nfft = 4096 plans)
    ("sdrk_plan_set_fir", c_int, [c_void_p, c_int, c_void_p]),
    ("sdrk_plan_fir_taps", c_int, [c_void_p]),
    ("sdrk_exec_device_fir", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("sdrk_exec_device_fir_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("sdrk_exec_device_fir_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_fir", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_host_fir_ci16", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    # channel bank: C tuned channels from one pass over the input (the filter of sdrk_plan_set_fir; planes out_stride apart)
    ("sdrk_exec_device_chanbank", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_int), POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_chanbank_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_int), POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_chanbank_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_int), POINTER(c_int), c_void_p, c_size_t, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_chanbank", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_int), c_uint64, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("sdrk_exec_host_chanbank_ci16", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_int), c_uint64, c_void_p, c_size_t, POINTER(c_size_t)]),
    # digital down-converter: the two calls above tuned by a 32-bit frequency word, decimated by any integer 1..256
    ("sdrk_ddc_outputs", c_size_t, [c_size_t, c_int, c_int, c_uint64]),
    ("sdrk_exec_device_ddc", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_ddc_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_ddc_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_ddc", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_host_ddc_ci16", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_device_ddcbank", c_int, [c_void_p, c_void_p, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_ddcbank_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_ddcbank_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_ddcbank", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("sdrk_exec_host_ddcbank_ci16", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, POINTER(c_size_t)]),
    # ... from 8-bit I,Q (SigMF ci8 / cu8): the format (SDRK_IQ8_*) right after the samples pointer
    ("sdrk_exec_device_downconv_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_downconv_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_downconv_iq8", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_device_downconvbank_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_downconvbank_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_downconvbank_iq8", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_int, POINTER(c_uint32), c_int, c_uint64, c_void_p, c_size_t, POINTER(c_size_t)]),
    # filter bank and spectral kurtosis from 8-bit I,Q: the _ci16 twins' argument lists with the format after the samples pointer
    ("sdrk_exec_device_pfb_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_pfb_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_device_pfb_integrated_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                    c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_integrated_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                               c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_integrated_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                  c_void_p]),
    ("sdrk_exec_device_kurtosis_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_kurtosis_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_kurtosis_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    ("sdrk_exec_device_pfb_kurtosis_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_void_p]),
    ("sdrk_exec_device_pfb_kurtosis_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_pfb_kurtosis_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_float, c_void_p]),
    # filter-and-sum beamformer: 1..8 coherent channels in, one down-converted channel out (the DDC's argument lists, in elements)
    ("sdrk_plan_set_beam", c_int, [c_void_p, c_int, c_int, c_void_p]),
    ("sdrk_plan_beam_channels", c_int, [c_void_p]),
    ("sdrk_plan_beam_taps", c_int, [c_void_p]),
    ("sdrk_exec_device_beam", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_beam_ci16", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_beam_iq8", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_void_p]),
    ("sdrk_exec_device_beam_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_device_beam_ci16_timed_each", c_int, [c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_device_beam_iq8_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_beam", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_host_beam_ci16", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    ("sdrk_exec_host_beam_iq8", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_uint32, c_int, c_uint64, c_void_p, POINTER(c_size_t)]),
    # real-sampled input (SigMF rf32_le / ri16_le / ri8 / ru8): frames of 2 * nfft real samples, rows of nfft + 1 bins
    ("sdrk_plan_set_real_window", c_int, [c_void_p, c_void_p, c_size_t]),
    ("sdrk_exec_device_real", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_int, c_void_p, c_size_t, c_void_p]),
    ("sdrk_exec_device_real_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_int, c_void_p, c_size_t, c_int,
                                                 POINTER(c_float)]),
    ("sdrk_exec_host_real", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    ("sdrk_exec_fft_host_real", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]),
    # ... integrated: one row of nfft + 1 bins per k frames (format, groups, k, stride, detector, out form, scale)
    ("sdrk_exec_device_real_integrated", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                                 c_void_p, c_void_p]),
    ("sdrk_exec_device_real_integrated_timed_each", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int,
                                                            c_float, c_void_p, c_int, POINTER(c_float)]),
    ("sdrk_exec_host_real_integrated", c_int, [c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float,
                                               c_void_p]),
]

# sdrk_real_format / sdrk_real_out of include/sdrk.h
REAL_F32, REAL_S16, REAL_S8, REAL_U8 = 0, 1, 2, 3
REAL_OUT_DB, REAL_OUT_COMPLEX = 0, 1

_lib = None
_lib_lock = threading.Lock()


def library_path() -> str:
    return _LIB_PATH


def lib() -> ctypes.CDLL:
    """Load (once) and return the shared library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build it with `make -C {os.path.join(_PKG_DIR, 'csrc')}` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback for the spectrum path."
            )
        handle = ctypes.CDLL(_LIB_PATH)
        handle.sdrk_version.restype = c_int
        built = int(handle.sdrk_version())
        if built != ABI_VERSION:         # a stale build: say so, instead of an AttributeError on some newer symbol
            raise ImportError(f"{_LIB_PATH} reports ABI version {built}, this package expects {ABI_VERSION}: rebuild it "
                              f"with `make -C {os.path.join(_PKG_DIR, 'csrc')}`")
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(handle, name)  # AttributeError if the build lacks a symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
        return _lib


def check(status: int) -> int:
    """Raise for a negative sdrk_status; pass non-negative values through."""
    if status >= 0:
        return status
    msg = lib().sdrk_last_error()
    text = msg.decode("utf-8", "replace") if msg else "unknown error"
    if status == SDRK_ERR_INVALID:
        raise ValueError(f"libsdrk: {text}")
    if status == SDRK_ERR_NOMEM:
        raise MemoryError(f"libsdrk: {text}")
    raise SdrkError(status, text)


def device_count() -> int:
    return int(lib().sdrk_device_count())


def device_info(device: int = 0) -> str:
    buf = ctypes.create_string_buffer(256)
    check(lib().sdrk_device_info(device, buf, len(buf)))
    return buf.value.decode()


def require_device(device: int = 0) -> None:
    """Fail loudly when there is no usable GPU (no silent host path)."""
    n = device_count()
    if n <= 0:
        raise SdrkError(SDRK_ERR_NO_DEVICE, "no HIP device visible to this process")
    if not 0 <= device < n:
        raise SdrkError(SDRK_ERR_NO_DEVICE, f"device {device} out of range ({n} visible)")


__all__ = [
    "SdrkError", "SYMBOLS", "lib", "check", "device_count", "device_info", "require_device",
    "library_path", "byref", "c_void_p", "c_size_t", "c_float", "c_int",
    "WINDOW_RECT", "WINDOW_HANN", "WINDOW_CUSTOM", "MAX_LOG2_NFFT",
]

// integrate_api.hip — the integrated-spectrum entry points of include/sdrk.h (sdrk_exec_*_integrated, _integrated_ci16,
// _pfb_integrated, _pfb_integrated_ci16): per group of K consecutive frames ONE row — the mean, maximum or minimum over the
// frames of |fft(w x_f)|^2 per bin — as dB or as scaled linear power.  Video averaging / Welch, peak hold and noise-floor hold
// inside the transform.  The samples are complex64 or interleaved little-endian int16 I,Q (4 bytes per sample; x[n] =
// float32(I[n]) + i float32(Q[n]) exactly, then the bits of the complex64 call); the frames are cut from the stream as they
// are, or folded from T blocks under the plan's prototype first (the spectrometer form of the polyphase filter bank: bit for
// bit the integrated call on the packed folded frames).
//
// The call itself — the N = 4096 kernel on the caller's samples, every other length through the mode's own transform and at
// most 64 MiB of staging, carry rows across chunks, slices and their finalize, the numpy boundary through the three staging
// slots — is integrate_call.h.  This file gives it one IntIo per mode: the N = 4096 kernel that reduces inside the transform
// (fft4096_integrate.hip, fft4096_kgroup_ci16.hip, pfb4096_groups.hip, pfb4096_i16_groups.hip) and the per-frame transform of
// the other lengths (plan_launch, ci16_api.hip's launch_ci16, pfb_api.hip's launch_pfb / launch_pfb_ci16, which keep their own
// stagings and orderings).  The PFB entries refuse a plan without a prototype first (check_pfb_ready).
//
// The 8-bit forms (sdrk_exec_*_integrated_ci8, _pfb_integrated_iq8, _kurtosis_iq8, _pfb_kurtosis_iq8) bind the format into the
// launchers of their IntIo (kernels_ci8.h): fft4096_kgroup_ci8.hip, pfb4096_iq8_groups.hip and sk4096_iq8.hip at N = 4096,
// launch_ci8_fn / launch_pfb_iq8_fn elsewhere.
//
// The spectral-kurtosis entry points (sdrk_exec_*_sk, _sk_ci16, _pfb_sk, _pfb_sk_ci16) are the same call with the kernels of
// kernels_sk.h behind it: per group two planes, the mean power and the estimator from S1 = sum p and S2 = sum p^2.  N = 4096
// keeps the sums inside the transform (sk4096.hip); every other length, and the filter bank at every length (N = 4096 too: fold
// and transform through launch_pfb / launch_pfb_ci16, no folding SK kernel), reduces staged spectra with sk_rows.hip.
//
// The two-channel cross-spectrum entry points (sdrk_exec_*_xspec, _xspec_ci16) are the same call on a stream of elements (sample
// n of channel 0, then of channel 1: 16 bytes from complex64, 8 from int16) with the kernels of kernels_xspec.h behind it: per
// group four planes from four sums per bin.  N = 4096 transforms both channels inside one kernel (xspec4096.hip); every other
// length de-interleaves, runs the plan's transform once per channel and reduces both staged spectra (xspec_rows.hip).  The
// interleaved layout is what lets the chunking of exec_host_integrated serve as it is: a chunk of elements holds both channels.
//
// The correlation-matrix entry points (sdrk_exec_*_corrmat, _corrmat_ci16, _corrmat_iq8) carry that to `channels` = 2..8 samples
// per element (complex64, int16 or 8-bit; aligned to a sample) with the kernels of kernels_corrmat.h behind it: per group
// channels^2 planes from as many sums per bin.  Every route is staged: N = 4096 writes the channels' spectra from the element
// stream itself (corrmat4096.hip; complex64 above 5 channels de-interleaves first, which measured faster), every other length
// de-interleaves and runs the plan's transform once per channel, and corrmat_rows.hip reduces the staged spectra.
// Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include "integrate_call.h"
#include "kernels_ci8.h"
#include "kernels_integrate.h"
#include "kernels_kgroup_ci16.h"
#include "kernels_pfb.h"
#include "kernels_sk.h"
#include "kernels_xspec.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

using FusedFn = hipError_t (*)(const sdrk::IntegrateArgs&);

IntIo int_io(size_t in_elem, FusedFn fused, LaunchFn transform, const sdrk_plan* pfb_plan = nullptr) {
    IntIo io;
    io.in_elem = in_elem;
    io.fused = fused;
    io.transform = transform;
    if (pfb_plan) io.in_span = (size_t)pfb_plan->pfb_taps * (size_t)pfb_plan->nfft;
    return io;
}

IntIo c64_io() { return int_io(sizeof(float2), sdrk::launch_fft4096_integrate, launch_f32); }
IntIo ci16_io() { return int_io(4, sdrk::launch_fft4096_kgroup_ci16, launch_ci16); }
// 8-bit I,Q of format fmt (SDRK_IQ8_*, checked by the caller): the format is bound into both launchers
IntIo ci8_io(int fmt) {
    return fmt == SDRK_IQ8_SIGNED ? int_io(2, sdrk::launch_fft4096_kgroup_ci8<SDRK_IQ8_SIGNED>, launch_ci8_fn(fmt))
                                  : int_io(2, sdrk::launch_fft4096_kgroup_ci8<SDRK_IQ8_UNSIGNED>, launch_ci8_fn(fmt));
}
IntIo pfb_io(const sdrk_plan* p) { return int_io(sizeof(float2), sdrk::launch_pfb4096_groups, launch_pfb, p); }
IntIo pfb_ci16_io(const sdrk_plan* p) { return int_io(4, sdrk::launch_pfb4096_i16_groups, launch_pfb_ci16, p); }

// 8-bit I,Q behind the filter bank: the format bound into both launchers, as ci8_io
IntIo pfb_iq8_io(const sdrk_plan* p, int fmt) {
    return fmt == SDRK_IQ8_SIGNED ? int_io(2, sdrk::launch_pfb4096_iq8_groups<SDRK_IQ8_SIGNED>, launch_pfb_iq8_fn(fmt), p)
                                  : int_io(2, sdrk::launch_pfb4096_iq8_groups<SDRK_IQ8_UNSIGNED>, launch_pfb_iq8_fn(fmt), p);
}

// spectral kurtosis: the mode's IntIo with the SK kernels behind it (fused: the N = 4096 kernel, or none)
IntIo sk_io(IntIo io, FusedFn fused) {
    io.fused = fused;
    io.rows = sdrk::launch_sk_rows;
    io.finalize = sdrk::launch_sk_finalize;
    io.planes = 2;
    io.min_k = 2;
    return io;
}

IntIo sk_c64_io() { return sk_io(c64_io(), sdrk::launch_sk4096); }
IntIo sk_ci16_io() { return sk_io(ci16_io(), sdrk::launch_sk4096_i16); }
IntIo sk_iq8_io(int fmt) {
    return fmt == SDRK_IQ8_SIGNED ? sk_io(ci8_io(fmt), sdrk::launch_sk4096_iq8<SDRK_IQ8_SIGNED>)
                                  : sk_io(ci8_io(fmt), sdrk::launch_sk4096_iq8<SDRK_IQ8_UNSIGNED>);
}
IntIo sk_pfb_io(const sdrk_plan* p) { return sk_io(pfb_io(p), nullptr); }
IntIo sk_pfb_ci16_io(const sdrk_plan* p) { return sk_io(pfb_ci16_io(p), nullptr); }
IntIo sk_pfb_iq8_io(const sdrk_plan* p, int fmt) { return sk_io(pfb_iq8_io(p, fmt), nullptr); }

// two-channel cross-spectra: elements of 16 (complex64) or 8 (int16) bytes; always through the plan's plain complex64 transform
IntIo xspec_io(size_t in_elem, FusedFn fused) {
    IntIo io = int_io(in_elem, fused, launch_f32);
    io.rows = nullptr;
    io.rows2 = sdrk::launch_xspec_rows;
    io.finalize = sdrk::launch_xspec_finalize;
    io.planes = 4;
    io.state = 4;
    return io;
}

IntIo xspec_c64_io() { return xspec_io(2 * sizeof(float2), sdrk::launch_xspec4096); }
IntIo xspec_ci16_io() { return xspec_io(8, sdrk::launch_xspec4096_i16); }

// correlation matrix of `channels` channels (checked by the caller) from samples of format fmt (a sdrk::CmFormat): always
// through staged spectra, the plan's plain complex64 transform at the lengths without a reading kernel
IntIo corrmat_io(int channels, int fmt) {
    const size_t c = (size_t)channels;
    IntIo io = int_io(c * sdrk::cm_sample_bytes(fmt), nullptr, launch_f32);
    io.rows = nullptr;
    io.finalize = nullptr;
    io.planes = c * c;
    io.state = c * c;
    io.channels = channels;
    io.fmt = fmt;
    return io;
}

int cm_format_of_iq8(int iq8_format) { return iq8_format == SDRK_IQ8_SIGNED ? sdrk::CM_B8_SIGNED : sdrk::CM_B8_UNSIGNED; }

// What the correlation-matrix entry points refuse before the shared checks: a channel count outside 2..8; and behind them
// (the plan, the counts and the stride are sound by then) a stream whose element count or byte size does not fit a size_t.
int check_corrmat_channels(int channels) {
    if (channels < sdrk::CM_MIN_CHANNELS || channels > sdrk::CM_MAX_CHANNELS)
        return fail(SDRK_ERR_INVALID, "channels = %d is outside %d..%d", channels, sdrk::CM_MIN_CHANNELS, sdrk::CM_MAX_CHANNELS);
    return SDRK_OK;
}

int check_corrmat_extent(const IntIo& io, const sdrk_plan* p, size_t n_groups, size_t k, size_t stride) {
    const size_t max = ~(size_t)0 >> 1, last = n_groups * k - 1, nfft = (size_t)p->nfft;
    if (last != 0 && stride > (max - nfft) / last)
        return fail(SDRK_ERR_INVALID, "(n_groups * k_frames - 1) * frame_stride + nfft elements is out of range");
    const size_t elems = last * stride + nfft;
    if (elems > max / io.in_elem || n_groups > max / (io.planes * nfft * sizeof(float)))
        return fail(SDRK_ERR_INVALID, "%zu elements of %zu bytes, or the output, are out of range", elems, io.in_elem);
    return SDRK_OK;
}

int check_corrmat(const IntIo& io, const sdrk_plan* p, const void* in, size_t n_groups, size_t k, size_t stride, const void* out) {
    int st = check_call_args(io, p, in, n_groups, k, stride, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, out);
    return st == SDRK_OK ? check_corrmat_extent(io, p, n_groups, k, stride) : st;
}

}  // namespace

extern "C" {

int sdrk_exec_device_integrated(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                int detector, int out_form, float scale, float* d_out, void* stream) {
    return exec_device_integrated(c64_io(), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out, stream);
}

int sdrk_exec_device_integrated_timed_each(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                           size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                           int launches, float* each_ms) {
    return exec_device_integrated_timed_each(c64_io(), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                             launches, each_ms);
}

int sdrk_exec_host_integrated(sdrk_plan* p, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                              int detector, int out_form, float scale, float* out) {
    return exec_host_integrated(c64_io(), p, iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

int sdrk_exec_device_integrated_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                     int detector, int out_form, float scale, float* d_out, void* stream) {
    return exec_device_integrated(ci16_io(), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out, stream);
}

int sdrk_exec_device_integrated_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                int launches, float* each_ms) {
    return exec_device_integrated_timed_each(ci16_io(), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                             launches, each_ms);
}

int sdrk_exec_host_integrated_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                   int detector, int out_form, float scale, float* out) {
    return exec_host_integrated(ci16_io(), p, iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

int sdrk_exec_device_integrated_ci8(sdrk_plan* p, const void* d_iq_ci8, int iq8_format, size_t n_groups, size_t k_frames,
                                    size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_integrated(ci8_io(iq8_format), p, d_iq_ci8, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                  stream);
}

int sdrk_exec_device_integrated_ci8_timed_each(sdrk_plan* p, const void* d_iq_ci8, int iq8_format, size_t n_groups, size_t k_frames,
                                               size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                               int launches, float* each_ms) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(ci8_io(iq8_format), p, d_iq_ci8, n_groups, k_frames, frame_stride, detector, out_form,
                                             scale, d_out, launches, each_ms);
}

int sdrk_exec_host_integrated_ci8(sdrk_plan* p, const void* iq_ci8, int iq8_format, size_t n_groups, size_t k_frames,
                                  size_t frame_stride, int detector, int out_form, float scale, float* out) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_integrated(ci8_io(iq8_format), p, iq_ci8, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

int sdrk_exec_device_pfb_integrated(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                    int detector, int out_form, float scale, float* d_out, void* stream) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_device_integrated(pfb_io(p), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out, stream);
}

int sdrk_exec_device_pfb_integrated_timed_each(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                               size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                               int launches, float* each_ms) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(pfb_io(p), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                             launches, each_ms);
}

int sdrk_exec_host_pfb_integrated(sdrk_plan* p, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                  int detector, int out_form, float scale, float* out) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_host_integrated(pfb_io(p), p, iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

int sdrk_exec_device_pfb_integrated_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                         int detector, int out_form, float scale, float* d_out, void* stream) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_device_integrated(pfb_ci16_io(p), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out, stream);
}

int sdrk_exec_device_pfb_integrated_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                    size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                    int launches, float* each_ms) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(pfb_ci16_io(p), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                             launches, each_ms);
}

int sdrk_exec_host_pfb_integrated_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                       int detector, int out_form, float scale, float* out) {
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;
    return exec_host_integrated(pfb_ci16_io(p), p, iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

// 8-bit I,Q behind the filter bank: the plan's refusals first (the _ci16 twin's words), then the format's
#define SDRK_PFB_IQ8_READY                                                                                                        \
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st;                                                                    \
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st

int sdrk_exec_device_pfb_integrated_iq8(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                        size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream) {
    SDRK_PFB_IQ8_READY;
    return exec_device_integrated(pfb_iq8_io(p, iq8_format), p, d_iq8, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                  stream);
}

int sdrk_exec_device_pfb_integrated_iq8_timed_each(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                                   size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                   int launches, float* each_ms) {
    SDRK_PFB_IQ8_READY;
    return exec_device_integrated_timed_each(pfb_iq8_io(p, iq8_format), p, d_iq8, n_groups, k_frames, frame_stride, detector, out_form,
                                             scale, d_out, launches, each_ms);
}

int sdrk_exec_host_pfb_integrated_iq8(sdrk_plan* p, const void* iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                      size_t frame_stride, int detector, int out_form, float scale, float* out) {
    SDRK_PFB_IQ8_READY;
    return exec_host_integrated(pfb_iq8_io(p, iq8_format), p, iq8, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

// ---- spectral kurtosis: two planes per group (the detector of the shared call is the mean's, and is not read) ----

#define SDRK_SK_ENTRIES(SUFFIX, IO, READY)                                                                                        \
    int sdrk_exec_device_##SUFFIX(sdrk_plan* p, const void* d_iq, size_t n_groups, size_t k_frames, size_t frame_stride,          \
                                  int out_form, float scale, float* d_out, void* stream) {                                       \
        READY;                                                                                                                    \
        return exec_device_integrated(IO, p, d_iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale, d_out, stream); \
    }                                                                                                                             \
    int sdrk_exec_device_##SUFFIX##_timed_each(sdrk_plan* p, const void* d_iq, size_t n_groups, size_t k_frames,                  \
                                               size_t frame_stride, int out_form, float scale, float* d_out, int launches,       \
                                               float* each_ms) {                                                                  \
        READY;                                                                                                                    \
        return exec_device_integrated_timed_each(IO, p, d_iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale,  \
                                                 d_out, launches, each_ms);                                                       \
    }                                                                                                                             \
    int sdrk_exec_host_##SUFFIX(sdrk_plan* p, const void* iq, size_t n_groups, size_t k_frames, size_t frame_stride,              \
                                int out_form, float scale, float* out) {                                                         \
        READY;                                                                                                                    \
        return exec_host_integrated(IO, p, iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale, out);           \
    }
#define SDRK_PFB_READY                                                                                                            \
    if (int st = check_pfb_ready(p); st != SDRK_OK) return st

SDRK_SK_ENTRIES(sk, sk_c64_io(), (void)0)
SDRK_SK_ENTRIES(sk_ci16, sk_ci16_io(), (void)0)
SDRK_SK_ENTRIES(pfb_sk, sk_pfb_io(p), SDRK_PFB_READY)
SDRK_SK_ENTRIES(pfb_sk_ci16, sk_pfb_ci16_io(p), SDRK_PFB_READY)
#undef SDRK_PFB_READY
#undef SDRK_SK_ENTRIES

// the same three from 8-bit I,Q, the format right after the samples (spelled out: the _sk names are the complex64 / int16 family's)
#define SDRK_KURTOSIS_IQ8_ENTRIES(SUFFIX, IO, READY)                                                                              \
    int sdrk_exec_device_##SUFFIX(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,              \
                                  size_t frame_stride, int out_form, float scale, float* d_out, void* stream) {                  \
        READY;                                                                                                                    \
        return exec_device_integrated(IO, p, d_iq8, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale, d_out, stream); \
    }                                                                                                                             \
    int sdrk_exec_device_##SUFFIX##_timed_each(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames, \
                                               size_t frame_stride, int out_form, float scale, float* d_out, int launches,       \
                                               float* each_ms) {                                                                  \
        READY;                                                                                                                    \
        return exec_device_integrated_timed_each(IO, p, d_iq8, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale, \
                                                 d_out, launches, each_ms);                                                       \
    }                                                                                                                             \
    int sdrk_exec_host_##SUFFIX(sdrk_plan* p, const void* iq8, int iq8_format, size_t n_groups, size_t k_frames,                  \
                                size_t frame_stride, int out_form, float scale, float* out) {                                    \
        READY;                                                                                                                    \
        return exec_host_integrated(IO, p, iq8, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, out_form, scale, out);          \
    }
#define SDRK_IQ8_READY                                                                                                            \
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st

SDRK_KURTOSIS_IQ8_ENTRIES(kurtosis_iq8, sk_iq8_io(iq8_format), SDRK_IQ8_READY)
SDRK_KURTOSIS_IQ8_ENTRIES(pfb_kurtosis_iq8, sk_pfb_iq8_io(p, iq8_format), SDRK_PFB_IQ8_READY)
#undef SDRK_IQ8_READY
#undef SDRK_PFB_IQ8_READY
#undef SDRK_KURTOSIS_IQ8_ENTRIES

// ---- two-channel cross-spectra: four planes per group, always the scaled-power form (detector and out_form are not read) ----

#define SDRK_XSPEC_ENTRIES(SUFFIX, IO)                                                                                             \
    int sdrk_exec_device_##SUFFIX(sdrk_plan* p, const void* d_iq2, size_t n_groups, size_t k_frames, size_t frame_stride,         \
                                  float scale, float* d_out, void* stream) {                                                      \
        return exec_device_integrated(IO, p, d_iq2, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, scale,   \
                                      d_out, stream);                                                                             \
    }                                                                                                                             \
    int sdrk_exec_device_##SUFFIX##_timed_each(sdrk_plan* p, const void* d_iq2, size_t n_groups, size_t k_frames,                 \
                                               size_t frame_stride, float scale, float* d_out, int launches, float* each_ms) {   \
        return exec_device_integrated_timed_each(IO, p, d_iq2, n_groups, k_frames, frame_stride, SDRK_DET_MEAN,                   \
                                                 SDRK_INT_OUT_POWER, scale, d_out, launches, each_ms);                            \
    }                                                                                                                             \
    int sdrk_exec_host_##SUFFIX(sdrk_plan* p, const void* iq2, size_t n_groups, size_t k_frames, size_t frame_stride,             \
                                float scale, float* out) {                                                                        \
        return exec_host_integrated(IO, p, iq2, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, scale, out); \
    }

SDRK_XSPEC_ENTRIES(xspec, xspec_c64_io())
SDRK_XSPEC_ENTRIES(xspec_ci16, xspec_ci16_io())
#undef SDRK_XSPEC_ENTRIES

// ---- correlation matrix of 2..8 channels: channels * channels planes per group, always the scaled-power form ----
// (FMT_ARG: nothing, or the 8-bit format right after the samples; READY: its refusal; FMT: the sdrk::CmFormat)

#define SDRK_CORRMAT_ENTRIES(SUFFIX, FMT_ARG, READY, FMT)                                                                          \
    int sdrk_exec_device_##SUFFIX(sdrk_plan* p, const void* d_iq FMT_ARG, int channels, size_t n_groups, size_t k_frames,         \
                                  size_t frame_stride, float scale, float* d_out, void* stream) {                                \
        READY;                                                                                                                    \
        if (int st = check_corrmat_channels(channels); st != SDRK_OK) return st;                                                  \
        const IntIo io = corrmat_io(channels, FMT);                                                                               \
        if (int st = check_corrmat(io, p, d_iq, n_groups, k_frames, frame_stride, d_out); st != SDRK_OK) return st;               \
        return exec_device_integrated(io, p, d_iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, scale,    \
                                      d_out, stream);                                                                             \
    }                                                                                                                             \
    int sdrk_exec_device_##SUFFIX##_timed_each(sdrk_plan* p, const void* d_iq FMT_ARG, int channels, size_t n_groups,             \
                                               size_t k_frames, size_t frame_stride, float scale, float* d_out, int launches,    \
                                               float* each_ms) {                                                                  \
        READY;                                                                                                                    \
        if (int st = check_corrmat_channels(channels); st != SDRK_OK) return st;                                                  \
        const IntIo io = corrmat_io(channels, FMT);                                                                               \
        if (int st = check_corrmat(io, p, d_iq, n_groups, k_frames, frame_stride, d_out); st != SDRK_OK) return st;               \
        return exec_device_integrated_timed_each(io, p, d_iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN,                    \
                                                 SDRK_INT_OUT_POWER, scale, d_out, launches, each_ms);                            \
    }                                                                                                                             \
    int sdrk_exec_host_##SUFFIX(sdrk_plan* p, const void* iq FMT_ARG, int channels, size_t n_groups, size_t k_frames,             \
                                size_t frame_stride, float scale, float* out) {                                                  \
        READY;                                                                                                                    \
        if (int st = check_corrmat_channels(channels); st != SDRK_OK) return st;                                                  \
        const IntIo io = corrmat_io(channels, FMT);                                                                               \
        if (int st = check_corrmat(io, p, iq, n_groups, k_frames, frame_stride, out); st != SDRK_OK) return st;                   \
        return exec_host_integrated(io, p, iq, n_groups, k_frames, frame_stride, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, scale, out); \
    }
#define SDRK_NO_ARG
#define SDRK_IQ8_ARG , int iq8_format
#define SDRK_IQ8_READY                                                                                                            \
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st

SDRK_CORRMAT_ENTRIES(corrmat, SDRK_NO_ARG, (void)0, sdrk::CM_C64)
SDRK_CORRMAT_ENTRIES(corrmat_ci16, SDRK_NO_ARG, (void)0, sdrk::CM_S16)
SDRK_CORRMAT_ENTRIES(corrmat_iq8, SDRK_IQ8_ARG, SDRK_IQ8_READY, cm_format_of_iq8(iq8_format))
#undef SDRK_IQ8_READY
#undef SDRK_IQ8_ARG
#undef SDRK_NO_ARG
#undef SDRK_CORRMAT_ENTRIES

}  // extern "C"

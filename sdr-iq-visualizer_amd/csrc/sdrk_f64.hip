// sdrk_f64.hip — host side of the double-precision entry points of include/sdrk.h (sdrk_plan_create_f64, sdrk_exec_*_f64):
// the reference's own arithmetic, complex128 samples in and float64 power_db out (app/sdr/streamer.py:119-121).  An f64 plan
// is an ordinary sdrk_plan with precision 64; the numpy boundary is sdrk_host_pipeline.hip's (sdrk_host::exec_host) with
// 16-byte samples, and the transforms are fft_f64.hip's.  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "kernels_f64.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

// Scratch between the two passes of nfft > 4096: up to 192 MiB of complex128 frames (at least one frame: 64 MiB at 2^22).
constexpr size_t SCRATCH64_BYTES = (size_t)192 << 20;

int launch64(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t s) {
    if (p->precision != 64) return fail(SDRK_ERR_INVALID, "float64 transform requested of a float32 plan");
    sdrk::F64Args a;
    a.d_iq = d_in;
    a.frame_stride = stride;
    a.d_out = d_out;
    a.n_frames = n_frames;
    a.nfft = p->nfft;
    a.d_window = p->d_window64;
    a.d_twiddle = p->d_tw64;
    a.d_scratch = p->d_scratch64;
    a.scratch_frames = p->scratch_frames;
    a.eps = p->eps64;
    a.shift = p->shift;
    a.epilogue = epilogue;
    a.stream = s;
    const hipError_t e = sdrk::launch_fft_f64(a);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "float64 transform launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

// complex128 in; float64 rows or complex128 out.  Only the one-pass lengths read and write pinned host memory from the kernel
// (the column pass of the two-pass lengths reads short segments: the copy engines move them faster).
sdrk_host::HostIo f64_io(int epilogue) {
    sdrk_host::HostIo io;
    io.in_elem = 2 * sizeof(double);
    io.out_elem = epilogue == sdrk::EPI64_DB ? sizeof(double) : 2 * sizeof(double);
    io.epilogue = epilogue;
    io.precision = 64;
    io.zero_copy_max_nfft = sdrk::F64_TILE;
    io.launch = launch64;
    return io;
}

}  // namespace

extern "C" {

int sdrk_plan_create_f64(int device, int nfft, size_t max_batch, int window_kind, const double* window, double eps,
                         int shift, sdrk_plan** out) {
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (nfft < 2 || nfft > (1 << SDRK_MAX_LOG2_NFFT))
        return fail(SDRK_ERR_INVALID, "nfft=%d: float64 plans take powers of two in [2, 2^%d]", nfft, SDRK_MAX_LOG2_NFFT);
    if (!is_pow2(nfft))
        return fail(SDRK_ERR_UNSUPPORTED, "nfft=%d: float64 plans take powers of two in [2, 2^%d] only (no chirp-z in double)",
                    nfft, SDRK_MAX_LOG2_NFFT);
    if (max_batch == 0) return fail(SDRK_ERR_INVALID, "max_batch must be >= 1");
    if (window_kind < SDRK_WINDOW_RECT || window_kind > SDRK_WINDOW_CUSTOM)
        return fail(SDRK_ERR_INVALID, "unknown window_kind %d", window_kind);
    if (window_kind == SDRK_WINDOW_CUSTOM && !window)
        return fail(SDRK_ERR_INVALID, "SDRK_WINDOW_CUSTOM needs a window pointer");
    if (!(eps >= 0.0)) return fail(SDRK_ERR_INVALID, "eps must be >= 0");
    int st = sdrk_host::check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SDRK_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);

    sdrk_plan* p = new (std::nothrow) sdrk_plan();
    if (!p) return fail(SDRK_ERR_NOMEM, "out of host memory");
    p->precision = 64;
    p->device = device;
    p->nfft = nfft;
    p->max_batch = max_batch;
    p->eps = (float)eps;          // (reported only; the transform uses eps64)
    p->eps64 = eps;
    p->shift = shift ? 1 : 0;
    p->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

#define PLAN_TRY(expr)                                                                     \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            int s__ = fail(e__ == hipErrorOutOfMemory ? SDRK_ERR_NOMEM : SDRK_ERR_HIP,     \
                           "%s failed: %s", #expr, hipGetErrorString(e__));                \
            sdrk_plan_destroy(p);                                                          \
            return s__;                                                                    \
        }                                                                                  \
    } while (0)

    PLAN_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    PLAN_TRY(hipEventCreate(&p->ev0));
    PLAN_TRY(hipEventCreate(&p->ev1));
    if (window_kind != SDRK_WINDOW_RECT) {
        std::vector<double> w((size_t)nfft);
        if (window_kind == SDRK_WINDOW_HANN) {
            // numpy.hanning(M) as numpy forms it: n = arange(1-M, M, 2); 0.5 + 0.5*cos(pi*n/(M-1))
            const double m1 = (double)(nfft - 1);
            for (int i = 0; i < nfft; ++i) w[(size_t)i] = 0.5 + 0.5 * std::cos(M_PI * (double)(1 - nfft + 2 * i) / m1);
        } else {
            memcpy(w.data(), window, sizeof(double) * (size_t)nfft);
        }
        PLAN_TRY(hipMalloc((void**)&p->d_window64, sizeof(double) * (size_t)nfft));
        PLAN_TRY(hipMemcpy(p->d_window64, w.data(), sizeof(double) * (size_t)nfft, hipMemcpyHostToDevice));
    }
    // W_4096^m = exp(-2 pi i m / 4096): every sub-transform of fft_f64.hip indexes this one table
    std::vector<double> tw(2 * (size_t)sdrk::F64_TWIDDLES);
    for (int m = 0; m < sdrk::F64_TWIDDLES; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)sdrk::F64_TWIDDLES;
        tw[2 * (size_t)m] = std::cos(a);
        tw[2 * (size_t)m + 1] = std::sin(a);
    }
    PLAN_TRY(hipMalloc((void**)&p->d_tw64, sizeof(double) * tw.size()));
    PLAN_TRY(hipMemcpy(p->d_tw64, tw.data(), sizeof(double) * tw.size(), hipMemcpyHostToDevice));
    if (nfft > sdrk::F64_TILE) {
        size_t frames = SCRATCH64_BYTES / ((size_t)nfft * 2 * sizeof(double));
        if (frames < 1) frames = 1;
        if (frames > max_batch) frames = max_batch;
        p->scratch_frames = frames;
        PLAN_TRY(hipMalloc(&p->d_scratch64, frames * (size_t)nfft * 2 * sizeof(double)));
    }
#undef PLAN_TRY
    *out = p;
    return SDRK_OK;
}

int sdrk_plan_precision(const sdrk_plan* p) { return p ? p->precision : fail(SDRK_ERR_INVALID, "plan is NULL"); }

int sdrk_exec_host_f64(sdrk_plan* p, const void* iq_c128, size_t n_frames, size_t frame_stride, double* out_db) {
    return sdrk_host::exec_host(p, iq_c128, n_frames, frame_stride, out_db, f64_io(sdrk::EPI64_DB));
}

int sdrk_exec_fft_host_f64(sdrk_plan* p, const void* iq_c128, size_t n_frames, size_t frame_stride, void* out_c128) {
    return sdrk_host::exec_host(p, iq_c128, n_frames, frame_stride, out_c128, f64_io(sdrk::EPI64_COMPLEX));
}

int sdrk_exec_device_f64(sdrk_plan* p, const void* d_iq_c128, size_t n_frames, size_t frame_stride, double* d_out_db,
                         void* stream) {
    int st = sdrk_host::check_exec_args(p, d_iq_c128, n_frames, frame_stride, d_out_db, 64);
    if (st != SDRK_OK || n_frames == 0) return st;
    HIP_TRY(hipSetDevice(p->device));
    return launch64(p, d_iq_c128, n_frames, frame_stride, d_out_db, sdrk::EPI64_DB,
                    stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int sdrk_exec_device_f64_timed_each(sdrk_plan* p, const void* d_iq_c128, size_t n_frames, size_t frame_stride,
                                    double* d_out_db, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = sdrk_host::check_exec_args(p, d_iq_c128, n_frames, frame_stride, d_out_db, 64);
    if (st != SDRK_OK) return st;
    if (n_frames == 0) return fail(SDRK_ERR_INVALID, "nothing to time (n_frames is 0)");
    return sdrk_host::timed_each(
        p, launches, each_ms, [&] { return launch64(p, d_iq_c128, n_frames, frame_stride, d_out_db, sdrk::EPI64_DB, p->stream); });
}

}  // extern "C"

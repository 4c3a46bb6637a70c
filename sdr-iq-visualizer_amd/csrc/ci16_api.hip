// ci16_api.hip — host side of the int16 entry points of include/sdrk.h (sdrk_exec_*_ci16, sdrk_synth_fill_ci16): interleaved
// little-endian int16 I,Q in — what the AD936x behind app/sdr/streamer.py:114 produces and SigMF calls ci16_le — and the rows or
// spectra of an ordinary float32 plan out, bit-identical to the complex64 entry points on the widened samples.
//
// Lengths with an int16-reading transform (4096: fft4096_ci16.hip; 256 ... 16384: fft_lds.hip) are one launch on the caller's
// data.  Every other length (N < 256, the two-pass lengths 2^15 ... 2^22 with the persistent N = 65536 form, chirp-z) runs
// "widen a chunk of frames into plan-owned complex64 staging, then plan_launch" on the same stream, the staging capped at
// 64 MiB however many frames the call has.  The numpy boundary is sdrk_host_pipeline.hip's exec_host with 4-byte samples.
// The integrated int16 entries are integrate_api.hip.
//
// The 8-bit entry points (sdrk_exec_*_ci8: SigMF ci8 / cu8, 2 bytes per sample, the format right after the input pointer) live
// here too, on the same machinery: N = 4096 is one launch of fft4096_ci8.hip on the caller's data, every other length the same
// unpack route with kernels_ci8.h's widening copy in front (launch_ci8).  Their integrated forms are integrate_api.hip's.
//
// The real-input entry points (sdrk_plan_set_real_window, sdrk_exec_*_real: SigMF rf32_le / ri16_le / ri8 / ru8) live here as
// well: a frame of 2 * nfft real samples is a frame of nfft pairs in the complex format of the same width, so the pointers,
// strides and staging are these (kernels_real.h has the arithmetic, rspec4096.hip and real_kernels.hip the kernels).  Their
// integrated forms (sdrk_exec_*_real_integrated) are integrate_call.h's call with rows of nfft + 1 bins: rspec4096_groups.hip
// reduces inside the transform at N = 4096, every other length runs launch_real into staging and integrate_rows.hip over it.
// Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "integrate_call.h"
#include "kernels_ci16.h"
#include "kernels_ci8.h"
#include "kernels_real.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

constexpr size_t CI16_STAGE_BYTES = (size_t)64 << 20;   // complex64 staging of the unpack route, per plan
constexpr size_t CI16_ELEM = 4;                          // bytes per int16 I,Q sample
constexpr size_t CI8_ELEM = 2;                           // bytes per 8-bit I,Q sample
constexpr int FMT_CI16 = -1;                             // unpack_route's format: int16, or an SDRK_IQ8_* value

// in_elem: bytes per input sample; fmt: FMT_CI16, or the 8-bit format whose widening copy feeds the staging instead.
int unpack_route(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream,
                 size_t in_elem = CI16_ELEM, int fmt = FMT_CI16) {
    auto unpack = [&](const void* src, size_t row_stride, void* dst, size_t n_rows, size_t row_len) {
        return fmt == FMT_CI16 ? sdrk::launch_unpack_ci16(src, row_stride, dst, n_rows, row_len, p->num_cus, stream)
                               : sdrk::launch_unpack_ci8(src, fmt, row_stride, dst, n_rows, row_len, p->num_cus, stream);
    };
    const size_t nfft = (size_t)p->nfft;
    const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    if (n_frames == 1) stride = nfft;
    // Overlapped frames are widened as the one contiguous run they are cut from (each sample once, the halo of a chunk's
    // last frame included) and keep their stride; packed or spaced frames are widened frame by frame into packed staging.
    const bool overlapped = stride < nfft;
    const size_t cap = CI16_STAGE_BYTES / sizeof(float2);   // samples; one frame is at most 2^22 of them
    size_t per = overlapped ? (cap - nfft) / stride + 1 : cap / nfft;
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    const size_t st_stride = overlapped ? stride : nfft;
    sdrk_host::Staging& sg = p->ci16;   // one staging per plan (int16 and 8-bit calls share it: complex64 either way): a call
                                        // on another stream waits for the last one's reads
    int st = sg.reserve(0, ((per - 1) * st_stride + nfft) * sizeof(float2));
    if (st == SDRK_OK) st = sg.enter(stream);
    if (st != SDRK_OK) return st;
    void* const d_stage = sg.buf[0].d;
    // N = 65536: the form is chosen for the call, not for its chunks (plan_launch's call_frames) — 128-frame chunks would never
    // reach the persistent kernel's threshold.  Two consequences: a short last chunk (513 frames: 128 x 4 + 1) runs the persistent
    // kernel too, and fused_check's mailbox holds the last 64 launches, so of a call of more than 64 chunks (8192 frames) only
    // the last 64 are covered by the error check behind sdrk_plan_sync.
    for (size_t f0 = 0; f0 < n_frames && st == SDRK_OK; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        const char* src = static_cast<const char*>(d_in) + f0 * stride * in_elem;
        hipError_t e;
        if (overlapped || stride == nfft)
            e = unpack(src, 0, d_stage, 1, (nf - 1) * st_stride + nfft);
        else
            e = unpack(src, stride, d_stage, nf, nfft);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "%s unpack launch failed: %s", fmt == FMT_CI16 ? "ci16" : "ci8", hipGetErrorString(e));
            break;
        }
        st = plan_launch(p, d_stage, nf, st_stride, static_cast<char*>(d_out) + f0 * nfft * out_elem, epilogue, stream,
                         nullptr, nullptr, nullptr, n_frames);
    }
    return sg.leave(stream, st);   // (also after a failed launch: earlier chunks are in flight)
}

}  // namespace

// One transform of a float32 plan on int16 input: the ci16 form of plan_launch, the LaunchFn of the ci16 numpy boundary
// and the transform of the int16 integrated calls (integrate_api.hip); declared in plan_internal.h.
int sdrk_host::launch_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "ci16 transform requested of a float64 plan");
    if (n_frames == 0) return SDRK_OK;
    const bool flagship = p->nfft == 4096 && !p->blu_inner;
    if (!flagship && (p->blu_inner || !sdrk::fft_lds_ci16_supports(p->nfft, stride)))
        return unpack_route(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = flagship ? sdrk::launch_fft4096_ci16(a) : sdrk::launch_fft_lds_ci16(a);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "ci16 kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

// One transform of a float32 plan on 8-bit I,Q input of format `fmt` (SDRK_IQ8_*): N = 4096 is fft4096_ci8.hip on the caller's
// data, every other length (the fft_lds lengths too: that kernel has no 8-bit format) the unpack route.  launch_ci8_fn gives
// the LaunchFn of a format, for the numpy boundary and the integrated calls; declared in plan_internal.h.
int sdrk_host::launch_ci8(sdrk_plan* p, const void* d_in, int fmt, size_t n_frames, size_t stride, void* d_out, int epilogue,
                          hipStream_t stream) {
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "ci8 transform requested of a float64 plan");
    if (n_frames == 0) return SDRK_OK;
    if (p->nfft != 4096 || p->blu_inner) return unpack_route(p, d_in, n_frames, stride, d_out, epilogue, stream, CI8_ELEM, fmt);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = sdrk::launch_fft4096_ci8(a, fmt);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "ci8 kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

namespace {

template <int FMT>
int launch_ci8_bound(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return launch_ci8(p, d_in, FMT, n_frames, stride, d_out, epilogue, stream);
}

}  // namespace

LaunchFn sdrk_host::launch_ci8_fn(int fmt) {
    return fmt == SDRK_IQ8_SIGNED ? launch_ci8_bound<SDRK_IQ8_SIGNED> : launch_ci8_bound<SDRK_IQ8_UNSIGNED>;
}

int sdrk_host::check_iq8_format(const sdrk_plan* p, int fmt) {
    if (fmt != SDRK_IQ8_SIGNED && fmt != SDRK_IQ8_UNSIGNED)
        return fail(SDRK_ERR_INVALID, "iq8_format %d is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED", fmt);
    if (p && p->precision != 32) return fail(SDRK_ERR_INVALID, "8-bit I,Q input needs a float32 plan: this one is float64");
    return SDRK_OK;
}

namespace {

// byte pairs in; float32 rows or complex64 out.  The kernel reads and writes pinned host memory itself at N = 4096 only (every
// other length is the unpack route).  SDRK_CI8_ZERO_COPY=0 sends those chunks through the copy engines instead: A/B work
// (tools/bench_ci8.py).
HostIo ci8_io(int fmt, int epilogue) {
    HostIo io = frames_io(CI8_ELEM, 0, launch_ci8_fn(fmt), epilogue);
    const char* env = getenv("SDRK_CI8_ZERO_COPY");
    if (!(env && env[0] == '0')) io.zero_copy_min_nfft = io.zero_copy_max_nfft = 4096;
    return io;
}

// int16 pairs in; float32 rows or complex64 out.  The kernel reads and writes pinned host memory itself only at the lengths
// whose transform reads int16 (the unpack route would cross PCIe for its staging's sake).
HostIo ci16_io(int epilogue) {
    HostIo io = frames_io(CI16_ELEM, 0, launch_ci16, epilogue);
    io.zero_copy_min_nfft = 256;
    io.zero_copy_max_nfft = 16384;
    return io;
}

// ---- real-sampled input (sdrk_exec_*_real): frames of 2 * nfft real samples read as nfft pairs, rows of nfft + 1 bins ----
// N = 4096 is one launch of rspec4096.hip on the caller's data.  Every other power of two 16 ... 2^20 runs, per chunk of
// frames, "widen and window into complex64 pairs -> the plan's own transform with its window and fftshift off -> split into the
// caller's rows" on the same stream, each of the two stagings capped at 64 MiB however many frames the call has.

constexpr size_t REAL_STAGE_BYTES = (size_t)64 << 20;
constexpr int REAL_MIN_NFFT = 16, REAL_MAX_NFFT = 1 << 20;

int check_real_plan(const sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "real-sampled input needs a float32 plan: this one is float64");
    if (p->blu_inner || !is_pow2(p->nfft))
        return fail(SDRK_ERR_UNSUPPORTED, "real-sampled input needs a power-of-two plan length: nfft=%d is a chirp-z plan", p->nfft);
    if (p->nfft < REAL_MIN_NFFT || p->nfft > REAL_MAX_NFFT)
        return fail(SDRK_ERR_UNSUPPORTED, "real-sampled input serves nfft = 16 ... 2^20 (real frames of 32 ... 2^21): this plan has nfft=%d",
                    p->nfft);
    return SDRK_OK;
}

int real_epilogue(int out_form) { return out_form == SDRK_REAL_OUT_DB ? sdrk::EPI_LOGPSD : sdrk::EPI_COMPLEX; }

// Everything a real-input entry refuses, nothing launched: frame_stride in REAL samples, out_stride in output elements.
int check_real_exec(const sdrk_plan* p, const void* x, int fmt, size_t n_frames, size_t frame_stride, int out_form, const void* out,
                    size_t out_stride) {
    int st = check_real_plan(p);
    if (st != SDRK_OK) return st;
    if (fmt != SDRK_REAL_F32 && fmt != SDRK_REAL_S16 && fmt != SDRK_REAL_S8 && fmt != SDRK_REAL_U8)
        return fail(SDRK_ERR_INVALID, "real_format %d is none of SDRK_REAL_F32, _S16, _S8, _U8", fmt);
    if (out_form != SDRK_REAL_OUT_DB && out_form != SDRK_REAL_OUT_COMPLEX)
        return fail(SDRK_ERR_INVALID, "out_form %d is neither SDRK_REAL_OUT_DB nor SDRK_REAL_OUT_COMPLEX", out_form);
    if (n_frames == 0) return SDRK_OK;
    if (!x || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1 for more than one frame");
    if (frame_stride & 1)
        return fail(SDRK_ERR_INVALID, "frame_stride %zu is odd: real frames start at a pair of samples (odd hops are not provided)",
                    frame_stride);
    const size_t pair = sdrk::real_pair_bytes(fmt);
    if (reinterpret_cast<uintptr_t>(x) % pair != 0)
        return fail(SDRK_ERR_INVALID, "input pointer %p is not aligned to a pair of samples (%zu bytes)", x, pair);
    const size_t bins = (size_t)p->nfft + 1;
    if (out_stride != 0 && out_stride < bins)
        return fail(SDRK_ERR_INVALID, "out_stride %zu is below the row length nfft + 1 = %zu (0: packed)", out_stride, bins);
    const size_t out_elem = out_form == SDRK_REAL_OUT_DB ? sizeof(float) : sizeof(float2);
    if (reinterpret_cast<uintptr_t>(out) % out_elem != 0)
        return fail(SDRK_ERR_INVALID, "output pointer %p is not aligned to its element (%zu bytes)", out, out_elem);
    return SDRK_OK;
}

int ensure_real_tab(sdrk_plan* p) {   // exp(-i pi k / N) in double, rounded once
    if (p->d_real_tab) return SDRK_OK;
    const size_t n = (size_t)p->nfft;
    std::vector<float2> t(n);
    for (size_t k = 0; k < n; ++k) {
        const double a = -M_PI * (double)k / (double)n;
        t[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    float2* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, n * sizeof(float2)));
    const hipError_t e = hipMemcpy(d, t.data(), n * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(SDRK_ERR_HIP, "hipMemcpy of the split table failed: %s", hipGetErrorString(e));
    }
    p->d_real_tab = d;
    return SDRK_OK;
}

// One real-input transform of the plan: `stride` in PAIRS, out_stride in output elements (>= nfft + 1).
int launch_real(sdrk_plan* p, const void* d_x, int fmt, size_t n_frames, size_t stride, void* d_out, size_t out_stride, int epilogue,
                hipStream_t stream) {
    if (n_frames == 0) return SDRK_OK;
    int st = ensure_real_tab(p);
    if (st != SDRK_OK) return st;
    const size_t nfft = (size_t)p->nfft;
    if (n_frames == 1) stride = nfft;
    sdrk::RealArgs a;
    a.d_x = d_x;
    a.fmt = fmt;
    a.frame_stride = stride;
    a.n_frames = n_frames;
    a.nfft = p->nfft;
    a.d_window = p->d_real_win;
    a.d_tab = p->d_real_tab;
    a.d_twiddle = p->d_twiddle;
    a.eps = p->eps;
    a.epilogue = epilogue;
    a.d_out = d_out;
    a.out_stride = out_stride;
    a.stream = stream;
    a.num_cus = p->num_cus;
    if (p->nfft == 4096) {
        const hipError_t e = sdrk::launch_rspec4096(a);
        if (e != hipSuccess) return fail(SDRK_ERR_HIP, "real-input kernel launch failed: %s", hipGetErrorString(e));
        return SDRK_OK;
    }
    const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    size_t per = REAL_STAGE_BYTES / (nfft * sizeof(float2));   // one frame is at most 2^20 pairs = 8 MiB
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    sdrk_host::Staging& sg = p->real;   // one staging per plan: a call on another stream waits for the last one's reads
    st = sg.reserve(0, per * nfft * sizeof(float2));
    if (st == SDRK_OK) st = sg.reserve(1, per * nfft * sizeof(float2));
    if (st == SDRK_OK) st = sg.enter(stream);
    if (st != SDRK_OK) return st;
    // the plan's transform with its own window and fftshift off: the mode has its own window, and the split reads natural order
    float* const plan_window = p->d_window;
    const int plan_shift = p->shift;
    p->d_window = nullptr;
    p->shift = 0;
    for (size_t f0 = 0; f0 < n_frames && st == SDRK_OK; f0 += per) {
        a.n_frames = n_frames - f0 < per ? n_frames - f0 : per;
        a.d_x = static_cast<const char*>(d_x) + f0 * stride * sdrk::real_pair_bytes(fmt);
        a.d_out = static_cast<char*>(d_out) + f0 * out_stride * out_elem;
        hipError_t e = sdrk::launch_real_pairs(a, sg.buf[0].d);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "real-input pairs launch failed: %s", hipGetErrorString(e));
            break;
        }
        // N = 65536: the form is chosen for the call, not for its chunks, as in the int16 route
        st = plan_launch(p, sg.buf[0].d, a.n_frames, nfft, sg.buf[1].d, sdrk::EPI_COMPLEX, stream, nullptr, nullptr, nullptr, n_frames);
        if (st != SDRK_OK) break;
        e = sdrk::launch_real_split(a, sg.buf[1].d);
        if (e != hipSuccess) st = fail(SDRK_ERR_HIP, "real-input split launch failed: %s", hipGetErrorString(e));
    }
    p->d_window = plan_window;
    p->shift = plan_shift;
    return sg.leave(stream, st);   // (also after a failed launch: earlier chunks are in flight)
}

// The LaunchFn of a format for the numpy boundary: packed rows of nfft + 1 bins.
template <int FMT>
int launch_real_bound(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return launch_real(p, d_in, FMT, n_frames, stride, d_out, (size_t)p->nfft + 1, epilogue, stream);
}

LaunchFn real_launch_fn(int fmt) {
    return fmt == SDRK_REAL_F32   ? launch_real_bound<SDRK_REAL_F32>
           : fmt == SDRK_REAL_S16 ? launch_real_bound<SDRK_REAL_S16>
           : fmt == SDRK_REAL_S8  ? launch_real_bound<SDRK_REAL_S8>
                                  : launch_real_bound<SDRK_REAL_U8>;
}

// pairs in (8 / 4 / 2 bytes, the stride in pairs); float32 rows or complex64 of nfft + 1 bins out; through the copy engines
HostIo real_io(const sdrk_plan* p, int fmt, int epilogue) {
    HostIo io = frames_io(sdrk::real_pair_bytes(fmt), 0, real_launch_fn(fmt), epilogue);
    io.out_bins = (size_t)p->nfft + 1;
    return io;
}

// ---- integrated real input: one row of nfft + 1 bins per k frames ----

// pairs in, the stride in pairs; N = 4096: the kernel that reduces behind the split; every other length: packed complex64 rows
// of nfft + 1 bins from launch_real (its two stagings) into the call's own staging, reduced down the columns
IntIo real_int_io(const sdrk_plan* p, int fmt) {
    IntIo io;
    io.in_elem = sdrk::real_pair_bytes(fmt);
    io.fused = sdrk::launch_rspec4096_groups;
    io.transform = real_launch_fn(fmt);
    io.bins = (size_t)p->nfft + 1;
    io.real_fmt = fmt;
    return io;
}

// What the integrated real entries refuse: what a per-frame real entry does (check_real_exec), then what an integrated entry
// does (check_int_args); frame_stride in REAL samples.
int check_real_integrated(const sdrk_plan* p, const void* x, int fmt, size_t n_groups, size_t k, size_t frame_stride, int detector,
                          int out_form, const float* out) {
    int st = check_real_exec(p, x, fmt, 1, frame_stride, SDRK_REAL_OUT_DB, out, 0);
    if (st != SDRK_OK) return st;
    return check_int_args(p, x, n_groups, k, frame_stride, detector, out_form, out);
}

}  // namespace

extern "C" {

int sdrk_exec_host_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host(p, iq_ci16, n_frames, frame_stride, out_db, ci16_io(sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64) {
    return exec_host(p, iq_ci16, n_frames, frame_stride, out_c64, ci16_io(sdrk::EPI_COMPLEX));
}

int sdrk_exec_device_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                          void* stream) {
    return exec_device_frames(check_exec_f32, launch_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                     float* d_out_db, int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_exec_f32, launch_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, launches,
                                         each_ms);
}

int sdrk_exec_host_ci8(sdrk_plan* p, const void* iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride, float* out_db) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host(p, iq_ci8, n_frames, frame_stride, out_db, ci8_io(iq8_format, sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host_ci8(sdrk_plan* p, const void* iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride, void* out_c64) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host(p, iq_ci8, n_frames, frame_stride, out_c64, ci8_io(iq8_format, sdrk::EPI_COMPLEX));
}

int sdrk_exec_device_ci8(sdrk_plan* p, const void* d_iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride, float* d_out_db,
                         void* stream) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_frames(check_exec_f32, launch_ci8_fn(iq8_format), p, d_iq_ci8, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_ci8_timed_each(sdrk_plan* p, const void* d_iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride,
                                    float* d_out_db, int launches, float* each_ms) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_frames_timed_each(check_exec_f32, launch_ci8_fn(iq8_format), p, d_iq_ci8, n_frames, frame_stride, d_out_db,
                                         launches, each_ms);
}

int sdrk_plan_set_real_window(sdrk_plan* p, const float* w, size_t n) {
    int st = check_real_plan(p);
    if (st != SDRK_OK) return st;
    const size_t len = 2 * (size_t)p->nfft;
    if (n != 0 && n != len)
        return fail(SDRK_ERR_INVALID, "real window of %zu coefficients: a plan of nfft=%d takes 2*nfft = %zu (or NULL / 0 for none)",
                    n, p->nfft, len);
    if (n != 0 && !w) return fail(SDRK_ERR_INVALID, "real window pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    // not with work in flight; safe all the same for work on the plan's own stream and staging
    HIP_TRY(hipStreamSynchronize(p->stream));
    st = p->real.wait();
    if (st != SDRK_OK) return st;
    if (n == 0) {
        if (p->d_real_win) HIP_TRY(hipFree(p->d_real_win));
        p->d_real_win = nullptr;
        return SDRK_OK;
    }
    if (!p->d_real_win) HIP_TRY(hipMalloc((void**)&p->d_real_win, len * sizeof(float)));
    HIP_TRY(hipMemcpy(p->d_real_win, w, len * sizeof(float), hipMemcpyHostToDevice));   // (the coefficients are copied)
    return SDRK_OK;
}

int sdrk_exec_device_real(sdrk_plan* p, const void* d_x, int real_format, size_t n_frames, size_t frame_stride, int out_form,
                          void* d_out, size_t out_stride, void* stream) {
    int st = check_real_exec(p, d_x, real_format, n_frames, frame_stride, out_form, d_out, out_stride);
    if (st != SDRK_OK || n_frames == 0) return st;
    HIP_TRY(hipSetDevice(p->device));
    return launch_real(p, d_x, real_format, n_frames, frame_stride / 2, d_out, out_stride ? out_stride : (size_t)p->nfft + 1,
                       real_epilogue(out_form), stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int sdrk_exec_device_real_timed_each(sdrk_plan* p, const void* d_x, int real_format, size_t n_frames, size_t frame_stride,
                                     int out_form, void* d_out, size_t out_stride, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_real_exec(p, d_x, real_format, n_frames, frame_stride, out_form, d_out, out_stride);
    if (st != SDRK_OK) return st;
    st = timed_each(p, launches, each_ms, [&] {
        return launch_real(p, d_x, real_format, n_frames, frame_stride / 2, d_out, out_stride ? out_stride : (size_t)p->nfft + 1,
                           real_epilogue(out_form), p->stream);
    });
    return st == SDRK_OK ? fused_check(p) : st;
}

int sdrk_exec_host_real(sdrk_plan* p, const void* x, int real_format, size_t n_frames, size_t frame_stride, float* out_db) {
    int st = check_real_exec(p, x, real_format, n_frames, frame_stride, SDRK_REAL_OUT_DB, out_db, 0);
    if (st != SDRK_OK) return st;
    return exec_host(p, x, n_frames, frame_stride / 2, out_db, real_io(p, real_format, sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host_real(sdrk_plan* p, const void* x, int real_format, size_t n_frames, size_t frame_stride, void* out_c64) {
    int st = check_real_exec(p, x, real_format, n_frames, frame_stride, SDRK_REAL_OUT_COMPLEX, out_c64, 0);
    if (st != SDRK_OK) return st;
    return exec_host(p, x, n_frames, frame_stride / 2, out_c64, real_io(p, real_format, sdrk::EPI_COMPLEX));
}

int sdrk_exec_device_real_integrated(sdrk_plan* p, const void* d_x, int real_format, size_t n_groups, size_t k_frames,
                                     size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream) {
    int st = check_real_integrated(p, d_x, real_format, n_groups, k_frames, frame_stride, detector, out_form, d_out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    st = ensure_real_tab(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated(real_int_io(p, real_format), p, d_x, n_groups, k_frames, frame_stride / 2, detector, out_form,
                                  scale, d_out, stream);
}

int sdrk_exec_device_real_integrated_timed_each(sdrk_plan* p, const void* d_x, int real_format, size_t n_groups, size_t k_frames,
                                                size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_real_integrated(p, d_x, real_format, n_groups, k_frames, frame_stride, detector, out_form, d_out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    st = ensure_real_tab(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(real_int_io(p, real_format), p, d_x, n_groups, k_frames, frame_stride / 2, detector,
                                             out_form, scale, d_out, launches, each_ms);
}

int sdrk_exec_host_real_integrated(sdrk_plan* p, const void* x, int real_format, size_t n_groups, size_t k_frames,
                                   size_t frame_stride, int detector, int out_form, float scale, float* out) {
    int st = check_real_integrated(p, x, real_format, n_groups, k_frames, frame_stride, detector, out_form, out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    st = ensure_real_tab(p);
    if (st != SDRK_OK) return st;
    return exec_host_integrated(real_int_io(p, real_format), p, x, n_groups, k_frames, frame_stride / 2, detector, out_form, scale,
                                out);
}

int sdrk_synth_fill_ci16(int device, uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft, void* d_iq_ci16,
                         void* stream) {
    if (n_frames == 0) return SDRK_OK;
    if (!d_iq_ci16) return fail(SDRK_ERR_INVALID, "d_iq is NULL");
    if (nfft < 2 || (nfft & 1)) return fail(SDRK_ERR_INVALID, "nfft must be even and >= 2");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = sdrk::launch_synth_fill_ci16(seed, first_frame, n_frames, nfft, d_iq_ci16, s);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "synth launch failed: %s", hipGetErrorString(e));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SDRK_OK;
}

}  // extern "C"

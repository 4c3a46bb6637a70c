// pfb_api.hip — host side of the per-frame polyphase-filter-bank entry points of include/sdrk.h (sdrk_plan_set_pfb,
// sdrk_plan_pfb_taps, sdrk_exec_*_pfb, sdrk_exec_*_pfb_ci16, sdrk_exec_*_pfb_iq8): a prototype filter of T * nfft coefficients
// folds T consecutive blocks of a stream into each frame in front of the plan's transform (kernels_pfb.h has the exact
// arithmetic).  The stream is complex64, or interleaved little-endian int16 I,Q at 4 bytes per sample: x[n] = float32(I[n]) +
// i float32(Q[n]) exactly, then the bits of the complex64 call; or interleaved 8-bit I,Q (ci8 / cu8) at 2 bytes per sample,
// widened as kernels_ci8.h says, with the format bound into the launchers (launch_pfb_iq8_fn).  Sits in front of
// app/sdr/streamer.py:119-121; the reference has no counterpart.
//
// N = 4096 is one launch on the caller's stream (pfb4096.hip, pfb4096_i16.hip, pfb4096_iq8.hip: the fold in the transform's
// registers).  Every other length (single-pass, two-pass with the persistent N = 65536 form, chirp-z) runs "fold a chunk of
// frames into plan-owned complex64 staging (pfb_fold.hip, pfb_fold_i16.hip, pfb_fold_iq8.hip: no widened copy of an integer
// stream), then plan_launch" on the same stream, the staging capped at 64 MiB and cut at frame boundaries however many frames
// the call has.  The numpy boundary is sdrk_host_pipeline.hip's exec_host with an input span of T * nfft samples per frame: a
// chunk carries its (T - 1) * nfft samples of overlap.
// Integration over K folded frames is integrate_api.hip, with this file's launchers and checks.  Out of scope: double
// precision, waterfall appends.
// Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "kernels_pfb.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

constexpr size_t PFB_STAGE_BYTES = (size_t)64 << 20;   // folded complex64 frames of the generic route, per plan

// How pfb4096_kernel shares the frames among its workgroups: SDRK_PFB_ASSIGN = 0 / 1 / 2 (kernels_pfb.h) for A/B work,
// read when the prototype is set; the default is what measured fastest (profiles/pfb/SUMMARY.md).
int pfb_assign_default() {
    if (const char* env = getenv("SDRK_PFB_ASSIGN")) {
        const long v = atol(env);
        if (v >= sdrk::PFB_ASSIGN_STRIDE && v <= sdrk::PFB_ASSIGN_RUNS) return (int)v;
    }
    return sdrk::PFB_ASSIGN_XCD;
}

}  // namespace

// Which plans the PFB entry points serve: float32, rectangular window (the prototype is the window), taps set.
int sdrk_host::check_pfb_plan(const sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "the polyphase filter bank serves float32 plans only (this is a float64 plan)");
    if (p->d_window)
        return fail(SDRK_ERR_INVALID, "the polyphase filter bank needs a plan created with SDRK_WINDOW_RECT: the prototype is the window");
    return SDRK_OK;
}

int sdrk_host::check_pfb_ready(const sdrk_plan* p) {
    int st = check_pfb_plan(p);
    if (st != SDRK_OK) return st;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    return SDRK_OK;
}

int sdrk_host::check_pfb_exec(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    if (n_frames == 0) return fail(SDRK_ERR_INVALID, "n_frames must be >= 1");
    if (!in || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1 for more than one frame");
    return SDRK_OK;
}

namespace {

// The generic route of a PFB transform, for samples of in_elem bytes and the fold kernel that reads them (kernels_pfb.h's
// launch_pfb_fold or its int16 form).
using PfbFoldFn = hipError_t (*)(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                                 void* d_out, int num_cus, hipStream_t stream);
int pfb_fold_route(sdrk_plan* p, const void* d_in, size_t in_elem, PfbFoldFn fold, size_t n_frames, size_t stride, void* d_out,
                   int epilogue, hipStream_t stream) {
    const size_t nfft = (size_t)p->nfft;
    const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    size_t per = PFB_STAGE_BYTES / (nfft * sizeof(float2));   // one frame is at most 2^22 samples = 32 MiB
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    sdrk_host::Staging& sg = p->pfb;   // one staging per plan: a call on another stream waits for the last one's reads
    int st = sg.reserve(0, per * nfft * sizeof(float2));
    if (st == SDRK_OK) st = sg.enter(stream);
    if (st != SDRK_OK) return st;
    void* const d_stage = sg.buf[0].d;
    // N = 65536: the form is chosen for the call, not for its chunks (plan_launch's call_frames), as in the int16 route
    for (size_t f0 = 0; f0 < n_frames && st == SDRK_OK; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        const hipError_t e = fold(static_cast<const char*>(d_in) + f0 * stride * in_elem, stride, nf, p->nfft, p->d_pfb_h, p->pfb_taps,
                                  d_stage, p->num_cus, stream);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "pfb fold launch failed: %s", hipGetErrorString(e));
            break;
        }
        st = plan_launch(p, d_stage, nf, nfft, static_cast<char*>(d_out) + f0 * nfft * out_elem, epilogue, stream,
                         nullptr, nullptr, nullptr, n_frames);
    }
    return sg.leave(stream, st);   // (also after a failed launch: earlier chunks are in flight)
}

// One PFB transform of the plan on a raw stream of in_elem-byte samples: the folding N = 4096 kernel `flagship`, else the
// generic route with `fold`.
template <class Flagship>
int launch_pfb_any(sdrk_plan* p, const void* d_in, size_t in_elem, PfbFoldFn fold, Flagship flagship, size_t n_frames, size_t stride,
                   void* d_out, int epilogue, hipStream_t stream) {
    if (n_frames == 0) return SDRK_OK;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    if (p->nfft != 4096 || p->blu_inner) return pfb_fold_route(p, d_in, in_elem, fold, n_frames, stride, d_out, epilogue, stream);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = flagship(a, p->d_pfb_h, p->pfb_taps, p->pfb_assign);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "pfb kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

// The numpy boundary of a PFB mode: T * nfft samples of in_elem bytes per frame in; float32 rows or complex64 out; always
// through the copy engines (every sample is read T times: over PCIe it would cross T times)
int exec_host_pfb(size_t in_elem, LaunchFn launch, int epilogue, sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride,
                  void* out) {
    int st = check_pfb_exec(p, iq, n_frames, frame_stride, out);
    if (st != SDRK_OK) return st;
    const size_t span = (size_t)p->pfb_taps * (size_t)p->nfft;
    return exec_host(p, iq, n_frames, frame_stride, out, frames_io(in_elem, span, launch, epilogue));
}

}  // namespace

// The LaunchFns of the two PFB modes (the transforms of the numpy boundary and of integrate_api.hip's generic route too;
// declared in plan_internal.h).
int sdrk_host::launch_pfb(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return launch_pfb_any(p, d_in, sizeof(float2), sdrk::launch_pfb_fold, sdrk::launch_pfb4096, n_frames, stride, d_out, epilogue, stream);
}

int sdrk_host::launch_pfb_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue,
                               hipStream_t stream) {
    return launch_pfb_any(p, d_in, 4, sdrk::launch_pfb_fold_i16, sdrk::launch_pfb4096_i16, n_frames, stride, d_out, epilogue, stream);
}

namespace {

// 8-bit I,Q of format FMT (SDRK_IQ8_*): neither PfbFoldFn nor LaunchFn carries a format, so it is bound into the functions the
// tables hold, as ci16_api.hip's launch_ci8_fn binds it.  2 bytes per sample in.
template <int FMT>
int launch_pfb_iq8_bound(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return launch_pfb_any(
        p, d_in, 2, sdrk::launch_pfb_fold_iq8<FMT>,
        [](const sdrk::LaunchArgs& a, const float* d_h, int taps, int assign) { return sdrk::launch_pfb4096_iq8(a, FMT, d_h, taps, assign); },
        n_frames, stride, d_out, epilogue, stream);
}

// The refusals of an 8-bit PFB entry in front of the call's own: the plan's (the _ci16 twin's words), then the format's.
int check_pfb_iq8(const sdrk_plan* p, int fmt) {
    int st = check_pfb_ready(p);
    if (st == SDRK_OK) st = check_iq8_format(p, fmt);
    return st;
}

}  // namespace

LaunchFn sdrk_host::launch_pfb_iq8_fn(int fmt) {
    return fmt == SDRK_IQ8_SIGNED ? launch_pfb_iq8_bound<SDRK_IQ8_SIGNED> : launch_pfb_iq8_bound<SDRK_IQ8_UNSIGNED>;
}

extern "C" {

int sdrk_plan_set_pfb(sdrk_plan* p, int taps, const float* h) {
    int st = check_pfb_plan(p);
    if (st != SDRK_OK) return st;
    if (taps < 1 || taps > sdrk::PFB_MAX_TAPS) return fail(SDRK_ERR_INVALID, "taps=%d: must be in [1, %d]", taps, sdrk::PFB_MAX_TAPS);
    if (!h) return fail(SDRK_ERR_INVALID, "prototype pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    // not with work in flight, says the header; make it safe all the same for work on the plan's own stream and staging
    HIP_TRY(hipStreamSynchronize(p->stream));
    st = p->pfb.wait();
    if (st == SDRK_OK) st = p->integ.wait();   // sdrk_exec_*_pfb_integrated reads the prototype too
    if (st != SDRK_OK) return st;
    const size_t bytes = (size_t)taps * (size_t)p->nfft * sizeof(float);
    p->pfb_taps = 0;
    if (p->d_pfb_h) {
        HIP_TRY(hipFree(p->d_pfb_h));
        p->d_pfb_h = nullptr;
    }
    HIP_TRY(hipMalloc((void**)&p->d_pfb_h, bytes));
    HIP_TRY(hipMemcpy(p->d_pfb_h, h, bytes, hipMemcpyHostToDevice));
    p->pfb_taps = taps;
    p->pfb_assign = pfb_assign_default();
    return SDRK_OK;
}

int sdrk_plan_pfb_taps(const sdrk_plan* p) { return p ? p->pfb_taps : fail(SDRK_ERR_INVALID, "plan is NULL"); }

int sdrk_exec_device_pfb(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db, void* stream) {
    return exec_device_frames(check_pfb_exec, launch_pfb, p, d_iq, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_pfb_timed_each(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db,
                                    int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_pfb_exec, launch_pfb, p, d_iq, n_frames, frame_stride, d_out_db, launches, each_ms);
}

int sdrk_exec_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host_pfb(sizeof(float2), launch_pfb, sdrk::EPI_LOGPSD, p, iq, n_frames, frame_stride, out_db);
}

int sdrk_exec_fft_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out_c64) {
    return exec_host_pfb(sizeof(float2), launch_pfb, sdrk::EPI_COMPLEX, p, iq, n_frames, frame_stride, out_c64);
}

int sdrk_exec_device_pfb_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                              void* stream) {
    return exec_device_frames(check_pfb_exec, launch_pfb_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_pfb_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                         float* d_out_db, int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_pfb_exec, launch_pfb_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, launches,
                                         each_ms);
}

int sdrk_exec_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host_pfb(4, launch_pfb_ci16, sdrk::EPI_LOGPSD, p, iq_ci16, n_frames, frame_stride, out_db);
}

int sdrk_exec_fft_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64) {
    return exec_host_pfb(4, launch_pfb_ci16, sdrk::EPI_COMPLEX, p, iq_ci16, n_frames, frame_stride, out_c64);
}

int sdrk_exec_device_pfb_iq8(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_frames, size_t frame_stride, float* d_out_db,
                             void* stream) {
    if (int st = check_pfb_iq8(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_frames(check_pfb_exec, launch_pfb_iq8_fn(iq8_format), p, d_iq8, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_pfb_iq8_timed_each(sdrk_plan* p, const void* d_iq8, int iq8_format, size_t n_frames, size_t frame_stride,
                                        float* d_out_db, int launches, float* each_ms) {
    if (int st = check_pfb_iq8(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_frames_timed_each(check_pfb_exec, launch_pfb_iq8_fn(iq8_format), p, d_iq8, n_frames, frame_stride, d_out_db,
                                         launches, each_ms);
}

int sdrk_exec_host_pfb_iq8(sdrk_plan* p, const void* iq8, int iq8_format, size_t n_frames, size_t frame_stride, float* out_db) {
    if (int st = check_pfb_iq8(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_pfb(2, launch_pfb_iq8_fn(iq8_format), sdrk::EPI_LOGPSD, p, iq8, n_frames, frame_stride, out_db);
}

int sdrk_exec_fft_host_pfb_iq8(sdrk_plan* p, const void* iq8, int iq8_format, size_t n_frames, size_t frame_stride, void* out_c64) {
    if (int st = check_pfb_iq8(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_pfb(2, launch_pfb_iq8_fn(iq8_format), sdrk::EPI_COMPLEX, p, iq8, n_frames, frame_stride, out_c64);
}

}  // extern "C"

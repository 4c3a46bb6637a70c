// pfb_api.hip — host side of the polyphase-filter-bank entry points of include/sdrk.h (sdrk_plan_set_pfb, sdrk_plan_pfb_taps,
// sdrk_exec_*_pfb): a prototype filter of T * nfft coefficients folds T consecutive blocks of a stream into each frame in front
// of the plan's transform (kernels_pfb.h has the exact arithmetic).  Sits in front of app/sdr/streamer.py:119-121; the reference
// has no counterpart.
//
// N = 4096 is one launch on the caller's stream (pfb4096.hip: the fold in the transform's registers).  Every other length
// (single-pass, two-pass with the persistent N = 65536 form, chirp-z) runs "fold a chunk of frames into plan-owned complex64
// staging, then plan_launch" on the same stream, the staging capped at 64 MiB and cut at frame boundaries however many frames
// the call has.  The numpy boundary is sdrk_host_pipeline.hip's exec_host with an input span of T * nfft samples per frame:
// a chunk carries its (T - 1) * nfft samples of overlap.
// Integration over K folded frames is pfb_groups_api.hip; int16 I,Q input is pfb_ci16_api.hip, which runs this file's generic
// route and argument checks with its own fold kernel.  Out of scope: double precision, waterfall appends.
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

// The staging only grows, and never under work that still reads it: whatever was enqueued on it last is waited for first.
int pfb_stage_reserve(sdrk_plan* p, size_t need) {
    if (!p->ev_pfb) HIP_TRY(hipEventCreateWithFlags(&p->ev_pfb, hipEventDisableTiming));
    if (need <= p->pfb_stage_cap) return SDRK_OK;
    if (p->pfb_busy) HIP_TRY(hipEventSynchronize(p->ev_pfb));
    if (p->d_pfb_stage) {
        HIP_TRY(hipFree(p->d_pfb_stage));
        p->d_pfb_stage = nullptr;
        p->pfb_stage_cap = 0;
    }
    HIP_TRY(hipMalloc(&p->d_pfb_stage, need));
    p->pfb_stage_cap = need;
    return SDRK_OK;
}

}  // namespace

// The generic route of a PFB transform, for samples of in_elem bytes and the fold kernel that reads them (declared in
// plan_internal.h: pfb_ci16_api.hip hands in its own).
int sdrk_host::pfb_fold_route(sdrk_plan* p, const void* d_in, size_t in_elem, PfbFoldFn fold, size_t n_frames, size_t stride,
                              void* d_out, int epilogue, hipStream_t stream) {
    const size_t nfft = (size_t)p->nfft;
    const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    size_t per = PFB_STAGE_BYTES / (nfft * sizeof(float2));   // one frame is at most 2^22 samples = 32 MiB
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    int st = pfb_stage_reserve(p, per * nfft * sizeof(float2));
    if (st != SDRK_OK) return st;
    // one staging per plan: a call on another stream waits for the last one's reads
    if (p->pfb_busy && p->pfb_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, p->ev_pfb, 0));
    // N = 65536: the form is chosen for the call, not for its chunks (plan_launch's call_frames), as in the int16 route
    for (size_t f0 = 0; f0 < n_frames && st == SDRK_OK; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        const hipError_t e = fold(static_cast<const char*>(d_in) + f0 * stride * in_elem, stride, nf, p->nfft, p->d_pfb_h, p->pfb_taps,
                                  p->d_pfb_stage, p->num_cus, stream);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "pfb fold launch failed: %s", hipGetErrorString(e));
            break;
        }
        st = plan_launch(p, p->d_pfb_stage, nf, nfft, static_cast<char*>(d_out) + f0 * nfft * out_elem, epilogue, stream,
                         nullptr, nullptr, nullptr, n_frames);
    }
    const hipError_t e = hipEventRecord(p->ev_pfb, stream);   // (also after a failed launch: earlier chunks are in flight)
    p->pfb_stream = stream;
    p->pfb_busy = true;
    if (st == SDRK_OK && e != hipSuccess) st = fail(SDRK_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    return st;
}

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

// complex64 stream in, T * nfft samples per frame; float32 rows or complex64 out; always through the copy engines (every
// sample is read T times: over PCIe it would cross T times)
HostIo pfb_io(const sdrk_plan* p, int epilogue) {
    HostIo io;
    io.in_elem = sizeof(float2);
    io.out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    io.epilogue = epilogue;
    io.precision = 32;
    io.in_span = (size_t)p->pfb_taps * (size_t)p->nfft;
    io.launch = launch_pfb;
    return io;
}

}  // namespace

// One PFB transform of the plan on a raw complex64 stream: a LaunchFn (the transform of the numpy boundary and of
// pfb_groups_api.hip's generic route too; declared in plan_internal.h).
int sdrk_host::launch_pfb(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    if (n_frames == 0) return SDRK_OK;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    if (p->nfft != 4096 || p->blu_inner)
        return pfb_fold_route(p, d_in, sizeof(float2), sdrk::launch_pfb_fold, n_frames, stride, d_out, epilogue, stream);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = sdrk::launch_pfb4096(a, p->d_pfb_h, p->pfb_taps, p->pfb_assign);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "pfb kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
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
    if (p->pfb_busy) HIP_TRY(hipEventSynchronize(p->ev_pfb));
    if (p->int_busy) HIP_TRY(hipEventSynchronize(p->ev_int));   // sdrk_exec_*_pfb_integrated reads the prototype too
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
    int st = check_pfb_exec(p, d_iq, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return launch_pfb(p, d_iq, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD,
                      stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int sdrk_exec_device_pfb_timed_each(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db,
                                    int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_pfb_exec(p, d_iq, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    st = timed_each(p, launches, each_ms,
                    [&] { return launch_pfb(p, d_iq, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, p->stream); });
    return st == SDRK_OK ? fused_check(p) : st;
}

int sdrk_exec_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, float* out_db) {
    int st = check_pfb_exec(p, iq, n_frames, frame_stride, out_db);
    if (st != SDRK_OK) return st;
    return exec_host(p, iq, n_frames, frame_stride, out_db, pfb_io(p, sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out_c64) {
    int st = check_pfb_exec(p, iq, n_frames, frame_stride, out_c64);
    if (st != SDRK_OK) return st;
    return exec_host(p, iq, n_frames, frame_stride, out_c64, pfb_io(p, sdrk::EPI_COMPLEX));
}

}  // extern "C"

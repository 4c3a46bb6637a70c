// pfb_ci16_api.hip — the int16 polyphase-filter-bank entry points of include/sdrk.h (sdrk_exec_*_pfb_ci16 and
// sdrk_exec_*_pfb_integrated_ci16): the plan's prototype of T * nfft coefficients folds T consecutive blocks of a stream of
// interleaved little-endian int16 I,Q — 4 bytes per sample, as a radio or a SigMF ci16_le recording delivers it — into each
// frame in front of the plan's transform, per frame or reduced over K folded frames.  x[n] = float32(I[n]) + i float32(Q[n])
// exactly, then the bits sdrk_exec_*_pfb / sdrk_exec_*_pfb_integrated return for those widened samples: every length of a
// float32 rectangular plan, every T, hop, count, detector and form, device and host entries alike.
//
// N = 4096 is one launch on the caller's samples (pfb4096_i16.hip, pfb4096_i16_groups.hip).  Every other length folds the
// int16 samples straight into the plan's complex64 PFB staging (pfb_fold_i16.hip; no widened copy of the stream), then runs
// the plan's transform: pfb_api.hip's generic route with this file's fold kernel and 4-byte samples, under the same ev_pfb
// ordering.  The integrated call is integrate_call.h's with these launchers; the numpy boundary is exec_host /
// exec_host_integrated with 4-byte samples and an input span of T * nfft, so a chunk carries (T - 1) * nfft samples of overlap
// at half the bytes.  sdrk_plan_set_pfb waits on ev_pfb and ev_int, which covers these calls.
// Host code only (not named sdrk_*.hip, and not part of pfb_api.hip / pfb_groups_api.hip: their sanitizer builds link without
// stand-ins for the int16 kernels).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include "integrate_call.h"
#include "kernels_integrate.h"
#include "kernels_pfb.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

// int16 I,Q stream in, T * nfft samples per frame; float32 rows or complex64 out; always through the copy engines (every
// sample is read T times: over PCIe it would cross T times)
HostIo pfb_ci16_io(const sdrk_plan* p, int epilogue) {
    HostIo io;
    io.in_elem = 4;
    io.out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    io.epilogue = epilogue;
    io.precision = 32;
    io.in_span = (size_t)p->pfb_taps * (size_t)p->nfft;
    io.launch = launch_pfb_ci16;
    return io;
}

IntIo pfb_ci16_groups_io(const sdrk_plan* p) {
    IntIo io;
    io.in_elem = 4;
    io.fused = sdrk::launch_pfb4096_i16_groups;
    io.transform = launch_pfb_ci16;
    io.in_span = (size_t)p->pfb_taps * (size_t)p->nfft;
    return io;
}

}  // namespace

// One PFB transform of the plan on a raw int16 I,Q stream: a LaunchFn (declared in plan_internal.h).
int sdrk_host::launch_pfb_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue,
                               hipStream_t stream) {
    if (n_frames == 0) return SDRK_OK;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    if (p->nfft != 4096 || p->blu_inner)
        return pfb_fold_route(p, d_in, 4, sdrk::launch_pfb_fold_i16, n_frames, stride, d_out, epilogue, stream);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = sdrk::launch_pfb4096_i16(a, p->d_pfb_h, p->pfb_taps, p->pfb_assign);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "pfb kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

extern "C" {

int sdrk_exec_device_pfb_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                              void* stream) {
    int st = check_pfb_exec(p, d_iq_ci16, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return launch_pfb_ci16(p, d_iq_ci16, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD,
                           stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int sdrk_exec_device_pfb_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                         float* d_out_db, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_pfb_exec(p, d_iq_ci16, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    st = timed_each(p, launches, each_ms,
                    [&] { return launch_pfb_ci16(p, d_iq_ci16, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, p->stream); });
    return st == SDRK_OK ? fused_check(p) : st;
}

int sdrk_exec_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db) {
    int st = check_pfb_exec(p, iq_ci16, n_frames, frame_stride, out_db);
    if (st != SDRK_OK) return st;
    return exec_host(p, iq_ci16, n_frames, frame_stride, out_db, pfb_ci16_io(p, sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64) {
    int st = check_pfb_exec(p, iq_ci16, n_frames, frame_stride, out_c64);
    if (st != SDRK_OK) return st;
    return exec_host(p, iq_ci16, n_frames, frame_stride, out_c64, pfb_ci16_io(p, sdrk::EPI_COMPLEX));
}

int sdrk_exec_device_pfb_integrated_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                         size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated(pfb_ci16_groups_io(p), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale,
                                  d_out, stream);
}

int sdrk_exec_device_pfb_integrated_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                    size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                    int launches, float* each_ms) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(pfb_ci16_groups_io(p), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector,
                                             out_form, scale, d_out, launches, each_ms);
}

int sdrk_exec_host_pfb_integrated_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                       int detector, int out_form, float scale, float* out) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_host_integrated(pfb_ci16_groups_io(p), p, iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

}  // extern "C"

// ci16_api.hip — host side of the int16 entry points of include/sdrk.h (sdrk_exec_*_ci16, sdrk_synth_fill_ci16): interleaved
// little-endian int16 I,Q in — what the AD936x behind app/sdr/streamer.py:114 produces and SigMF calls ci16_le — and the rows or
// spectra of an ordinary float32 plan out, bit-identical to the complex64 entry points on the widened samples.
//
// Lengths with an int16-reading transform (4096: fft4096_ci16.hip; 256 ... 16384: fft_lds.hip) are one launch on the caller's
// data.  Every other length (N < 256, the two-pass lengths 2^15 ... 2^22 with the persistent N = 65536 form, chirp-z) runs
// "widen a chunk of frames into plan-owned complex64 staging, then plan_launch" on the same stream, the staging capped at
// 64 MiB however many frames the call has.  The numpy boundary is sdrk_host_pipeline.hip's exec_host with 4-byte samples.
// The integrated int16 entries are integrate_api.hip.  Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <vector>

#include "kernels_ci16.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

constexpr size_t CI16_STAGE_BYTES = (size_t)64 << 20;   // complex64 staging of the unpack route, per plan
constexpr size_t CI16_ELEM = 4;                          // bytes per int16 I,Q sample

int unpack_route(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
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
    sdrk_host::Staging& sg = p->ci16;   // one staging per plan: a call on another stream waits for the last one's reads
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
        const char* src = static_cast<const char*>(d_in) + f0 * stride * CI16_ELEM;
        hipError_t e;
        if (overlapped || stride == nfft)
            e = sdrk::launch_unpack_ci16(src, 0, d_stage, 1, (nf - 1) * st_stride + nfft, p->num_cus, stream);
        else
            e = sdrk::launch_unpack_ci16(src, stride, d_stage, nf, nfft, p->num_cus, stream);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "ci16 unpack launch failed: %s", hipGetErrorString(e));
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

namespace {

// int16 pairs in; float32 rows or complex64 out.  The kernel reads and writes pinned host memory itself only at the lengths
// whose transform reads int16 (the unpack route would cross PCIe for its staging's sake).
HostIo ci16_io(int epilogue) {
    HostIo io = frames_io(CI16_ELEM, 0, launch_ci16, epilogue);
    io.zero_copy_min_nfft = 256;
    io.zero_copy_max_nfft = 16384;
    return io;
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

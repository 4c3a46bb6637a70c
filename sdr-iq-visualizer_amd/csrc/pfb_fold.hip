// pfb_fold.hip — the polyphase-filter-bank fold for every length without a folding transform of its own (all but N = 4096:
// the single-pass lengths, the two-pass lengths, chirp-z): T blocks of nfft samples under T * nfft coefficients -> one folded
// frame of nfft complex64, packed, in plan-owned staging that the plan's own transform then reads (pfb_api.hip).
//   y[n] = (((h[n] x[n]) + h[N+n] x[N+n]) + h[2N+n] x[2N+n]) + ...      per real component, float32, no fused multiply-add
// the arithmetic of pfb4096.hip (kernels_pfb.h), which numpy reproduces on float32 arrays.
#include "kernels_pfb.h"
#include "pfb_fold_body.h"

namespace sdrk {

// One thread, one complex sample; a workgroup walks tiles of 256 consecutive samples of one frame (512 B per wave and load).
__global__ __launch_bounds__(256) void pfb_fold_kernel(const float2* __restrict__ iq, size_t frame_stride, size_t n_frames,
                                                       int nfft, const float* __restrict__ h, int taps,
                                                       float2* __restrict__ out) {
    pfb_fold_body<PfbFoldInC64>(iq, frame_stride, n_frames, nfft, h, taps, out);
}

hipError_t launch_pfb_fold(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                           void* d_out, int num_cus, hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    if (nfft < 1 || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const size_t tiles = n_frames * (((size_t)nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 256) * 16;
    hipLaunchKernelGGL(pfb_fold_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, stream,
                       static_cast<const float2*>(d_iq), frame_stride, n_frames, nfft, d_h, taps, static_cast<float2*>(d_out));
    return hipGetLastError();
}

}  // namespace sdrk

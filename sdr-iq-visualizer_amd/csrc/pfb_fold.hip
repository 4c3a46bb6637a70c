// pfb_fold.hip — the polyphase-filter-bank fold for every length without a folding transform of its own (all but N = 4096:
// the single-pass lengths, the two-pass lengths, chirp-z): T blocks of nfft samples under T * nfft coefficients -> one folded
// frame of nfft complex64, packed, in plan-owned staging that the plan's own transform then reads (pfb_api.hip).
//   y[n] = (((h[n] x[n]) + h[N+n] x[N+n]) + h[2N+n] x[2N+n]) + ...      per real component, float32, no fused multiply-add
// the arithmetic of pfb4096.hip (kernels_pfb.h), which numpy reproduces on float32 arrays.
#include "kernels_pfb.h"

namespace sdrk {

// One thread, one complex sample; a workgroup walks tiles of 256 consecutive samples of one frame (512 B per wave and load).
__global__ __launch_bounds__(256) void pfb_fold_kernel(const float2* __restrict__ iq, size_t frame_stride, size_t n_frames,
                                                       int nfft, const float* __restrict__ h, int taps,
                                                       float2* __restrict__ out) {
    const size_t tiles_per_frame = ((size_t)nfft + 255) / 256;
    const size_t tiles = n_frames * tiles_per_frame;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t f = tile / tiles_per_frame;
        const size_t n = (tile - f * tiles_per_frame) * 256 + threadIdx.x;
        if (n >= (size_t)nfft) continue;
        const float2* __restrict__ x = iq + f * frame_stride + n;
        const float* __restrict__ c = h + n;
        const float2 x0 = x[0];
        pfb_v2f acc = pfb_mul(pfb_v2f{x0.x, x0.y}, c[0]);
        for (int t = 1; t < taps; ++t) {
            const float2 xt = x[(size_t)t * nfft];
            acc = pfb_mac(acc, pfb_v2f{xt.x, xt.y}, c[(size_t)t * nfft]);
        }
        out[f * (size_t)nfft + n] = make_float2(acc.x, acc.y);
    }
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

// pfb_fold_iq8.hip — pfb_fold.hip's fold reading interleaved 8-bit I,Q (SigMF ci8 / cu8, 2 bytes per sample), for every length
// without a folding transform of its own: T blocks of nfft samples under T * nfft coefficients -> one folded frame of nfft
// complex64, packed, straight into the plan's PFB staging (pfb_api.hip) — one pass, no widened copy of the stream.
// x[n] is kernels_ci8.h's conversion, exact, then the arithmetic of pfb_fold_kernel (kernels_pfb.h).  The conversion is a
// run-time argument of the one kernel; the format is bound into the launcher, which a host table holds.
#include "kernels_ci8.h"
#include "kernels_pfb.h"
#include "pfb_fold_body.h"

namespace sdrk {

// One thread, one sample; a workgroup walks tiles of 256 consecutive samples of one frame (128 B per wave and load).
__global__ __launch_bounds__(256) void pfb_fold_iq8_kernel(const unsigned short* __restrict__ iq, Iq8Conv conv, size_t frame_stride,
                                                           size_t n_frames, int nfft, const float* __restrict__ h, int taps,
                                                           float2* __restrict__ out) {
    pfb_fold_body<PfbFoldInIq8>(iq, frame_stride, n_frames, nfft, h, taps, out, PfbFoldInIq8{conv});
}

template <int FMT>
hipError_t launch_pfb_fold_iq8(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                               void* d_out, int num_cus, hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    if (nfft < 1 || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const size_t tiles = n_frames * (((size_t)nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 256) * 16;
    hipLaunchKernelGGL(pfb_fold_iq8_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(256), 0, stream,
                       static_cast<const unsigned short*>(d_iq), iq8_conv(FMT), frame_stride, n_frames, nfft, d_h, taps,
                       static_cast<float2*>(d_out));
    return hipGetLastError();
}

template hipError_t launch_pfb_fold_iq8<IQ8_SIGNED>(const void*, size_t, size_t, int, const float*, int, void*, int, hipStream_t);
template hipError_t launch_pfb_fold_iq8<IQ8_UNSIGNED>(const void*, size_t, size_t, int, const float*, int, void*, int, hipStream_t);

}  // namespace sdrk

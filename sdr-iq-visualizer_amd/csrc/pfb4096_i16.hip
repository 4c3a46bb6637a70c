// pfb4096_i16.hip — pfb4096.hip's kernel reading interleaved little-endian int16 I,Q, 4 bytes per sample: the T-tap fold in the
// transform's registers, then fft4096.hip's transform, fftshift and log epilogue.  x[n] = float32(I[n]) + i float32(Q[n])
// exactly, then pfb_mul / pfb_mac on the widened samples: the row is, bit for bit, pfb4096_kernel's for those samples.
// 4 T bytes read per output sample (4 from HBM at hop = N), 4 written.
//
// The body is pfb4096_body.h's — persistent grid, the three frame assignments, tap loop, one tap block in flight — with the
// int16 input policy of pfb4096_in.h: the block in flight is 16 dwords per thread beside its 16 coefficients, widened where it
// is multiplied in.  frame_stride counts samples; frame starts need 4-byte alignment only.
#include "pfb4096_body.h"

namespace sdrk {

// (integer template arguments only, and no format name in the parameter types: the code-object tests count kernels by
// fragments of their mangled names)
template <int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_i16_kernel(
    const unsigned* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw, size_t n_frames,
    const float* __restrict__ h, int taps, const float2* __restrict__ tw4096, float eps, int shift, int assign) {
    pfb4096_body<EPILOGUE, F4kInPfbI16>(iq, frame_stride, out_raw, n_frames, h, taps, tw4096, eps, shift, assign);
}

hipError_t launch_pfb4096_i16(const LaunchArgs& a, const float* d_h, int taps, int assign) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const unsigned* iq = static_cast<const unsigned*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    if (a.epilogue == EPI_LOGPSD)
        hipLaunchKernelGGL((pfb4096_i16_kernel<EPI_LOGPSD>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps,
                           tw, a.eps, a.shift, assign);
    else if (a.epilogue == EPI_COMPLEX)
        hipLaunchKernelGGL((pfb4096_i16_kernel<EPI_COMPLEX>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps,
                           tw, a.eps, a.shift, assign);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sdrk

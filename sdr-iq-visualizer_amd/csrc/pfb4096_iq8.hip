// pfb4096_iq8.hip — pfb4096.hip's kernel reading interleaved 8-bit I,Q (SigMF ci8 / cu8), 2 bytes per sample: the T-tap fold in
// the transform's registers, then fft4096.hip's transform, fftshift and log epilogue.
//   signed    x[n] = float32(I[n]) + i float32(Q[n])
//   unsigned  x[n] = (float32(I[n]) - 127.5f) + i (float32(Q[n]) - 127.5f)        (both exact)
// then pfb_mul / pfb_mac on the widened samples: the row is, bit for bit, pfb4096_kernel's for those samples.  2 T bytes read
// per output sample (2 from HBM at hop = N), 4 written.
//
// The body is pfb4096_body.h's — persistent grid, the three frame assignments, tap loop, one tap block in flight — with the
// 8-bit input policy of pfb4096_in.h: the block in flight is 16 zero-extended 16-bit words per thread beside its 16
// coefficients, widened where it is multiplied in with the call's conversion, a run-time argument: a format adds no
// instantiation.  frame_stride counts samples; frame starts need 2-byte alignment only, so any hop serves.
#include "pfb4096_body.h"

namespace sdrk {

// (integer template arguments only, and no counted fragment in the parameter types: the code-object tests count kernels by
// fragments of their mangled names)
template <int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_iq8_kernel(
    const unsigned short* __restrict__ iq, Iq8Conv conv, size_t frame_stride, void* __restrict__ out_raw, size_t n_frames,
    const float* __restrict__ h, int taps, const float2* __restrict__ tw4096, float eps, int shift, int assign) {
    pfb4096_body<EPILOGUE, F4kInPfbIq8>(iq, frame_stride, out_raw, n_frames, h, taps, tw4096, eps, shift, assign, F4kInPfbIq8{conv});
}

hipError_t launch_pfb4096_iq8(const LaunchArgs& a, int fmt, const float* d_h, int taps, int assign) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    if (fmt != IQ8_SIGNED && fmt != IQ8_UNSIGNED) return hipErrorInvalidValue;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const unsigned short* iq = static_cast<const unsigned short*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const Iq8Conv conv = iq8_conv(fmt);
    if (a.epilogue == EPI_LOGPSD)
        hipLaunchKernelGGL((pfb4096_iq8_kernel<EPI_LOGPSD>), g, b, 0, a.stream, iq, conv, a.frame_stride, a.d_out, a.n_frames, d_h,
                           taps, tw, a.eps, a.shift, assign);
    else if (a.epilogue == EPI_COMPLEX)
        hipLaunchKernelGGL((pfb4096_iq8_kernel<EPI_COMPLEX>), g, b, 0, a.stream, iq, conv, a.frame_stride, a.d_out, a.n_frames, d_h,
                           taps, tw, a.eps, a.shift, assign);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sdrk

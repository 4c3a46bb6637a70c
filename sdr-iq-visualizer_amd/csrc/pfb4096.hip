// pfb4096.hip — polyphase filter bank front end at N = 4096: T blocks of 4096 samples folded under a prototype filter of
// T * 4096 coefficients inside the transform's registers, then fft4096.hip's transform, fftshift and log epilogue unchanged.
// Sits in front of the reference's
//   app/sdr/streamer.py:119  fft_data = np.fft.fftshift(np.fft.fft(samples))
//   app/sdr/streamer.py:121  power_db = 20 * np.log10(np.abs(fft_data) + 1e-12)
// which has no counterpart of the fold (a build-side extension, like the decimated waterfall read-out): `samples` becomes
//   y[n] = (((h[n] x[n]) + h[N+n] x[N+n]) + h[2N+n] x[2N+n]) + ...      per real component, float32, no fused multiply-add
// 8 T bytes read per output sample where frames do not overlap their neighbours' blocks, 8 from HBM at hop = N (the other
// T - 1 readers of a block find it in cache), 4 bytes written.
//
// The kernel keeps fft4096_kernel's shape (persistent grid of three workgroups per CU, buffer loads, tables in LDS,
// f4k_transform, f4k_store_row).  Its input policy loads one tap block — 16 words per thread — and that block's 16
// coefficients, and accumulates into the 16 cf the transform takes.  One tap block is in flight beside the accumulators: the
// next tap's while this one is multiplied in, the next frame's first while this frame is transformed.  T is a run-time loop
// bound; the coefficients come through the cache with ordinary loads (T * 16 KiB does not fit beside the exchange buffer in LDS
// at three workgroups per CU).
//
// The body is pfb4096_body.h's (shared with the int16 form, pfb4096_i16.hip); this file instantiates it with F4kInPfb.
// Integration over K folded frames is pfb4096_groups.hip.  Out of scope here: double precision, waterfall appends.
#include "fft4096_core.h"
#include "kernels_pfb.h"
#include "pfb4096_body.h"
#include "pfb4096_in.h"

namespace sdrk {

template <int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw, size_t n_frames,
    const float* __restrict__ h, int taps, const float2* __restrict__ tw4096, float eps, int shift, int assign) {
    pfb4096_body<EPILOGUE, F4kInPfb>(iq, frame_stride, out_raw, n_frames, h, taps, tw4096, eps, shift, assign);
}

hipError_t launch_pfb4096(const LaunchArgs& a, const float* d_h, int taps, int assign) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    if (a.epilogue == EPI_LOGPSD)
        hipLaunchKernelGGL((pfb4096_kernel<EPI_LOGPSD>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps, tw,
                           a.eps, a.shift, assign);
    else if (a.epilogue == EPI_COMPLEX)
        hipLaunchKernelGGL((pfb4096_kernel<EPI_COMPLEX>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps, tw,
                           a.eps, a.shift, assign);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sdrk

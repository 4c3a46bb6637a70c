// pfb4096_groups.hip — the polyphase filter bank spectrometer at N = 4096 in one kernel: the T-tap fold of pfb4096.hip in the
// transform's registers, fft4096.hip's transform, and the reduction over K consecutive folded frames of fft4096_integrate.hip
// (mean with compensation, maximum or minimum of |Y|^2 per bin) — ONE row per group out, 4/K bytes written per sample where
// pfb4096_kernel writes 4.  The row is, bit for bit, what fft4096_integrate_kernel returns for the packed folded frames.
//
// Outer structure: fft4096_integrate_kernel's — persistent grid of F4K_WAVES workgroups per CU, whole units
// (integrate_split.h) grid-stride, carry-in / carry-out / partials rows, int_init / int_accumulate / int_reduced / int_epilogue.
// Per-frame input: pfb4096_kernel's — F4kInPfb, pfb_mul / pfb_mac, one tap block in flight beside the accumulators: the next
// tap's, the next frame's first, or across a unit boundary the next unit's first.  The K frames of a unit run back to back on
// one workgroup, so at hop = N a frame's first T - 1 blocks are the ones its predecessor just read.
//
// Registers: a tap block in flight (32 + 16) beside the transform's 32 + 32 and the accumulators does not fit the 168 VGPRs of
// three workgroups per CU.  So (1) the mean keeps its 16 compensation terms in LDS, in the 16 KiB where the windowed kernels keep
// the window (a PFB plan has none): 53376 bytes, the figure those kernels run three workgroups per CU at.  A thread touches
// only its own 16 words, once per frame, so they need no barrier.  Maximum and minimum have no compensation and stay at 36992
// bytes.  (2) Of the next frame's first tap only the samples are in flight during the transform; its 16 coefficients — the same
// 16 KiB of h for every frame — are issued right behind the transform, under the accumulation.
// The accumulation order per bin is frame-ascending whatever holds the state.
// The body is pfb4096_body.h's (shared with the int16 form, pfb4096_i16_groups.hip); this file instantiates it with F4kInPfb.
#include "fft4096_core.h"
#include "kernels_integrate.h"
#include "kernels_pfb.h"
#include "pfb4096_body.h"
#include "pfb4096_in.h"

namespace sdrk {

template <int DET>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_groups_kernel(
    const float2* __restrict__ iq, size_t frame_stride, IntUnits c, float* __restrict__ out, float2* __restrict__ partials,
    const float2* __restrict__ carry_in, float2* __restrict__ carry_out, const float* __restrict__ h, int taps,
    const float2* __restrict__ tw4096, int shift) {
    pfb4096_groups_body<DET, F4kInPfb>(iq, frame_stride, c, out, partials, carry_in, carry_out, h, taps, tw4096, shift);
}

hipError_t launch_pfb4096_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const IntUnits c = int_units(a);
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(D)                                                                                                   \
    hipLaunchKernelGGL((pfb4096_groups_kernel<D>), g, b, 0, a.stream, iq, a.in_stride, c, a.d_out, a.d_partials, a.d_carry_in, \
                       a.d_carry_out, a.d_pfb_h, a.pfb_taps, tw, a.shift)
    if (a.detector == INT_DET_MEAN) SDRK_LAUNCH(INT_DET_MEAN);
    else if (a.detector == INT_DET_MAX) SDRK_LAUNCH(INT_DET_MAX);
    else SDRK_LAUNCH(INT_DET_MIN);
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

// pfb4096_iq8_groups.hip — pfb4096_groups.hip's spectrometer kernel reading interleaved 8-bit I,Q (SigMF ci8 / cu8), 2 bytes per
// sample: the T-tap fold, the transform and the reduction over K consecutive folded frames (mean with compensation, maximum
// or minimum of |Y|^2 per bin) in one kernel, ONE row per group out.  Rows, partial rows and carry rows are, bit for bit,
// pfb4096_groups_kernel's for the widened samples (kernels_ci8.h has the conversion), so integrate_rows.hip's finalize serves.
//
// The body is pfb4096_body.h's with the 8-bit input policy of pfb4096_in.h: the same unit bookkeeping, carry and partial rows,
// the mean's compensation in the same 16 KiB of LDS, and across the transform only the next frame's samples in flight — 16
// zero-extended 16-bit words.  The conversion is a run-time argument: a format adds no instantiation.
#include "pfb4096_body.h"

namespace sdrk {

template <int DET>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_iq8_groups_kernel(
    const unsigned short* __restrict__ iq, Iq8Conv conv, size_t frame_stride, IntUnits c, float* __restrict__ out,
    float2* __restrict__ partials, const float2* __restrict__ carry_in, float2* __restrict__ carry_out, const float* __restrict__ h,
    int taps, const float2* __restrict__ tw4096, int shift) {
    pfb4096_groups_body<DET, F4kInPfbIq8>(iq, frame_stride, c, out, partials, carry_in, carry_out, h, taps, tw4096, shift,
                                          F4kInPfbIq8{conv});
}

template <int FMT>
hipError_t launch_pfb4096_iq8_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const IntUnits c = int_units(a);
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const unsigned short* iq = static_cast<const unsigned short*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const Iq8Conv conv = iq8_conv(FMT);
#define SDRK_LAUNCH(D)                                                                                                        \
    hipLaunchKernelGGL((pfb4096_iq8_groups_kernel<D>), g, b, 0, a.stream, iq, conv, a.in_stride, c, a.d_out, a.d_partials,    \
                       a.d_carry_in, a.d_carry_out, a.d_pfb_h, a.pfb_taps, tw, a.shift)
    if (a.detector == INT_DET_MEAN) SDRK_LAUNCH(INT_DET_MEAN);
    else if (a.detector == INT_DET_MAX) SDRK_LAUNCH(INT_DET_MAX);
    else SDRK_LAUNCH(INT_DET_MIN);
#undef SDRK_LAUNCH
    return hipGetLastError();
}

template hipError_t launch_pfb4096_iq8_groups<IQ8_SIGNED>(const IntegrateArgs&);
template hipError_t launch_pfb4096_iq8_groups<IQ8_UNSIGNED>(const IntegrateArgs&);

}  // namespace sdrk

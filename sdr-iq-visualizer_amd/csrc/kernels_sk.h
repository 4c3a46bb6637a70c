// kernels_sk.h — interface between integrate_api.hip and the spectral-kurtosis kernels (sk4096.hip: the N = 4096 transform with
// the two running sums in its registers; sk_rows.hip: the sums over complex spectra of any length, and the finalize of split
// groups).  Same calls, units, carry rows and partial rows as the integrating kernels (kernels_integrate.h, integrate_split.h);
// what differs is the unit state — a float2 per bin {S1, S2} = {sum p, sum p^2}, plain float32 sums in frame order — and the
// output: two planes of nfft float32 per group, the mean power S1 / K through the integrating epilogue and the estimator
//   SK = (K+1)/(K-1) * (K * S2 / S1^2 - 1)                                   (Nita & Gary; 1 for Gaussian noise at any level)
// IntegrateArgs::detector is not read.  The row of group g is at d_out + (g - out_row0) * 2 * nfft.
#pragma once
#include "kernels_integrate.h"

namespace sdrk {

hipError_t launch_sk4096(const IntegrateArgs& a);       // complex64 samples
hipError_t launch_sk4096_i16(const IntegrateArgs& a);   // interleaved int16 I,Q: the same bits on the widened samples
// sk4096_iq8.hip: interleaved 8-bit I,Q of format FMT (an SDRK_IQ8_* value, bound in as kernels_ci8.h's launchers bind it;
// explicitly instantiated for the two formats): the same bits on the widened samples
template <int FMT>
hipError_t launch_sk4096_iq8(const IntegrateArgs& a);
hipError_t launch_sk_rows(const IntegrateArgs& a);      // complex64 spectra in staging (EPI_COMPLEX, the plan's shift order)
// slices > 1: S1, S2 of group g = the partials[g * slices + s] added in ascending s in float64 and rounded to float32 once
// (the argument list of launch_integrate_finalize; `detector` is not read)
hipError_t launch_sk_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int detector,
                              int out_form, float scale, float eps, float* d_out, int num_cus, hipStream_t stream);

// The estimator from the float32 sums of a group of kf = (float)K frames: the one place it is written — the fused epilogue,
// the column kernel, the finalize and the host stand-in (tests/fake_sk_kernels.cpp) all call it.  IEEE division, no
// reciprocal.  A bin without power (S1 = 0, or S1^2 below the float32 range) gives 0, never NaN: a dead bin is as
// non-Gaussian as a carrier.  No guard where p^2 or S1^2 leaves the float32 range upwards (|X| above about 4e9).
__host__ __device__ __forceinline__ float sk_estimate(float s1, float s2, float kf) {
    const float d = s1 * s1;
    if (d == 0.0f) return 0.0f;
    const float c = (kf + 1.0f) / (kf - 1.0f);   // (the same for every bin: computed once per unit)
    return c * (kf * s2 / d - 1.0f);
}

// One more frame's power.
__host__ __device__ __forceinline__ void sk_accumulate(float& s1, float& s2, float p) {
    s1 += p;
    s2 = __builtin_fmaf(p, p, s2);
}

}  // namespace sdrk

// kernels_xspec.h — interface between integrate_api.hip and the two-channel cross-spectrum kernels (xspec4096.hip: the N = 4096
// transform run on both channels of an element frame with the four running sums in its registers; xspec_rows.hip: the
// de-interleave, the sums down the columns of two staged spectra of any length, and the finalize of split groups).  Same calls,
// units, carry rows and partial rows as the integrating kernels (kernels_integrate.h, integrate_split.h); what differs is
//   - the input: a stream of ELEMENTS, element n = sample n of channel 0 then sample n of channel 1 (complex64: 4 float32
//     I0 Q0 I1 Q1; int16: 4 little-endian int16, x = float32(I) + i float32(Q) exactly).  IntegrateArgs::in_stride counts elements;
//   - the unit state: FOUR floats per bin {Saa, Sbb, Sre, Sim}, plain float32 sums in frame order of (xs_accumulate)
//         paa = fmaf(ar, ar, ai*ai)   pbb = fmaf(br, br, bi*bi)   cre = (ar*br) + (ai*bi)   cim = (ai*br) - (ar*bi)     A conj(B)
//     so carry rows and partial rows are nfft float4 (the float2 pointers of IntegrateArgs are cast: row r of the partials is
//     at float4 index r * nfft);
//   - the output: four planes of nfft float32 per group, scale * S / K each (the POWER form of the integrating epilogue).
// IntegrateArgs::detector, out_form and eps are not read.  The row of group g is at d_out + (g - out_row0) * 4 * nfft.
#pragma once
#include "kernels_integrate.h"

namespace sdrk {

hipError_t launch_xspec4096(const IntegrateArgs& a);       // complex64 elements
hipError_t launch_xspec4096_i16(const IntegrateArgs& a);   // int16 elements: the same bits on the widened elements
// `n_frames` frames of nfft elements, `stride` elements apart, from d_in (`i16`: int16 elements) -> packed complex64 frames:
// channel 0's at d_ch0[f * nfft + n], channel 1's at d_ch1[f * nfft + n]
hipError_t launch_xspec_split(const void* d_in, bool i16, size_t n_frames, size_t stride, int nfft, float2* d_ch0, float2* d_ch1,
                              int num_cus, hipStream_t stream);
// complex64 spectra in staging (EPI_COMPLEX, the plan's shift order): channel 0's frames at d_in, channel 1's at d_in2, both
// in_stride complex64 apart
hipError_t launch_xspec_rows(const IntegrateArgs& a, const float2* d_in2);
// slices > 1: the four sums of group g = the partials[g * slices + s] added in ascending s in float64 and rounded to float32
// once (the argument list of launch_integrate_finalize; `detector`, `out_form` and `eps` are not read)
hipError_t launch_xspec_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int detector,
                                 int out_form, float scale, float eps, float* d_out, int num_cus, hipStream_t stream);

// The four sums of a bin.  (A type of this header: the stand-in runtime of the sanitizer builds has no float4.)
struct XsState {
    float aa, bb, re, im;
};

// One more frame's spectra A = (ar, ai), B = (br, bi): the one place the arithmetic is written — the fused epilogue, the column
// kernel and the host stand-in (tests/fake_xspec_kernels.cpp) all call it.  The build contracts within a statement
// (-ffp-contract=on), so the four products of the cross term sit in statements of their own and are rounded to float32 before
// they are added: swapping the channels then gives the exact conjugate, and two identical channels give im = 0 exactly.
// Its two terms stand on their own for the kernels that keep more than two channels (kernels_corrmat.h): xs_auto is |X|^2 of
// one spectrum, xs_cross the two parts of A conj(B).
__host__ __device__ __forceinline__ float xs_auto(float r, float i) { return __builtin_fmaf(r, r, i * i); }

__host__ __device__ __forceinline__ void xs_cross(float ar, float ai, float br, float bi, float& cre, float& cim) {
    const float rr = ar * br;
    const float ii = ai * bi;
    const float ir = ai * br;
    const float ri = ar * bi;
    cre = rr + ii;
    cim = ir - ri;
}

__host__ __device__ __forceinline__ void xs_accumulate(XsState& s, float ar, float ai, float br, float bi) {
    const float paa = xs_auto(ar, ai);
    const float pbb = xs_auto(br, bi);
    float cre, cim;
    xs_cross(ar, ai, br, bi, cre, cim);
    s.aa += paa;
    s.bb += pbb;
    s.re += cre;
    s.im += cim;
}

// A sum -> its output value, as int_epilogue's POWER form gives it from the mean: scale * (S * (1 / K)).
__host__ __device__ __forceinline__ float xs_output(float sum, float inv_k, float scale) {
    const float r = sum * inv_k;
    return scale * r;
}

}  // namespace sdrk

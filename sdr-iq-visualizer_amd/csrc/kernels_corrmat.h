// kernels_corrmat.h — interface between integrate_api.hip and the correlation-matrix kernels: the F-X split of a correlator for
// C = 2..8 coherent channels.  F: every channel of a frame is transformed ONCE and its complex64 spectrum kept in plan-owned
// staging (corrmat4096.hip reads the element stream itself at N = 4096; every other length de-interleaves with
// corrmat_split_kernel and runs the plan's own transform once per channel).  X: corrmat_rows.hip walks the frames of a unit
// down the C staged spectra with the whole C x C state of a bin in one thread's registers.  Same calls, units, carry rows and
// partial rows as the two-channel kernels (kernels_xspec.h, integrate_split.h); what differs is
//   - the input: element n = sample n of channel 0, 1, ... C - 1 (complex64, little-endian int16 pairs or byte pairs), aligned
//     to ONE SAMPLE of one channel only (C = 3, 5, 6, 7 make elements no power of two long);
//   - the unit state: C * C floats per bin, in the order of the output planes: the C autos, then for the pairs (0,1), (0,2), ...,
//     (C-2,C-1) the real and the imaginary sum.  Every term is xs_auto / xs_cross (kernels_xspec.h: the arithmetic is written
//     there once), every sum plain float32 in frame order.  Carry rows and partial rows are C * C PLANES of nfft floats (row r of
//     the partials at float index r * C * C * nfft, sum q of bin b at + q * nfft + b);
//   - the output: C * C planes of nfft float32 per group, xs_output of each sum.
// IntegrateArgs::detector, out_form and eps are not read.  The row of group g is at d_out + (g - out_row0) * C * C * nfft.
#pragma once
#include "kernels_ci8.h"
#include "kernels_integrate.h"
#include "kernels_xspec.h"

namespace sdrk {

constexpr int CM_MIN_CHANNELS = 2, CM_MAX_CHANNELS = 8;

// sample formats of an element stream
enum CmFormat : int { CM_C64 = 0, CM_S16 = 1, CM_B8_SIGNED = 2, CM_B8_UNSIGNED = 3 };
inline size_t cm_sample_bytes(int fmt) { return fmt == CM_C64 ? 8 : fmt == CM_S16 ? 4 : 2; }

// N = 4096: does the spectra kernel read this element stream itself, or do the split and the plan's transform come first?
// Measured (profiles/corrmat/SUMMARY.md: 2^13 frames, K = 16): the int16 and 8-bit forms are faster read directly at every C
// (C = 8: 2.81 against 3.53 ms, 2.17 against 3.23 ms); complex64 is at C = 2 (0.45 against 0.90 ms), level at C = 4 and 5
// (1.33 / 1.36, 1.89 / 1.91 ms) and slower at C = 8 (4.49 against 3.75 ms: its 8-byte loads stand 64 bytes apart, and a
// wave instruction touches 4 KiB for 512 bytes), so complex64 above 5 channels takes the split route.
constexpr int CM4K_C64_DIRECT_MAX_CHANNELS = 5;
inline bool cm4k_reads_directly(int fmt, int channels) { return fmt != CM_C64 || channels <= CM4K_C64_DIRECT_MAX_CHANNELS; }

// N = 4096: the frames [a.f0, a.f1) cut from the element stream at a.d_in (frame a.f0's first element; a.in_stride elements
// apart) -> shift-ordered complex64 spectra, channel c's frame f at d_spec[c * plane + (f - a.f0) * 4096]
hipError_t launch_corrmat4096_spectra(const IntegrateArgs& a, int fmt, int channels, float2* d_spec, size_t plane);
// any length: `n_frames` frames of nfft elements, `stride` elements apart -> packed complex64 frames, channel c's at
// d_ch[c * plane + f * nfft + n]
hipError_t launch_corrmat_split(const void* d_in, int fmt, int channels, size_t n_frames, size_t stride, int nfft, float2* d_ch,
                                size_t plane, int num_cus, hipStream_t stream);
// complex64 spectra in staging (the plan's shift order): channel c's frames at a.d_in + c * plane, a.in_stride complex64 apart
hipError_t launch_corrmat_rows(const IntegrateArgs& a, int channels, size_t plane);
// slices > 1: the sums of group g = the partials[g * slices + s] added in ascending s in float64, rounded to float32 once
hipError_t launch_corrmat_finalize(const float* d_partials, int channels, size_t n_groups, size_t k, size_t slices, int nfft,
                                   float scale, float* d_out, int num_cus, hipStream_t stream);

// One more frame's spectra x[c] = (xr[c], xi[c]) into the C * C sums of a bin, in plane order.  The one place the loop over
// the matrix is written: the column kernel and the host stand-in (tests/fake_corrmat_kernels.cpp) both call it.
template <int C>
__host__ __device__ __forceinline__ void cm_accumulate(float (&s)[C * C], const float (&xr)[C], const float (&xi)[C]) {
#pragma unroll
    for (int i = 0; i < C; ++i) s[i] += xs_auto(xr[i], xi[i]);
    int q = C;
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = i + 1; j < C; ++j, q += 2) {
            float cre, cim;
            xs_cross(xr[i], xi[i], xr[j], xi[j], cre, cim);
            s[q] += cre;
            s[q + 1] += cim;
        }
    }
}

}  // namespace sdrk

// kernels_pfb.h — internal interface between the polyphase-filter-bank entry points of the C ABI (pfb_api.hip) and their two
// gfx950 kernels.  A frame is the fold of `taps` consecutive blocks of nfft samples under a prototype h of taps * nfft float32
// coefficients, per real component in float32, every product and every sum rounded (no fused multiply-add), taps ascending:
//     y_f[n] = (((h[n] x[s+n]) + h[N+n] x[s+N+n]) + h[2N+n] x[s+2N+n]) + ...          s = f * frame_stride
// and the row is what the plan's complex64 transform with a rectangular window returns for y_f, bit for bit.
// LaunchArgs is kernels.h's; d_iq is the raw stream, (n_frames - 1) * frame_stride + taps * nfft samples.  Nothing here is exported.
#pragma once
#include "kernels.h"

namespace sdrk {

constexpr int PFB_MAX_TAPS = 32;

// How pfb4096_kernel's persistent workgroups share the frames (every input block is read by `taps` frames at hop = nfft):
enum PfbAssign : int {
    PFB_ASSIGN_STRIDE = 0,   // frame f -> workgroup f mod grid, as fft4096_kernel: the readers of a block sit on different XCDs
    PFB_ASSIGN_XCD = 1,      // workgroups b = x (mod 8) walk the x-th eighth of the frames together: a block's readers share an L2
                             // where workgroups are dealt round-robin to the XCDs (the result does not depend on it)
    PFB_ASSIGN_RUNS = 2,     // each workgroup a contiguous run of frames
};

// pfb4096.hip: N = 4096, fold in registers in front of f4k_transform; a.d_window must be null, a.nfft 4096
hipError_t launch_pfb4096(const LaunchArgs& a, const float* d_h, int taps, int assign);
// pfb_fold.hip: every other length — n_frames folded frames of nfft complex64, packed, into d_out
hipError_t launch_pfb_fold(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                           void* d_out, int num_cus, hipStream_t stream);

// The same two on interleaved little-endian int16 I,Q, 4 bytes per sample (pfb4096_i16.hip, pfb_fold_i16.hip): d_iq points at
// int16 pairs, frame_stride counts samples, x = float32(I) + i float32(Q) exactly, then the arithmetic above.
hipError_t launch_pfb4096_i16(const LaunchArgs& a, const float* d_h, int taps, int assign);
hipError_t launch_pfb_fold_i16(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                               void* d_out, int num_cus, hipStream_t stream);

// pfb4096_groups.hip: N = 4096, the fold in front of the transform and the reduction over K folded frames behind it, ONE row
// per group; an IntegrateArgs (kernels_integrate.h) with d_pfb_h / pfb_taps set, d_in the raw stream, d_window null
struct IntegrateArgs;
hipError_t launch_pfb4096_groups(const IntegrateArgs& a);
hipError_t launch_pfb4096_i16_groups(const IntegrateArgs& a);   // pfb4096_i16_groups.hip: d_in points at int16 pairs

// The three on interleaved 8-bit I,Q, 2 bytes per sample (pfb4096_iq8.hip, pfb_fold_iq8.hip, pfb4096_iq8_groups.hip): d_iq
// points at byte pairs, frame_stride counts samples, fmt / FMT is an SDRK_IQ8_* value and x the conversion of kernels_ci8.h,
// exact in float32, then the arithmetic above.  Where a host table holds the launcher the format is bound into it (explicitly
// instantiated for the two formats), as kernels_ci8.h does.
hipError_t launch_pfb4096_iq8(const LaunchArgs& a, int fmt, const float* d_h, int taps, int assign);
template <int FMT>
hipError_t launch_pfb_fold_iq8(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                               void* d_out, int num_cus, hipStream_t stream);
template <int FMT>
hipError_t launch_pfb4096_iq8_groups(const IntegrateArgs& a);

#ifdef __HIPCC__
typedef float pfb_v2f __attribute__((ext_vector_type(2)));
// One tap of the fold on a complex sample: the product rounded, then the sum rounded.  Contraction is switched off here whatever
// the build's -ffp-contract says: a fused multiply-add would differ from numpy's float32 arrays in the last bit.
__device__ __forceinline__ pfb_v2f pfb_mul(pfb_v2f x, float c) {
#pragma clang fp contract(off)
    const pfb_v2f p = x * c;
    return p;
}
__device__ __forceinline__ pfb_v2f pfb_mac(pfb_v2f acc, pfb_v2f x, float c) {
#pragma clang fp contract(off)
    const pfb_v2f p = x * c;
    const pfb_v2f s = acc + p;
    return s;
}
#endif

}  // namespace sdrk

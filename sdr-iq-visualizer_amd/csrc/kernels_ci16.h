// kernels_ci16.h — internal interface between the ci16 entry points of the C ABI (ci16_api.hip) and the gfx950 kernels that
// read interleaved little-endian int16 I,Q (4 bytes per sample).  x[n] = float32(I[n]) + i float32(Q[n]) exactly, then the
// arithmetic of the complex64 kernels: a ci16 call returns the bits the complex64 call returns for the same values.
// LaunchArgs is kernels.h's; d_iq points at int16 pairs, frame_stride counts samples.  Nothing here is exported.
#pragma once
#include "kernels.h"

namespace sdrk {

hipError_t launch_fft4096_ci16(const LaunchArgs& a);    // fft4096_ci16.hip: the flagship transform, 4 B in + 4 B out per sample
bool fft_lds_ci16_supports(int nfft, size_t frame_stride);   // 256 .. 16384 except 4096 (and a group span below 2 GiB)
hipError_t launch_fft_lds_ci16(const LaunchArgs& a);    // fft_lds.hip with the int16 input format
// int16 pairs -> complex64 for every other length: n_rows rows of row_len samples, row r read at sample r * in_row_stride and
// written packed (at r * row_len).  Row starts need 4-byte alignment only.
hipError_t launch_unpack_ci16(const void* d_in, size_t in_row_stride, void* d_out, size_t n_rows, size_t row_len, int num_cus,
                              hipStream_t stream);
hipError_t launch_synth_fill_ci16(uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft, void* d_iq,
                                  hipStream_t stream);

#ifdef __HIPCC__
// one dword = (I, Q) as two little-endian int16 -> float32 each (exact: |value| <= 32768 < 2^24)
__device__ __forceinline__ void ci16_unpack(unsigned w, float& re, float& im) {
    re = (float)(int)(short)(w & 0xFFFFu);
    im = (float)((int)w >> 16);
}
#endif

}  // namespace sdrk

// kernels_ci8.h — internal interface between the 8-bit entry points of the C ABI (ci16_api.hip, integrate_api.hip) and the
// gfx950 kernels that read interleaved 8-bit I,Q (2 bytes per sample, I then Q): SigMF ci8 (signed, what a HackRF writes) and
// cu8 (unsigned, what an RTL-SDR writes).
//   signed    x[n] = float32(I[n]) + i float32(Q[n])
//   unsigned  x[n] = (float32(I[n]) - 127.5f) + i (float32(Q[n]) - 127.5f)        (127.5: the mid-scale of 0 ... 255)
// both exact in float32, then the arithmetic of the complex64 kernels: an 8-bit call returns the bits the complex64 call
// returns for the same values.  One conversion serves both formats with run-time arguments (Iq8Conv), so a format adds no
// kernel instantiation.  LaunchArgs is kernels.h's and IntegrateArgs kernels_integrate.h's; the input pointers are to byte
// pairs, strides count samples.  The format is bound into the launchers the host tables hold (template argument FMT: an
// SDRK_IQ8_* value), so neither argument struct changes.  Nothing here is exported.
#pragma once
#include "kernels.h"
#include "kernels_integrate.h"

namespace sdrk {

constexpr int IQ8_SIGNED = 0, IQ8_UNSIGNED = 1;   // SDRK_IQ8_SIGNED / SDRK_IQ8_UNSIGNED of include/sdrk.h

// per component: (float)((w ^ mask) >> s & 0xFF) - off.  Signed bytes are biased to 0 ... 255 by flipping their sign bits and
// the bias comes off in float32, so byte 0 gives 128.0f - 128.0f = +0.0f: the conversion never produces -0.0f.
struct Iq8Conv {
    unsigned mask;
    float off;
};
inline Iq8Conv iq8_conv(int fmt) { return fmt == IQ8_SIGNED ? Iq8Conv{0x8080u, 128.0f} : Iq8Conv{0u, 127.5f}; }

#ifdef __HIPCC__
#define SDRK_CI8_FN __host__ __device__ __forceinline__
#else
#define SDRK_CI8_FN inline
#endif
// one 16-bit word = (I, Q), I in the low byte -> float32 each (the compiler has v_cvt_f32_ubyte0 / 1 for the two bytes)
SDRK_CI8_FN void ci8_unpack(unsigned w, Iq8Conv c, float& re, float& im) {
    const unsigned u = w ^ c.mask;
    re = (float)(u & 0xFFu) - c.off;
    im = (float)((u >> 8) & 0xFFu) - c.off;
}
#undef SDRK_CI8_FN

hipError_t launch_fft4096_ci8(const LaunchArgs& a, int fmt);   // fft4096_ci8.hip: the flagship transform, 2 B in + 4 B out per sample
// fft4096_kgroup_ci8.hip: one row per K frames, 2 + 4/K B per sample; explicitly instantiated for the two formats
template <int FMT>
hipError_t launch_fft4096_kgroup_ci8(const IntegrateArgs& a);
// byte pairs -> complex64 for every other length, with launch_unpack_ci16's interface: n_rows rows of row_len samples, row r
// read at sample r * in_row_stride and written packed (at r * row_len).  Row starts need 2-byte alignment only.
hipError_t launch_unpack_ci8(const void* d_in, int fmt, size_t in_row_stride, void* d_out, size_t n_rows, size_t row_len,
                             int num_cus, hipStream_t stream);

}  // namespace sdrk

// kernels_beam.h — interface between fir_api.hip and the filter-and-sum beamformer kernel (beamsum.hip), and the one place the
// beamformer's own arithmetic is written: the kernel and the host stand-in (tests/fake_beam_kernels.cpp) both call the functions
// below.
//
// The beamformer is the down-converter of kernels_ddc.h with C coherent channels in front of the second transform.  The input
// is a stream of ELEMENTS, one sample of every channel (sample c of element n at (n C + c) sample widths); n_in, the blocks, the
// keeping and the output count are the down-converter's with "sample" read as "element".  Per block of 4096 elements, with
// s = ddc_bin(freq_word), for c = 0 .. C - 1 in this order
//     X_c = DFT_4096(widen(x_c))                                 the plan's forward transform on channel c of the block
//     z_c = ols_filter(X_c[k], H_c[ols_h_index(k, s)])           the product ROUNDED as the single-channel call rounds it
//     u   = beam_sum(u, z_c, c == 0)                             u = z_0, then u + z_c: plain float32 adds per component
// and after the last channel the down-converter's epilogue on u: the transform again, ols_unscale, ddc_mix unless freq_word is 0,
// the keeping (index0 + i) % D == 0.  No multiply-add spans the product and the sum, so C = 1 carries the bits of the
// single-channel call with H_0, and the sum of two channels does not depend on which of them is channel 0.
// Positions at or past n_in are +0.0 + 0.0i in every channel, for every format (kernels_ci8.h: byte 0 of cu8 is -127.5).
#pragma once
#include <stdint.h>

#include "kernels_ci8.h"
#include "kernels_ddc.h"

namespace sdrk {

constexpr int BEAM_MAX_CHANNELS = 8;
// what a launch reads: complex64, int16 pairs or byte pairs of an 8-bit format (>= 0: IQ8_SIGNED / IQ8_UNSIGNED)
constexpr int BEAM_IN_C64 = -2, BEAM_IN_S16 = -1;
inline size_t beam_sample_bytes(int in) { return in == BEAM_IN_C64 ? 8 : in == BEAM_IN_S16 ? 4 : 2; }

// ---- the sum over the channels ----
// `first`: channel 0 starts the sum with its product as it is (-0.0 stays -0.0); every later channel is added to it.  z is
// ols_filter's result, rounded; the adds are separate statements on rounded values, so nothing here contracts into an fma.
__host__ __device__ __forceinline__ OlsC beam_sum(OlsC u, OlsC z, bool first) {
    const float re = u.x + z.x;
    const float im = u.y + z.y;
    return first ? z : OlsC{re, im};
}

// One launch.  d_h: channels x 4096 complex64, channel-major, H_c = DFT_4096(taps of channel c) in natural bin order.
struct BeamArgs {
    const void* d_in = nullptr;          // n_in elements of `channels` samples each
    size_t n_in = 0;                     // elements, >= taps
    int channels = 0;                    // C in 1 .. BEAM_MAX_CHANNELS
    int taps = 0;                        // M
    int decim = 1;                       // D: any integer in 1 .. 256
    uint32_t freq_word = 0;              // 0: no mixer
    uint64_t index0 = 0;                 // stream index of valid-convolution output 0
    const float2* d_h = nullptr;
    const float2* d_twiddle = nullptr;   // W4096^m
    float2* d_out = nullptr;             // beam_launch_outputs() complex64
    size_t max_blocks = 0;               // 0: every block; else only the outputs i < max_blocks L (a chunk of a host call)
    int num_cus = 256;
    hipStream_t stream = nullptr;
};

// in: BEAM_IN_C64, BEAM_IN_S16, IQ8_SIGNED or IQ8_UNSIGNED.  The integer forms return the bits of the complex64 form on the
// widened elements.
hipError_t launch_beamsum(const BeamArgs& a, int in);

// blocks, valid-convolution outputs and kept outputs of a launch: all of them, or what max_blocks leaves (valid arguments only)
inline size_t beam_launch_blocks(const BeamArgs& a) {
    const size_t n = ols_blocks(a.n_in, a.taps);
    return a.max_blocks && a.max_blocks < n ? a.max_blocks : n;
}
inline size_t beam_launch_valid(const BeamArgs& a) {
    const size_t n = a.n_in - (size_t)a.taps + 1, cut = a.max_blocks * (size_t)ols_block_len(a.taps);
    return a.max_blocks && cut < n ? cut : n;
}
inline size_t beam_launch_outputs(const BeamArgs& a) { return ddc_count(beam_launch_valid(a), a.decim, a.index0); }

// What both the kernel's launcher and its stand-in refuse.
inline bool beam_args_ok(const BeamArgs& a, int in) {
    if (in != BEAM_IN_C64 && in != BEAM_IN_S16 && in != IQ8_SIGNED && in != IQ8_UNSIGNED) return false;
    if (a.channels < 1 || a.channels > BEAM_MAX_CHANNELS) return false;
    if (a.taps < 1 || a.taps > OLS_MAX_TAPS || a.n_in < (size_t)a.taps || !a.d_in || !a.d_out || !a.d_h || !a.d_twiddle) return false;
    return a.decim >= 1 && a.decim <= DDC_MAX_DECIM;
}

}  // namespace sdrk

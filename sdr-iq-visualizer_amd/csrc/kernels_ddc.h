// kernels_ddc.h — interface between fir_api.hip and the digital down-converter kernels (ddc4096.hip), and the one place the
// DDC's own arithmetic is written: the kernels and the host stand-in (tests/fake_ddc_kernels.cpp) both call the functions below.
//
// The DDC is the overlap-save call of kernels_ols.h with another epilogue.  Blocks, transforms, ols_filter and ols_unscale are
// kernels_ols.h's, in ols4096_kernel's order; what differs is
//   the mixer     a 32-bit frequency word instead of a bin: the factor of valid-convolution output i is
//                 exp(-2 pi i phase / 2^32), phase = freq_word * (uint32)(index0 + i) (wraps: exact mod 2^32), formed as the
//                 table entry W4096^(phase >> 20) turned by the remaining 20 bits (ddc_factor);
//   the filter    H rotated to the nearest bin, ddc_bin(freq_word);
//   the keeping   output i is kept iff (index0 + i) % D == 0 for ANY D in 1 .. 256 (ddc_div), stored in ascending i.
#pragma once
#include <stdint.h>

#include "kernels_ols_bank.h"

namespace sdrk {

constexpr int DDC_MAX_DECIM = OLS_MAX_DECIM;
constexpr int DDC_MAX_CHAN = OLS_BANK_MAX_CHAN;   // the frequency words travel by value in the kernel's arguments

// the bin of 4096 nearest to the tuned frequency: the filter is centred there, within fs / 8192 of the tuned frequency
__host__ __device__ __forceinline__ unsigned ddc_bin(uint32_t freq_word) { return ((freq_word + 0x80000u) >> 20) & (OLS_N - 1); }

// ---- keeping: n / D for n < 8704 by a multiplication with ceil(2^24 / D), 32-bit operands ----
inline unsigned ddc_recip(unsigned decim) { return ((1u << 24) + decim - 1) / decim; }
__host__ __device__ __forceinline__ unsigned ddc_div(unsigned n, unsigned recip) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n << 8, recip);   // (n recip) >> 24
#else
    return (unsigned)(((unsigned long long)(n << 8) * recip) >> 32);
#endif
}

// kept samples among the valid-convolution outputs i = 0 .. n_valid - 1 of a stream whose output 0 has stream index index0
inline size_t ddc_count(size_t n_valid, int decim, uint64_t index0) {
    const size_t D = (size_t)decim, i_first = (size_t)((D - index0 % D) % D);
    return i_first >= n_valid ? 0 : (n_valid - 1 - i_first) / D + 1;
}
inline size_t ddc_outputs(size_t n_in, int taps, int decim, uint64_t index0) {
    return n_in < (size_t)taps ? 0 : ddc_count(n_in - (size_t)taps + 1, decim, index0);
}

// The keeping of a persistent workgroup, block by block.  With T_b = index0 % D + b L = S D + rem (rem < D), output i = b L + rel
// of block b is kept iff (rem + rel) % D == 0, and is then output sample S + (rem + rel) / D - (index0 % D != 0) of the launch.
// first_block L and grid L stay below 2^32 (a grid has a few hundred workgroups), so nothing here divides 64-bit values.
struct DdcKeep {
    size_t S;
    unsigned rem;
};
__host__ __device__ __forceinline__ DdcKeep ddc_keep_first(unsigned r0, unsigned first_block, unsigned L, unsigned decim) {
    const unsigned t0 = r0 + first_block * L, s = t0 / decim;
    return DdcKeep{s, t0 - s * decim};
}
// to block b + grid: step_q = (grid L) / D, step_r = (grid L) % D
__host__ __device__ __forceinline__ void ddc_keep_next(DdcKeep& k, unsigned step_q, unsigned step_r, unsigned decim) {
    k.S += step_q;
    k.rem += step_r;
    if (k.rem >= decim) {
        k.rem -= decim;
        ++k.S;
    }
}
// the output sample of the block's first kept output = the kept outputs before the block; its (rem + rel) / D is (rem != 0)
__host__ __device__ __forceinline__ size_t ddc_keep_base(const DdcKeep& k, unsigned r0) { return k.S + (k.rem != 0) - (r0 != 0); }

// ---- the mixer ----
__host__ __device__ __forceinline__ uint32_t ddc_phase(uint32_t freq_word, uint32_t index) { return freq_word * index; }
__host__ __device__ __forceinline__ unsigned ddc_table_index(uint32_t phase) { return phase >> 20; }
// W = W4096^(phase >> 20) turned by the low 20 bits r: exp(-i a), a = 2 pi r / 2^32 < 1.54e-3, by its series to a^3 —
// the cosine within 2^-25 and the sine within 1.6e-10 of the exact ones over all r.  r = 0 is W itself.
__host__ __device__ __forceinline__ OlsC ddc_factor(OlsC W, uint32_t phase) {
    const uint32_t r = phase & 0xFFFFFu;
    const float a = (float)r * 0x1.921fb6p-30f;   // 2 pi 2^-32 rounded to float32
    const float c = __builtin_fmaf(-0.5f * a, a, 1.0f);
    const float t = (a * a) * (1.0f / 6.0f);
    const float sn = __builtin_fmaf(-t, a, a);
    const OlsC f = ols_cmul(W, OlsC{c, -sn});
    return r == 0 ? W : f;
}
__host__ __device__ __forceinline__ OlsC ddc_mix(OlsC v, OlsC W, uint32_t phase) { return ols_mix(v, ddc_factor(W, phase)); }

// One launch: a single channel (n_chan = 1, out_stride ignored) or the bank (plane c at d_out + c out_stride).
struct DdcArgs {
    const void* d_in = nullptr;          // complex64, or int16 / 8-bit I,Q pairs
    size_t n_in = 0;                     // samples, >= taps
    int taps = 0;                        // M
    int decim = 1;                       // D: any integer in 1 .. 256
    int n_chan = 1;                      // C in 1 .. DDC_MAX_CHAN
    const uint32_t* freq_word = nullptr;   // host: C words, read before the launcher returns; 0: that channel runs no mixer
    uint64_t index0 = 0;                 // stream index of valid-convolution output 0
    const float2* d_h = nullptr;         // H = DFT_4096(taps), natural bin order
    const float2* d_twiddle = nullptr;   // W4096^m
    float2* d_out = nullptr;             // ddc_launch_outputs() complex64 a plane
    size_t out_stride = 0;               // bank: complex64 between two planes, >= ddc_launch_outputs()
    size_t max_blocks = 0;               // 0: every block; else only the outputs i < max_blocks L (a chunk of a host call)
    int num_cus = 256;
    hipStream_t stream = nullptr;
};

hipError_t launch_ddc(const DdcArgs& a);           // complex64 samples, freq_word[0]
hipError_t launch_ddc_i16(const DdcArgs& a);       // int16 I,Q: the same bits on the widened samples
hipError_t launch_ddcbank(const DdcArgs& a);       // C planes, plane c = launch_ddc with freq_word[c]
hipError_t launch_ddcbank_i16(const DdcArgs& a);
// downconv_iq8.hip: interleaved 8-bit I,Q (2 bytes per sample), fmt = IQ8_SIGNED / IQ8_UNSIGNED of kernels_ci8.h: the bits of
// launch_ddc / launch_ddcbank on the widened samples, the padding past n_in included (+0.0, also for unsigned bytes)
hipError_t launch_downconv_iq8(const DdcArgs& a, int fmt);
hipError_t launch_downconvbank_iq8(const DdcArgs& a, int fmt);

// blocks, valid-convolution outputs and kept outputs of a launch: all of them, or what max_blocks leaves (valid arguments only)
inline size_t ddc_launch_blocks(const DdcArgs& a) {
    const size_t n = ols_blocks(a.n_in, a.taps);
    return a.max_blocks && a.max_blocks < n ? a.max_blocks : n;
}
inline size_t ddc_launch_valid(const DdcArgs& a) {
    const size_t n = a.n_in - (size_t)a.taps + 1, cut = a.max_blocks * (size_t)ols_block_len(a.taps);
    return a.max_blocks && cut < n ? cut : n;
}
inline size_t ddc_launch_outputs(const DdcArgs& a) { return ddc_count(ddc_launch_valid(a), a.decim, a.index0); }

// What both the kernels' launchers and their stand-ins refuse.
inline bool ddc_args_ok(const DdcArgs& a, bool bank) {
    if (a.taps < 1 || a.taps > OLS_MAX_TAPS || a.n_in < (size_t)a.taps || !a.d_in || !a.d_out || !a.d_h || !a.d_twiddle) return false;
    if (a.decim < 1 || a.decim > DDC_MAX_DECIM || !a.freq_word) return false;
    if (!bank) return a.n_chan == 1;
    return a.n_chan >= 1 && a.n_chan <= DDC_MAX_CHAN && a.out_stride >= ddc_launch_outputs(a);
}

}  // namespace sdrk

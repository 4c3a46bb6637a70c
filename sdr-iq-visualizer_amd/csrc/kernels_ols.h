// kernels_ols.h — interface between fir_api.hip and the overlap-save FIR kernel (ols4096.hip), and the one place the arithmetic
// of a block is written: the kernel and the host stand-in (tests/fake_ols_kernels.cpp) both call the functions below.
//
// A block is 4096 consecutive samples.  With M taps, L = ols_block_len(M) outputs come out of each block; block b reads samples
// b L .. b L + 4095 (past the end of the input: zeros), and its block-local positions M - 1 .. M - 2 + L are the valid-convolution
// outputs i = b L .. b L + L - 1.  Per block, with X = DFT_4096(block) from the plan's forward transform (cplx.h's convention):
//     Z'[k] = ols_filter(X[k], H_s[k])      = conj(X[k] H_s[k]),   H_s[k] = H[ols_h_index(k, s)]: H rotated by s bins, exact
//     y'    = DFT_4096(Z')                    the SAME forward transform: the inverse runs by conjugation,
//                                             IDFT(Z) = conj(DFT(conj Z)) / 4096
//     v[i]  = ols_unscale(y'[p])            = conj(y'[p]) 2^-12, exact scaling;  p = i - b L + M - 1
//     out   = ols_mix(v[i], W4096[ols_mix_index(phase0, s, i)])    s != 0 only; W4096^q = exp(-2 pi i q / 4096) from the plan's table
// and output sample m = i / D is stored where D divides i.  L is a multiple of 256 and D divides 256, so whether a block-local
// position is kept, and at which offset, does not depend on the block.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sdrk {

constexpr int OLS_N = 4096;
constexpr int OLS_MAX_TAPS = 2049;
constexpr int OLS_MAX_DECIM = 256;
// How the blocks are dealt to the workgroups of the persistent grid: grid-stride, or contiguous runs (the 4096 - L samples two
// neighbouring blocks share are then re-read by the same workgroup one iteration later).  SDRK_OLS_ASSIGN = 0 / 1 for A/B work;
// grid-stride is the default: runs measured 1.15 x slower at (M, D) = (257, 1) and equal elsewhere (profiles/fir/SUMMARY.md).
enum OlsAssign : int { OLS_ASSIGN_STRIDE = 0, OLS_ASSIGN_RUNS = 1 };

// outputs per block: the largest multiple of 256 with L <= 4097 - M
inline int ols_block_len(int taps) { return ((OLS_N + 1 - taps) / 256) * 256; }
// blocks of a call: every valid output i = 0 .. n_in - M lies in one
inline size_t ols_blocks(size_t n_in, int taps) { return (n_in - (size_t)taps) / (size_t)ols_block_len(taps) + 1; }
inline size_t ols_outputs(size_t n_in, int taps, int decim) { return (n_in - (size_t)taps) / (size_t)decim + 1; }

struct OlsArgs {
    const void* d_in = nullptr;       // complex64, or int16 I,Q pairs
    size_t n_in = 0;                  // samples, >= taps
    int taps = 0;                     // M
    int decim = 1;                    // D: a power of two in 1 .. 256
    int shift_bins = 0;               // s in -2048 .. 2047
    int phase0 = 0;                   // any int; taken mod 4096
    const float2* d_h = nullptr;      // H = DFT_4096(taps), natural bin order
    const float2* d_twiddle = nullptr;   // W4096^m
    float2* d_out = nullptr;          // ols_outputs() complex64
    size_t max_blocks = 0;            // 0: every block; else only the first max_blocks blocks and their outputs (a chunk of a
                                      // host call: its last block's overlap reaches past the blocks it is to compute)
    int num_cus = 256;
    int assign = OLS_ASSIGN_STRIDE;
    hipStream_t stream = nullptr;
};

hipError_t launch_ols4096(const OlsArgs& a);       // complex64 samples
hipError_t launch_ols4096_i16(const OlsArgs& a);   // int16 I,Q: the same bits on the widened samples

// ---- the arithmetic of a block ----
struct OlsC {
    float x, y;
};

// a b = (a.x b.x - [a.y b.y], a.x b.y + [a.y b.x]), the bracketed products rounded first: cplx.h's cmul
__host__ __device__ __forceinline__ OlsC ols_cmul(OlsC a, OlsC b) {
    const float m0 = a.y * b.y;
    const float m1 = a.y * b.x;
    return OlsC{__builtin_fmaf(a.x, b.x, -m0), __builtin_fmaf(a.x, b.y, m1)};
}
__host__ __device__ __forceinline__ int ols_h_index(int k, int shift_bins) { return (k - shift_bins) & (OLS_N - 1); }
__host__ __device__ __forceinline__ OlsC ols_filter(OlsC X, OlsC Hs) {
    const OlsC z = ols_cmul(X, Hs);
    return OlsC{z.x, -z.y};
}
__host__ __device__ __forceinline__ OlsC ols_unscale(OlsC y) {
    const float k = 1.0f / 4096.0f;
    const float re = y.x * k;
    const float im = y.y * k;
    return OlsC{re, -im};
}
// (phase0 + s i) mod 4096 for the valid-convolution index i; 2^32 is a multiple of 4096, so unsigned wrap-around is harmless
__host__ __device__ __forceinline__ unsigned ols_mix_index(unsigned phase0, unsigned shift_bins, unsigned long long i) {
    return (phase0 + shift_bins * (unsigned)(i & (OLS_N - 1))) & (OLS_N - 1);
}
__host__ __device__ __forceinline__ OlsC ols_mix(OlsC v, OlsC w) { return ols_cmul(v, w); }

}  // namespace sdrk

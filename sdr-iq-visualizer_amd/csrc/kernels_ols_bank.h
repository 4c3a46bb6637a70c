// kernels_ols_bank.h — interface between fir_api.hip and the channel-bank kernel (ols_bank.hip): C channels out of one pass over
// the input.  The block geometry and every formula are kernels_ols.h's; channel c of a bank launch carries the bits of
// launch_ols4096 with (shift_bins[c], phase0[c]) on the same input.  tests/fake_bank_kernels.cpp is the host stand-in.
#pragma once
#include "kernels_ols.h"

namespace sdrk {

// per-channel shift and phase travel by value in the kernel's arguments (two arrays of 16-bit values): hence the cap
constexpr int OLS_BANK_MAX_CHAN = 64;

// OlsArgs with per-channel tuning: the scalar shift and phase become host arrays of n_chan values, and channel c's outputs go to
// d_out + c * out_stride.
struct OlsBankArgs {
    const void* d_in = nullptr;       // complex64, or int16 I,Q pairs
    size_t n_in = 0;                  // samples, >= taps
    int taps = 0;                     // M
    int decim = 1;                    // D: a power of two in 1 .. 256
    int n_chan = 0;                   // C in 1 .. OLS_BANK_MAX_CHAN
    const int* shift_bins = nullptr;  // host: C values in -2048 .. 2047, duplicates allowed
    const int* phase0 = nullptr;      // host: C values, any int, taken mod 4096
    const float2* d_h = nullptr;      // H = DFT_4096(taps), natural bin order
    const float2* d_twiddle = nullptr;   // W4096^m
    float2* d_out = nullptr;          // C planes of ols_outputs() complex64, out_stride apart
    size_t out_stride = 0;            // complex64 between two planes, >= ols_outputs()
    size_t max_blocks = 0;            // as in OlsArgs
    int num_cus = 256;
    hipStream_t stream = nullptr;
};

hipError_t launch_chanbank(const OlsBankArgs& a);       // complex64 samples
hipError_t launch_chanbank_i16(const OlsBankArgs& a);   // int16 I,Q: the same bits on the widened samples

// blocks and outputs per channel of a launch: all of them, or what max_blocks leaves (valid arguments only)
inline size_t ols_bank_blocks(const OlsBankArgs& a) {
    const size_t n = ols_blocks(a.n_in, a.taps);
    return a.max_blocks && a.max_blocks < n ? a.max_blocks : n;
}
inline size_t ols_bank_outputs(const OlsBankArgs& a) {
    const size_t n = ols_outputs(a.n_in, a.taps, a.decim), cut = ols_bank_blocks(a) * (size_t)(ols_block_len(a.taps) / a.decim);
    return cut < n ? cut : n;
}

// What both the kernel's launcher and its stand-in refuse.
inline bool ols_bank_args_ok(const OlsBankArgs& a) {
    if (a.taps < 1 || a.taps > OLS_MAX_TAPS || a.n_in < (size_t)a.taps || !a.d_in || !a.d_out || !a.d_h || !a.d_twiddle) return false;
    if (a.decim < 1 || a.decim > OLS_MAX_DECIM || (a.decim & (a.decim - 1))) return false;
    if (a.n_chan < 1 || a.n_chan > OLS_BANK_MAX_CHAN || !a.shift_bins || !a.phase0) return false;
    for (int c = 0; c < a.n_chan; ++c)
        if (a.shift_bins[c] < -OLS_N / 2 || a.shift_bins[c] >= OLS_N / 2) return false;
    return a.out_stride >= ols_bank_outputs(a);
}

}  // namespace sdrk

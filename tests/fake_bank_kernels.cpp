// tests/fake_bank_kernels.cpp — stand-ins for the channel-bank launchers of csrc/kernels_ols_bank.h, for the host-only sanitizer
// build of csrc/fir_api.hip (beside tests/fake_ols_kernels.cpp and the other stand-in kernels).  The real kernel's contract block
// by block: the block geometry of kernels_ols.h, ONE forward transform per block shared by all channels, then per channel the
// shared arithmetic (ols_filter with H rotated by that channel's shift, the transform again, ols_unscale, ols_mix unless the
// shift is 0) and every D-th output stored into the channel's plane, out_stride apart; max_blocks cuts a launch.  The transform
// is the float64 radix-2 FFT of fake_ols_kernels.cpp rounded to float32 at the same places, so plane c equals the stand-in's
// single-channel launch with (shift_bins[c], phase0[c]) element for element — which is what the driver checks.
#include "../sdr-iq-visualizer_amd/csrc/kernels_ols_bank.h"

#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace sdrk {

namespace {

typedef std::complex<double> cd;

// forward DFT in place, exp(-2 pi i n k / N): the one of fake_ols_kernels.cpp
void fft4096(std::vector<cd>& a) {
    const int n = OLS_N;
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * 3.14159265358979323846 / len;
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const cd w(cos(ang * k), sin(ang * k));
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
}

OlsC rounded(cd z) { return OlsC{(float)z.real(), (float)z.imag()}; }

struct Bank {
    OlsBankArgs a;
    std::vector<int> shift, phase;   // copies: the caller's arrays need not outlive the call
};

template <class Sample>
void bank_run(const Bank& k, Sample sample) {
    const OlsBankArgs& a = k.a;
    const size_t L = (size_t)ols_block_len(a.taps), D = (size_t)a.decim, M = (size_t)a.taps;
    const size_t n_blocks = ols_bank_blocks(a), n_out = ols_bank_outputs(a);
    std::vector<cd> X(OLS_N), y(OLS_N);
    for (size_t b = 0; b < n_blocks; ++b) {
        for (size_t p = 0; p < (size_t)OLS_N; ++p) X[p] = b * L + p < a.n_in ? sample(b * L + p) : cd(0.0, 0.0);
        fft4096(X);   // once per block
        for (int c = 0; c < a.n_chan; ++c) {
            const unsigned s = (unsigned)k.shift[c] & (OLS_N - 1), phase0 = (unsigned)k.phase[c] & (OLS_N - 1);
            for (int q = 0; q < OLS_N; ++q) {
                const float2 h = a.d_h[ols_h_index(q, (int)s)];
                const OlsC z = ols_filter(rounded(X[q]), OlsC{h.x, h.y});
                y[q] = cd(z.x, z.y);
            }
            fft4096(y);
            float2* plane = a.d_out + (size_t)c * a.out_stride;
            for (size_t rel = 0; rel < L; ++rel) {
                const size_t i = b * L + rel;
                if (i % D || i / D >= n_out) continue;
                OlsC o = ols_unscale(rounded(y[rel + M - 1]));
                if (s) {
                    const float2 w = a.d_twiddle[ols_mix_index(phase0, s, i)];
                    o = ols_mix(o, OlsC{w.x, w.y});
                }
                plane[i / D] = make_float2(o.x, o.y);
            }
        }
    }
}

template <class Sample>
hipError_t bank_push(const OlsBankArgs& a, Sample (*make)(const void*)) {
    if (!ols_bank_args_ok(a)) return hipErrorInvalidValue;
    Bank k{a, std::vector<int>(a.shift_bins, a.shift_bins + a.n_chan), std::vector<int>(a.phase0, a.phase0 + a.n_chan)};
    fakehip::of(a.stream).push([k, make] { bank_run(k, make(k.a.d_in)); });
    return hipSuccess;
}

struct FromC64 {
    const float* x;
    cd operator()(size_t n) const { return cd(x[2 * n], x[2 * n + 1]); }
};
struct FromI16 {
    const int16_t* x;
    cd operator()(size_t n) const { return cd((double)(float)x[2 * n], (double)(float)x[2 * n + 1]); }
};
FromC64 from_c64(const void* p) { return FromC64{static_cast<const float*>(p)}; }
FromI16 from_i16(const void* p) { return FromI16{static_cast<const int16_t*>(p)}; }

}  // namespace

hipError_t launch_chanbank(const OlsBankArgs& a) { return bank_push(a, from_c64); }
hipError_t launch_chanbank_i16(const OlsBankArgs& a) { return bank_push(a, from_i16); }

}  // namespace sdrk

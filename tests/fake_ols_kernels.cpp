// tests/fake_ols_kernels.cpp — stand-ins for the overlap-save FIR launchers of csrc/kernels_ols.h, for the host-only sanitizer
// build of csrc/fir_api.hip (with the stand-in runtime of tests/fake_hip, beside the other stand-in kernels).  They keep the
// real kernel's contract block by block — ols_block_len / ols_blocks / ols_outputs, block b reads samples b L .. b L + 4095 with
// zeros past n_in, positions M - 1 .. M - 2 + L are outputs b L .. b L + L - 1, every D-th is stored, max_blocks cuts a launch —
// and the arithmetic between the two transforms is kernels_ols.h's own (ols_filter, ols_unscale, ols_mix, the two index
// functions): the expressions the real kernel runs.  The 4096-point forward transform itself is a plain radix-2 FFT in float64
// rounded to float32, so with small integer samples and taps every output is within 1e-3 of the direct convolution, which is
// what the driver checks element by element whatever the chunking was.
#include "../sdr-iq-visualizer_amd/csrc/kernels_ols.h"

#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

namespace sdrk {

namespace {

typedef std::complex<double> cd;

// forward DFT in place, exp(-2 pi i n k / N)
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

template <class Sample>
void ols_run(const OlsArgs& a, Sample sample) {
    const size_t L = (size_t)ols_block_len(a.taps), D = (size_t)a.decim, M = (size_t)a.taps;
    size_t n_blocks = ols_blocks(a.n_in, a.taps), n_out = ols_outputs(a.n_in, a.taps, a.decim);
    if (a.max_blocks && a.max_blocks < n_blocks) {
        n_blocks = a.max_blocks;
        if (n_blocks * (L / D) < n_out) n_out = n_blocks * (L / D);
    }
    const unsigned s = (unsigned)a.shift_bins & (OLS_N - 1), phase0 = (unsigned)a.phase0 & (OLS_N - 1);
    std::vector<cd> x(OLS_N);
    for (size_t b = 0; b < n_blocks; ++b) {
        for (size_t p = 0; p < (size_t)OLS_N; ++p) x[p] = b * L + p < a.n_in ? sample(b * L + p) : cd(0.0, 0.0);
        fft4096(x);
        for (int k = 0; k < OLS_N; ++k) {
            const float2 h = a.d_h[ols_h_index(k, (int)s)];
            const OlsC z = ols_filter(rounded(x[k]), OlsC{h.x, h.y});
            x[k] = cd(z.x, z.y);
        }
        fft4096(x);
        for (size_t rel = 0; rel < L; ++rel) {
            const size_t i = b * L + rel;
            if (i % D || i / D >= n_out) continue;
            OlsC o = ols_unscale(rounded(x[rel + M - 1]));
            if (s) {
                const float2 w = a.d_twiddle[ols_mix_index(phase0, s, i)];
                o = ols_mix(o, OlsC{w.x, w.y});
            }
            a.d_out[i / D] = make_float2(o.x, o.y);
        }
    }
}

bool ols_args_ok(const OlsArgs& a) {
    return a.taps >= 1 && a.taps <= OLS_MAX_TAPS && a.n_in >= (size_t)a.taps && a.d_in && a.d_out && a.d_h && a.d_twiddle &&
           a.decim >= 1 && a.decim <= OLS_MAX_DECIM && !(a.decim & (a.decim - 1)) && a.shift_bins >= -OLS_N / 2 &&
           a.shift_bins < OLS_N / 2;
}

}  // namespace

hipError_t launch_ols4096(const OlsArgs& a) {
    if (!ols_args_ok(a)) return hipErrorInvalidValue;
    const OlsArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float* x = static_cast<const float*>(c.d_in);
        ols_run(c, [x](size_t n) { return cd(x[2 * n], x[2 * n + 1]); });
    });
    return hipSuccess;
}

hipError_t launch_ols4096_i16(const OlsArgs& a) {
    if (!ols_args_ok(a)) return hipErrorInvalidValue;
    const OlsArgs c = a;
    fakehip::of(a.stream).push([c] {
        const int16_t* x = static_cast<const int16_t*>(c.d_in);
        ols_run(c, [x](size_t n) { return cd((double)(float)x[2 * n], (double)(float)x[2 * n + 1]); });
    });
    return hipSuccess;
}

}  // namespace sdrk

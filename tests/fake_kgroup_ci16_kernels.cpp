// tests/fake_kgroup_ci16_kernels.cpp — stand-in for the int16 integrate kernel of csrc/kernels_kgroup_ci16.h, for the host-only
// sanitizer build of csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip, and beside fake_integrate_kernels.cpp
// and fake_ci16_kernels.cpp, which serve the staged lengths of the same calls).  It keeps the real kernel's contract — units
// from integrate_split.h, the frames [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows — on
// fake_integrate_kernels.cpp's checkable "transform" of the widened samples: the spectrum of a frame is (I + 1, Q - 1) at
// position k, its power fmaf(x, x, y*y), the epilogue 3 R + (k & 1023) for the dB form and scale * R for the power form: what
// the staged route delivers through fake_ci16_kernels.cpp's EPI_COMPLEX and fake_integrate_kernels.cpp's row reduction.
#include "../sdr-iq-visualizer_amd/csrc/kernels_kgroup_ci16.h"

#include <cmath>
#include <cstdint>
#include <limits>

namespace sdrk {

namespace {

float fake_epilogue(float r, int out_form, float scale, int k) {
    return out_form == INT_OUT_POWER ? scale * r : 3.0f * r + (float)(k & 1023);
}

// The unit walk of fake_integrate_kernels.cpp (its copy is file-local); power(f - f0, k) is the frame's |X[k]|^2.
template <class Power>
void reduce_units(const IntegrateArgs& a, Power power) {
    const IntSplit sp{a.slices, a.slice_len};
    const size_t u_first = integrate_unit_of(a.f0, a.k, sp), u_last = integrate_unit_of(a.f1 - 1, a.k, sp);
    const float inv_k = 1.0f / (float)a.k;
    for (size_t u = u_first; u <= u_last; ++u) {
        const size_t g = u / a.slices, s = u - g * a.slices;
        const size_t off = s * a.slice_len, rem = a.k - off;
        const size_t ub = g * a.k + off, ue = ub + (rem < a.slice_len ? rem : a.slice_len);
        const size_t fb = ub > a.f0 ? ub : a.f0, fe = ue < a.f1 ? ue : a.f1;
        const bool starts = fb == ub, ends = fe == ue;
        for (int k = 0; k < a.nfft; ++k) {
            float acc = a.detector == INT_DET_MEAN ? 0.0f
                                                   : (a.detector == INT_DET_MAX ? -std::numeric_limits<float>::infinity()
                                                                                : std::numeric_limits<float>::infinity());
            float cmp = 0.0f;
            if (!starts) {
                acc = a.d_carry_in[k].x;
                cmp = a.d_carry_in[k].y;
            }
            for (size_t f = fb; f < fe; ++f) {
                const float p = power(f - a.f0, k);
                if (a.detector == INT_DET_MEAN) {
                    const float y = p - cmp, t = acc + y;
                    cmp = (t - acc) - y;
                    acc = t;
                } else {
                    acc = a.detector == INT_DET_MAX ? std::fmax(acc, p) : std::fmin(acc, p);
                }
            }
            if (ends && a.slices == 1) {
                const float r = a.detector == INT_DET_MEAN ? (acc - cmp) * inv_k : acc;
                a.d_out[(g - a.out_row0) * (size_t)a.nfft + k] = fake_epilogue(r, a.out_form, a.scale, k);
            } else {
                (ends ? a.d_partials + u * (size_t)a.nfft : a.d_carry_out)[k] = make_float2(acc, cmp);
            }
        }
    }
}

}  // namespace

hipError_t launch_fft4096_kgroup_ci16(const IntegrateArgs& a) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const int16_t* x = static_cast<const int16_t*>(c.d_in);
        reduce_units(c, [&](size_t f, int k) {
            const float re = (float)x[2 * (f * c.in_stride + (size_t)k)], im = (float)x[2 * (f * c.in_stride + (size_t)k) + 1];
            return std::fma(re + 1.0f, re + 1.0f, (im - 1.0f) * (im - 1.0f));
        });
    });
    return hipSuccess;
}

}  // namespace sdrk

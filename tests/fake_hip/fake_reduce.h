// tests/fake_hip/fake_reduce.h — what the integrating stand-in kernels (tests/fake_integrate_kernels.cpp,
// fake_kgroup_ci16_kernels.cpp, fake_pfb_groups_kernels.cpp) share: the real kernels' contract — units from integrate_split.h,
// the frames [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows — over a "power" each stand-in
// supplies, and the checkable epilogue: 3 R + (k & 1023) for the dB form, scale * R for the power form.
#pragma once
#include "../../sdr-iq-visualizer_amd/csrc/kernels_integrate.h"

#include <cmath>
#include <limits>

namespace sdrk {

inline float fake_epilogue(float r, int out_form, float scale, int k) {
    return out_form == INT_OUT_POWER ? scale * r : 3.0f * r + (float)(k & 1023);
}

// The unit walk of every integrating stand-in; power(f - f0, k) is the frame's |X[k]|^2.
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

}  // namespace sdrk

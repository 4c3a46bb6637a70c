// tests/fake_sk_kernels.cpp — stand-ins for the spectral-kurtosis kernels of csrc/kernels_sk.h, for the host-only sanitizer
// build of csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip, beside fake_integrate_kernels.cpp and the
// stand-in transforms that serve the staged lengths of the same calls).  They keep the real kernels' contract — units from
// integrate_split.h, the frames [f0, f1) of a launch, {S1, S2} state as plain float32 sums in frame order, carry rows in and
// out, partial rows, finalize in slice order in float64 rounded once, two planes per group at d_out + (g - out_row0) * 2 * nfft
// — on fake_integrate_kernels.cpp's checkable "transform": the spectrum of a frame is (re + 1, im - 1) at position k, its power
// fmaf(x, x, y*y).  Plane 0 is fake_reduce.h's epilogue of S1 / K; plane 1 is kernels_sk.h's own sk_estimate, the expression the
// real kernels share.  With small integer samples every sum is exact, so the driver checks every output element for equality
// whatever the chunking was.
#include "../sdr-iq-visualizer_amd/csrc/kernels_sk.h"

#include "fake_hip/fake_reduce.h"

#include <cstdint>

namespace sdrk {

namespace {

void sk_planes(float* row, int nfft, int k, float s1, float s2, size_t k_frames, int out_form, float scale) {
    row[k] = fake_epilogue(s1 * (1.0f / (float)k_frames), out_form, scale, k);
    row[(size_t)nfft + k] = sk_estimate(s1, s2, (float)k_frames);
}

// The unit walk of fake_reduce.h's reduce_units with the SK state; power(f - f0, k) is the frame's |X[k]|^2.
template <class Power>
void sk_units(const IntegrateArgs& a, Power power) {
    const IntSplit sp{a.slices, a.slice_len};
    const size_t u_first = integrate_unit_of(a.f0, a.k, sp), u_last = integrate_unit_of(a.f1 - 1, a.k, sp);
    for (size_t u = u_first; u <= u_last; ++u) {
        const size_t g = u / a.slices, s = u - g * a.slices;
        const size_t off = s * a.slice_len, rem = a.k - off;
        const size_t ub = g * a.k + off, ue = ub + (rem < a.slice_len ? rem : a.slice_len);
        const size_t fb = ub > a.f0 ? ub : a.f0, fe = ue < a.f1 ? ue : a.f1;
        const bool starts = fb == ub, ends = fe == ue;
        for (int k = 0; k < a.nfft; ++k) {
            float s1 = 0.0f, s2 = 0.0f;
            if (!starts) {
                s1 = a.d_carry_in[k].x;
                s2 = a.d_carry_in[k].y;
            }
            for (size_t f = fb; f < fe; ++f) sk_accumulate(s1, s2, power(f - a.f0, k));
            if (ends && a.slices == 1)
                sk_planes(a.d_out + (g - a.out_row0) * 2 * (size_t)a.nfft, a.nfft, k, s1, s2, a.k, a.out_form, a.scale);
            else
                (ends ? a.d_partials + u * (size_t)a.nfft : a.d_carry_out)[k] = make_float2(s1, s2);
        }
    }
}

}  // namespace

hipError_t launch_sk4096(const IntegrateArgs& a) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* x = static_cast<const float2*>(c.d_in);
        sk_units(c, [&](size_t f, int k) {
            const float2 v = x[f * c.in_stride + (size_t)k];
            return std::fma(v.x + 1.0f, v.x + 1.0f, (v.y - 1.0f) * (v.y - 1.0f));
        });
    });
    return hipSuccess;
}

hipError_t launch_sk4096_i16(const IntegrateArgs& a) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const int16_t* x = static_cast<const int16_t*>(c.d_in);
        sk_units(c, [&](size_t f, int k) {
            const float re = (float)x[2 * (f * c.in_stride + (size_t)k)], im = (float)x[2 * (f * c.in_stride + (size_t)k) + 1];
            return std::fma(re + 1.0f, re + 1.0f, (im - 1.0f) * (im - 1.0f));
        });
    });
    return hipSuccess;
}

hipError_t launch_sk_rows(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* z = static_cast<const float2*>(c.d_in);
        sk_units(c, [&](size_t f, int k) {
            const float2 v = z[f * c.in_stride + (size_t)k];
            return std::fma(v.x, v.x, v.y * v.y);
        });
    });
    return hipSuccess;
}

hipError_t launch_sk_finalize(const float2* d_partials, size_t n_groups, size_t k_frames, size_t slices, int nfft, int,
                              int out_form, float scale, float, float* d_out, int, hipStream_t stream) {
    fakehip::of(stream).push([=] {
        for (size_t g = 0; g < n_groups; ++g)
            for (int k = 0; k < nfft; ++k) {
                const float2* x = d_partials + g * slices * (size_t)nfft + k;
                double t1 = 0.0, t2 = 0.0;
                for (size_t s = 0; s < slices; ++s) {
                    t1 += (double)x[s * (size_t)nfft].x;
                    t2 += (double)x[s * (size_t)nfft].y;
                }
                sk_planes(d_out + g * 2 * (size_t)nfft, nfft, k, (float)t1, (float)t2, k_frames, out_form, scale);
            }
    });
    return hipSuccess;
}

}  // namespace sdrk

// tests/fake_integrate_kernels.cpp — stand-ins for the integrated-spectrum kernels of csrc/kernels_integrate.h, for the host-only
// sanitizer build of csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip).  A "launch" enqueues a host function
// on the stream it was given.  The stand-ins keep the real kernels' contract — units from integrate_split.h, the frames
// [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows, finalize in slice order in float64 — on a
// checkable "transform": the spectrum of a frame is fake_kernels.cpp's EPI_COMPLEX value (re + 1, im - 1) at position k, its
// power fmaf(x, x, y*y), and the epilogue is 3 R + (k & 1023) for the dB form and scale * R for the power form.  With small
// integer samples every sum is exact, so the driver checks every output element for equality whatever the chunking was.
#include "../sdr-iq-visualizer_amd/csrc/kernels_integrate.h"

#include <cmath>
#include <limits>

namespace sdrk {

namespace {

float fake_epilogue(float r, int out_form, float scale, int k) {
    return out_form == INT_OUT_POWER ? scale * r : 3.0f * r + (float)(k & 1023);
}

// The unit walk of both kernels; power(f - f0, k) is the frame's |X[k]|^2.
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

hipError_t launch_fft4096_integrate(const IntegrateArgs& a) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* x = static_cast<const float2*>(c.d_in);
        reduce_units(c, [&](size_t f, int k) {
            const float2 v = x[f * c.in_stride + (size_t)k];
            return std::fma(v.x + 1.0f, v.x + 1.0f, (v.y - 1.0f) * (v.y - 1.0f));
        });
    });
    return hipSuccess;
}

hipError_t launch_integrate_rows(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* z = static_cast<const float2*>(c.d_in);
        reduce_units(c, [&](size_t f, int k) {
            const float2 v = z[f * c.in_stride + (size_t)k];
            return std::fma(v.x, v.x, v.y * v.y);
        });
    });
    return hipSuccess;
}

hipError_t launch_integrate_finalize(const float2* d_partials, size_t n_groups, size_t k_frames, size_t slices, int nfft,
                                     int detector, int out_form, float scale, float, float* d_out, int, hipStream_t stream) {
    fakehip::of(stream).push([=] {
        for (size_t g = 0; g < n_groups; ++g)
            for (int k = 0; k < nfft; ++k) {
                const float2* x = d_partials + g * slices * (size_t)nfft + k;
                float r;
                if (detector == INT_DET_MEAN) {
                    double t = 0.0;
                    for (size_t s = 0; s < slices; ++s) t += (double)x[s * (size_t)nfft].x - (double)x[s * (size_t)nfft].y;
                    r = (float)(t * (1.0 / (double)k_frames));
                } else {
                    r = x[0].x;
                    for (size_t s = 1; s < slices; ++s)
                        r = detector == INT_DET_MAX ? std::fmax(r, x[s * (size_t)nfft].x) : std::fmin(r, x[s * (size_t)nfft].x);
                }
                d_out[g * (size_t)nfft + k] = fake_epilogue(r, out_form, scale, k);
            }
    });
    return hipSuccess;
}

}  // namespace sdrk

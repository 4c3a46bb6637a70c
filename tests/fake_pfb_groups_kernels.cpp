// tests/fake_pfb_groups_kernels.cpp — stand-in for launch_pfb4096_groups (csrc/kernels_pfb.h), for the host-only sanitizer build
// of csrc/integrate_api.hip beside fake_pfb_kernels.cpp and fake_integrate_kernels.cpp (with the stand-in runtime of
// tests/fake_hip).  A "launch" enqueues a host function on the stream it was given.  It keeps the real kernel's contract — units
// from integrate_split.h, the frames [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows — on the
// composition of the other stand-ins: the real float32 fold of fake_pfb_kernels.cpp, fake_kernels.cpp's EPI_COMPLEX "spectrum"
// (re + 1, im - 1) of the folded sample at position k, its power fmaf(x, x, y*y), and fake_integrate_kernels.cpp's epilogue
// 3 R + (k & 1023) (dB form) or scale * R.  So N = 4096 and the lengths that go fold -> transform -> integrate_rows through the
// two stagings must deliver the same values.
#include "../sdr-iq-visualizer_amd/csrc/kernels_integrate.h"
#include "../sdr-iq-visualizer_amd/csrc/kernels_pfb.h"

#include <cmath>
#include <limits>

namespace sdrk {

hipError_t launch_pfb4096_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != 4096 || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* x = static_cast<const float2*>(c.d_in);
        const size_t n = (size_t)c.nfft;
        auto power = [&](size_t f, size_t k) {   // frame f - f0 of this launch
            const float2* s = x + f * c.in_stride + k;
            volatile float re = s[0].x * c.d_pfb_h[k], im = s[0].y * c.d_pfb_h[k];   // (volatile: products and sums rounded one by one)
            for (int t = 1; t < c.pfb_taps; ++t) {
                volatile float pr = s[t * n].x * c.d_pfb_h[t * n + k], pi = s[t * n].y * c.d_pfb_h[t * n + k];
                re = re + pr;
                im = im + pi;
            }
            const float zr = re + 1.0f, zi = im - 1.0f;
            return std::fma(zr, zr, zi * zi);
        };
        const IntSplit sp{c.slices, c.slice_len};
        const size_t u_first = integrate_unit_of(c.f0, c.k, sp), u_last = integrate_unit_of(c.f1 - 1, c.k, sp);
        const float inv_k = 1.0f / (float)c.k, inf = std::numeric_limits<float>::infinity();
        for (size_t u = u_first; u <= u_last; ++u) {
            const size_t g = u / c.slices, s = u - g * c.slices;
            const size_t off = s * c.slice_len, rem = c.k - off;
            const size_t ub = g * c.k + off, ue = ub + (rem < c.slice_len ? rem : c.slice_len);
            const size_t fb = ub > c.f0 ? ub : c.f0, fe = ue < c.f1 ? ue : c.f1;
            const bool starts = fb == ub, ends = fe == ue;
            for (size_t k = 0; k < n; ++k) {
                float acc = c.detector == INT_DET_MEAN ? 0.0f : (c.detector == INT_DET_MAX ? -inf : inf), cmp = 0.0f;
                if (!starts) {
                    acc = c.d_carry_in[k].x;
                    cmp = c.d_carry_in[k].y;
                }
                for (size_t f = fb; f < fe; ++f) {
                    const float p = power(f - c.f0, k);
                    if (c.detector == INT_DET_MEAN) {
                        const float y = p - cmp, t = acc + y;
                        cmp = (t - acc) - y;
                        acc = t;
                    } else {
                        acc = c.detector == INT_DET_MAX ? std::fmax(acc, p) : std::fmin(acc, p);
                    }
                }
                if (ends && c.slices == 1) {
                    const float r = c.detector == INT_DET_MEAN ? (acc - cmp) * inv_k : acc;
                    c.d_out[(g - c.out_row0) * n + k] = c.out_form == INT_OUT_POWER ? c.scale * r : 3.0f * r + (float)(k & 1023);
                } else {
                    (ends ? c.d_partials + u * n : c.d_carry_out)[k] = make_float2(acc, cmp);
                }
            }
        }
    });
    return hipSuccess;
}

}  // namespace sdrk

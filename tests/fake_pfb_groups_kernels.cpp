// tests/fake_pfb_groups_kernels.cpp — stand-in for launch_pfb4096_groups (csrc/kernels_pfb.h), for the host-only sanitizer build
// of csrc/integrate_api.hip beside fake_pfb_kernels.cpp and fake_integrate_kernels.cpp (with the stand-in runtime of
// tests/fake_hip).  A "launch" enqueues a host function on the stream it was given.  It keeps the real kernel's contract — units
// from integrate_split.h, the frames [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows — on the
// composition of the other stand-ins: the real float32 fold of fake_pfb_kernels.cpp, fake_kernels.cpp's EPI_COMPLEX "spectrum"
// (re + 1, im - 1) of the folded sample at position k, its power fmaf(x, x, y*y), and fake_integrate_kernels.cpp's epilogue
// 3 R + (k & 1023) (dB form) or scale * R.  So N = 4096 and the lengths that go fold -> transform -> integrate_rows through the
// two stagings must deliver the same values.
#include "../sdr-iq-visualizer_amd/csrc/kernels_pfb.h"
#include "fake_hip/fake_reduce.h"

namespace sdrk {

hipError_t launch_pfb4096_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != 4096 || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const float2* x = static_cast<const float2*>(c.d_in);
        const size_t n = (size_t)c.nfft;
        auto power = [&](size_t f, int k) {   // frame f - f0 of this launch
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
        reduce_units(c, power);
    });
    return hipSuccess;
}

}  // namespace sdrk

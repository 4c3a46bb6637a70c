// tests/fake_kgroup_ci16_kernels.cpp — stand-in for the int16 integrate kernel of csrc/kernels_kgroup_ci16.h, for the host-only
// sanitizer build of csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip, and beside fake_integrate_kernels.cpp
// and fake_ci16_kernels.cpp, which serve the staged lengths of the same calls).  It keeps the real kernel's contract — units
// from integrate_split.h, the frames [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows — on
// fake_integrate_kernels.cpp's checkable "transform" of the widened samples: the spectrum of a frame is (I + 1, Q - 1) at
// position k, its power fmaf(x, x, y*y), the epilogue 3 R + (k & 1023) for the dB form and scale * R for the power form: what
// the staged route delivers through fake_ci16_kernels.cpp's EPI_COMPLEX and fake_integrate_kernels.cpp's row reduction.
#include "../sdr-iq-visualizer_amd/csrc/kernels_kgroup_ci16.h"

#include "fake_hip/fake_reduce.h"

#include <cstdint>

namespace sdrk {

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

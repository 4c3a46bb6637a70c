// tests/fake_integrate_kernels.cpp — stand-ins for the integrated-spectrum kernels of csrc/kernels_integrate.h, for the host-only
// sanitizer build of csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip).  A "launch" enqueues a host function
// on the stream it was given.  The stand-ins keep the real kernels' contract — units from integrate_split.h, the frames
// [f0, f1) of a launch, Kahan / max / min state, carry rows in and out, partial rows, finalize in slice order in float64 — on a
// checkable "transform": the spectrum of a frame is fake_kernels.cpp's EPI_COMPLEX value (re + 1, im - 1) at position k, its
// power fmaf(x, x, y*y), and the epilogue is 3 R + (k & 1023) for the dB form and scale * R for the power form.  With small
// integer samples every sum is exact, so the driver checks every output element for equality whatever the chunking was.
#include "fake_hip/fake_reduce.h"

namespace sdrk {

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

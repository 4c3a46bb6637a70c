// tests/fake_pfb_kernels.cpp — stand-ins for the two polyphase-filter-bank kernels of csrc/kernels_pfb.h, for the host-only
// sanitizer build of csrc/pfb_api.hip (with the stand-in runtime of tests/fake_hip).  Like fake_kernels.cpp, a "launch"
// enqueues a host function on the stream it was given.  The fold is the real one (float32, products and sums rounded one by
// one); the "transform" behind it is fake_kernels.cpp's checkable function of the folded sample: row[f][k] = 3 re - im +
// (k & 1023) (dB epilogue) or (re + 1, im - 1) (complex) — so N = 4096 and the lengths folded into the plan's staging first
// must deliver the same values.
#include "../sdr-iq-visualizer_amd/csrc/kernels_pfb.h"

namespace sdrk {

static float2 fake_fold(const float2* x, const float* h, size_t nfft, int taps) {
    volatile float re = x[0].x * h[0], im = x[0].y * h[0];      // (volatile: no contraction of the products into the sums)
    for (int t = 1; t < taps; ++t) {
        volatile float pr = x[t * nfft].x * h[t * nfft], pi = x[t * nfft].y * h[t * nfft];
        re = re + pr;
        im = im + pi;
    }
    return make_float2(re, im);
}

hipError_t launch_pfb4096(const LaunchArgs& a, const float* d_h, int taps, int) {
    if (a.nfft != 4096 || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    LaunchArgs c = a;
    fakehip::of(a.stream).push([c, d_h, taps] {
        const float2* x = static_cast<const float2*>(c.d_iq);
        for (size_t f = 0; f < c.n_frames; ++f)
            for (int k = 0; k < c.nfft; ++k) {
                const float2 v = fake_fold(x + f * c.frame_stride + (size_t)k, d_h + k, (size_t)c.nfft, taps);
                if (c.epilogue == EPI_LOGPSD) static_cast<float*>(c.d_out)[f * (size_t)c.nfft + k] = 3.0f * v.x - v.y + (float)(k & 1023);
                else static_cast<float2*>(c.d_out)[f * (size_t)c.nfft + k] = make_float2(v.x + 1.0f, v.y - 1.0f);
            }
    });
    return hipSuccess;
}

hipError_t launch_pfb_fold(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps, void* d_out,
                           int, hipStream_t s) {
    if (!d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    fakehip::of(s).push([=] {
        const float2* x = static_cast<const float2*>(d_iq);
        for (size_t f = 0; f < n_frames; ++f)
            for (size_t k = 0; k < (size_t)nfft; ++k)
                static_cast<float2*>(d_out)[f * (size_t)nfft + k] = fake_fold(x + f * frame_stride + k, d_h + k, (size_t)nfft, taps);
    });
    return hipSuccess;
}

}  // namespace sdrk

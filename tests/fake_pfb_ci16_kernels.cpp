// tests/fake_pfb_ci16_kernels.cpp — stand-ins for the three int16 polyphase-filter-bank launchers of csrc/kernels_pfb.h
// (launch_pfb4096_i16, launch_pfb_fold_i16, launch_pfb4096_i16_groups), for the host-only sanitizer build of
// csrc/pfb_api.hip and csrc/integrate_api.hip beside fake_pfb_kernels.cpp, fake_pfb_groups_kernels.cpp and fake_integrate_kernels.cpp (with the
// stand-in runtime of tests/fake_hip).  Each widens the int16 pairs of the launch into complex64 on the host and hands them to
// the complex64 stand-in, whose values the drivers know — so the byte offsets the host code computes for 4-byte samples
// (chunks, overlap, strides) are what is under test.  The widened copy lives until the enqueued work has run.
#include "../sdr-iq-visualizer_amd/csrc/kernels_integrate.h"
#include "../sdr-iq-visualizer_amd/csrc/kernels_pfb.h"

#include <cstdint>
#include <memory>
#include <vector>

namespace sdrk {

static std::shared_ptr<std::vector<float2>> widened(const void* d_iq, size_t n_samples, hipStream_t s) {
    auto w = std::make_shared<std::vector<float2>>(n_samples);
    fakehip::of(s).push([w, d_iq, n_samples] {   // (on the stream: the samples arrive by an earlier copy on it)
        const int16_t* x = static_cast<const int16_t*>(d_iq);
        for (size_t i = 0; i < n_samples; ++i) (*w)[i] = make_float2((float)x[2 * i], (float)x[2 * i + 1]);
    });
    return w;
}

static void release(std::shared_ptr<std::vector<float2>> w, hipStream_t s) {
    fakehip::of(s).push([w] {});   // keeps the copy alive until the work in front of it has run
}

hipError_t launch_pfb4096_i16(const LaunchArgs& a, const float* d_h, int taps, int assign) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.nfft != 4096 || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    auto w = widened(a.d_iq, (a.n_frames - 1) * a.frame_stride + (size_t)taps * a.nfft, a.stream);
    LaunchArgs c = a;
    c.d_iq = w->data();
    const hipError_t e = launch_pfb4096(c, d_h, taps, assign);
    release(w, a.stream);
    return e;
}

hipError_t launch_pfb_fold_i16(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                               void* d_out, int num_cus, hipStream_t s) {
    if (n_frames == 0) return hipSuccess;
    if (!d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    auto w = widened(d_iq, (n_frames - 1) * frame_stride + (size_t)taps * nfft, s);
    const hipError_t e = launch_pfb_fold(w->data(), frame_stride, n_frames, nfft, d_h, taps, d_out, num_cus, s);
    release(w, s);
    return e;
}

hipError_t launch_pfb4096_i16_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != 4096 || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    auto w = widened(a.d_in, (a.f1 - a.f0 - 1) * a.in_stride + (size_t)a.pfb_taps * a.nfft, a.stream);
    IntegrateArgs c = a;
    c.d_in = w->data();
    const hipError_t e = launch_pfb4096_groups(c);
    release(w, a.stream);
    return e;
}

}  // namespace sdrk

// tests/fake_ci8_kernels.cpp — stand-ins for the 8-bit-input kernels of csrc/kernels_ci8.h, for the host-only sanitizer build of
// csrc/ci16_api.hip and csrc/integrate_api.hip (with the stand-in runtime of tests/fake_hip).  Like fake_ci16_kernels.cpp and
// fake_kgroup_ci16_kernels.cpp, a "launch" enqueues a host function on the stream it was given and the "transform" is the same
// checkable function of the widened samples — row[f][k] = 3 I - Q + (k & 1023) (dB epilogue) or (I + 1, Q - 1) (complex), its
// power fmaf(x, x, y*y) — so the N = 4096 stand-ins, which read the bytes themselves, and the unpack route, which widens them
// into the plan's staging first, must deliver the same values.  The widening is kernels_ci8.h's own ci8_unpack.
#include "../sdr-iq-visualizer_amd/csrc/kernels_ci8.h"

#include "fake_hip/fake_reduce.h"

#include <cstdint>
#include <cstring>

namespace sdrk {

namespace {

// sample n of a byte-pair stream (2-byte aligned at most: read through memcpy)
inline void sample_at(const void* base, size_t n, Iq8Conv conv, float& re, float& im) {
    uint16_t w;
    std::memcpy(&w, static_cast<const unsigned char*>(base) + 2 * n, 2);
    ci8_unpack(w, conv, re, im);
}

}  // namespace

hipError_t launch_fft4096_ci8(const LaunchArgs& a, int fmt) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    const LaunchArgs c = a;
    const Iq8Conv conv = iq8_conv(fmt);
    fakehip::of(a.stream).push([c, conv] {
        for (size_t f = 0; f < c.n_frames; ++f)
            for (int k = 0; k < c.nfft; ++k) {
                float re, im;
                sample_at(c.d_iq, f * c.frame_stride + (size_t)k, conv, re, im);
                if (c.epilogue == EPI_LOGPSD) static_cast<float*>(c.d_out)[f * (size_t)c.nfft + k] = 3.0f * re - im + (float)(k & 1023);
                else static_cast<float2*>(c.d_out)[f * (size_t)c.nfft + k] = make_float2(re + 1.0f, im - 1.0f);
            }
    });
    return hipSuccess;
}

template <int FMT>
hipError_t launch_fft4096_kgroup_ci8(const IntegrateArgs& a) {
    if (a.nfft != 4096) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    const Iq8Conv conv = iq8_conv(FMT);
    fakehip::of(a.stream).push([c, conv] {
        reduce_units(c, [&](size_t f, int k) {
            float re, im;
            sample_at(c.d_in, f * c.in_stride + (size_t)k, conv, re, im);
            return std::fma(re + 1.0f, re + 1.0f, (im - 1.0f) * (im - 1.0f));
        });
    });
    return hipSuccess;
}

template hipError_t launch_fft4096_kgroup_ci8<IQ8_SIGNED>(const IntegrateArgs&);
template hipError_t launch_fft4096_kgroup_ci8<IQ8_UNSIGNED>(const IntegrateArgs&);

hipError_t launch_unpack_ci8(const void* d_in, int fmt, size_t in_row_stride, void* d_out, size_t n_rows, size_t row_len, int,
                             hipStream_t s) {
    const Iq8Conv conv = iq8_conv(fmt);
    fakehip::of(s).push([=] {
        float2* o = static_cast<float2*>(d_out);
        for (size_t r = 0; r < n_rows; ++r)
            for (size_t n = 0; n < row_len; ++n) {
                float re, im;
                sample_at(d_in, r * in_row_stride + n, conv, re, im);
                o[r * row_len + n] = make_float2(re, im);
            }
    });
    return hipSuccess;
}

}  // namespace sdrk

// tests/fake_real_groups_kernels.cpp — stand-in for the integrated real-input kernel of csrc/rspec4096_groups.hip
// (launch_rspec4096_groups, kernels_real.h), for the host-only sanitizer build of csrc/ci16_api.hip (with the stand-in runtime of
// tests/fake_hip).  A "launch" enqueues a host function on the stream it was given.  The frame's "spectrum" is the per-frame
// stand-in's complex row (fake_real_kernels.cpp): with Z[k] = (w[2k] x[2k] + 1, w[2k+1] x[2k+1] - 1), zk = Z[k mod N] and
// zm = Z[(N - k) mod N],  X[k] = (zk.x + zm.y, zk.y - zm.x)  for k = 0 ... N; its power fmaf(re, re, im*im) goes through the unit
// walk of fake_hip/fake_reduce.h (units, carry rows, partial rows of N + 1 elements) and the checkable epilogue there.  So the
// N = 4096 stand-in, which reads the samples itself, and the staged route (launch_real's stand-ins into staging, then
// launch_integrate_rows with rows of N + 1) deliver the same values, bin N included.
#include "../sdr-iq-visualizer_amd/csrc/kernels_ci8.h"
#include "../sdr-iq-visualizer_amd/csrc/kernels_real.h"
#include "fake_hip/fake_reduce.h"

#include <cstdint>
#include <cstring>

namespace sdrk {

namespace {

// pair m of a real-sampled stream in format fmt (aligned to a pair at most: read through memcpy), widened and windowed
inline float2 groups_pair_at(const IntegrateArgs& c, size_t m_stream, size_t m) {
    const unsigned char* p = static_cast<const unsigned char*>(c.d_in) + m_stream * real_pair_bytes(c.real_fmt);
    float2 v;
    if (c.real_fmt == REAL_F32) {
        float t[2];
        std::memcpy(t, p, 8);
        v = make_float2(t[0], t[1]);
    } else if (c.real_fmt == REAL_S16) {
        int16_t t[2];
        std::memcpy(t, p, 4);
        v = make_float2((float)t[0], (float)t[1]);
    } else {
        uint16_t w;
        std::memcpy(&w, p, 2);
        ci8_unpack(w, iq8_conv(c.real_fmt == REAL_U8 ? IQ8_UNSIGNED : IQ8_SIGNED), v.x, v.y);
    }
    if (c.d_real_window) v.x *= c.d_real_window[2 * m], v.y *= c.d_real_window[2 * m + 1];
    return v;
}

}  // namespace

hipError_t launch_rspec4096_groups(const IntegrateArgs& a) {
    if (a.nfft != 4097 || !a.d_real_tab) return hipErrorInvalidValue;
    if (a.f1 <= a.f0) return hipSuccess;
    const IntegrateArgs c = a;
    fakehip::of(a.stream).push([c] {
        const size_t n = 4096;
        reduce_units(c, [&](size_t f, int k) {   // f counts from the launch's first frame, as d_in does
            const size_t mk = (size_t)k % n, mm = (n - (size_t)k) % n;
            float2 zk = groups_pair_at(c, f * c.in_stride + mk, mk), zm = groups_pair_at(c, f * c.in_stride + mm, mm);
            zk.x += 1.0f, zk.y -= 1.0f, zm.x += 1.0f, zm.y -= 1.0f;
            const float re = zk.x + zm.y, im = zk.y - zm.x;
            return std::fma(re, re, im * im);
        });
    });
    return hipSuccess;
}

}  // namespace sdrk

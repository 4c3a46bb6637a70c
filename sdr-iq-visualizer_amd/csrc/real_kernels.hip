// real_kernels.hip — the staged route of the real-input spectra (kernels_real.h) at every plan length but 4096: a pre-pass that
// widens and windows real samples into the complex64 pairs the plan's own transform reads, and the split that forms the N + 1
// bins X[k] from that transform's natural-order output and applies the epilogue into the caller's rows.  rspec4096.hip does
// all of it in one kernel at N = 4096.
#include "cplx.h"
#include "kernels_ci16.h"
#include "kernels_ci8.h"
#include "kernels_real.h"

namespace sdrk {

// z[f][m] = (w[2m] x[2m], w[2m+1] x[2m+1]) of frame f, packed.  RFMT: 0 float32 pairs, 1 int16 pairs, 2 byte pairs (the
// conversion's arguments at run time, as everywhere).  One float32 product per sample; no window: no product.
template <int RFMT>
__global__ __launch_bounds__(256) void real_pairs_kernel(const void* __restrict__ x_raw, unsigned conv_mask, float conv_off,
                                                         size_t frame_stride, size_t n_frames, int log2n,
                                                         const float2* __restrict__ window, float2* __restrict__ out) {
    const size_t total = n_frames << log2n;
    const size_t mask = ((size_t)1 << log2n) - 1;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i >> log2n, m = i & mask;
        const size_t at = f * frame_stride + m;
        float re, im;
        if (RFMT == 0) {
            const float2 p = static_cast<const float2*>(x_raw)[at];
            re = p.x, im = p.y;
        } else if (RFMT == 1) {
            ci16_unpack(static_cast<const unsigned*>(x_raw)[at], re, im);
        } else {
            ci8_unpack(static_cast<const unsigned short*>(x_raw)[at], Iq8Conv{conv_mask, conv_off}, re, im);
        }
        if (window) {
            const float2 w = window[m];
            re *= w.x, im *= w.y;
        }
        out[i] = make_float2(re, im);
    }
}

// X[f][k], k = 0 ... N, from Z[f][0 ... N-1] (packed, natural order) and tab[k] = exp(-i pi k / N); row f at element
// f * out_stride.
template <int EPILOGUE>
__global__ __launch_bounds__(256) void real_split_kernel(const float2* __restrict__ z_all, size_t n_frames, int log2n,
                                                         const float2* __restrict__ tab, float eps, void* __restrict__ out_raw,
                                                         size_t out_stride) {
    const size_t n = (size_t)1 << log2n, bins = n + 1;
    const size_t total = n_frames * bins;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / bins, k = i - f * bins;
        const float2* __restrict__ zf = z_all + (f << log2n);
        float re, im;
        if (k == 0 || k == n) {
            const float2 z = zf[0];
            re = k == 0 ? z.x + z.y : z.x - z.y;
            im = 0.0f;
        } else {
            const float2 z = zf[k], m = zf[n - k], t = tab[k];
            const float ex = 0.5f * (z.x + m.x), ey = 0.5f * (z.y - m.y);   // E = (Z + conj M) / 2
            const float ox = 0.5f * (z.y + m.y), oy = 0.5f * (m.x - z.x);   // O = -(i/2) (Z - conj M)
            const cf to = cmul(cf{t.x, t.y}, cf{ox, oy});
            re = ex + to.x, im = ey + to.y;
        }
        if (EPILOGUE == EPI_LOGPSD)
            static_cast<float*>(out_raw)[f * out_stride + k] = logpsd_db(re, im, eps);
        else
            static_cast<float2*>(out_raw)[f * out_stride + k] = make_float2(re, im);
    }
}

namespace {

int real_log2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

unsigned real_grid(size_t total, int num_cus) {
    const size_t want = (total + 255) / 256, cap = (size_t)num_cus * 16;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

}  // namespace

hipError_t launch_real_pairs(const RealArgs& a, void* d_pairs) {
    if (a.n_frames == 0) return hipSuccess;
    const int l2 = real_log2(a.nfft);
    dim3 g(real_grid(a.n_frames << l2, a.num_cus)), b(256);
    const Iq8Conv conv = iq8_conv(a.fmt == REAL_U8 ? IQ8_UNSIGNED : IQ8_SIGNED);
    const float2* win = reinterpret_cast<const float2*>(a.d_window);
    float2* out = static_cast<float2*>(d_pairs);
#define SDRK_LAUNCH(R) \
    hipLaunchKernelGGL((real_pairs_kernel<R>), g, b, 0, a.stream, a.d_x, conv.mask, conv.off, a.frame_stride, a.n_frames, l2, win, out)
    if (a.fmt == REAL_F32) SDRK_LAUNCH(0);
    else if (a.fmt == REAL_S16) SDRK_LAUNCH(1);
    else SDRK_LAUNCH(2);
#undef SDRK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_real_split(const RealArgs& a, const void* d_z) {
    if (a.n_frames == 0) return hipSuccess;
    const int l2 = real_log2(a.nfft);
    dim3 g(real_grid(a.n_frames * ((size_t)a.nfft + 1), a.num_cus)), b(256);
    const float2* z = static_cast<const float2*>(d_z);
    if (a.epilogue == EPI_LOGPSD)
        hipLaunchKernelGGL((real_split_kernel<EPI_LOGPSD>), g, b, 0, a.stream, z, a.n_frames, l2, a.d_tab, a.eps, a.d_out, a.out_stride);
    else
        hipLaunchKernelGGL((real_split_kernel<EPI_COMPLEX>), g, b, 0, a.stream, z, a.n_frames, l2, a.d_tab, a.eps, a.d_out, a.out_stride);
    return hipGetLastError();
}

}  // namespace sdrk

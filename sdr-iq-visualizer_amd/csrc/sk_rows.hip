// sk_rows.hip — the spectral-kurtosis route of every frame length without a fused kernel (and of both polyphase-filter-bank
// modes at every length, N = 4096 included), and the finalize of split groups for both routes.
//
// sk_rows_kernel: the mode's own transform has left complex64 spectra (EPI_COMPLEX, already in the plan's shift order) in
// staging; one thread per bin walks the frames of a unit (integrate_split.h) down its column — every wave reads 64 consecutive
// complex64 per frame — and keeps the state the fused N = 4096 kernel keeps: S1 += p, S2 = fmaf(p, p, S2) of
// p = fmaf(re, re, im*im), in frame order.  End of unit as there: the group's two rows, a partial row or the carry row.
//
// sk_finalize_kernel: a group cut into S slices -> its two rows.  The S partial sums are added in slice order in float64 (S is
// at most a few hundred; the order and therefore the bits are fixed), rounded to float32 once, and go through the same
// expressions as an unsplit group's.
#include "kernels_sk.h"

namespace sdrk {

// plane 0: the mean power through the integrating epilogue; plane 1: the estimator
__device__ __forceinline__ void sk_store_planes(float* __restrict__ row, int nfft, int col, float s1, float s2, const IntUnits& c,
                                                float kf) {
    row[col] = int_epilogue(s1 * c.inv_k, c.out_form, c.scale, c.eps);
    row[(size_t)nfft + col] = sk_estimate(s1, s2, kf);
}

__global__ __launch_bounds__(256) void sk_rows_kernel(const float2* __restrict__ spec, size_t in_stride, IntUnits c, float kf,
                                                      int nfft, unsigned col_blocks, size_t n_items, float* __restrict__ out,
                                                      float2* __restrict__ partials, const float2* __restrict__ carry_in,
                                                      float2* __restrict__ carry_out) {
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t u = c.u_first + item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const IntUnit cur = int_unit(c, u);
        float s1 = 0.0f, s2 = 0.0f;
        if (!cur.starts) {
            const float2 s = carry_in[col];
            s1 = s.x;
            s2 = s.y;
        }
        const float2* __restrict__ x = spec + (cur.fb - c.f0) * in_stride + col;
        for (size_t f = cur.fb; f < cur.fe; ++f, x += in_stride) {
            const float2 z = *x;
            sk_accumulate(s1, s2, fmaf(z.x, z.x, z.y * z.y));
        }
        if (cur.ends && c.slices == 1)
            sk_store_planes(out + (cur.g - c.out_row0) * 2 * (size_t)nfft, nfft, col, s1, s2, c, kf);
        else
            (cur.ends ? partials + u * (size_t)nfft : carry_out)[col] = make_float2(s1, s2);
    }
}

hipError_t launch_sk_rows(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntUnits c = int_units(a);
    const unsigned col_blocks = (unsigned)((a.nfft + 255) / 256);
    const size_t n_items = (c.u_last - c.u_first + 1) * col_blocks;
    const size_t cap = (size_t)a.num_cus * 32;
    hipLaunchKernelGGL(sk_rows_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, a.stream,
                       static_cast<const float2*>(a.d_in), a.in_stride, c, (float)a.k, a.nfft, col_blocks, n_items, a.d_out,
                       a.d_partials, a.d_carry_in, a.d_carry_out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void sk_finalize_kernel(const float2* __restrict__ partials, size_t n_groups, IntUnits c,
                                                          float kf, int nfft, float* __restrict__ out) {
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_groups * col_blocks;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t g = item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const float2* __restrict__ x = partials + g * c.slices * (size_t)nfft + col;
        double t1 = 0.0, t2 = 0.0;
        for (unsigned s = 0; s < c.slices; ++s) {
            const float2 p = x[(size_t)s * nfft];
            t1 += (double)p.x;
            t2 += (double)p.y;
        }
        sk_store_planes(out + g * 2 * (size_t)nfft, nfft, col, (float)t1, (float)t2, c, kf);
    }
}

hipError_t launch_sk_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int, int out_form,
                              float scale, float eps, float* d_out, int num_cus, hipStream_t stream) {
    if (n_groups == 0) return hipSuccess;
    IntUnits c{};   // (the finalize reads the slice count and what the epilogue takes)
    c.k = k;
    c.slices = (unsigned)slices;
    c.out_form = out_form;
    c.scale = scale;
    c.eps = eps;
    c.inv_k = 1.0f / (float)k;
    const size_t n_items = n_groups * (size_t)((nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    hipLaunchKernelGGL(sk_finalize_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, stream, d_partials,
                       n_groups, c, (float)k, nfft, d_out);
    return hipGetLastError();
}

}  // namespace sdrk

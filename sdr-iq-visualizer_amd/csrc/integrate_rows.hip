// integrate_rows.hip — the integrated-spectrum route of every frame length without a fused kernel, and the finalize of split
// groups for both routes.
//
// integrate_rows_kernel: the plan's own transform has left complex64 spectra (EPI_COMPLEX, already in the plan's shift order)
// in staging; one thread per bin walks the frames of a unit (integrate_split.h) down its column — every wave reads 64
// consecutive complex64 per frame — and keeps the same state the fused N = 4096 kernel keeps: Kahan sum and compensation, or
// the running maximum / minimum of fmaf(re, re, im*im).  End of unit as there: final row, partial row or carry row.
//
// integrate_finalize_kernel: a group cut into S slices -> its row.  The S partial states are combined in slice order, sums in
// float64 (S is at most a few hundred; the order and therefore the bits are fixed), then the epilogue.
#include "kernels_integrate.h"

namespace sdrk {

template <int DET>
__global__ __launch_bounds__(256) void integrate_rows_kernel(const float2* __restrict__ spec, size_t in_stride, IntUnits c,
                                                             int nfft, unsigned col_blocks, size_t n_items,
                                                             float* __restrict__ out, float2* __restrict__ partials,
                                                             const float2* __restrict__ carry_in,
                                                             float2* __restrict__ carry_out) {
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t u = c.u_first + item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const IntUnit cur = int_unit(c, u);
        float acc, cmp;
        if (cur.starts) {
            int_init<DET>(acc, cmp);
        } else {
            const float2 s = carry_in[col];
            acc = s.x;
            cmp = s.y;
        }
        const float2* __restrict__ x = spec + (cur.fb - c.f0) * in_stride + col;
        for (size_t f = cur.fb; f < cur.fe; ++f, x += in_stride) {
            const float2 z = *x;
            int_accumulate<DET>(acc, cmp, fmaf(z.x, z.x, z.y * z.y));
        }
        if (cur.ends && c.slices == 1)
            out[(cur.g - c.out_row0) * (size_t)nfft + col] =
                int_epilogue(int_reduced<DET>(acc, cmp, c.inv_k), c.out_form, c.scale, c.eps);
        else
            (cur.ends ? partials + u * (size_t)nfft : carry_out)[col] = make_float2(acc, cmp);
    }
}

hipError_t launch_integrate_rows(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntUnits c = int_units(a);
    const unsigned col_blocks = (unsigned)((a.nfft + 255) / 256);
    const size_t n_items = (c.u_last - c.u_first + 1) * col_blocks;
    const size_t cap = (size_t)a.num_cus * 32;
    dim3 g((unsigned)(n_items < cap ? n_items : cap)), b(256);
    const float2* spec = static_cast<const float2*>(a.d_in);
#define SDRK_LAUNCH(D)                                                                                                  \
    hipLaunchKernelGGL((integrate_rows_kernel<D>), g, b, 0, a.stream, spec, a.in_stride, c, a.nfft, col_blocks, n_items,  \
                       a.d_out, a.d_partials, a.d_carry_in, a.d_carry_out)
    if (a.detector == INT_DET_MEAN) SDRK_LAUNCH(INT_DET_MEAN);
    else if (a.detector == INT_DET_MAX) SDRK_LAUNCH(INT_DET_MAX);
    else SDRK_LAUNCH(INT_DET_MIN);
#undef SDRK_LAUNCH
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void integrate_finalize_kernel(const float2* __restrict__ partials, size_t n_groups,
                                                                 double inv_k, unsigned slices, int nfft, int detector,
                                                                 int out_form, float scale, float eps,
                                                                 float* __restrict__ out) {
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_groups * col_blocks;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t g = item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const float2* __restrict__ x = partials + g * slices * (size_t)nfft + col;
        float r;
        if (detector == INT_DET_MEAN) {
            double t = 0.0;
            for (unsigned s = 0; s < slices; ++s) {
                const float2 p = x[(size_t)s * nfft];
                t += (double)p.x - (double)p.y;
            }
            r = (float)(t * inv_k);
        } else {
            r = x[0].x;
            for (unsigned s = 1; s < slices; ++s) {
                const float v = x[(size_t)s * nfft].x;
                r = detector == INT_DET_MAX ? fmaxf(r, v) : fminf(r, v);
            }
        }
        out[g * (size_t)nfft + col] = int_epilogue(r, out_form, scale, eps);
    }
}

hipError_t launch_integrate_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int detector,
                                     int out_form, float scale, float eps, float* d_out, int num_cus, hipStream_t stream) {
    if (n_groups == 0) return hipSuccess;
    const size_t n_items = n_groups * (size_t)((nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    hipLaunchKernelGGL(integrate_finalize_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, stream,
                       d_partials, n_groups, 1.0 / (double)k, (unsigned)slices, nfft, detector, out_form, scale, eps, d_out);
    return hipGetLastError();
}

}  // namespace sdrk

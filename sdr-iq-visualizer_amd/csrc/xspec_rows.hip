// xspec_rows.hip — the two-channel cross-spectrum route of every frame length without a fused kernel, and the finalize of split
// groups for both routes.
//
// xspec_split_kernel: the frames of a chunk, cut from the element stream (I0 Q0 I1 Q1 per element, complex64 or int16), ->
// two packed complex64 frame arrays, one per channel, which the plan's own transform then takes like any caller's frames.
// int16 is widened here, x = float32(I) + i float32(Q) exactly, so both formats meet in the same complex64 values.
//
// xspec_rows_kernel: the plan's transform has left both channels' complex64 spectra (EPI_COMPLEX, already in the plan's shift
// order) in staging; one thread per bin walks the frames of a unit (integrate_split.h) down its column in both and keeps the
// state the fused N = 4096 kernel keeps (xs_accumulate, kernels_xspec.h), in frame order.  End of unit as there: the group's
// four rows, a partial row or the carry row.
//
// xspec_finalize_kernel: a group cut into S slices -> its four rows.  The S partial sums are added in slice order in float64
// (the order and therefore the bits are fixed), rounded to float32 once, and go through the same expression as an unsplit
// group's.
#include "kernels_ci16.h"
#include "kernels_xspec.h"

namespace sdrk {

template <bool I16>
__global__ __launch_bounds__(256) void xspec_split_kernel(const void* __restrict__ in, size_t stride, int nfft, unsigned col_blocks,
                                                          size_t n_items, float2* __restrict__ ch0, float2* __restrict__ ch1) {
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t f = item / col_blocks;
        const int n = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (n >= nfft) continue;
        const size_t e = f * stride + (size_t)n, o = f * (size_t)nfft + (size_t)n;
        if (I16) {
            const uint2 w = static_cast<const uint2*>(in)[e];
            float re, im;
            ci16_unpack(w.x, re, im);
            ch0[o] = make_float2(re, im);
            ci16_unpack(w.y, re, im);
            ch1[o] = make_float2(re, im);
        } else {
            const float4 x = static_cast<const float4*>(in)[e];
            ch0[o] = make_float2(x.x, x.y);
            ch1[o] = make_float2(x.z, x.w);
        }
    }
}

hipError_t launch_xspec_split(const void* d_in, bool i16, size_t n_frames, size_t stride, int nfft, float2* d_ch0, float2* d_ch1,
                              int num_cus, hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_frames * col_blocks;
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    const dim3 g((unsigned)(n_items < cap ? n_items : cap)), b(256);
    if (i16)
        hipLaunchKernelGGL(xspec_split_kernel<true>, g, b, 0, stream, d_in, stride, nfft, col_blocks, n_items, d_ch0, d_ch1);
    else
        hipLaunchKernelGGL(xspec_split_kernel<false>, g, b, 0, stream, d_in, stride, nfft, col_blocks, n_items, d_ch0, d_ch1);
    return hipGetLastError();
}

// the four planes of a group from its sums
__device__ __forceinline__ void xs_store_planes(float* __restrict__ row, int nfft, int col, const XsState& s, const IntUnits& c) {
    row[col] = xs_output(s.aa, c.inv_k, c.scale);
    row[(size_t)nfft + col] = xs_output(s.bb, c.inv_k, c.scale);
    row[2 * (size_t)nfft + col] = xs_output(s.re, c.inv_k, c.scale);
    row[3 * (size_t)nfft + col] = xs_output(s.im, c.inv_k, c.scale);
}

__global__ __launch_bounds__(256) void xspec_rows_kernel(const float2* __restrict__ spec0, const float2* __restrict__ spec1,
                                                         size_t in_stride, IntUnits c, int nfft, unsigned col_blocks,
                                                         size_t n_items, float* __restrict__ out, float4* __restrict__ partials,
                                                         const float4* __restrict__ carry_in, float4* __restrict__ carry_out) {
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t u = c.u_first + item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const IntUnit cur = int_unit(c, u);
        XsState s{0.0f, 0.0f, 0.0f, 0.0f};
        if (!cur.starts) {
            const float4 t = carry_in[col];
            s = XsState{t.x, t.y, t.z, t.w};
        }
        const size_t at = (cur.fb - c.f0) * in_stride + col;
        const float2* __restrict__ x0 = spec0 + at;
        const float2* __restrict__ x1 = spec1 + at;
        for (size_t f = cur.fb; f < cur.fe; ++f, x0 += in_stride, x1 += in_stride) {
            const float2 a = *x0, b = *x1;
            xs_accumulate(s, a.x, a.y, b.x, b.y);
        }
        if (cur.ends && c.slices == 1)
            xs_store_planes(out + (cur.g - c.out_row0) * 4 * (size_t)nfft, nfft, col, s, c);
        else
            (cur.ends ? partials + u * (size_t)nfft : carry_out)[col] = make_float4(s.aa, s.bb, s.re, s.im);
    }
}

hipError_t launch_xspec_rows(const IntegrateArgs& a, const float2* d_in2) {
    if (a.f1 <= a.f0) return hipSuccess;
    IntUnits c = int_units(a);   // power planes, whatever the call's out_form says
    c.out_form = INT_OUT_POWER;
    c.eps = 0.0f;
    const unsigned col_blocks = (unsigned)((a.nfft + 255) / 256);
    const size_t n_items = (c.u_last - c.u_first + 1) * col_blocks;
    const size_t cap = (size_t)a.num_cus * 32;
    hipLaunchKernelGGL(xspec_rows_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, a.stream,
                       static_cast<const float2*>(a.d_in), d_in2, a.in_stride, c, a.nfft, col_blocks, n_items, a.d_out,
                       reinterpret_cast<float4*>(a.d_partials), reinterpret_cast<const float4*>(a.d_carry_in),
                       reinterpret_cast<float4*>(a.d_carry_out));
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void xspec_finalize_kernel(const float4* __restrict__ partials, size_t n_groups, IntUnits c,
                                                             int nfft, float* __restrict__ out) {
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_groups * col_blocks;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t g = item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const float4* __restrict__ x = partials + g * c.slices * (size_t)nfft + col;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (unsigned s = 0; s < c.slices; ++s) {
            const float4 p = x[(size_t)s * nfft];
            t0 += (double)p.x;
            t1 += (double)p.y;
            t2 += (double)p.z;
            t3 += (double)p.w;
        }
        xs_store_planes(out + g * 4 * (size_t)nfft, nfft, col, XsState{(float)t0, (float)t1, (float)t2, (float)t3}, c);
    }
}

hipError_t launch_xspec_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int, int,
                                 float scale, float, float* d_out, int num_cus, hipStream_t stream) {
    if (n_groups == 0) return hipSuccess;
    IntUnits c{};   // (the finalize reads the slice count and what the epilogue takes)
    c.k = k;
    c.slices = (unsigned)slices;
    c.out_form = INT_OUT_POWER;
    c.scale = scale;
    c.inv_k = 1.0f / (float)k;
    const size_t n_items = n_groups * (size_t)((nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    hipLaunchKernelGGL(xspec_finalize_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(d_partials), n_groups, c, nfft, d_out);
    return hipGetLastError();
}

}  // namespace sdrk

// corrmat_rows.hip — the X-engine of the correlation-matrix calls, the de-interleave of the lengths without a reading
// transform, and the finalize of split groups.
//
// corrmat_split_kernel: the frames of a chunk, cut from the element stream (C samples per element: complex64, int16 pairs or
// byte pairs), -> C packed complex64 frame arrays, which the plan's own transform then takes like any caller's frames.  The
// integer formats are widened here exactly, so all three meet in the same complex64 values.  Every access is one sample wide:
// the stream is aligned to a sample, not to an element.
//
// corrmat_rows_kernel<C>: the C channels' complex64 spectra (already in the plan's shift order) lie in staging; one thread per
// bin walks the frames of a unit (integrate_split.h) down its column in all of them and keeps the C * C sums of
// kernels_corrmat.h in registers, in frame order.  End of unit as in xspec_rows.hip: the group's planes, a partial row or the
// carry row.
//
// corrmat_finalize_kernel: a group cut into S slices -> its planes.  The S partial sums are added in slice order in float64,
// rounded to float32 once, and go through the same expression as an unsplit group's.
#include "kernels_ci16.h"
#include "kernels_corrmat.h"

namespace sdrk {

// Input policies: one sample of one channel as loaded, and its complex64 value.
struct CmSmpC64 {
    typedef float2 sample;
    static __device__ __forceinline__ float2 widen(sample w, Iq8Conv) { return w; }
};
struct CmSmpS16 {
    typedef unsigned sample;
    static __device__ __forceinline__ float2 widen(sample w, Iq8Conv) {
        float re, im;
        ci16_unpack(w, re, im);
        return make_float2(re, im);
    }
};
struct CmSmpB8 {
    typedef unsigned short sample;
    static __device__ __forceinline__ float2 widen(sample w, Iq8Conv c) {
        float re, im;
        ci8_unpack(w, c, re, im);
        return make_float2(re, im);
    }
};

template <class In>
__global__ __launch_bounds__(256) void corrmat_split_kernel(const typename In::sample* __restrict__ in, Iq8Conv conv, int channels,
                                                            size_t stride, int nfft, unsigned col_blocks, size_t n_items,
                                                            float2* __restrict__ ch, size_t plane) {
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t f = item / col_blocks;
        const int n = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (n >= nfft) continue;
        const typename In::sample* __restrict__ e = in + (f * stride + (size_t)n) * (size_t)channels;
        float2* __restrict__ o = ch + f * (size_t)nfft + (size_t)n;
        for (int c = 0; c < channels; ++c) o[(size_t)c * plane] = In::widen(e[c], conv);
    }
}

hipError_t launch_corrmat_split(const void* d_in, int fmt, int channels, size_t n_frames, size_t stride, int nfft, float2* d_ch,
                                size_t plane, int num_cus, hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_frames * col_blocks;
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    const dim3 g((unsigned)(n_items < cap ? n_items : cap)), b(256);
    const Iq8Conv conv = iq8_conv(fmt == CM_B8_UNSIGNED ? IQ8_UNSIGNED : IQ8_SIGNED);
    if (fmt == CM_C64)
        hipLaunchKernelGGL(corrmat_split_kernel<CmSmpC64>, g, b, 0, stream, static_cast<const float2*>(d_in), conv, channels, stride,
                           nfft, col_blocks, n_items, d_ch, plane);
    else if (fmt == CM_S16)
        hipLaunchKernelGGL(corrmat_split_kernel<CmSmpS16>, g, b, 0, stream, static_cast<const unsigned*>(d_in), conv, channels,
                           stride, nfft, col_blocks, n_items, d_ch, plane);
    else
        hipLaunchKernelGGL(corrmat_split_kernel<CmSmpB8>, g, b, 0, stream, static_cast<const unsigned short*>(d_in), conv, channels,
                           stride, nfft, col_blocks, n_items, d_ch, plane);
    return hipGetLastError();
}

template <int C>
__global__ __launch_bounds__(256) void corrmat_rows_kernel(const float2* __restrict__ spec, size_t plane, size_t in_stride,
                                                           IntUnits c, int nfft, unsigned col_blocks, size_t n_items,
                                                           float* __restrict__ out, float* __restrict__ partials,
                                                           const float* __restrict__ carry_in, float* __restrict__ carry_out) {
    constexpr int Q = C * C;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t u = c.u_first + item / col_blocks;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const IntUnit cur = int_unit(c, u);
        float s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = cur.starts ? 0.0f : carry_in[(size_t)q * nfft + col];
        const float2* __restrict__ x = spec + (cur.fb - c.f0) * in_stride + col;
        for (size_t f = cur.fb; f < cur.fe; ++f, x += in_stride) {
            float xr[C], xi[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const float2 v = x[(size_t)ch * plane];
                xr[ch] = v.x;
                xi[ch] = v.y;
            }
            cm_accumulate<C>(s, xr, xi);
        }
        if (cur.ends && c.slices == 1) {
            float* __restrict__ row = out + (cur.g - c.out_row0) * Q * (size_t)nfft + col;
#pragma unroll
            for (int q = 0; q < Q; ++q) row[(size_t)q * nfft] = xs_output(s[q], c.inv_k, c.scale);
        } else {
            float* __restrict__ row = (cur.ends ? partials + u * Q * (size_t)nfft : carry_out) + col;
#pragma unroll
            for (int q = 0; q < Q; ++q) row[(size_t)q * nfft] = s[q];
        }
    }
}

template <int C>
static void corrmat_rows_launch(const IntegrateArgs& a, const IntUnits& c, size_t plane) {
    const unsigned col_blocks = (unsigned)((a.nfft + 255) / 256);
    const size_t n_items = (c.u_last - c.u_first + 1) * col_blocks;
    const size_t cap = (size_t)(a.num_cus > 0 ? a.num_cus : 1) * 32;
    hipLaunchKernelGGL(corrmat_rows_kernel<C>, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, a.stream,
                       static_cast<const float2*>(a.d_in), plane, a.in_stride, c, a.nfft, col_blocks, n_items, a.d_out,
                       reinterpret_cast<float*>(a.d_partials), reinterpret_cast<const float*>(a.d_carry_in),
                       reinterpret_cast<float*>(a.d_carry_out));
}

hipError_t launch_corrmat_rows(const IntegrateArgs& a, int channels, size_t plane) {
    if (a.f1 <= a.f0) return hipSuccess;
    IntUnits c = int_units(a);   // power planes, whatever the call's out_form says
    c.out_form = INT_OUT_POWER;
    c.eps = 0.0f;
    switch (channels) {
        case 2: corrmat_rows_launch<2>(a, c, plane); break;
        case 3: corrmat_rows_launch<3>(a, c, plane); break;
        case 4: corrmat_rows_launch<4>(a, c, plane); break;
        case 5: corrmat_rows_launch<5>(a, c, plane); break;
        case 6: corrmat_rows_launch<6>(a, c, plane); break;
        case 7: corrmat_rows_launch<7>(a, c, plane); break;
        case 8: corrmat_rows_launch<8>(a, c, plane); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// (one thread per bin and sum: q is the slowest index of an item, so a wave reads one plane's consecutive bins)
__global__ __launch_bounds__(256) void corrmat_finalize_kernel(const float* __restrict__ partials, int q_count, size_t n_groups,
                                                               IntUnits c, int nfft, float* __restrict__ out) {
    const unsigned col_blocks = (unsigned)((nfft + 255) / 256);
    const size_t n_items = n_groups * (size_t)q_count * col_blocks;
    const size_t group = (size_t)q_count * (size_t)nfft;
    for (size_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const size_t gq = item / col_blocks;   // = g * q_count + q: planes of a group lie one behind the other
        const size_t g = gq / (size_t)q_count;
        const int col = (int)(item % col_blocks) * 256 + (int)threadIdx.x;
        if (col >= nfft) continue;
        const size_t at = (gq - g * (size_t)q_count) * (size_t)nfft + col;
        const float* __restrict__ x = partials + g * c.slices * group + at;
        double t = 0.0;
        for (unsigned s = 0; s < c.slices; ++s) t += (double)x[(size_t)s * group];
        out[g * group + at] = xs_output((float)t, c.inv_k, c.scale);
    }
}

hipError_t launch_corrmat_finalize(const float* d_partials, int channels, size_t n_groups, size_t k, size_t slices, int nfft,
                                   float scale, float* d_out, int num_cus, hipStream_t stream) {
    if (n_groups == 0) return hipSuccess;
    IntUnits c{};   // (the finalize reads the slice count and what the epilogue takes)
    c.k = k;
    c.slices = (unsigned)slices;
    c.out_form = INT_OUT_POWER;
    c.scale = scale;
    c.inv_k = 1.0f / (float)k;
    const int q_count = channels * channels;
    const size_t n_items = n_groups * (size_t)q_count * (size_t)((nfft + 255) / 256);
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 1) * 32;
    hipLaunchKernelGGL(corrmat_finalize_kernel, dim3((unsigned)(n_items < cap ? n_items : cap)), dim3(256), 0, stream, d_partials,
                       q_count, n_groups, c, nfft, d_out);
    return hipGetLastError();
}

}  // namespace sdrk

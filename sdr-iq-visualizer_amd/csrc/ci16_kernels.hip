// ci16_kernels.hip — the two small kernels of the int16 input format (kernels_ci16.h): the widening copy that feeds every frame
// length without an int16-reading transform of its own, and the synthetic generator in int16 form.
#include "kernels_ci16.h"
#include "synth_hash.h"

namespace sdrk {

// Row starts are only 4-byte aligned on the way in and 8-byte aligned on the way out (a row is a frame, or a run of overlapped
// frames, cut out of the caller's stream at an arbitrary sample): gfx950 global memory instructions take any dword-aligned
// address, and saying so in the types lets the compiler keep the 16-byte accesses.
typedef unsigned v4u_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));

// int16 pairs -> complex64.  One lane per 4 consecutive samples of a row: one 16-byte load, two 16-byte stores; the last
// 1-3 samples of a row whose length is not a multiple of 4 go one by one.  Grid-stride over (row, group of 4).
__global__ __launch_bounds__(256) void unpack_ci16_kernel(const unsigned* __restrict__ in, size_t in_row_stride,
                                                          float2* __restrict__ out, size_t n_rows, size_t row_len) {
    const size_t groups = (row_len + 3) / 4;
    const size_t total = n_rows * groups;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / groups, n = (i - r * groups) * 4;
        const unsigned* __restrict__ src = in + r * in_row_stride + n;
        float2* __restrict__ dst = out + r * row_len + n;
        if (n + 4 <= row_len) {
            const v4u_a4 w = __builtin_nontemporal_load(reinterpret_cast<const v4u_a4*>(src));
            float f[8];
            ci16_unpack(w.x, f[0], f[1]);
            ci16_unpack(w.y, f[2], f[3]);
            ci16_unpack(w.z, f[4], f[5]);
            ci16_unpack(w.w, f[6], f[7]);
            const v4f_a8 lo = {f[0], f[1], f[2], f[3]}, hi = {f[4], f[5], f[6], f[7]};
            reinterpret_cast<v4f_a8*>(dst)[0] = lo;
            reinterpret_cast<v4f_a8*>(dst)[1] = hi;
        } else {
            for (size_t k = 0; n + k < row_len; ++k) {
                float re, im;
                ci16_unpack(src[k], re, im);
                dst[k] = make_float2(re, im);
            }
        }
    }
}

hipError_t launch_unpack_ci16(const void* d_in, size_t in_row_stride, void* d_out, size_t n_rows, size_t row_len, int num_cus,
                              hipStream_t stream) {
    const size_t total = n_rows * ((row_len + 3) / 4);
    if (total == 0) return hipSuccess;
    size_t blocks = (total + 255) / 256;
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 256) * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(unpack_ci16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const unsigned*>(d_in),
                       in_row_stride, static_cast<float2*>(d_out), n_rows, row_len);
    return hipGetLastError();
}

// synth_fill_kernel's values as int16 pairs.  One thread -> two consecutive samples (one 8-byte store).
__global__ __launch_bounds__(256) void synth_fill_ci16_kernel(uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft,
                                                              uint2* __restrict__ out) {
    const size_t pairs_per_frame = (size_t)nfft / 2;
    const size_t total = n_frames * pairs_per_frame;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t f = i / pairs_per_frame;
        const uint32_t n = (uint32_t)(i - f * pairs_per_frame) * 2u;
        const uint64_t F = first_frame + f;
        const uint32_t base = synth_frame_base(seed, F);
        auto pack = [base](uint32_t k) {
            int i16, q16;
            synth_codes(base, k, i16, q16);
            return ((uint32_t)i16 & 0xFFFFu) | ((uint32_t)q16 << 16);
        };
        out[i] = make_uint2(pack(n), pack(n + 1u));
    }
}

hipError_t launch_synth_fill_ci16(uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft, void* d_iq,
                                  hipStream_t stream) {
    if (n_frames == 0) return hipSuccess;
    const size_t total = n_frames * (size_t)(nfft / 2);
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(synth_fill_ci16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, seed, first_frame, n_frames, nfft,
                       static_cast<uint2*>(d_iq));
    return hipGetLastError();
}

}  // namespace sdrk

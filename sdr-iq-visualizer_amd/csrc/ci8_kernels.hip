// ci8_kernels.hip — the small kernel of the 8-bit input formats (kernels_ci8.h): the widening copy that feeds every frame
// length without an 8-bit-reading transform of its own.
#include "kernels_ci8.h"

namespace sdrk {

// Row starts are only 2-byte aligned on the way in and 8-byte aligned on the way out (a row is a frame, or a run of overlapped
// frames, cut out of the caller's stream at an arbitrary sample); saying so in the types leaves the access widths to the compiler.
typedef unsigned short v4us_a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef float v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));

// byte pairs -> complex64.  One lane per 4 consecutive samples of a row: 8 bytes in, two 16-byte stores; the last 1-3 samples
// of a row whose length is not a multiple of 4 go one by one.  Grid-stride over (row, group of 4).
__global__ __launch_bounds__(256) void unpack_ci8_kernel(const unsigned short* __restrict__ in, Iq8Conv conv, size_t in_row_stride,
                                                         float2* __restrict__ out, size_t n_rows, size_t row_len) {
    const size_t groups = (row_len + 3) / 4;
    const size_t total = n_rows * groups;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / groups, n = (i - r * groups) * 4;
        const unsigned short* __restrict__ src = in + r * in_row_stride + n;
        float2* __restrict__ dst = out + r * row_len + n;
        if (n + 4 <= row_len) {
            const v4us_a2 w = __builtin_nontemporal_load(reinterpret_cast<const v4us_a2*>(src));
            float f[8];
            ci8_unpack(w.x, conv, f[0], f[1]);
            ci8_unpack(w.y, conv, f[2], f[3]);
            ci8_unpack(w.z, conv, f[4], f[5]);
            ci8_unpack(w.w, conv, f[6], f[7]);
            const v4f_a8 lo = {f[0], f[1], f[2], f[3]}, hi = {f[4], f[5], f[6], f[7]};
            reinterpret_cast<v4f_a8*>(dst)[0] = lo;
            reinterpret_cast<v4f_a8*>(dst)[1] = hi;
        } else {
            for (size_t k = 0; n + k < row_len; ++k) {
                float re, im;
                ci8_unpack(src[k], conv, re, im);
                dst[k] = make_float2(re, im);
            }
        }
    }
}

hipError_t launch_unpack_ci8(const void* d_in, int fmt, size_t in_row_stride, void* d_out, size_t n_rows, size_t row_len,
                             int num_cus, hipStream_t stream) {
    const size_t total = n_rows * ((row_len + 3) / 4);
    if (total == 0) return hipSuccess;
    size_t blocks = (total + 255) / 256;
    const size_t cap = (size_t)(num_cus > 0 ? num_cus : 256) * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(unpack_ci8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const unsigned short*>(d_in),
                       iq8_conv(fmt), in_row_stride, static_cast<float2*>(d_out), n_rows, row_len);
    return hipGetLastError();
}

}  // namespace sdrk

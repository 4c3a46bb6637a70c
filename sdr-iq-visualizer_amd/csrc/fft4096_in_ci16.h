// fft4096_in_ci16.h — the int16 input policy of the N = 4096 streaming kernels (fft4096_core.h has the complex64 one, F4kInC64):
// fft4096_ci16.hip (per-frame rows and spectra, both load forms) and fft4096_kgroup_ci16.hip (one row per K frames, the direct
// form only).  See fft4096_ci16.hip for the two load forms and what each measured.
#pragma once
#include "fft4096_core.h"
#include "kernels_ci16.h"

namespace sdrk {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// Input policy, int16 pairs: one dword per sample, widened by ci16_unpack.
// x: the frame's raw dwords — direct: x[j] = sample tid + 256 j; WIDE: dwords 4 i .. 4 i + 3 = samples 1024 i + 4 tid + 0..3 until
// to_owners has sent them through the exchange LDS to the lanes that own them.
template <bool WIDE>
struct F4kInCi16 {
    typedef unsigned word;
    typedef unsigned sample;
    static __device__ __forceinline__ void issue(word (&x)[16], const sample* frame, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * 4);
        if constexpr (WIDE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const v4u q = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, tid * 16, i * 4096, F4K_NT));
                x[4 * i] = q.x, x[4 * i + 1] = q.y, x[4 * i + 2] = q.z, x[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b32(r, tid * 4, j * 1024, F4K_NT);
        }
    }
    // The direct form's 16 loads with each offset split into j / 4 * 4096 (scalar) + j % 4 * 1024 (which fits the instruction's
    // 12-bit immediate): 3 scalar registers hold offsets where issue() takes 15.  For the kernel whose unit bookkeeping leaves
    // the scalar file none to spare (fft4096_kgroup_ci16.hip); the same addresses, the same order.
    static __device__ __forceinline__ void issue_few_sgprs(word (&x)[16], const sample* frame, int tid) {
        static_assert(!WIDE, "the direct load form only");
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * 4);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            x[j] = __builtin_amdgcn_raw_buffer_load_b32(r, tid * 4 + (j & 3) * 1024, (j >> 2) * 4096, F4K_NT);
    }
    static __device__ __forceinline__ void to_owners(word (&x)[16], float2* lds, int tid) {
        if constexpr (WIDE) {
            unsigned* __restrict__ raw = reinterpret_cast<unsigned*>(lds);   // the exchange buffer, 16 KiB of it
            __syncthreads();   // the previous frame's pass-3 reads of the exchange buffer are done
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const v4u q = {x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
                *reinterpret_cast<v4u*>(raw + 1024 * i + 4 * tid) = q;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = raw[tid + 256 * j];
            // (f4k_transform's first barrier stands between these reads and its exchange-1 writes)
        }
    }
    static __device__ __forceinline__ cf widen(word w) {
        float re, im;
        ci16_unpack(w, re, im);
        return cf{re, im};
    }
};

}  // namespace sdrk

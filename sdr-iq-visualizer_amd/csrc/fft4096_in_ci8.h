// fft4096_in_ci8.h — the 8-bit input policy of the N = 4096 streaming kernels (fft4096_core.h has the complex64 one, F4kInC64,
// fft4096_in_ci16.h the int16 one): fft4096_ci8.hip (per-frame rows and spectra) and fft4096_kgroup_ci8.hip (one row per K
// frames).  The direct load form only: thread tid loads sample tid + 256 j as one 16-bit buffer load, 16 per thread and frame,
// every wave instruction reading 64 consecutive samples (128 B).  A frame may start at any sample: 2-byte alignment.
#pragma once
#include "fft4096_core.h"
#include "kernels_ci8.h"

namespace sdrk {

// Input policy, byte pairs: one 16-bit word per sample (zero-extended into its register), widened by ci8_unpack with the
// call's format.  x[j] = sample tid + 256 j.
struct F4kInCi8 {
    typedef unsigned word;
    typedef unsigned short sample;
    static __device__ __forceinline__ void issue(word (&x)[16], const sample* frame, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * 2);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b16(r, tid * 2, j * 512, F4K_NT);
    }
    // The same 16 loads with each offset split into j / 8 * 4096 (scalar) + j % 8 * 512 (which fits the instruction's 12-bit
    // immediate): one scalar register holds an offset where issue() may take 15.  For the kernel whose unit bookkeeping leaves
    // the scalar file none to spare (fft4096_kgroup_ci8.hip); the same addresses, the same order.  The empty asm makes the
    // lane's offset opaque at each call: inside a loop the compiler otherwise hoists the eight sums tid * 2 + j % 8 * 512 into
    // eight registers that live across the transform (7 VGPRs more than the immediates cost, which cost none).
    static __device__ __forceinline__ void issue_few_sgprs(word (&x)[16], const sample* frame, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * 2);
        int voff = tid * 2;
        asm volatile("" : "+v"(voff));
#pragma unroll
        for (int j = 0; j < 16; ++j)
            x[j] = __builtin_amdgcn_raw_buffer_load_b16(r, voff + (j & 7) * 512, (j >> 3) * 4096, F4K_NT);
    }
    static __device__ __forceinline__ void to_owners(word (&)[16], float2*, int) {}   // the loads are per owner already
    static __device__ __forceinline__ cf widen(word w, Iq8Conv c) {
        float re, im;
        ci8_unpack(w, c, re, im);
        return cf{re, im};
    }
};

}  // namespace sdrk

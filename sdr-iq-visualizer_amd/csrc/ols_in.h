// ols_in.h — the input policies of the overlap-save kernels (ols4096.hip, ols_bank.hip): F4kInC64 / F4kInCi16<false> under a
// descriptor clipped to the samples that exist, so the last block of a call reads zeros past n_in.  Device code only.
#pragma once
#include "fft4096_in_ci16.h"

namespace sdrk {

struct OlsInC64 {
    typedef v2u word;
    static constexpr int ELEM = 8;
    static __device__ __forceinline__ void load(word (&x)[16], const char* blk, unsigned bytes, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(blk, bytes);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b64(r, tid * ELEM, j * 256 * ELEM, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w) { return F4kInC64::widen(w); }
};
struct OlsInI16 {
    typedef unsigned word;
    static constexpr int ELEM = 4;
    static __device__ __forceinline__ void load(word (&x)[16], const char* blk, unsigned bytes, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(blk, bytes);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b32(r, tid * ELEM, j * 256 * ELEM, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w) { return F4kInCi16<false>::widen(w); }
};

}  // namespace sdrk

// pfb4096_in.h — the input policy of the N = 4096 polyphase-filter-bank kernels (pfb4096.hip, pfb4096_groups.hip), the PFB
// counterpart of fft4096_core.h's F4kInC64 and fft4096_in_ci16.h's F4kInCi16.
#pragma once
#include "fft4096_core.h"

namespace sdrk {

// Input policy: one tap block (16 words per thread, sample tid + 256 j) and its coefficients h[tid + 256 j].  The samples are
// read T times at hop = N, so unlike the flagship's they are loaded with the default cache policy.
struct F4kInPfb {
    typedef v2u word;
    static __device__ __forceinline__ void issue_samples(word (&x)[16], const float2* block, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(block, F4K_N * 8);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b64(r, tid * 8, j * 2048, 0);
    }
    static __device__ __forceinline__ void issue_coeffs(float (&c)[16], const float* hblock, int tid) {
        __amdgpu_buffer_rsrc_t rh = frame_rsrc(hblock, F4K_N * 4);
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rh, tid * 4, j * 1024, 0));
    }
    static __device__ __forceinline__ void issue(word (&x)[16], float (&c)[16], const float2* block, const float* hblock, int tid) {
        issue_samples(x, block, tid);
        issue_coeffs(c, hblock, tid);
    }
    static __device__ __forceinline__ cf widen(word w) {
        v2f t = __builtin_bit_cast(v2f, w);
        return cf{t.x, t.y};
    }
};

}  // namespace sdrk

// pfb4096_in.h — the input policies of the N = 4096 polyphase-filter-bank kernels (pfb4096_body.h), the PFB counterparts of
// fft4096_core.h's F4kInC64 and fft4096_in_ci16.h's F4kInCi16: F4kInPfb reads complex64 (pfb4096.hip, pfb4096_groups.hip),
// F4kInPfbI16 interleaved int16 I,Q (pfb4096_i16.hip, pfb4096_i16_groups.hip), F4kInPfbIq8 interleaved 8-bit I,Q of either
// format (pfb4096_iq8.hip, pfb4096_iq8_groups.hip).
#pragma once
#include "fft4096_core.h"
#include "kernels_ci16.h"
#include "kernels_ci8.h"

namespace sdrk {

// Input policy: one tap block (16 words per thread, sample tid + 256 j) and its coefficients h[tid + 256 j].  The samples are
// read T times at hop = N, so unlike the flagship's they are loaded with the default cache policy.
struct F4kInPfb {
    typedef float2 sample;   // what the stream pointer counts in
    typedef v2u word;        // a loaded sample on its way to widen()
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

// The same for int16 I,Q, 4 bytes per sample: the tap block in flight is 16 dwords per thread, not 16 qwords.  Each sample is
// one dword load through a resource of exactly the block's 4096 * 4 bytes, so block starts need 4-byte alignment only and no
// load can leave the block.  x = float32(I) + i float32(Q) exactly (ci16_unpack), at the point the complex64 policy bit-casts.
// (The 128-bit form of fft4096_in_ci16.h wants 16-byte-aligned starts and an LDS round trip per tap block: not here.)
struct F4kInPfbI16 {
    typedef unsigned sample;
    typedef unsigned word;
    static __device__ __forceinline__ void issue_samples(word (&x)[16], const unsigned* block, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(block, F4K_N * 4);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b32(r, tid * 4, j * 1024, 0);
    }
    static __device__ __forceinline__ void issue_coeffs(float (&c)[16], const float* hblock, int tid) {
        F4kInPfb::issue_coeffs(c, hblock, tid);
    }
    // Coefficients first: a sample word and a coefficient are both one dword, and where one path ends in issue() and its
    // sibling in issue_samples() (pfb4096_groups_body) the compiler merges the two trailing dword stores into one store through
    // a selected pointer, which pins both arrays in scratch.  With the samples last on both paths the trailing stores are the
    // same stores.  (Loads return in issue order either way, and the consumer waits for all 32.)
    static __device__ __forceinline__ void issue(word (&x)[16], float (&c)[16], const unsigned* block, const float* hblock, int tid) {
        issue_coeffs(c, hblock, tid);
        issue_samples(x, block, tid);
    }
    static __device__ __forceinline__ cf widen(word w) {
        float re, im;
        ci16_unpack(w, re, im);
        return cf{re, im};
    }
};

// The same for 8-bit I,Q (SigMF ci8 / cu8), 2 bytes per sample: each sample is one 16-bit load, zero-extended into its dword,
// through a resource of exactly the block's 4096 * 2 bytes, so block starts need 2-byte alignment only (any hop, odd ones
// too) and no load can leave the block.  Default cache policy, as above.  The policy is an object: it carries the call's
// conversion (kernels_ci8.h: a run-time kernel argument, so a format adds no instantiation) to the point of use, where
// x = ci8_unpack(word) exactly.  Coefficients first, for F4kInPfbI16's reason: the sample word is one dword here too.
struct F4kInPfbIq8 {
    typedef unsigned short sample;
    typedef unsigned word;
    Iq8Conv conv;
    static __device__ __forceinline__ void issue_samples(word (&x)[16], const unsigned short* block, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(block, F4K_N * 2);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b16(r, tid * 2, j * 512, 0);
    }
    static __device__ __forceinline__ void issue_coeffs(float (&c)[16], const float* hblock, int tid) {
        F4kInPfb::issue_coeffs(c, hblock, tid);
    }
    static __device__ __forceinline__ void issue(word (&x)[16], float (&c)[16], const unsigned short* block, const float* hblock,
                                                 int tid) {
        issue_coeffs(c, hblock, tid);
        issue_samples(x, block, tid);
    }
    __device__ __forceinline__ cf widen(word w) const {
        float re, im;
        ci8_unpack(w, conv, re, im);
        return cf{re, im};
    }
};

}  // namespace sdrk

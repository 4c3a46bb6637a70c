// pfb_fold_body.h — the body of the fold kernels of the lengths without a folding transform (pfb_fold.hip: complex64 samples,
// pfb_fold_i16.hip: int16 I,Q, pfb_fold_iq8.hip: 8-bit I,Q), a __device__ template over how one sample is read.  The policy is
// passed as an object too, for the 8-bit one's run-time conversion; the others are empty.
//   y[n] = (((h[n] x[n]) + h[N+n] x[N+n]) + h[2N+n] x[2N+n]) + ...      per real component, float32, no fused multiply-add
#pragma once
#include "kernels_ci16.h"
#include "kernels_ci8.h"
#include "kernels_pfb.h"

namespace sdrk {

struct PfbFoldInC64 {
    typedef float2 sample;
    static __device__ __forceinline__ pfb_v2f load(const float2* p) {
        const float2 x = *p;
        return pfb_v2f{x.x, x.y};
    }
};
struct PfbFoldInI16 {   // one dword = (I, Q): 4-byte alignment at any stride
    typedef unsigned sample;
    static __device__ __forceinline__ pfb_v2f load(const unsigned* p) {
        float re, im;
        ci16_unpack(*p, re, im);
        return pfb_v2f{re, im};
    }
};

struct PfbFoldInIq8 {   // one 16-bit word = (I, Q): 2-byte alignment at any stride; the call's conversion (kernels_ci8.h)
    typedef unsigned short sample;
    Iq8Conv conv;
    __device__ __forceinline__ pfb_v2f load(const unsigned short* p) const {
        float re, im;
        ci8_unpack(*p, conv, re, im);
        return pfb_v2f{re, im};
    }
};

// One thread, one complex sample; a workgroup walks tiles of 256 consecutive samples of one frame.
template <class In>
__device__ __forceinline__ void pfb_fold_body(const typename In::sample* __restrict__ iq, size_t frame_stride, size_t n_frames, int nfft,
                                              const float* __restrict__ h, int taps, float2* __restrict__ out, In in = In{}) {
    const size_t tiles_per_frame = ((size_t)nfft + 255) / 256;
    const size_t tiles = n_frames * tiles_per_frame;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t f = tile / tiles_per_frame;
        const size_t n = (tile - f * tiles_per_frame) * 256 + threadIdx.x;
        if (n >= (size_t)nfft) continue;
        const typename In::sample* __restrict__ x = iq + f * frame_stride + n;
        const float* __restrict__ c = h + n;
        pfb_v2f acc = pfb_mul(in.load(x), c[0]);
        for (int t = 1; t < taps; ++t) acc = pfb_mac(acc, in.load(x + (size_t)t * nfft), c[(size_t)t * nfft]);
        out[f * (size_t)nfft + n] = make_float2(acc.x, acc.y);
    }
}

}  // namespace sdrk

// synth_hash.h — the integer hash behind the synthetic IQ generator (sdrk_synth_fill, sdrk_synth_fill_ci16; numpy mirror:
// synth.py), shared by its complex64 and int16 kernels so that the two cannot drift apart.
#pragma once
#include <stdint.h>

namespace sdrk {

// MurmurHash3's 32-bit finaliser
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The two 12-bit codes of sample n of frame F under `seed`: I = (h & 0xFFF) - 2048, Q = ((h >> 12) & 0xFFF) - 2048.
__host__ __device__ inline uint32_t synth_frame_base(uint32_t seed, uint64_t F) {
    return fmix32(seed ^ (uint32_t)F) ^ fmix32((uint32_t)(F >> 32) + 0x9E3779B1u);
}
__host__ __device__ inline void synth_codes(uint32_t base, uint32_t n, int& i, int& q) {
    const uint32_t h = fmix32(base ^ n);
    i = (int)(h & 0xFFFu) - 2048;
    q = (int)((h >> 12) & 0xFFFu) - 2048;
}

}  // namespace sdrk

// f4k_split.h — into how many launches plan_launch (sdrk_plan.hip) cuts one N = 4096 call.  Pure arithmetic, no HIP.
//
// The time fft4096_kernel needs per frame grows with the length of the launch, on every buffer pair: 2^20 Hann frames take
// 8.63-9.60 ms as one launch (which of these: the pair's "level") and 8.58-8.88 ms as 16 back-to-back
// launches of 65536 frames, gaps included, on the same 18 pairs (profiles/placement_chunks/SUMMARY.md); 4 launches 8.81-9.26,
// 64 launches 8.71-8.91, 256 launches 9.85-9.95 (launch gaps and ramps take over).  Most of what a pair's level costs arises
// only inside a long launch; a launch boundary, which brings the persistent workgroups back into step, undoes it.
#pragma once
#include <cstddef>

namespace sdrk_host {

constexpr size_t F4K_SPLIT_FRAMES = 65536;   // 2 GiB of complex64 in, 1 GiB of rows out: about 0.54 ms of the kernel

// The number of launches for a call of n_frames frames: n_frames / F4K_SPLIT_FRAMES rounded to nearest, at least 1 — so every
// launch has between 2/3 and 3/2 of F4K_SPLIT_FRAMES frames once there is more than one, and no call ends in a short stub.
constexpr size_t f4k_split_parts(size_t n_frames) {
    return n_frames < F4K_SPLIT_FRAMES + F4K_SPLIT_FRAMES / 2 ? 1 : (n_frames + F4K_SPLIT_FRAMES / 2) / F4K_SPLIT_FRAMES;
}

}  // namespace sdrk_host

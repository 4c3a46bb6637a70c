// kernels_real.h — internal interface between the real-input entry points of the C ABI (sdrk_exec_*_real, ci16_api.hip) and the
// gfx950 kernels behind them.  A frame of L = 2 N real samples is, bit for bit, a frame of N pairs (x[2m], x[2m+1]): float32
// pairs are complex64 samples, int16 pairs int16 I,Q, byte pairs 8-bit I,Q — so the input policies and widenings of those
// formats serve unchanged.  With y = w x (one float32 product per sample; no window: no product), z[m] = y[2m] + i y[2m+1]
// and Z = DFT_N(z), for k = 0 ... N (Z[N] = Z[0]):
//   E = (Z[k] + conj Z[N-k]) / 2,  O = -(i/2) (Z[k] - conj Z[N-k]),  X[k] = E + exp(-i pi k / N) O
//   X[0] = Re Z[0] + Im Z[0],  X[N] = Re Z[0] - Im Z[0], imaginary parts +0.0
// Rows of N + 1 bins, ascending from 0 to fs/2, no fftshift; complex64, or float32 dB through logpsd_db with the plan's eps.
// Nothing here is exported.
#pragma once
#include "kernels.h"
#include "kernels_integrate.h"

namespace sdrk {

constexpr int REAL_F32 = 0, REAL_S16 = 1, REAL_S8 = 2, REAL_U8 = 3;   // SDRK_REAL_* of include/sdrk.h
constexpr size_t real_pair_bytes(int fmt) { return fmt == REAL_F32 ? 8 : fmt == REAL_S16 ? 4 : 2; }

struct RealArgs {
    const void* d_x = nullptr;         // pairs of real samples, frame f at pair f * frame_stride
    int fmt = REAL_F32;
    size_t frame_stride = 0;           // PAIRS between frame starts
    size_t n_frames = 0;
    int nfft = 0;                      // N: pairs per frame
    const float* d_window = nullptr;   // 2 N floats (a pair of coefficients per element) or nullptr
    const float2* d_tab = nullptr;     // exp(-i pi k / N), k < N, float64 rounded once
    const void* d_twiddle = nullptr;   // the plan's W4096^m
    float eps = 1e-12f;
    int epilogue = EPI_LOGPSD;         // EPI_LOGPSD or EPI_COMPLEX
    void* d_out = nullptr;             // rows of N + 1 bins, row f at element f * out_stride
    size_t out_stride = 0;             // elements, >= N + 1
    hipStream_t stream = nullptr;
    int num_cus = 256;
};

// rspec4096.hip: N = 4096 (real frames of 8192) in one launch on the caller's data — widening, window, transform, the
// mirrored exchange, the split butterfly, the epilogue and the row stores inside one persistent kernel
hipError_t launch_rspec4096(const RealArgs& a);
// real_kernels.hip, the staged route of every other length: widen and window n_frames frames into packed complex64 pairs ...
hipError_t launch_real_pairs(const RealArgs& a, void* d_pairs);
// ... and, behind the plan's own transform of those (natural order, complex64: d_z, packed), X and the epilogue into the rows
hipError_t launch_real_split(const RealArgs& a, const void* d_z);
// rspec4096_groups.hip (built into the companion library): N = 4096 with the reduction over K frames behind the split, in the
// transform's registers — one row of 4097 float32 per group; the real-input fields of IntegrateArgs say what the samples are
hipError_t launch_rspec4096_groups(const IntegrateArgs& a);

}  // namespace sdrk

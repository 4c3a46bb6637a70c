// kernels_f64.h — launchers of the double-precision transforms (fft_f64.hip), for the host side of the f64 entry points
// (sdrk_f64.hip).  Plain pointer types only: complex128 arrays are interleaved doubles.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace sdrk {

enum F64Epilogue {
    EPI64_DB = 0,       // float64 20*log10(|X| + eps)   (streamer.py:121, in the reference's order: abs, + eps, log10, * 20)
    EPI64_COMPLEX = 1,  // complex128 X                  (streamer.py:119 only)
};

constexpr int F64_TILE = 4096;        // complex128 elements one workgroup holds in LDS (64 KiB)
constexpr int F64_TWIDDLES = 4096;    // W_4096^m, m < 4096: every sub-transform length divides 4096

struct F64Args {
    const void* d_iq = nullptr;       // complex128 input, frame f at sample f * frame_stride
    size_t frame_stride = 0;          // samples
    void* d_out = nullptr;            // n_frames * nfft float64 (EPI64_DB) or complex128 (EPI64_COMPLEX)
    size_t n_frames = 0;
    int nfft = 0;                     // power of two, 2 ... 2^22
    const double* d_window = nullptr; // nfft doubles or nullptr (rectangular)
    const double* d_twiddle = nullptr;// F64_TWIDDLES complex128: exp(-2 pi i m / 4096)
    void* d_scratch = nullptr;        // nfft > F64_TILE: scratch_frames * nfft complex128 between the two passes
    size_t scratch_frames = 0;
    double eps = 0.0;
    int shift = 0;
    int epilogue = EPI64_DB;
    hipStream_t stream = nullptr;
};

// 2 <= nfft <= 4096: one pass in LDS (several frames per workgroup below 4096); 8192 <= nfft <= 2^22: a column pass into the
// scratch (four-step twiddle on its stores) and a row pass out of it, both sub-transforms <= 4096, scratch_frames at a time.
hipError_t launch_fft_f64(const F64Args& a);
// The split of a two-pass length: nfft = 2^l_col (column transforms) * 2^l_row (row transforms); false if none.
bool fft_f64_split(int nfft, int* l_col, int* l_row);

}  // namespace sdrk

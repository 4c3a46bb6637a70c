// fft4096_ci16.hip — the flagship N = 4096 transform (fft4096.hip) reading interleaved little-endian int16 I,Q: what the
// AD936x behind the reference's self.sdr.rx() delivers (app/sdr/streamer.py:114) before pyadi-iio widens it, and SigMF's
// ci16_le.  One HBM read of 4 B/sample and one HBM write of 4 B/sample per frame (the complex64 kernel: 8 + 4).
//
//   x[n] = float32(I[n]) + i float32(Q[n])     (exact)
// then fft4096.hip's arithmetic through the same f4k_transform and epilogues, so the rows and spectra are bit-identical to
// the complex64 kernel's on the widened samples.
//
// Two load forms, the same 16 KiB per workgroup in flight as the one-frame prefetch:
//   direct  x[tid + 256 j] as one dword per lane, 16 per thread: every wave instruction reads 64 consecutive samples (256 B),
//           the shape of the kernel's own row stores.  Frame starts need 4-byte alignment only (frame_stride is arbitrary).
//   WIDE    4 consecutive samples (16 B) per lane, 4 loads per thread (1 KiB per wave instruction); the dwords then go through
//           the exchange LDS (ds_write_b128 at their sample index, ds_read_b32 at tid + 256 j: both conflict free) to the lanes
//           that own them, at the price of two more workgroup barriers per frame.  Needs 16-byte aligned frame starts.
// launch_fft4096_ci16 says which one runs, and what each measured.
#include "fft4096_in_ci16.h"

#include <cstdlib>

namespace sdrk {

constexpr bool CI16_WIDE_DEFAULT = false;

// fft4096_kernel (fft4096.hip) with the int16 input policy, statement for statement; see there.
template <bool HAS_WINDOW, int EPILOGUE, bool WIDE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_ci16_kernel(
    const unsigned* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift) {
    typedef F4kInCi16<WIDE> In;
    __shared__ __attribute__((aligned(16))) float2 lds[f4k_lds_elems(HAS_WINDOW)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;

    const size_t first = blockIdx.x;
    const size_t step = gridDim.x;

    auto issue = [&](typename In::word (&x)[16], size_t fr) {
        if (fr >= n_frames) fr = first;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    auto process = [&](typename In::word (&x)[16], size_t f) {
        In::to_owners(x, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(x[j]);
        issue(x, f + step);
        f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + f * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
    };
    typename In::word nxt[16];
    issue(nxt, first);
    for (size_t f = first; f < n_frames; f += step) process(nxt, f);
}

hipError_t launch_fft4096_ci16(const LaunchArgs& a) {
    if (a.n_frames == 0) return hipSuccess;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const unsigned* iq = static_cast<const unsigned*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    // Which load form: measured in one process on 2^20 Hann frames, alternating (tools/bench_ci16.py, profiles/ci16/SUMMARY.md),
    // direct 7.18 ms, wide 7.38 ms per launch — the two extra barriers per frame cost more than twelve load instructions save.
    // The direct form is the default; the wide one is kept for A/B work and applies to 16-byte aligned frame starts only.
    bool wide = CI16_WIDE_DEFAULT;
    if (const char* env = getenv("SDRK_CI16_FORM")) wide = env[0] == 'w';   // "wide" / "direct": A/B work (tools/bench_ci16.py)
    if (a.frame_stride % 4 != 0 || reinterpret_cast<uintptr_t>(a.d_iq) % 16 != 0) wide = false;
#define SDRK_LAUNCH_F(W, E, F)                                                                       \
    hipLaunchKernelGGL((fft4096_ci16_kernel<W, E, F>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,   \
                       a.n_frames, a.d_window, tw, a.eps, a.shift)
#define SDRK_LAUNCH(W, E) do { if (wide) SDRK_LAUNCH_F(W, E, true); else SDRK_LAUNCH_F(W, E, false); } while (0)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
#undef SDRK_LAUNCH_F
    return hipGetLastError();
}

}  // namespace sdrk

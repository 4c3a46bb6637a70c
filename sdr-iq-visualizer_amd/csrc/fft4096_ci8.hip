// fft4096_ci8.hip — the flagship N = 4096 transform (fft4096.hip) reading interleaved 8-bit I,Q, signed (SigMF ci8: a HackRF)
// or unsigned (cu8: an RTL-SDR).  One HBM read of 2 B/sample and one HBM write of 4 B/sample per frame (the int16 kernel:
// 4 + 4, the complex64 kernel: 8 + 4).
//
//   signed    x[n] = float32(I[n]) + i float32(Q[n])
//   unsigned  x[n] = (float32(I[n]) - 127.5f) + i (float32(Q[n]) - 127.5f)        (both exact)
// then fft4096.hip's arithmetic through the same f4k_transform and epilogues, so the rows and spectra are bit-identical to
// the complex64 kernel's on the widened samples.  The format is a pair of run-time arguments of one conversion (kernels_ci8.h):
// it adds no instantiation.
//
// The direct load form of fft4096_ci16.hip: x[tid + 256 j] as one 16-bit word per lane, 16 per thread, every wave instruction
// reading 64 consecutive samples (128 B); 8 KiB per workgroup in flight as the one-frame prefetch.  Frame starts need 2-byte
// alignment only (frame_stride is arbitrary).  No wide form through LDS: it measured slower for int16 (fft4096_ci16.hip).
#include "fft4096_in_ci8.h"

namespace sdrk {

// fft4096_ci16_kernel's direct form (fft4096_ci16.hip) with the 8-bit input policy, statement for statement; see there.
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_ci8_kernel(
    const unsigned short* __restrict__ iq, Iq8Conv conv, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift) {
    typedef F4kInCi8 In;
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

    auto issue = [&](In::word (&x)[16], size_t fr) {
        if (fr >= n_frames) fr = first;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    auto process = [&](In::word (&x)[16], size_t f) {
        In::to_owners(x, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(x[j], conv);
        issue(x, f + step);
        f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + f * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
    };
    In::word nxt[16];
    issue(nxt, first);
    for (size_t f = first; f < n_frames; f += step) process(nxt, f);
}

hipError_t launch_fft4096_ci8(const LaunchArgs& a, int fmt) {
    if (a.n_frames == 0) return hipSuccess;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const unsigned short* iq = static_cast<const unsigned short*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const Iq8Conv conv = iq8_conv(fmt);
#define SDRK_LAUNCH(W, E)                                                                                        \
    hipLaunchKernelGGL((fft4096_ci8_kernel<W, E>), g, b, 0, a.stream, iq, conv, a.frame_stride, a.d_out, a.n_frames, \
                       a.d_window, tw, a.eps, a.shift)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

// pfb4096.hip — polyphase filter bank front end at N = 4096: T blocks of 4096 samples folded under a prototype filter of
// T * 4096 coefficients inside the transform's registers, then fft4096.hip's transform, fftshift and log epilogue unchanged.
// Sits in front of the reference's
//   app/sdr/streamer.py:119  fft_data = np.fft.fftshift(np.fft.fft(samples))
//   app/sdr/streamer.py:121  power_db = 20 * np.log10(np.abs(fft_data) + 1e-12)
// which has no counterpart of the fold (a build-side extension, like the decimated waterfall read-out): `samples` becomes
//   y[n] = (((h[n] x[n]) + h[N+n] x[N+n]) + h[2N+n] x[2N+n]) + ...      per real component, float32, no fused multiply-add
// 8 T bytes read per output sample where frames do not overlap their neighbours' blocks, 8 from HBM at hop = N (the other
// T - 1 readers of a block find it in cache), 4 bytes written.
//
// The kernel keeps fft4096_kernel's shape (persistent grid of three workgroups per CU, buffer loads, tables in LDS,
// f4k_transform, f4k_store_row).  Its input policy loads one tap block — 16 words per thread — and that block's 16
// coefficients, and accumulates into the 16 cf the transform takes.  One tap block is in flight beside the accumulators: the
// next tap's while this one is multiplied in, the next frame's first while this frame is transformed.  T is a run-time loop
// bound; the coefficients come through the cache with ordinary loads (T * 16 KiB does not fit beside the exchange buffer in LDS
// at three workgroups per CU).
//
// Integration over K folded frames is pfb4096_groups.hip.  Out of scope here: int16 input, double precision, waterfall appends.
#include "fft4096_core.h"
#include "kernels_pfb.h"
#include "pfb4096_in.h"

namespace sdrk {

template <int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw, size_t n_frames,
    const float* __restrict__ h, int taps, const float2* __restrict__ tw4096, float eps, int shift, int assign) {
    typedef F4kInPfb In;
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid

    // This workgroup's frames: first, first + step, ... below end.  Any partition gives the same rows; the choice decides which
    // L2 the T readers of a block meet in (kernels_pfb.h).
    size_t first = blockIdx.x, step = gridDim.x, end = n_frames;
    if (assign == PFB_ASSIGN_XCD && gridDim.x >= 8) {
        const size_t x = blockIdx.x & 7;
        first = x * n_frames / 8 + (blockIdx.x >> 3);
        end = (x + 1) * n_frames / 8;
        step = (gridDim.x - x + 7) >> 3;   // workgroups with this x
    } else if (assign == PFB_ASSIGN_RUNS) {
        first = (size_t)blockIdx.x * n_frames / gridDim.x;
        end = ((size_t)blockIdx.x + 1) * n_frames / gridDim.x;
        step = 1;
    }
    if (first >= end) return;   // (the whole workgroup)

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;

    In::word nxt[16];
    float cn[16];
    auto issue = [&](size_t fr, int t) {
        if (fr >= end) fr = first;  // harmless re-read past the end
        In::issue(nxt, cn, iq + fr * frame_stride + (size_t)t * F4K_N, h + (size_t)t * F4K_N, tid);
    };
    // the block in flight -> w, c; the one after it (this frame's next tap, or the next frame's first) on its way
    auto take = [&](cf (&w)[16], float (&c)[16], size_t f, int t) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            w[j] = In::widen(nxt[j]);
            c[j] = cn[j];
        }
        if (t + 1 < taps) issue(f, t + 1); else issue(f + step, 0);
    };
    issue(first, 0);
    for (size_t f = first; f < end; f += step) {
        cf v[16];
        {
            cf w[16];
            float c[16];
            take(w, c, f, 0);
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = pfb_mul(w[j], c[j]);
        }
        for (int t = 1; t < taps; ++t) {
            cf w[16];
            float c[16];
            take(w, c, f, t);
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = pfb_mac(v[j], w[j], c[j]);
        }
        f4k_transform(v, lds, tw256, tw1, A, tid);
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + f * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
    }
}

hipError_t launch_pfb4096(const LaunchArgs& a, const float* d_h, int taps, int assign) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !d_h || taps < 1 || taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    if (a.epilogue == EPI_LOGPSD)
        hipLaunchKernelGGL((pfb4096_kernel<EPI_LOGPSD>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps, tw,
                           a.eps, a.shift, assign);
    else if (a.epilogue == EPI_COMPLEX)
        hipLaunchKernelGGL((pfb4096_kernel<EPI_COMPLEX>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out, a.n_frames, d_h, taps, tw,
                           a.eps, a.shift, assign);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sdrk

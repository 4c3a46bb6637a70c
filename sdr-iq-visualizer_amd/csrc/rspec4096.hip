// rspec4096.hip — one-sided spectra of real-sampled frames of L = 8192 through the flagship N = 4096 transform: the frame is
// read as 4096 pairs (x[2m], x[2m+1]) by the input policy of its format (float32 pairs: F4kInC64; int16 pairs: F4kInCi16's
// direct form; byte pairs: F4kInCi8, signed or unsigned at run time), windowed with a pair of coefficients per element,
// transformed by f4k_transform, and split into the 4097 bins X[0 ... 4096] inside the same registers and LDS (kernels_real.h
// has the arithmetic).  One HBM read of 4 / 2 / 1 bytes per real sample and one write of about 2 (dB) or 4 (complex64).
//
// The split.  After f4k_transform thread tid holds Z[tid + 256 k2], k2 = 0 ... 15.  X[k] needs Z[(4096 - k) mod 4096], which
// is thread (256 - tid) mod 256's bin k2' = 15 - k2 (for tid = 0: k2' = (16 - k2) mod 16).  One exchange through the exchange
// buffer brings it over: every thread writes its 16 bins at index k (lanes consecutive, ascending) and, behind a barrier, reads
// index (4096 - k) & 4095 (lanes consecutive, descending) — both conflict free.  Two more workgroup barriers per frame than
// the complex kernels: one in front of the writes (the transform's pass-3 reads of the same buffer), one behind them; the next
// transform's entry barrier stands between these reads and its exchange-1 writes.  Then
//   X[k] = E + T O,  T = exp(-i pi tid / 4096) exp(-i pi k2 / 16)
// with the first factor from the plan's table (float64, rounded once; one register pair per thread, loaded once per launch)
// and the second a compile-time constant.  Bin 0 and bin 4096 are written from Z[0] alone, imaginary parts +0.0; bin 4096 by
// lane 0.  Rows start at any multiple of the element size (4097 is odd): dword / dwordx2 buffer stores.
//
// The window (8192 floats, 32 KiB) is read from global memory, a float2 per element and frame: with the 36,992 B of exchange
// buffer and tables, 32 KiB more LDS would make 69,760 B per workgroup — past the 64 KiB a workgroup may have, and two
// workgroups per CU where the registers allow three.  All workgroups read the same 32 KiB, which stays in L2; the 16 loads
// are issued at the top of a frame, in front of the widening, with the next frame's prefetch behind them.  Measured
// (tools/bench_real.py, 2^17 frames, Hann): 1.34 ms from float32, 1.16 from int16, 1.15 from bytes.
#include "rspec4096_in.h"

namespace sdrk {

// fft4096_ci16_kernel's persistent loop with a one-frame prefetch (fft4096_ci16.hip), the pair window in front of the
// transform and the split behind it.  frame_stride in pairs, out_stride in output elements.
template <int RFMT, bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void rspec4096_kernel(
    const void* __restrict__ x_raw, unsigned conv_mask, float conv_off, size_t frame_stride, void* __restrict__ out_raw,
    size_t out_stride, size_t n_frames, const float2* __restrict__ window, const float2* __restrict__ tw4096,
    const float2* __restrict__ rtab, float eps) {
    typedef typename RspecIn<RFMT>::In In;
    __shared__ __attribute__((aligned(16))) float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    const float2 t1 = rtab[tid];   // exp(-i pi tid / 4096)
    __syncthreads();

    const Iq8Conv conv = {conv_mask, conv_off};
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;
    const int mirror = F4K_N - tid;   // bin tid + 256 k2 reads index (mirror - 256 k2) & 4095
    const typename In::sample* __restrict__ x = static_cast<const typename In::sample*>(x_raw);

    const size_t first = blockIdx.x;
    const size_t step = gridDim.x;

    auto issue = [&](typename In::word (&w)[16], size_t fr) {
        if (fr >= n_frames) fr = first;  // harmless re-read past the end
        In::issue(w, x + fr * frame_stride, tid);
    };
    auto store = [&](__amdgpu_buffer_rsrc_t row, float re, float im, int voff, int soff) {
        if (EPILOGUE == EPI_LOGPSD) {
            const float db = logpsd_db(re, im, eps);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, db), row, voff, soff, F4K_NT);
        } else {
            const v2f o = {re, im};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, o), row, voff, soff, 0);
        }
    };
    auto process = [&](typename In::word (&w)[16], size_t f) {
        float2 win[16];
        if (HAS_WINDOW) {
#pragma unroll
            for (int j = 0; j < 16; ++j) win[j] = window[tid + 256 * j];
        }
        In::to_owners(w, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            v[j] = RspecIn<RFMT>::widen(w[j], conv);
            if (HAS_WINDOW) v[j] = cf{v[j].x * win[j].x, v[j].y * win[j].y};
        }
        // (the windowed products end here: left to itself the scheduler carries the 32 coefficient registers into the
        // transform's first pass, up to the 168-register budget and, in one instantiation, five registers past it)
        if (HAS_WINDOW) __builtin_amdgcn_sched_barrier(0);
        issue(w, f + step);
        f4k_transform<false>(v, lds, tw256, tw1, A, tid);
        __syncthreads();   // the transform's pass-3 reads of the exchange buffer are done
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) lds[tid + 256 * k2] = make_float2(v[rev16(k2)].x, v[rev16(k2)].y);
        __syncthreads();
        const __amdgpu_buffer_rsrc_t row =
            frame_rsrc(static_cast<char*>(out_raw) + f * out_stride * OUT_ELEM, (F4K_N + 1) * OUT_ELEM);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const cf z = v[rev16(k2)];
            const float2 m = lds[(mirror - 256 * k2) & (F4K_N - 1)];
            const float ex = 0.5f * (z.x + m.x), ey = 0.5f * (z.y - m.y);   // E = (Z + conj M) / 2
            const float ox = 0.5f * (z.y + m.y), oy = 0.5f * (m.x - z.x);   // O = -(i/2) (Z - conj M)
            const cf t = k2 == 0 ? cf{t1.x, t1.y} : cmul(cf{t1.x, t1.y}, cf{RS_C[k2], -RS_S[k2]});
            const cf to = cmul(t, cf{ox, oy});
            float re = ex + to.x, im = ey + to.y;
            if (k2 == 0 && tid == 0) re = z.x + z.y, im = 0.0f;             // X[0] from Z[0] alone
            store(row, re, im, voff_out, k2 * 256 * OUT_ELEM);
        }
        if (tid == 0) store(row, v[0].x - v[0].y, 0.0f, 0, F4K_N * OUT_ELEM);   // X[4096]; v[rev16(0)] = Z[0]
    };
    typename In::word nxt[16];
    issue(nxt, first);
    for (size_t f = first; f < n_frames; f += step) process(nxt, f);
}

hipError_t launch_rspec4096(const RealArgs& a) {
    if (a.n_frames == 0) return hipSuccess;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const float2* win = reinterpret_cast<const float2*>(a.d_window);
    const Iq8Conv conv = iq8_conv(a.fmt == REAL_U8 ? IQ8_UNSIGNED : IQ8_SIGNED);
#define SDRK_LAUNCH_R(R, W, E)                                                                                          \
    hipLaunchKernelGGL((rspec4096_kernel<R, W, E>), g, b, 0, a.stream, a.d_x, conv.mask, conv.off, a.frame_stride, a.d_out, \
                       a.out_stride, a.n_frames, win, tw, a.d_tab, a.eps)
#define SDRK_LAUNCH_WE(R)                                                                        \
    do {                                                                                         \
        if (a.epilogue == EPI_LOGPSD) {                                                          \
            if (win) SDRK_LAUNCH_R(R, true, EPI_LOGPSD); else SDRK_LAUNCH_R(R, false, EPI_LOGPSD);   \
        } else {                                                                                 \
            if (win) SDRK_LAUNCH_R(R, true, EPI_COMPLEX); else SDRK_LAUNCH_R(R, false, EPI_COMPLEX); \
        }                                                                                        \
    } while (0)
    if (a.fmt == REAL_F32) SDRK_LAUNCH_WE(0);
    else if (a.fmt == REAL_S16) SDRK_LAUNCH_WE(1);
    else SDRK_LAUNCH_WE(2);
#undef SDRK_LAUNCH_WE
#undef SDRK_LAUNCH_R
    return hipGetLastError();
}

}  // namespace sdrk

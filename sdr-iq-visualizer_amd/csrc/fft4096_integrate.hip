// fft4096_integrate.hip — the flagship transform (fft4096.hip: window * x -> 4096-point FFT -> fftshift) with the reduction
// over K consecutive frames in its registers: per bin the mean (Kahan), the maximum or the minimum of |X|^2 over the frames
// of a group, and ONE row per group out — 8 + 4/K bytes per sample through HBM where the per-frame kernel moves 12.
//
// Same shape as fft4096_kernel: persistent grid of F4K_WAVES workgroups per CU, buffer loads with the next frame's 16 loads
// per thread in flight while the current frame is transformed (across unit boundaries too), window from LDS, f4k_transform.
// Between frames the only additions are the accumulators: 16 VGPRs per thread (MAX / MIN), 32 with the compensation (MEAN).
// A workgroup takes whole units (integrate_split.h) grid-stride; at the end of a unit it writes, once,
//   - the group's row through the epilogue (dB or scaled power, nt stores) when the unit is a whole group,
//   - the unit's state into the partials (a group split into slices: integrate_rows.hip finalizes), or
//   - the state into the carry row when the launch ends inside the unit (chunked calls); the next launch picks it up.
#include "fft4096_core.h"
#include "kernels_integrate.h"

namespace sdrk {

template <bool HAS_WINDOW, int DET>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_integrate_kernel(
    const float2* __restrict__ iq, size_t frame_stride, IntUnits c, float* __restrict__ out, float2* __restrict__ partials,
    const float2* __restrict__ carry_in, float2* __restrict__ carry_out, const float* __restrict__ window,
    const float2* __restrict__ tw4096, int shift) {
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;   // bin k = tid + 256 k2 -> position tid + 256 (k2 ^ xor), as in fft4096.hip
    const int voff_in = tid * 8;

    auto issue = [&](v2u (&x)[16], size_t fr) { F4kInC64::issue(x, iq + (fr - c.f0) * frame_stride, tid); };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    v2u nxt[16];
    issue(nxt, int_unit(c, u).fb);
    for (;;) {
        // (the unit bookkeeping is wave-uniform and lives in SGPRs; of the next unit only its first frame is kept)
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        float acc[16], cmp[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) int_init<DET>(acc[k2], cmp[k2]);
        if (!starts) {   // state rows go through buffer instructions too: one VGPR offset, the row position in the SGPR offset
            __amdgpu_buffer_rsrc_t r = frame_rsrc(carry_in, F4K_N * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff_in, (k2 ^ xor_k2) * 2048, 0));
                acc[k2] = s.x;
                cmp[k2] = s.y;
            }
        }
        const size_t u_next = u + gridDim.x;
        const bool more = u_next <= c.u_last;
        const size_t n_fb = more ? int_unit(c, u_next).fb : fb;
        for (size_t f = fb; f < fe; ++f) {
            cf v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = F4kInC64::widen(nxt[j]);
            issue(nxt, f + 1 < fe ? f + 1 : n_fb);   // the last unit's last frame: a harmless re-read of its first
            // (not f4k_windowed_transform: through it this kernel compiles to other machine code)
            if (HAS_WINDOW) {
                float win[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) win[j] = lds_win[tid + 256 * j];
                f4k_transform<true>(v, lds, tw256, tw1, A, tid, win);
            } else {
                f4k_transform(v, lds, tw256, tw1, A, tid);
            }
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const cf z = v[rev16(k2)];
                int_accumulate<DET>(acc[k2], cmp[k2], fmaf(z.x, z.x, z.y * z.y));
            }
        }
        // ---- end of the unit ----
        if (ends && c.slices == 1) {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (g - c.out_row0) * (size_t)F4K_N, F4K_N * 4);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const float r = int_reduced<DET>(acc[k2], cmp[k2], c.inv_k);
                const float o = int_epilogue(r, c.out_form, c.scale, c.eps);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, tid * 4, (k2 ^ xor_k2) * 1024, F4K_NT);
            }
        } else {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(ends ? partials + u * (size_t)F4K_N : carry_out, F4K_N * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = {acc[k2], cmp[k2]};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, s), w, voff_in, (k2 ^ xor_k2) * 2048, 0);
            }
        }
        if (!more) break;
        u = u_next;
    }
}

hipError_t launch_fft4096_integrate(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntUnits c = int_units(a);
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, D)                                                                                               \
    hipLaunchKernelGGL((fft4096_integrate_kernel<W, D>), g, b, 0, a.stream, iq, a.in_stride, c, a.d_out, a.d_partials,    \
                       a.d_carry_in, a.d_carry_out, a.d_window, tw, a.shift)
#define SDRK_LAUNCH_W(D)                                                                                                \
    do {                                                                                                                \
        if (a.d_window) SDRK_LAUNCH(true, D); else SDRK_LAUNCH(false, D);                                               \
    } while (0)
    if (a.detector == INT_DET_MEAN) SDRK_LAUNCH_W(INT_DET_MEAN);
    else if (a.detector == INT_DET_MAX) SDRK_LAUNCH_W(INT_DET_MAX);
    else SDRK_LAUNCH_W(INT_DET_MIN);
#undef SDRK_LAUNCH_W
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

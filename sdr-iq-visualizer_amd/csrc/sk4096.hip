// sk4096.hip — spectral kurtosis at N = 4096: the flagship transform (fft4096.hip: window * x -> 4096-point FFT -> fftshift) with
// the two running sums of the estimator in its registers.  Per bin and group of K frames S1 = sum p and S2 = sum p^2 of
// p = |X|^2, and TWO rows per group out: the mean power S1 / K through the integrating epilogue (dB or scaled power) and
// SK = (K+1)/(K-1) (K S2 / S1^2 - 1) (kernels_sk.h) — 8 + 8/K bytes per sample through HBM from complex64, 4 + 8/K from int16 I,Q,
// where pulling every per-frame row back for numpy moves 12.
//
// The streaming skeleton of fft4096_integrate.hip, written once over the input policy: persistent grid of F4K_WAVES workgroups
// per CU, buffer loads with the next frame's 16 loads per thread in flight while the current frame is transformed (across unit
// boundaries too), window from LDS, f4k_transform.  Between frames the only additions are the sums: the 32 VGPRs per thread the
// compensated mean keeps there, with an add and an fma per bin and frame where Kahan takes four operations.  A workgroup takes
// whole units (integrate_split.h) grid-stride; at the end of a unit it writes, once,
//   - the group's two rows (nt stores; the estimator's divisions run here, outside the frame loop) when the unit is a whole group,
//   - the unit's {S1, S2} into the partials (a group split into slices: sk_rows.hip finalizes), or
//   - the state into the carry row when the launch ends inside the unit (chunked calls); the next launch picks it up.
// The int16 policy gives x[n] = float32(I[n]) + i float32(Q[n]) exactly and then the same arithmetic in the same order: rows,
// partial rows and carry rows have the bits of the complex64 instantiation on the widened samples.
#include "fft4096_in_ci16.h"
#include "kernels_sk.h"

namespace sdrk {

// The input policies of fft4096_core.h / fft4096_in_ci16.h with the load form this kernel takes under one name.  (int16: the
// direct loads with 3 offset registers, as in fft4096_kgroup_ci16.hip — the unit bookkeeping leaves the scalar file none to spare.)
struct SkInC64 : F4kInC64 {
    static __device__ __forceinline__ void load(word (&x)[16], const sample* frame, int tid) { issue(x, frame, tid); }
};
struct SkInI16 : F4kInCi16<false> {
    static __device__ __forceinline__ void load(word (&x)[16], const sample* frame, int tid) { issue_few_sgprs(x, frame, tid); }
};

template <class In, bool HAS_WINDOW>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void sk4096_kernel(
    const typename In::sample* __restrict__ iq, size_t frame_stride, IntUnits c, float kf, float* __restrict__ out,
    float2* __restrict__ partials, const float2* __restrict__ carry_in, float2* __restrict__ carry_out,
    const float* __restrict__ window, const float2* __restrict__ tw4096, int shift) {
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

    auto issue = [&](typename In::word (&x)[16], size_t fr) { In::load(x, iq + (fr - c.f0) * frame_stride, tid); };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    typename In::word nxt[16];
    issue(nxt, int_unit(c, u).fb);
    for (;;) {
        // (the unit bookkeeping is wave-uniform and lives in SGPRs; of the next unit only its first frame is kept)
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        float s1[16], s2[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) s1[k2] = s2[k2] = 0.0f;
        if (!starts) {   // state rows go through buffer instructions too: one VGPR offset, the row position in the SGPR offset
            __amdgpu_buffer_rsrc_t r = frame_rsrc(carry_in, F4K_N * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff_in, (k2 ^ xor_k2) * 2048, 0));
                s1[k2] = s.x;
                s2[k2] = s.y;
            }
        }
        const size_t u_next = u + gridDim.x;
        const bool more = u_next <= c.u_last;
        const size_t n_fb = more ? int_unit(c, u_next).fb : fb;
        for (size_t f = fb; f < fe; ++f) {
            cf v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
            issue(nxt, f + 1 < fe ? f + 1 : n_fb);   // the last unit's last frame: a harmless re-read of its first
            f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const cf z = v[rev16(k2)];
                sk_accumulate(s1[k2], s2[k2], fmaf(z.x, z.x, z.y * z.y));
            }
        }
        // ---- end of the unit ----
        if (ends && c.slices == 1) {   // plane 0 at the group's first nfft floats, plane 1 behind it: one descriptor, 32 KiB
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (g - c.out_row0) * (size_t)(2 * F4K_N), 2 * F4K_N * 4);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const float o = int_epilogue(s1[k2] * c.inv_k, c.out_form, c.scale, c.eps);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, tid * 4, (k2 ^ xor_k2) * 1024, F4K_NT);
            }
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const float o = sk_estimate(s1[k2], s2[k2], kf);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, tid * 4,
                                                      F4K_N * 4 + (k2 ^ xor_k2) * 1024, F4K_NT);
            }
        } else {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(ends ? partials + u * (size_t)F4K_N : carry_out, F4K_N * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = {s1[k2], s2[k2]};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, s), w, voff_in, (k2 ^ xor_k2) * 2048, 0);
            }
        }
        if (!more) break;
        u = u_next;
    }
}

template <class In>
static hipError_t launch_sk4096_of(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntUnits c = int_units(a);
    const float kf = (float)a.k;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const typename In::sample* iq = static_cast<const typename In::sample*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    if (a.d_window)
        hipLaunchKernelGGL((sk4096_kernel<In, true>), g, b, 0, a.stream, iq, a.in_stride, c, kf, a.d_out, a.d_partials,
                           a.d_carry_in, a.d_carry_out, a.d_window, tw, a.shift);
    else
        hipLaunchKernelGGL((sk4096_kernel<In, false>), g, b, 0, a.stream, iq, a.in_stride, c, kf, a.d_out, a.d_partials,
                           a.d_carry_in, a.d_carry_out, a.d_window, tw, a.shift);
    return hipGetLastError();
}

hipError_t launch_sk4096(const IntegrateArgs& a) { return launch_sk4096_of<SkInC64>(a); }
hipError_t launch_sk4096_i16(const IntegrateArgs& a) { return launch_sk4096_of<SkInI16>(a); }

}  // namespace sdrk

// sk4096_iq8.hip — spectral kurtosis at N = 4096 from interleaved 8-bit I,Q (SigMF ci8 / cu8, 2 bytes per sample): sk4096.hip's
// kernel with the 8-bit input policy (fft4096_in_ci8.h), 2 + 8/K bytes per sample through HBM where the int16 form moves
// 4 + 8/K and the complex64 form 8 + 8/K.
//
//   signed    x[n] = float32(I[n]) + i float32(Q[n])
//   unsigned  x[n] = (float32(I[n]) - 127.5f) + i (float32(Q[n]) - 127.5f)        (both exact)
// then the arithmetic of sk4096_kernel in the same order — f4k_windowed_transform, sk_accumulate, the two epilogues — so rows,
// partial rows and carry rows have the bits the complex64 instantiation produces on the widened samples, and sk_rows.hip's
// finalize serves as it is.  16 16-bit buffer loads per thread and frame (every wave instruction reads 64 consecutive samples),
// the next frame's in flight while the current one is transformed, across unit boundaries too; frame starts need 2-byte
// alignment only.  The format is two run-time arguments of one conversion: it adds no instantiation.
#include "fft4096_in_ci8.h"
#include "kernels_sk.h"

namespace sdrk {

// sk4096_kernel (sk4096.hip) with the 8-bit input policy, statement for statement; see there.  (The loads are the policy's
// issue_few_sgprs: the unit bookkeeping leaves the scalar file none to spare, as in fft4096_kgroup_ci8.hip.)
template <bool HAS_WINDOW>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void sk4096_iq8_kernel(
    const unsigned short* __restrict__ iq, Iq8Conv conv, size_t frame_stride, IntUnits c, float kf, float* __restrict__ out,
    float2* __restrict__ partials, const float2* __restrict__ carry_in, float2* __restrict__ carry_out,
    const float* __restrict__ window, const float2* __restrict__ tw4096, int shift) {
    typedef F4kInCi8 In;
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

    auto issue = [&](In::word (&x)[16], size_t fr) { In::issue_few_sgprs(x, iq + (fr - c.f0) * frame_stride, tid); };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    In::word nxt[16];
    issue(nxt, int_unit(c, u).fb);
    for (;;) {
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        float s1[16], s2[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) s1[k2] = s2[k2] = 0.0f;
        if (!starts) {
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
            for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j], conv);
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

template <int FMT>
hipError_t launch_sk4096_iq8(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    const IntUnits c = int_units(a);
    const float kf = (float)a.k;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const unsigned short* iq = static_cast<const unsigned short*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const Iq8Conv conv = iq8_conv(FMT);
    if (a.d_window)
        hipLaunchKernelGGL((sk4096_iq8_kernel<true>), g, b, 0, a.stream, iq, conv, a.in_stride, c, kf, a.d_out, a.d_partials,
                           a.d_carry_in, a.d_carry_out, a.d_window, tw, a.shift);
    else
        hipLaunchKernelGGL((sk4096_iq8_kernel<false>), g, b, 0, a.stream, iq, conv, a.in_stride, c, kf, a.d_out, a.d_partials,
                           a.d_carry_in, a.d_carry_out, a.d_window, tw, a.shift);
    return hipGetLastError();
}

template hipError_t launch_sk4096_iq8<IQ8_SIGNED>(const IntegrateArgs&);
template hipError_t launch_sk4096_iq8<IQ8_UNSIGNED>(const IntegrateArgs&);

}  // namespace sdrk

// pfb4096_body.h — the bodies of the N = 4096 polyphase-filter-bank kernels as __device__ templates over the input policy
// (pfb4096_in.h): F4kInPfb gives pfb4096_kernel and pfb4096_groups_kernel (pfb4096.hip, pfb4096_groups.hip), F4kInPfbI16
// gives their int16 forms (pfb4096_i16.hip, pfb4096_i16_groups.hip).  A policy names the sample type the stream pointer
// counts in (`sample`), the word a loaded sample travels in (`word`), and issues, and widens at the point of use; everything
// else — frame assignment, tap loop, one block in flight, transform, epilogue, unit bookkeeping — is the same text.
// The bodies take the policy as an object too (`in`), for what its widen() needs at run time: the 8-bit policy's conversion
// (F4kInPfbIq8; pfb4096_iq8.hip, pfb4096_iq8_groups.hip).  The other policies are empty, and compile as they did without it.
#pragma once
#include "fft4096_core.h"
#include "kernels_integrate.h"
#include "kernels_pfb.h"
#include "pfb4096_in.h"

namespace sdrk {

// pfb4096_kernel<EPILOGUE> / pfb4096_i16_kernel<EPILOGUE>
template <int EPILOGUE, class In>
__device__ __forceinline__ void pfb4096_body(
    const typename In::sample* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw, size_t n_frames,
    const float* __restrict__ h, int taps, const float2* __restrict__ tw4096, float eps, int shift, int assign, In in = In{}) {
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

    typename In::word nxt[16];
    float cn[16];
    auto issue = [&](size_t fr, int t) {
        if (fr >= end) fr = first;  // harmless re-read past the end
        In::issue(nxt, cn, iq + fr * frame_stride + (size_t)t * F4K_N, h + (size_t)t * F4K_N, tid);
    };
    // the block in flight -> w, c; the one after it (this frame's next tap, or the next frame's first) on its way
    auto take = [&](cf (&w)[16], float (&c)[16], size_t f, int t) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            w[j] = in.widen(nxt[j]);
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

// pfb4096_groups_kernel<DET> / pfb4096_i16_groups_kernel<DET>
template <int DET, class In>
__device__ __forceinline__ void pfb4096_groups_body(
    const typename In::sample* __restrict__ iq, size_t frame_stride, IntUnits c, float* __restrict__ out, float2* __restrict__ partials,
    const float2* __restrict__ carry_in, float2* __restrict__ carry_out, const float* __restrict__ h, int taps,
    const float2* __restrict__ tw4096, int shift, In in = In{}) {
    constexpr bool CMP_LDS = DET == INT_DET_MEAN;
    __shared__ float2 lds[f4k_lds_elems(CMP_LDS)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;
    float* __restrict__ lds_cmp = reinterpret_cast<float*>(tw1 + 256);   // [k2][tid], MEAN only

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;   // bin k = tid + 256 k2 -> position tid + 256 (k2 ^ xor), as in fft4096.hip
    const int voff_in = tid * 8;

    typename In::word nxt[16];
    float cn[16];
    auto issue = [&](size_t fr, int t) {
        In::issue(nxt, cn, iq + (fr - c.f0) * frame_stride + (size_t)t * F4K_N, h + (size_t)t * F4K_N, tid);
    };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    issue(int_unit(c, u).fb, 0);
    for (;;) {
        // The 64-bit ordered compares of the unit bookkeeping run on the vector unit with one operand in VGPRs; left to itself
        // the compiler hoists those uniform copies out of this loop and keeps them through the frame loop — over the budget.
        // (Should a later toolchain undo this, tests/test_pfb_integrate_code_objects.py trips on the VGPR count or the spills.)
        asm volatile("" : "+s"(c.f0), "+s"(c.f1), "+s"(c.k), "+s"(c.slice_len), "+s"(c.u_last));
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        float acc[16], cmp[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) int_init<DET>(acc[k2], cmp[k2]);
        if (!starts) {
            __amdgpu_buffer_rsrc_t r = frame_rsrc(carry_in, F4K_N * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff_in, (k2 ^ xor_k2) * 2048, 0));
                acc[k2] = s.x;
                if (CMP_LDS) cmp[k2] = s.y;   // (MAX / MIN: 0, and written back as 0)
            }
        }
        if (CMP_LDS) {
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) lds_cmp[tid + 256 * k2] = cmp[k2];
        }
        const size_t u_next = u + gridDim.x;
        const bool more = u_next <= c.u_last;
        const size_t n_fb = more ? int_unit(c, u_next).fb : fb;
        size_t f = fb;
        for (size_t left = fe - fb; left != 0; --left, ++f) {   // (counted down: equality tests stay on the scalar unit)
            const size_t f_next = left != 1 ? f + 1 : n_fb;   // the last unit's last frame: a harmless re-read of its first
            // the block in flight -> w, cw; the one after it (this frame's next tap, or the next frame's first) on its way
            auto take = [&](cf (&w)[16], float (&cw)[16], int t) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    w[j] = in.widen(nxt[j]);
                    cw[j] = cn[j];
                }
                if (t + 1 < taps) issue(f, t + 1); else In::issue_samples(nxt, iq + (f_next - c.f0) * frame_stride, tid);
            };
            cf v[16];
            {
                cf w[16];
                float cw[16];
                take(w, cw, 0);
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = pfb_mul(w[j], cw[j]);
            }
            for (int t = 1; t < taps; ++t) {
                cf w[16];
                float cw[16];
                take(w, cw, t);
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = pfb_mac(v[j], w[j], cw[j]);
            }
            f4k_transform(v, lds, tw256, tw1, A, tid);
            In::issue_coeffs(cn, h, tid);   // the next frame's first tap: the same 16 KiB for every frame
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const cf z = v[rev16(k2)];
                const float pw = fmaf(z.x, z.x, z.y * z.y);
                if (CMP_LDS) {
                    float cm = lds_cmp[tid + 256 * k2];
                    int_accumulate<DET>(acc[k2], cm, pw);
                    lds_cmp[tid + 256 * k2] = cm;
                } else {
                    int_accumulate<DET>(acc[k2], cmp[k2], pw);
                }
            }
        }
        // ---- end of the unit ----
        if (CMP_LDS) {
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) cmp[k2] = lds_cmp[tid + 256 * k2];
        }
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
                const v2f s = {acc[k2], CMP_LDS ? cmp[k2] : 0.0f};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, s), w, voff_in, (k2 ^ xor_k2) * 2048, 0);
            }
        }
        if (!more) break;
        u = u_next;
    }
}

}  // namespace sdrk

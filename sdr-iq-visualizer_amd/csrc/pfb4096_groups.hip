// pfb4096_groups.hip — the polyphase filter bank spectrometer at N = 4096 in one kernel: the T-tap fold of pfb4096.hip in the
// transform's registers, fft4096.hip's transform, and the reduction over K consecutive folded frames of fft4096_integrate.hip
// (mean with compensation, maximum or minimum of |Y|^2 per bin) — ONE row per group out, 4/K bytes written per sample where
// pfb4096_kernel writes 4.  The row is, bit for bit, what fft4096_integrate_kernel returns for the packed folded frames.
//
// Outer structure: fft4096_integrate_kernel's — persistent grid of F4K_WAVES workgroups per CU, whole units
// (integrate_split.h) grid-stride, carry-in / carry-out / partials rows, int_init / int_accumulate / int_reduced / int_epilogue.
// Per-frame input: pfb4096_kernel's — F4kInPfb, pfb_mul / pfb_mac, one tap block in flight beside the accumulators: the next
// tap's, the next frame's first, or across a unit boundary the next unit's first.  The K frames of a unit run back to back on
// one workgroup, so at hop = N a frame's first T - 1 blocks are the ones its predecessor just read.
//
// Registers: a tap block in flight (32 + 16) beside the transform's 32 + 32 and the accumulators does not fit the 168 VGPRs of
// three workgroups per CU.  So (1) the mean keeps its 16 compensation terms in LDS, in the 16 KiB where the windowed kernels keep
// the window (a PFB plan has none): 53376 bytes, the figure those kernels run three workgroups per CU at.  A thread touches
// only its own 16 words, once per frame, so they need no barrier.  Maximum and minimum have no compensation and stay at 36992
// bytes.  (2) Of the next frame's first tap only the samples are in flight during the transform; its 16 coefficients — the same
// 16 KiB of h for every frame — are issued right behind the transform, under the accumulation.
// The accumulation order per bin is frame-ascending whatever holds the state.
#include "fft4096_core.h"
#include "kernels_integrate.h"
#include "kernels_pfb.h"
#include "pfb4096_in.h"

namespace sdrk {

template <int DET>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void pfb4096_groups_kernel(
    const float2* __restrict__ iq, size_t frame_stride, IntUnits c, float* __restrict__ out, float2* __restrict__ partials,
    const float2* __restrict__ carry_in, float2* __restrict__ carry_out, const float* __restrict__ h, int taps,
    const float2* __restrict__ tw4096, int shift) {
    typedef F4kInPfb In;
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

    In::word nxt[16];
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
                    w[j] = In::widen(nxt[j]);
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

hipError_t launch_pfb4096_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != F4K_N || a.d_window || !a.d_pfb_h || a.pfb_taps < 1 || a.pfb_taps > PFB_MAX_TAPS) return hipErrorInvalidValue;
    IntUnits c;
    const IntSplit sp{a.slices, a.slice_len};
    c.f0 = a.f0;
    c.f1 = a.f1;
    c.k = a.k;
    c.slice_len = a.slice_len;
    c.slices = (unsigned)a.slices;
    c.u_first = integrate_unit_of(a.f0, a.k, sp);
    c.u_last = integrate_unit_of(a.f1 - 1, a.k, sp);
    c.out_row0 = a.out_row0;
    c.out_form = a.out_form;
    c.scale = a.scale;
    c.eps = a.eps;
    c.inv_k = 1.0f / (float)a.k;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(D)                                                                                                   \
    hipLaunchKernelGGL((pfb4096_groups_kernel<D>), g, b, 0, a.stream, iq, a.in_stride, c, a.d_out, a.d_partials, a.d_carry_in, \
                       a.d_carry_out, a.d_pfb_h, a.pfb_taps, tw, a.shift)
    if (a.detector == INT_DET_MEAN) SDRK_LAUNCH(INT_DET_MEAN);
    else if (a.detector == INT_DET_MAX) SDRK_LAUNCH(INT_DET_MAX);
    else SDRK_LAUNCH(INT_DET_MIN);
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

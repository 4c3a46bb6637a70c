// rspec4096_groups.hip — integrated one-sided spectra of real-sampled frames of L = 8192: rspec4096_kernel's frame (pair read,
// pair window, f4k_transform, the mirrored exchange and the split butterfly: rspec4096.hip) inside fft4096_integrate_kernel's
// loop (whole units of integrate_split.h, a one-frame prefetch across unit boundaries, carry in, and at the end of a unit the
// row, the partial row or the carry row: fft4096_integrate.hip).  Per bin X[0 ... 4096] the mean (Kahan), the maximum or the
// minimum over the K frames of a group of fmaf(re, re, im*im), and ONE row of 4097 float32 per group: 4 / 2 / 1 bytes in and
// 4 / K out per real sample where the per-frame call writes about 2.
//
// The expressions up to (re, im) are rspec4096_kernel's, statement for statement: under -ffp-contract=on that is what makes
// the power of a frame the power of that kernel's complex row, and a K = 1 dB row that kernel's dB row, bit for bit.
//
// State.  A thread owns bins tid + 256 k2; per bin one float of state lives in a plane of LDS, 16 KiB, [k2][tid], as in
// pfb4096_groups_kernel — each thread reads and writes only its own words, no barrier is involved.  MEAN keeps the 16 Kahan
// sums in registers and the 16 compensation terms in the plane (both in registers was not tried: the per-frame kernel alone
// needs up to 164 of the 168 VGPRs).  MAX / MIN keep their 16 running values in the plane: in registers the float32 forms
// compiled to 168 VGPRs and 20 ... 28 bytes of scratch (the int16 and byte forms to 162 ... 164 without), from the plane every
// form to 107 ... 123 with none.  Bin 4096 belongs to lane 0; its {accumulator, compensation} are one more float2 of LDS
// behind everything else.  LDS is 36,992 + 16,384 + 8 = 53,384 B in every form: three workgroups per CU (54,613 B each).
//
// The pair window goes through a buffer descriptor (one lane offset; the element's position in the immediate and a scalar
// offset): as plain global loads its 16 addresses are loop invariants that the compiler keeps in VGPRs across the transform,
// which cost the windowed forms 60 ... 124 bytes of scratch.
//
// Rows, partial rows and carry rows have 4097 elements and start wherever that puts them: dword stores for the float32 rows,
// dwordx2 accesses for the float2 state rows (which stay 8-byte aligned: 4097 * 8), all through buffer descriptors of the
// row's own length.  Real-input rows are never shifted.
//
// This file is built into the companion library (libsdrk_ext.so; see the Makefile): it uses inline helpers only.
#include "kernels_integrate.h"
#include "rspec4096_in.h"

namespace sdrk {

constexpr int RG_BINS = F4K_N + 1;

template <int RFMT, bool HAS_WINDOW, int DET>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void rspec4096_groups_kernel(
    const void* __restrict__ x_raw, unsigned conv_mask, float conv_off, size_t frame_stride, IntUnits c, float* __restrict__ out,
    float2* __restrict__ partials, const float2* __restrict__ carry_in, float2* __restrict__ carry_out,
    const float2* __restrict__ window, const float2* __restrict__ tw4096, const float2* __restrict__ rtab) {
    typedef typename RspecIn<RFMT>::In In;
    constexpr bool CMP_LDS = DET == INT_DET_MEAN;   // the plane holds the compensation (MEAN) or the running value (MAX / MIN)
    __shared__ __attribute__((aligned(16))) float2 lds[f4k_lds_elems(true) + 1];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_st = reinterpret_cast<float*>(tw1 + 256);   // [k2][tid]: the state plane
    float2* __restrict__ nyq = lds + f4k_lds_elems(true);             // bin 4096's {acc, cmp}: lane 0 alone touches it

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    const float2 t1 = rtab[tid];   // exp(-i pi tid / 4096)
    __syncthreads();

    const Iq8Conv conv = {conv_mask, conv_off};
    const int voff_in = tid * 8;
    const int mirror = F4K_N - tid;   // bin tid + 256 k2 reads index (mirror - 256 k2) & 4095
    const typename In::sample* __restrict__ x = static_cast<const typename In::sample*>(x_raw);

    auto issue = [&](typename In::word (&w)[16], size_t fr) { In::issue(w, x + (fr - c.f0) * frame_stride, tid); };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    typename In::word nxt[16];
    issue(nxt, int_unit(c, u).fb);
    for (;;) {
        // (as in pfb4096_groups_body: keeps the uniform 64-bit operands of the unit bookkeeping out of VGPRs across the frame loop)
        asm volatile("" : "+s"(c.f0), "+s"(c.f1), "+s"(c.k), "+s"(c.slice_len), "+s"(c.u_last));
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        float acc[16], cmp[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) int_init<DET>(acc[k2], cmp[k2]);
        float2 top;   // lane 0: bin 4096
        int_init<DET>(top.x, top.y);
        if (!starts) {
            __amdgpu_buffer_rsrc_t r = frame_rsrc(carry_in, RG_BINS * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff_in, k2 * 2048, 0));
                acc[k2] = s.x;
                if (CMP_LDS) cmp[k2] = s.y;   // (MAX / MIN: 0, and written back as 0)
            }
            if (tid == 0) {
                const v2f s = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, 0, F4K_N * 8, 0));
                top = make_float2(s.x, CMP_LDS ? s.y : 0.0f);
            }
        }
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) lds_st[tid + 256 * k2] = CMP_LDS ? cmp[k2] : acc[k2];
        if (tid == 0) *nyq = top;
        const size_t u_next = u + gridDim.x;
        const bool more = u_next <= c.u_last;
        const size_t n_fb = more ? int_unit(c, u_next).fb : fb;
        size_t f = fb;
        for (size_t left = fe - fb; left != 0; --left, ++f) {   // (counted down: equality tests stay on the scalar unit)
            const size_t f_next = left != 1 ? f + 1 : n_fb;   // the last unit's last frame: a harmless re-read of its first
            float2 win[16];
            if (HAS_WINDOW) {
                const __amdgpu_buffer_rsrc_t wr = frame_rsrc(window, F4K_N * 8);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const v2f t = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(wr, voff_in + (j & 1) * 2048, (j >> 1) * 4096, 0));
                    win[j] = make_float2(t.x, t.y);
                }
            }
            In::to_owners(nxt, lds, tid);
            cf v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                v[j] = RspecIn<RFMT>::widen(nxt[j], conv);
                if (HAS_WINDOW) v[j] = cf{v[j].x * win[j].x, v[j].y * win[j].y};
            }
            // (the windowed products end here, as in rspec4096_kernel)
            if (HAS_WINDOW) __builtin_amdgcn_sched_barrier(0);
            issue(nxt, f_next);
            f4k_transform<false>(v, lds, tw256, tw1, A, tid);
            __syncthreads();   // the transform's pass-3 reads of the exchange buffer are done
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) lds[tid + 256 * k2] = make_float2(v[rev16(k2)].x, v[rev16(k2)].y);
            __syncthreads();
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
                const float pw = fmaf(re, re, im * im);
                if (CMP_LDS) {
                    float cm = lds_st[tid + 256 * k2];
                    int_accumulate<DET>(acc[k2], cm, pw);
                    lds_st[tid + 256 * k2] = cm;
                } else {
                    float a = lds_st[tid + 256 * k2], z0 = 0.0f;
                    int_accumulate<DET>(a, z0, pw);
                    lds_st[tid + 256 * k2] = a;
                }
            }
            if (tid == 0) {   // X[4096] = (Re Z[0] - Im Z[0], +0); v[rev16(0)] = Z[0]
                const float re = v[0].x - v[0].y, im = 0.0f;
                float2 s = *nyq;
                int_accumulate<DET>(s.x, s.y, fmaf(re, re, im * im));
                *nyq = s;
            }
        }
        // ---- end of the unit ----
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) (CMP_LDS ? cmp[k2] : acc[k2]) = lds_st[tid + 256 * k2];
        if (tid == 0) top = *nyq;
        if (ends && c.slices == 1) {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (g - c.out_row0) * (size_t)RG_BINS, RG_BINS * 4);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const float r = int_reduced<DET>(acc[k2], cmp[k2], c.inv_k);
                const float o = int_epilogue(r, c.out_form, c.scale, c.eps);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, tid * 4, k2 * 1024, F4K_NT);
            }
            if (tid == 0) {
                const float o = int_epilogue(int_reduced<DET>(top.x, top.y, c.inv_k), c.out_form, c.scale, c.eps);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, 0, F4K_N * 4, F4K_NT);
            }
        } else {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(ends ? partials + u * (size_t)RG_BINS : carry_out, RG_BINS * 8);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v2f s = {acc[k2], CMP_LDS ? cmp[k2] : 0.0f};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, s), w, voff_in, k2 * 2048, 0);
            }
            if (tid == 0) {
                const v2f s = {top.x, CMP_LDS ? top.y : 0.0f};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, s), w, 0, F4K_N * 8, 0);
            }
        }
        if (!more) break;
        u = u_next;
    }
}

hipError_t launch_rspec4096_groups(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (a.nfft != RG_BINS || !a.d_real_tab) return hipErrorInvalidValue;
    const IntUnits c = int_units(a);
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const float2* win = reinterpret_cast<const float2*>(a.d_real_window);
    const Iq8Conv conv = iq8_conv(a.real_fmt == REAL_U8 ? IQ8_UNSIGNED : IQ8_SIGNED);
#define SDRK_LAUNCH(R, W, D)                                                                                               \
    hipLaunchKernelGGL((rspec4096_groups_kernel<R, W, D>), g, b, 0, a.stream, a.d_in, conv.mask, conv.off, a.in_stride, c,  \
                       a.d_out, a.d_partials, a.d_carry_in, a.d_carry_out, win, tw, a.d_real_tab)
#define SDRK_LAUNCH_D(R, W)                                            \
    do {                                                               \
        if (a.detector == INT_DET_MEAN) SDRK_LAUNCH(R, W, INT_DET_MEAN); \
        else if (a.detector == INT_DET_MAX) SDRK_LAUNCH(R, W, INT_DET_MAX); \
        else SDRK_LAUNCH(R, W, INT_DET_MIN);                           \
    } while (0)
#define SDRK_LAUNCH_W(R)                                               \
    do {                                                               \
        if (win) SDRK_LAUNCH_D(R, true); else SDRK_LAUNCH_D(R, false); \
    } while (0)
    if (a.real_fmt == REAL_F32) SDRK_LAUNCH_W(0);
    else if (a.real_fmt == REAL_S16) SDRK_LAUNCH_W(1);
    else SDRK_LAUNCH_W(2);
#undef SDRK_LAUNCH_W
#undef SDRK_LAUNCH_D
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

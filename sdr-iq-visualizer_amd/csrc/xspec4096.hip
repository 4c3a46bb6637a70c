// xspec4096.hip — two-channel cross-spectra at N = 4096: the flagship transform (fft4096.hip: window * x -> 4096-point FFT ->
// fftshift) run on BOTH channels of a frame of interleaved elements (I0 Q0 I1 Q1), with the four running sums of kernels_xspec.h
// in its registers.  Per bin and group of K frames Saa = sum |A|^2, Sbb = sum |B|^2, Sre + i Sim = sum A conj(B), and FOUR rows per
// group out, scale * S / K each — 16 + 16/K bytes per element through HBM from complex64, 8 + 16/K from int16, where pulling both
// complex spectra of every frame back for numpy moves 32.
//
// The streaming skeleton of sk4096.hip, written once over the input policy: persistent grid, buffer loads, window from LDS,
// f4k_windowed_transform, units (integrate_split.h), carry and partial rows, non-temporal row stores.  One 16-byte (int16: 8-byte)
// load per lane and element serves both channels.  Per frame: channel 0's samples are widened into the working set and channel
// 1's halves of the words are held back; the NEXT frame's 16 loads per thread are issued (they stay in flight across both
// transforms, and across unit boundaries too); channel 0 is transformed and its 16 bins kept; channel 1 goes through the same
// exchange LDS (f4k_transform's first barrier separates the two); then the four sums take the 16 bins.
//
// Registers: 64 of state, 64 (int16: 32) of words in flight, 32 (int16: 16) of held halves or 32 of held spectrum, 32 of working
// set plus the transform's temporaries: above the 168 of three workgroups per CU.  The kernel is built for TWO workgroups per CU
// (at most 256 VGPRs, 80 KiB of LDS each; it takes 53 KiB with the window) and keeps everything in registers; DESIGN.md 4.19
// has the compiler's figures and the measurement.
// A workgroup takes whole units grid-stride; at the end of a unit it writes, once,
//   - the group's four rows (nt stores) when the unit is a whole group,
//   - the unit's four sums into the partials (a group split into slices: xspec_rows.hip finalizes), or
//   - the state into the carry row when the launch ends inside the unit (chunked calls); the next launch picks it up.
// The int16 policy gives x = float32(I) + i float32(Q) exactly and then the same arithmetic in the same order: rows, partial
// rows and carry rows have the bits of the complex64 instantiation on the widened elements.
#include "fft4096_in_ci16.h"
#include "kernels_xspec.h"

namespace sdrk {

constexpr int XS_WG_PER_CU = 2;

// Input policies: word = one element as loaded, half = channel 1's part of it, held back while channel 0 is transformed.
// (the 16 loads with each offset split into j % 4 quarters in the vector offset and j / 4 in the scalar one, as
// F4kInCi16::issue_few_sgprs does: the unit bookkeeping and the four planes' store offsets leave the scalar file little to spare)
struct XsInC64 {
    typedef v4u word;
    typedef v2u half;
    static constexpr int ELEM = 16;
    static __device__ __forceinline__ void load(word (&x)[16], const char* frame, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * ELEM);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            x[j] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, tid * ELEM + (j & 3) * 256 * ELEM,
                                                                                 (j >> 2) * 1024 * ELEM, F4K_NT));
    }
    static __device__ __forceinline__ cf first(word w) { return __builtin_bit_cast(v2f, v2u{w.x, w.y}); }
    static __device__ __forceinline__ half second(word w) { return v2u{w.z, w.w}; }
    static __device__ __forceinline__ cf widen(half h) { return __builtin_bit_cast(v2f, h); }
};
struct XsInI16 {
    typedef v2u word;
    typedef unsigned half;
    static constexpr int ELEM = 8;
    static __device__ __forceinline__ void load(word (&x)[16], const char* frame, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(frame, F4K_N * ELEM);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            x[j] = __builtin_amdgcn_raw_buffer_load_b64(r, tid * ELEM + (j & 3) * 256 * ELEM, (j >> 2) * 1024 * ELEM, F4K_NT);
    }
    static __device__ __forceinline__ cf first(word w) { return widen(w.x); }
    static __device__ __forceinline__ half second(word w) { return w.y; }
    static __device__ __forceinline__ cf widen(half h) {
        float re, im;
        ci16_unpack(h, re, im);
        return cf{re, im};
    }
};

template <class In, bool HAS_WINDOW>
__global__ __launch_bounds__(F4K_THREADS, XS_WG_PER_CU) void xspec4096_kernel(
    const char* __restrict__ iq, size_t frame_stride, IntUnits c, float* __restrict__ out, float* __restrict__ partials,
    const float* __restrict__ carry_in, float* __restrict__ carry_out, const float* __restrict__ window,
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
    const int voff_st = tid * 16;       // state rows: one float4 per bin

    auto issue = [&](typename In::word (&x)[16], size_t fr) { In::load(x, iq + (fr - c.f0) * frame_stride * In::ELEM, tid); };

    size_t u = c.u_first + blockIdx.x;   // (the launcher starts no more workgroups than there are units)
    typename In::word nxt[16];
    issue(nxt, int_unit(c, u).fb);
    for (;;) {
        // (the unit bookkeeping is wave-uniform and lives in SGPRs; of the next unit only its first frame is kept)
        const IntUnit cur = int_unit(c, u);
        const size_t g = cur.g, fb = cur.fb, fe = cur.fe;
        const bool starts = cur.starts, ends = cur.ends;
        XsState st[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) st[k2] = XsState{0.0f, 0.0f, 0.0f, 0.0f};
        if (!starts) {
            __amdgpu_buffer_rsrc_t r = frame_rsrc(carry_in, F4K_N * 16);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v4f s = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, voff_st, (k2 ^ xor_k2) * 4096, 0));
                st[k2] = XsState{s.x, s.y, s.z, s.w};
            }
        }
        const size_t u_next = u + gridDim.x;
        const bool more = u_next <= c.u_last;
        const size_t n_fb = more ? int_unit(c, u_next).fb : fb;
        for (size_t f = fb; f < fe; ++f) {
            cf v[16];
            typename In::half held[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                v[j] = In::first(nxt[j]);
                held[j] = In::second(nxt[j]);
            }
            issue(nxt, f + 1 < fe ? f + 1 : n_fb);   // the last unit's last frame: a harmless re-read of its first
            f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
            cf a[16];
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) a[k2] = v[rev16(k2)];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = In::widen(held[j]);
            f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const cf b = v[rev16(k2)];
                xs_accumulate(st[k2], a[k2].x, a[k2].y, b.x, b.y);
            }
        }
        // ---- end of the unit ----
        if (ends && c.slices == 1) {   // planes 0..3 one behind the other from the group's first float: one descriptor, 64 KiB
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (g - c.out_row0) * (size_t)(4 * F4K_N), 4 * F4K_N * 4);
#pragma unroll
            for (int pl = 0; pl < 4; ++pl) {
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2) {
                    const float sum = pl == 0 ? st[k2].aa : pl == 1 ? st[k2].bb : pl == 2 ? st[k2].re : st[k2].im;
                    const float o = xs_output(sum, c.inv_k, c.scale);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), w, tid * 4,
                                                          pl * F4K_N * 4 + (k2 ^ xor_k2) * 1024, F4K_NT);
                }
            }
        } else {
            __amdgpu_buffer_rsrc_t w = frame_rsrc(ends ? partials + u * (size_t)(4 * F4K_N) : carry_out, F4K_N * 16);
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const v4f s = {st[k2].aa, st[k2].bb, st[k2].re, st[k2].im};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, s), w, voff_st, (k2 ^ xor_k2) * 4096, 0);
            }
        }
        if (!more) break;
        u = u_next;
    }
}

template <class In>
static hipError_t launch_xspec4096_of(const IntegrateArgs& a) {
    if (a.f1 <= a.f0) return hipSuccess;
    IntUnits c = int_units(a);   // power planes, whatever the call's out_form says
    c.out_form = INT_OUT_POWER;
    c.eps = 0.0f;
    dim3 g(f4k_grid(a.num_cus, XS_WG_PER_CU, c.u_last - c.u_first + 1)), b(F4K_THREADS);
    const char* iq = static_cast<const char*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    float* partials = reinterpret_cast<float*>(a.d_partials);
    const float* carry_in = reinterpret_cast<const float*>(a.d_carry_in);
    float* carry_out = reinterpret_cast<float*>(a.d_carry_out);
    if (a.d_window)
        hipLaunchKernelGGL((xspec4096_kernel<In, true>), g, b, 0, a.stream, iq, a.in_stride, c, a.d_out, partials, carry_in,
                           carry_out, a.d_window, tw, a.shift);
    else
        hipLaunchKernelGGL((xspec4096_kernel<In, false>), g, b, 0, a.stream, iq, a.in_stride, c, a.d_out, partials, carry_in,
                           carry_out, a.d_window, tw, a.shift);
    return hipGetLastError();
}

hipError_t launch_xspec4096(const IntegrateArgs& a) { return launch_xspec4096_of<XsInC64>(a); }
hipError_t launch_xspec4096_i16(const IntegrateArgs& a) { return launch_xspec4096_of<XsInI16>(a); }

}  // namespace sdrk

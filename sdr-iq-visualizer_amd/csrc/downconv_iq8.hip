// downconv_iq8.hip — the down-converter of ddc4096.hip reading interleaved 8-bit I,Q (SigMF ci8 / cu8, 2 bytes per sample): the
// single call with the mixer on and off, and the bank.  Kernels of their own, written out on the skeleton of that file's two, so
// that its code objects stay what they are: persistent grid, grid-stride blocks, the NEXT block's 16 loads per thread in flight
// across both transforms, H_s in registers (single call) or loaded one channel ahead (bank), the keeping and the mixer of
// kernels_ddc.h unchanged.  What is new is the input:
//   loads     one 16-bit buffer load per sample, sample tid + 256 j (as F4kInCi8::issue), through a descriptor clipped to the
//             samples that exist; one register per sample, as for int16;
//   widening  ci8_unpack with the call's Iq8Conv as a run-time argument: a format adds no instantiation (three in all);
//   padding   a load at or past the descriptor's end returns 0, and byte 0 is -127.5 for unsigned input.  No kept output depends on
//             those positions mathematically, but every output of the block does through rounding, and the complex64 call pads
//             with +0.0.  So a block with fewer than a whole transform of samples left — a wave-uniform branch, not taken by any
//             other block — sets the positions at or past the end to +0.0 + 0.0i after widening (both formats alike).
// The structs that travel in the kernels' arguments are this file's own (their names are part of the kernels' names).
#include "fft4096_in_ci8.h"
#include "kernels_ddc.h"

namespace sdrk {

// Workgroups per CU, those of the int16 forms of ddc4096.hip: what the compiler fits without scratch and without a spilled VGPR
// (DESIGN.md 4.25 has the figures).
constexpr int DOWNCONV_IQ8_WG_PER_CU = 3, DOWNCONVBANK_IQ8_WG_PER_CU = 2;

struct DownconvGeom {
    size_t n_in, n_out, n_blocks, out_stride;
    int taps, L, n_chan;
    unsigned decim, recip;      // D, ceil(2^24 / D)
    unsigned r0;                // index0 % D
    unsigned step_q, step_r;    // (gridDim.x L) / D, (gridDim.x L) % D
    unsigned index_lo;          // (uint32) index0
};
// the keep bookkeeping multiplies the grid by L in 32 bits (kernels_ddc.h); a grid is a few hundred workgroups
constexpr unsigned DOWNCONV_MAX_GRID = 1u << 19;
struct DownconvWords {
    uint32_t w[DDC_MAX_CHAN];
};

// Input policy, byte pairs: x[j] = sample tid + 256 j of the block, zero-extended into its register.
struct DownconvInIq8 {
    typedef unsigned word;
    static constexpr int ELEM = 2;
    static __device__ __forceinline__ void load(word (&x)[16], const char* blk, unsigned bytes, int tid) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(blk, bytes);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = __builtin_amdgcn_raw_buffer_load_b16(r, tid * ELEM, j * 256 * ELEM, F4K_NT);
    }
    // the block's 16 samples of this thread, of which the first `left` positions of the block exist
    static __device__ __forceinline__ void widen(cf (&v)[16], const word (&x)[16], Iq8Conv conv, size_t left, int tid) {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = F4kInCi8::widen(x[j], conv);
        if (left < (size_t)F4K_N) {   // wave-uniform: the last block of a call only
            const unsigned have = (unsigned)left;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((unsigned)(tid + 256 * j) >= have) v[j] = cf{0.0f, 0.0f};
        }
    }
};

template <bool MIX>
__global__ __launch_bounds__(F4K_THREADS, DOWNCONV_IQ8_WG_PER_CU) void downconv_iq8_kernel(
    const char* __restrict__ in, DownconvGeom g, Iq8Conv conv, uint32_t freq_word, float2* __restrict__ out,
    const float2* __restrict__ H, const float2* __restrict__ tw4096) {
    typedef DownconvInIq8 In;
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    OlsC h[16];   // H_s[tid + 256 k2]
    {
        const int s = (int)ddc_bin(freq_word);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const float2 t = H[ols_h_index(tid + 256 * k2, s)];
            h[k2] = OlsC{t.x, t.y};
        }
    }
    const int rel0 = tid - (g.taps - 1);   // position p = tid + 256 k2 is output b L + rel0 + 256 k2

    size_t b = blockIdx.x;
    const size_t step = gridDim.x;
    if (b >= g.n_blocks) return;   // (the launcher starts no workgroup without a block)
    DdcKeep keep = ddc_keep_first(g.r0, blockIdx.x, (unsigned)g.L, g.decim);

    auto issue = [&](In::word (&x)[16], size_t blk) {
        const size_t s0 = blk * (size_t)g.L, left = g.n_in - s0;
        In::load(x, in + s0 * In::ELEM, (unsigned)(left < (size_t)F4K_N ? left : (size_t)F4K_N) * In::ELEM, tid);
    };

    In::word nxt[16];
    issue(nxt, b);
    for (;;) {
        cf v[16];
        In::widen(v, nxt, conv, g.n_in - b * (size_t)g.L, tid);
        const size_t b_next = b + step;
        const bool more = b_next < g.n_blocks;
        issue(nxt, more ? b_next : b);   // the last block: a re-read of itself that nothing uses
        f4k_transform(v, lds, tw256, tw1, A, tid);
        cf u[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {   // bin tid + 256 j, the second transform's input j
            const cf X = v[rev16(j)];
            const OlsC z = ols_filter(OlsC{X.x, X.y}, h[j]);
            u[j] = cf{z.x, z.y};
        }
        f4k_transform(u, lds, tw256, tw1, A, tid);
        {
            const unsigned qmin = keep.rem != 0;                       // (rem_b + rel) / D of the block's first kept output
            const size_t o0 = ddc_keep_base(keep, g.r0), left = o0 < g.n_out ? g.n_out - o0 : 0;   // its output sample
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + o0, (unsigned)(left < (size_t)g.L ? left : (size_t)g.L) * 8);
            const unsigned idx0 = g.index_lo + (unsigned)(b * (size_t)g.L);   // (uint32)(index0 + b L)
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const int rel = rel0 + 256 * k2;
                const unsigned n = keep.rem + (unsigned)rel, q = ddc_div(n, g.recip);
                if ((unsigned)rel < (unsigned)g.L && n == q * g.decim) {
                    const cf y = u[rev16(k2)];
                    OlsC o = ols_unscale(OlsC{y.x, y.y});
                    if (MIX) {
                        const uint32_t phase = ddc_phase(freq_word, idx0 + (unsigned)rel);
                        const float2 t = tw4096[ddc_table_index(phase)];
                        o = ddc_mix(o, OlsC{t.x, t.y}, phase);
                    }
                    const v2f ov = {o.x, o.y};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, ov), w, (q - qmin) * 8, 0, 0);
                }
            }
        }
        if (!more) break;
        b = b_next;
        ddc_keep_next(keep, g.step_q, g.step_r, g.decim);
    }
}

__global__ __launch_bounds__(F4K_THREADS, DOWNCONVBANK_IQ8_WG_PER_CU) void downconvbank_iq8_kernel(
    const char* __restrict__ in, DownconvGeom g, Iq8Conv conv, DownconvWords fw, float2* __restrict__ out,
    const float2* __restrict__ H, const float2* __restrict__ tw4096) {
    typedef DownconvInIq8 In;
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    const int rel0 = tid - (g.taps - 1);   // position p = tid + 256 k2 is output b L + rel0 + 256 k2

    size_t b = blockIdx.x;
    const size_t step = gridDim.x;
    if (b >= g.n_blocks) return;   // (the launcher starts no workgroup without a block)
    DdcKeep keep = ddc_keep_first(g.r0, blockIdx.x, (unsigned)g.L, g.decim);

    auto issue = [&](In::word (&x)[16], size_t blk) {
        const size_t s0 = blk * (size_t)g.L, left = g.n_in - s0;
        In::load(x, in + s0 * In::ELEM, (unsigned)(left < (size_t)F4K_N ? left : (size_t)F4K_N) * In::ELEM, tid);
    };
    auto issue_h = [&](float2 (&h)[16], uint32_t word) {   // H_s[tid + 256 k2]
        const int s = (int)ddc_bin(word);
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) h[k2] = H[ols_h_index(tid + 256 * k2, s)];
    };

    float2 h_next[16];
    issue_h(h_next, fw.w[0]);
    In::word nxt[16];
    issue(nxt, b);
    for (;;) {
        cf v[16];
        In::widen(v, nxt, conv, g.n_in - b * (size_t)g.L, tid);
        const size_t b_next = b + step;
        const bool more = b_next < g.n_blocks;
        issue(nxt, more ? b_next : b);   // the last block: a re-read of itself that nothing uses
        f4k_transform(v, lds, tw256, tw1, A, tid);   // X[tid + 256 j] = v[rev16(j)], kept for every channel
        const unsigned qmin = keep.rem != 0;
        const size_t o0 = ddc_keep_base(keep, g.r0), left = o0 < g.n_out ? g.n_out - o0 : 0;
        const unsigned out_bytes = (unsigned)(left < (size_t)g.L ? left : (size_t)g.L) * 8;
        const unsigned idx0 = g.index_lo + (unsigned)(b * (size_t)g.L);
        for (int c = 0; c < g.n_chan; ++c) {
            const uint32_t word = fw.w[c];
            cf u[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {   // bin tid + 256 j, the second transform's input j
                const cf X = v[rev16(j)];
                const OlsC z = ols_filter(OlsC{X.x, X.y}, OlsC{h_next[j].x, h_next[j].y});
                u[j] = cf{z.x, z.y};
            }
            issue_h(h_next, fw.w[c + 1 < g.n_chan ? c + 1 : 0]);   // one channel ahead (after the last: the next block's first)
            f4k_transform(u, lds, tw256, tw1, A, tid);
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (size_t)c * g.out_stride + o0, out_bytes);
            float2 t[16];
            if (word) {   // all 16 factors on their way at once, kept or not (the index is below the table's length): one wait
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2)
                    t[k2] = tw4096[ddc_table_index(ddc_phase(word, idx0 + (unsigned)(rel0 + 256 * k2)))];
            }
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const int rel = rel0 + 256 * k2;
                const unsigned n = keep.rem + (unsigned)rel, q = ddc_div(n, g.recip);
                if ((unsigned)rel < (unsigned)g.L && n == q * g.decim) {
                    const cf y = u[rev16(k2)];
                    OlsC o = ols_unscale(OlsC{y.x, y.y});
                    if (word) o = ddc_mix(o, OlsC{t[k2].x, t[k2].y}, ddc_phase(word, idx0 + (unsigned)rel));
                    const v2f ov = {o.x, o.y};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, ov), w, (q - qmin) * 8, 0, 0);
                }
            }
        }
        if (!more) break;
        b = b_next;
        ddc_keep_next(keep, g.step_q, g.step_r, g.decim);
    }
}

static DownconvGeom downconv_geom(const DdcArgs& a, unsigned grid) {
    DownconvGeom g;
    g.n_in = a.n_in;
    g.n_out = ddc_launch_outputs(a);
    g.n_blocks = ddc_launch_blocks(a);
    g.out_stride = a.out_stride;
    g.taps = a.taps;
    g.L = ols_block_len(a.taps);
    g.n_chan = a.n_chan;
    g.decim = (unsigned)a.decim;
    g.recip = ddc_recip(g.decim);
    g.r0 = (unsigned)(a.index0 % g.decim);
    const unsigned stride = grid * (unsigned)g.L;   // grid <= DOWNCONV_MAX_GRID: below 2^31
    g.step_q = stride / g.decim;
    g.step_r = stride % g.decim;
    g.index_lo = (unsigned)a.index0;
    return g;
}

static bool iq8_fmt_ok(int fmt) { return fmt == IQ8_SIGNED || fmt == IQ8_UNSIGNED; }

hipError_t launch_downconv_iq8(const DdcArgs& a, int fmt) {
    if (!ddc_args_ok(a, false) || !iq8_fmt_ok(fmt)) return hipErrorInvalidValue;
    const uint32_t word = a.freq_word[0];
    const unsigned grid = f4k_grid(a.num_cus, DOWNCONV_IQ8_WG_PER_CU, ddc_launch_blocks(a));
    if (grid > DOWNCONV_MAX_GRID) return hipErrorInvalidValue;
    const DownconvGeom g = downconv_geom(a, grid);
    const char* in = static_cast<const char*>(a.d_in);
    const Iq8Conv conv = iq8_conv(fmt);
    if (word)
        hipLaunchKernelGGL((downconv_iq8_kernel<true>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, conv, word, a.d_out, a.d_h, a.d_twiddle);
    else
        hipLaunchKernelGGL((downconv_iq8_kernel<false>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, conv, word, a.d_out, a.d_h, a.d_twiddle);
    return hipGetLastError();
}

hipError_t launch_downconvbank_iq8(const DdcArgs& a, int fmt) {
    if (!ddc_args_ok(a, true) || !iq8_fmt_ok(fmt)) return hipErrorInvalidValue;
    const unsigned grid = f4k_grid(a.num_cus, DOWNCONVBANK_IQ8_WG_PER_CU, ddc_launch_blocks(a));
    if (grid > DOWNCONV_MAX_GRID) return hipErrorInvalidValue;
    const DownconvGeom g = downconv_geom(a, grid);
    DownconvWords fw;
    for (int c = 0; c < DDC_MAX_CHAN; ++c) fw.w[c] = c < a.n_chan ? a.freq_word[c] : 0;
    hipLaunchKernelGGL(downconvbank_iq8_kernel, dim3(grid), dim3(F4K_THREADS), 0, a.stream, static_cast<const char*>(a.d_in), g,
                       iq8_conv(fmt), fw, a.d_out, a.d_h, a.d_twiddle);
    return hipGetLastError();
}

}  // namespace sdrk

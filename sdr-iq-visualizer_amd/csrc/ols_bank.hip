// ols_bank.hip — channel bank: C tuned channels out of ONE pass over the input (kernels_ols_bank.h).  ols4096.hip's kernel with
// its channel-dependent half in a loop: per block the samples are read once and transformed once, the spectrum X[tid + 256 j]
// stays in 16 complex registers, and per channel c only
//     u[j] = ols_filter(X_j, H[ols_h_index(tid + 256 j, s_c)]) -> f4k_transform -> ols_unscale -> ols_mix -> decimated store
// runs: 1 + C transforms per block where C single calls run 2 C, and the input is read once instead of C times.  Every formula
// is kernels_ols.h's, in ols4096_kernel's order, so plane c carries the bits of the single call with (s_c, phase0_c).
//
// The streaming skeleton of ols4096.hip: persistent grid, grid-stride blocks, descriptors clipped to the samples and the outputs
// that exist, the NEXT block's 16 loads per thread in flight across all 1 + C transforms of a block.
// H per channel: 16 cached global loads per thread from the plan's 32 KiB table (coalesced; the table stays in L2 and in the
// vector cache), issued ONE CHANNEL AHEAD — channel c + 1's while channel c is transformed, channel 0's of the next block during
// the last channel — so their latency hides behind a transform.  In LDS the table would take 32 KiB beside the 36,992 B of
// exchange buffer and tables and add a ninth 32 KiB LDS pass to each transform's eight; either way two workgroups fit a CU, and
// this form leaves the LDS pipe alone (profiles/fir_bank/SUMMARY.md).  The mixer's 16 factors are requested together AFTER the
// transform: requested before it they measured 3 - 6 % slower.
// s_c and phase0_c come by value in the kernel's arguments (two arrays of 64 16-bit values, already mod 4096): the call is
// stream-safe and needs no plan-owned table.  They are uniform, so the s_c == 0 test is a scalar branch: such a channel skips
// the mixer as the single call's MIX = false instantiation does (a product with (1, 0) would not keep -0.0, Inf and NaN).
#include "kernels_ols_bank.h"
#include "ols_in.h"

namespace sdrk {

// Workgroups per CU the kernel is built for: X, the product u, H one channel ahead, the next block's samples and the mixer's
// factors are 160 VGPRs before the transform's own — 224 from complex64, 210 from int16 — so two (at most 256 VGPRs) from both
// formats.  (Without the load-ahead of H int16 fits three, 162 VGPRs; complex64 spills there.)
template <class In>
constexpr int chanbank_wg_per_cu() { return 2; }

struct OlsBankGeom {
    size_t n_in, n_out, n_blocks, out_stride;
    int taps, L, log2d, n_chan;
    unsigned short shift_bins[OLS_BANK_MAX_CHAN], phase0[OLS_BANK_MAX_CHAN];   // both mod 4096
};

// Element c of one of the two: through the aligned 32-bit word that holds it, which is a scalar load (there is no 16-bit one, and
// a vector load would leave the uniform value, and the branch on it, to the vector unit).
__device__ __forceinline__ unsigned chanbank_arg(const unsigned short (&a)[OLS_BANK_MAX_CHAN], int c) {
    unsigned w;
    __builtin_memcpy(&w, &a[c & ~1], sizeof w);
    return (w >> (16 * (c & 1))) & 0xFFFFu;
}

template <class In>
__global__ __launch_bounds__(F4K_THREADS, (chanbank_wg_per_cu<In>())) void chanbank_kernel(
    const char* __restrict__ in, OlsBankGeom g, float2* __restrict__ out, const float2* __restrict__ H,
    const float2* __restrict__ tw4096) {
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    const int rel0 = tid - (g.taps - 1);                        // position p = tid + 256 k2 is output b L + rel0 + 256 k2
    const bool lane_kept = (rel0 & ((1 << g.log2d) - 1)) == 0;   // (two's complement: also right for rel0 < 0)
    const unsigned out_per_block = (unsigned)g.L >> g.log2d;

    size_t b = blockIdx.x;
    const size_t step = gridDim.x;
    if (b >= g.n_blocks) return;   // (the launcher starts no workgroup without a block)

    auto issue = [&](typename In::word (&x)[16], size_t blk) {
        const size_t s0 = blk * (size_t)g.L, left = g.n_in - s0;
        In::load(x, in + s0 * In::ELEM, (unsigned)(left < (size_t)F4K_N ? left : (size_t)F4K_N) * In::ELEM, tid);
    };
    auto issue_h = [&](float2 (&h)[16], unsigned s) {   // H_s[tid + 256 k2]
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) h[k2] = H[ols_h_index(tid + 256 * k2, (int)s)];
    };

    float2 h_next[16];
    issue_h(h_next, chanbank_arg(g.shift_bins, 0));
    typename In::word nxt[16];
    issue(nxt, b);
    for (;;) {
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
        const size_t b_next = b + step;
        const bool more = b_next < g.n_blocks;
        issue(nxt, more ? b_next : b);   // the last block: a harmless re-read of itself
        f4k_transform(v, lds, tw256, tw1, A, tid);   // X[tid + 256 j] = v[rev16(j)], kept for every channel
        const size_t o0 = b * (size_t)out_per_block, left = g.n_out - o0;
        const unsigned out_bytes = (unsigned)(left < out_per_block ? left : out_per_block) * 8;
        const size_t i0 = b * (size_t)g.L;
        for (int c = 0; c < g.n_chan; ++c) {
            const unsigned s = chanbank_arg(g.shift_bins, c), phase0 = chanbank_arg(g.phase0, c);
            cf u[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {   // bin tid + 256 j, the second transform's input j
                const cf X = v[rev16(j)];
                const OlsC z = ols_filter(OlsC{X.x, X.y}, OlsC{h_next[j].x, h_next[j].y});
                u[j] = cf{z.x, z.y};
            }
            issue_h(h_next, chanbank_arg(g.shift_bins, c + 1 < g.n_chan ? c + 1 : 0));   // one channel ahead (after the last: the next block's first)
            f4k_transform(u, lds, tw256, tw1, A, tid);
            if (lane_kept) {
                __amdgpu_buffer_rsrc_t w = frame_rsrc(out + (size_t)c * g.out_stride + o0, out_bytes);
                float2 t[16];
                if (s) {   // all 16 factors on their way at once, in range or not (the index is taken mod 4096): one wait
#pragma unroll
                    for (int k2 = 0; k2 < 16; ++k2) t[k2] = tw4096[ols_mix_index(phase0, s, i0 + (size_t)(rel0 + 256 * k2))];
                }
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2) {
                    const int rel = rel0 + 256 * k2;
                    if ((unsigned)rel < (unsigned)g.L) {
                        const cf y = u[rev16(k2)];
                        OlsC o = ols_unscale(OlsC{y.x, y.y});
                        if (s) o = ols_mix(o, OlsC{t[k2].x, t[k2].y});
                        const v2f ov = {o.x, o.y};
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, ov), w, (rel >> g.log2d) * 8, 0, 0);
                    }
                }
            }
        }
        if (!more) break;
        b = b_next;
    }
}

template <class In>
static hipError_t launch_chanbank_of(const OlsBankArgs& a) {
    if (!ols_bank_args_ok(a)) return hipErrorInvalidValue;
    OlsBankGeom g;
    g.n_in = a.n_in;
    g.n_out = ols_bank_outputs(a);
    g.n_blocks = ols_bank_blocks(a);
    g.out_stride = a.out_stride;
    g.taps = a.taps;
    g.L = ols_block_len(a.taps);
    g.log2d = __builtin_ctz((unsigned)a.decim);
    g.n_chan = a.n_chan;
    for (int c = 0; c < OLS_BANK_MAX_CHAN; ++c) {
        g.shift_bins[c] = c < a.n_chan ? (unsigned short)((unsigned)a.shift_bins[c] & (OLS_N - 1)) : 0;
        g.phase0[c] = c < a.n_chan ? (unsigned short)((unsigned)a.phase0[c] & (OLS_N - 1)) : 0;
    }
    const unsigned grid = f4k_grid(a.num_cus, chanbank_wg_per_cu<In>(), g.n_blocks);
    hipLaunchKernelGGL((chanbank_kernel<In>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, static_cast<const char*>(a.d_in), g, a.d_out,
                       a.d_h, a.d_twiddle);
    return hipGetLastError();
}

hipError_t launch_chanbank(const OlsBankArgs& a) { return launch_chanbank_of<OlsInC64>(a); }
hipError_t launch_chanbank_i16(const OlsBankArgs& a) { return launch_chanbank_of<OlsInI16>(a); }

}  // namespace sdrk

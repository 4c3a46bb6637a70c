// ddc4096.hip — digital down-converter: ols4096.hip's and ols_bank.hip's kernels with the epilogue of kernels_ddc.h — tuning by
// a 32-bit frequency word and any integer decimation 1 .. 256.  Kernels of their own, on the same skeleton, so that the FIR and
// channel-bank kernels keep their code objects: the epilogue below needs registers and branches those do not have to carry
// (DESIGN.md 4.23).  Everything up to the second transform is theirs, statement for statement: persistent grid, grid-stride
// blocks, buffer descriptors clipped to the samples and outputs that exist, the NEXT block's 16 loads per thread in flight across
// the transforms, H_s in registers (single call) or loaded one channel ahead (bank), s = ddc_bin(freq_word).
//
// Keeping.  Output i of block b sits at position rel = i - b L in 0 .. L - 1 and is kept iff (index0 + i) % D == 0.  With
// T_b = index0 % D + b L = S_b D + rem_b (rem_b < D), output i is kept iff (rem_b + rel) % D == 0 and is then output sample
// S_b + (rem_b + rel) / D - (index0 % D != 0) of the launch.  S_b and rem_b are wave-uniform and move from a workgroup's block to
// its next one (b + gridDim.x) by the launch's constants (gridDim.x L) / D and (gridDim.x L) % D with one carry: scalar integer
// adds, no division in the loop; the one division per workgroup is 32-bit (blockIdx.x L < 2^22).  Per element n = rem_b + rel
// < 256 + 4096 and n / D = ddc_div(n, ceil(2^24 / D)), one 32-bit multiply.  A lane keeps any subset of its 16 positions; a kept
// element is one 8-byte buffer store through a descriptor that starts at the block's first kept output and ends with the launch's.
// Mixer.  16 phases per thread from one 32-bit multiply each, freq_word * (uint32)(index0 + i); the table read sits where the
// bin mixer's does (single call: per kept element; bank: all 16 requested together after the transform).  freq_word == 0 runs
// no mixer: MIX = false in the single call, a wave-uniform branch per channel in the bank; -0.0, Inf and NaN pass as they are.
#include "kernels_ddc.h"
#include "ols_in.h"

namespace sdrk {

// Workgroups per CU an instantiation is built for: what the compiler fits without scratch and without a spilled VGPR
// (DESIGN.md 4.23 has the figures).
template <class In, bool MIX>
constexpr int ddc_wg_per_cu() { return (MIX && In::ELEM == 8) ? 2 : 3; }
template <class In>
constexpr int ddcbank_wg_per_cu() { return 2; }

struct DdcGeom {
    size_t n_in, n_out, n_blocks, out_stride;
    int taps, L, n_chan;
    unsigned decim, recip;      // D, ceil(2^24 / D)
    unsigned r0;                // index0 % D
    unsigned step_q, step_r;    // (gridDim.x L) / D, (gridDim.x L) % D
    unsigned index_lo;          // (uint32) index0
};
// the keep bookkeeping multiplies the grid by L in 32 bits (kernels_ddc.h); a grid is a few hundred workgroups
constexpr unsigned DDC_MAX_GRID = 1u << 19;
struct DdcWords {
    uint32_t w[DDC_MAX_CHAN];
};

template <class In, bool MIX>
__global__ __launch_bounds__(F4K_THREADS, (ddc_wg_per_cu<In, MIX>())) void ddc_kernel(
    const char* __restrict__ in, DdcGeom g, uint32_t freq_word, float2* __restrict__ out, const float2* __restrict__ H,
    const float2* __restrict__ tw4096) {
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

    auto issue = [&](typename In::word (&x)[16], size_t blk) {
        const size_t s0 = blk * (size_t)g.L, left = g.n_in - s0;
        In::load(x, in + s0 * In::ELEM, (unsigned)(left < (size_t)F4K_N ? left : (size_t)F4K_N) * In::ELEM, tid);
    };

    typename In::word nxt[16];
    issue(nxt, b);
    for (;;) {
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
        const size_t b_next = b + step;
        const bool more = b_next < g.n_blocks;
        issue(nxt, more ? b_next : b);   // the last block: a harmless re-read of itself
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

template <class In>
__global__ __launch_bounds__(F4K_THREADS, (ddcbank_wg_per_cu<In>())) void ddcbank_kernel(
    const char* __restrict__ in, DdcGeom g, DdcWords fw, float2* __restrict__ out, const float2* __restrict__ H,
    const float2* __restrict__ tw4096) {
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

    auto issue = [&](typename In::word (&x)[16], size_t blk) {
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
            if (word) {   // all 16 factors on their way at once, kept or not (the index is below 4096): one wait
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

static DdcGeom ddc_geom(const DdcArgs& a, unsigned grid) {
    DdcGeom g;
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
    const unsigned stride = grid * (unsigned)g.L;   // grid <= DDC_MAX_GRID: below 2^31
    g.step_q = stride / g.decim;
    g.step_r = stride % g.decim;
    g.index_lo = (unsigned)a.index0;
    return g;
}

template <class In>
static hipError_t launch_ddc_of(const DdcArgs& a) {
    if (!ddc_args_ok(a, false)) return hipErrorInvalidValue;
    const uint32_t word = a.freq_word[0];
    const int wg_per_cu = word ? ddc_wg_per_cu<In, true>() : ddc_wg_per_cu<In, false>();
    const unsigned grid = f4k_grid(a.num_cus, wg_per_cu, ddc_launch_blocks(a));
    if (grid > DDC_MAX_GRID) return hipErrorInvalidValue;
    const DdcGeom g = ddc_geom(a, grid);
    const char* in = static_cast<const char*>(a.d_in);
    if (word)
        hipLaunchKernelGGL((ddc_kernel<In, true>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, word, a.d_out, a.d_h, a.d_twiddle);
    else
        hipLaunchKernelGGL((ddc_kernel<In, false>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, word, a.d_out, a.d_h, a.d_twiddle);
    return hipGetLastError();
}

template <class In>
static hipError_t launch_ddcbank_of(const DdcArgs& a) {
    if (!ddc_args_ok(a, true)) return hipErrorInvalidValue;
    const unsigned grid = f4k_grid(a.num_cus, ddcbank_wg_per_cu<In>(), ddc_launch_blocks(a));
    if (grid > DDC_MAX_GRID) return hipErrorInvalidValue;
    const DdcGeom g = ddc_geom(a, grid);
    DdcWords fw;
    for (int c = 0; c < DDC_MAX_CHAN; ++c) fw.w[c] = c < a.n_chan ? a.freq_word[c] : 0;
    hipLaunchKernelGGL((ddcbank_kernel<In>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, static_cast<const char*>(a.d_in), g, fw,
                       a.d_out, a.d_h, a.d_twiddle);
    return hipGetLastError();
}

hipError_t launch_ddc(const DdcArgs& a) { return launch_ddc_of<OlsInC64>(a); }
hipError_t launch_ddc_i16(const DdcArgs& a) { return launch_ddc_of<OlsInI16>(a); }
hipError_t launch_ddcbank(const DdcArgs& a) { return launch_ddcbank_of<OlsInC64>(a); }
hipError_t launch_ddcbank_i16(const DdcArgs& a) { return launch_ddcbank_of<OlsInI16>(a); }

}  // namespace sdrk

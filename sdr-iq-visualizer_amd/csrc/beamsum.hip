// beamsum.hip — filter-and-sum beamformer: 1 .. 8 coherent channels in, one tuned, filtered and decimated channel out, in one pass
// over a stream of C-channel elements.  ddc_kernel (ddc4096.hip) with a channel loop in front of its second transform: per block
// of 4096 elements every channel is transformed once, its spectrum is multiplied by that channel's own H_c (rotated to
// s = ddc_bin(freq_word)), the products are summed in 16 complex registers per thread, and ONE more transform, the mixer and the
// keeping of kernels_ddc.h finish the block: C + 1 transforms where C single-channel calls run 2 C, and nothing staged in memory.
// kernels_beam.h has the arithmetic and its order.
//
// Skeleton: ddc_kernel's — persistent grid, blocks grid-stride, block b reads elements b L .. b L + 4095, the output descriptor
// runs from the block's first kept output to the launch's end, DdcKeep moves from a workgroup's block to its next one.
// Input: the element-stream read of corrmat4096.hip.  Thread tid owns the samples tid + 256 j of the channel in hand and loads each
// as ONE sample-wide buffer load (8, 4 or 2 bytes) at ((tid + 256 j) C + c) BYTES from the block's first element, through a
// descriptor clipped to min(4096, elements left) C BYTES: a position at or past n_in reads 0.  The stream needs the alignment of a
// sample, not of an element.  A block's cache lines hold samples of all channels: they are fetched once and found in cache by the
// block's next channel.  8-bit input: the format is a run-time Iq8Conv, and the last block of a call sets the positions past n_in
// to +0.0 after widening (byte 0 of cu8 is -127.5), as downconv_iq8.hip does.
// Loads in flight: the 16 loads of the NEXT channel (after the last one: of channel 0 of the workgroup's next block) are issued
// before the current transform and stay in flight across it; H_{c+1}'s 16 cached loads (after the last channel: H_0) are issued
// as soon as channel c's product is formed, one channel ahead as in ddcbank_kernel.
// One loop walks (block, channel) pairs, so the code holds the two transforms once each; the epilogue runs where the channel in
// hand is the block's last.
#include "fft4096_in_ci8.h"
#include "fft4096_in_ci16.h"
#include "kernels_beam.h"

namespace sdrk {

// Workgroups per CU the instantiations are built for: sum 32 + transform 32 + H ahead 32 + next samples 16 .. 32 VGPRs
// (DESIGN.md 4.28 has the compiler's figures).
constexpr int BEAM_WG_PER_CU = 2;

struct BeamGeom {
    size_t n_in, n_out, n_blocks;
    int taps, L, channels;
    unsigned decim, recip;      // D, ceil(2^24 / D)
    unsigned r0;                // index0 % D
    unsigned step_q, step_r;    // (gridDim.x L) / D, (gridDim.x L) % D
    unsigned index_lo;          // (uint32) index0
};
// the keep bookkeeping multiplies the grid by L in 32 bits (kernels_ddc.h); a grid is a few hundred workgroups
constexpr unsigned BEAM_MAX_GRID = 1u << 19;

// Input policies: word = one sample of one channel as loaded.  PAD: a load past the descriptor's end does not widen to +0.0.
struct BeamInC64 {
    typedef v2u word;
    static constexpr int BYTES = 8;
    static constexpr bool PAD = false;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv) {
        const v2f t = __builtin_bit_cast(v2f, w);
        return cf{t.x, t.y};
    }
};
struct BeamInS16 {
    typedef unsigned word;
    static constexpr int BYTES = 4;
    static constexpr bool PAD = false;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv) {
        float re, im;
        ci16_unpack(w, re, im);
        return cf{re, im};
    }
};
struct BeamInB8 {
    typedef unsigned word;
    static constexpr int BYTES = 2;
    static constexpr bool PAD = true;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv c) {
        float re, im;
        ci8_unpack(w, c, re, im);
        return cf{re, im};
    }
};

template <class In, bool MIX>
__global__ __launch_bounds__(F4K_THREADS, BEAM_WG_PER_CU) void beamsum_kernel(
    const char* __restrict__ in, BeamGeom g, Iq8Conv conv, uint32_t freq_word, float2* __restrict__ out,
    const float2* __restrict__ H, const float2* __restrict__ tw4096) {
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    const int rel0 = tid - (g.taps - 1);   // position p = tid + 256 k2 is output b L + rel0 + 256 k2
    const int channels = g.channels;
    const int elem = channels * In::BYTES;
    const int step_in = 256 * elem;        // from sample tid + 256 j to tid + 256 (j + 1): at most 16 KiB
    const int voff_in = tid * elem;

    size_t b = blockIdx.x;
    if (b >= g.n_blocks) return;   // (the launcher starts no workgroup without a block)
    DdcKeep keep = ddc_keep_first(g.r0, blockIdx.x, (unsigned)g.L, g.decim);

    // the 16 samples of channel ch of block blk that this thread owns: inside the block's own elements that exist
    auto issue = [&](typename In::word (&x)[16], size_t blk, int ch) {
        const size_t e0 = blk * (size_t)g.L, left = g.n_in - e0;
        __amdgpu_buffer_rsrc_t r =
            frame_rsrc(in + e0 * (size_t)elem, (unsigned)(left < (size_t)F4K_N ? left : (size_t)F4K_N) * (unsigned)elem);
        const int voff = voff_in + ch * In::BYTES;
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = In::load(r, voff, j * step_in);
    };
    const int s = (int)ddc_bin(freq_word);
    auto issue_h = [&](float2 (&h)[16], int ch) {   // H_ch rotated by s: bin tid + 256 k2
        const float2* __restrict__ Hc = H + (size_t)ch * F4K_N;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) h[k2] = Hc[ols_h_index(tid + 256 * k2, s)];
    };

    float2 h_next[16];
    issue_h(h_next, 0);
    int ch = 0;
    typename In::word nxt[16];
    issue(nxt, b, ch);
    cf u[16];   // the sum over the channels: bin tid + 256 j, the second transform's input j
#pragma unroll
    for (int j = 0; j < 16; ++j) u[j] = cf{0.0f, 0.0f};
    for (;;) {
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j], conv);
        if (In::PAD) {
            const size_t left = g.n_in - b * (size_t)g.L;
            if (left < (size_t)F4K_N) {   // wave-uniform: the last block of a call only
                const unsigned have = (unsigned)left;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if ((unsigned)(tid + 256 * j) >= have) v[j] = cf{0.0f, 0.0f};
            }
        }
        // what follows: the block's next channel, or channel 0 of this workgroup's next block
        const bool last_ch = ch + 1 == channels;
        const int n_ch = last_ch ? 0 : ch + 1;
        const size_t n_b = last_ch ? b + gridDim.x : b;
        const bool more = n_b < g.n_blocks;
        issue(nxt, more ? n_b : b, more ? n_ch : ch);   // behind the last one: a harmless re-read of it
        f4k_transform(v, lds, tw256, tw1, A, tid);
        const bool first = ch == 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const cf X = v[rev16(j)];
            const OlsC z = ols_filter(OlsC{X.x, X.y}, OlsC{h_next[j].x, h_next[j].y});
            const OlsC t = beam_sum(OlsC{u[j].x, u[j].y}, z, first);
            u[j] = cf{t.x, t.y};
        }
        issue_h(h_next, n_ch);   // one channel ahead (after the last: the next block's first)
        if (last_ch) {
            f4k_transform(u, lds, tw256, tw1, A, tid);   // (u is rebuilt from channel 0's product in the next block)
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
        ch = n_ch;
        if (last_ch) {
            b = n_b;
            ddc_keep_next(keep, g.step_q, g.step_r, g.decim);
        }
    }
}

static BeamGeom beam_geom(const BeamArgs& a, unsigned grid) {
    BeamGeom g;
    g.n_in = a.n_in;
    g.n_out = beam_launch_outputs(a);
    g.n_blocks = beam_launch_blocks(a);
    g.taps = a.taps;
    g.L = ols_block_len(a.taps);
    g.channels = a.channels;
    g.decim = (unsigned)a.decim;
    g.recip = ddc_recip(g.decim);
    g.r0 = (unsigned)(a.index0 % g.decim);
    const unsigned stride = grid * (unsigned)g.L;   // grid <= BEAM_MAX_GRID: below 2^31
    g.step_q = stride / g.decim;
    g.step_r = stride % g.decim;
    g.index_lo = (unsigned)a.index0;
    return g;
}

template <class In>
static hipError_t launch_beamsum_of(const BeamArgs& a, Iq8Conv conv) {
    const unsigned grid = f4k_grid(a.num_cus, BEAM_WG_PER_CU, beam_launch_blocks(a));
    if (grid > BEAM_MAX_GRID) return hipErrorInvalidValue;
    const BeamGeom g = beam_geom(a, grid);
    const char* in = static_cast<const char*>(a.d_in);
    if (a.freq_word)
        hipLaunchKernelGGL((beamsum_kernel<In, true>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, conv, a.freq_word, a.d_out,
                           a.d_h, a.d_twiddle);
    else
        hipLaunchKernelGGL((beamsum_kernel<In, false>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, conv, a.freq_word, a.d_out,
                           a.d_h, a.d_twiddle);
    return hipGetLastError();
}

hipError_t launch_beamsum(const BeamArgs& a, int in) {
    if (!beam_args_ok(a, in)) return hipErrorInvalidValue;
    if (in == BEAM_IN_C64) return launch_beamsum_of<BeamInC64>(a, iq8_conv(IQ8_SIGNED));
    if (in == BEAM_IN_S16) return launch_beamsum_of<BeamInS16>(a, iq8_conv(IQ8_SIGNED));
    return launch_beamsum_of<BeamInB8>(a, iq8_conv(in));
}

}  // namespace sdrk

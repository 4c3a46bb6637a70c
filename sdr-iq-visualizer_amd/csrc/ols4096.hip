// ols4096.hip — overlap-save FIR channel extraction at a block length of 4096: tune, filter and decimate in one pass.  One
// workgroup per block and iteration: forward transform (f4k_transform) -> multiply by the filter's frequency response rotated by
// the tuning offset -> inverse transform -> keep the valid samples -> mixer -> decimated store.  kernels_ols.h has the block
// geometry and the arithmetic (written once, shared with the host stand-in).
//
// f4k_transform takes v[j] = x[tid + 256 j] and returns X[tid + 256 k2] in v[rev16(k2)]: a thread owns the same 16 positions on
// entry and on exit, so the spectrum of the first transform is the input of the second after a compile-time renaming of
// registers, with no third exchange.  The inverse runs through the same transform by conjugation (ols_filter conjugates the
// product, ols_unscale conjugates the result and scales by the exact 2^-12).
//
// The streaming skeleton of fft4096.hip: persistent grid, buffer descriptors throughout, the NEXT block's 16 loads per thread in
// flight across both transforms.  A block's load descriptor is clipped to the input (the last block reads zeros past n_in) and
// its store descriptor to the outputs that exist.
// Per thread the 16 values H_s[tid + 256 k2] are read once per launch and stay in REGISTERS (32 VGPRs).  In LDS they would take
// 32 KiB beside the 37 KiB of exchange buffer and tables, which fits two workgroups per CU and not three; DESIGN.md 4.20 has the
// compiler's figures and the workgroups per CU of each instantiation (ols_wg_per_cu).
// Kept lanes: position p = tid + 256 k2 is output i = b L + p - (M - 1); L is a multiple of 256 and D divides 256, so
// (p - (M - 1)) mod D depends on tid alone: a thread stores all of its in-range positions or none, at offsets fixed per launch.
// The mixer's factor W4096^((phase0 + s i) mod 4096) comes from the plan's twiddle table (32 KiB, cache resident), one read per
// stored sample; s = 0 compiles it out.
// The int16 policy gives x = float32(I) + i float32(Q) exactly and then the same arithmetic in the same order.
#include "kernels_ols.h"
#include "ols_in.h"

namespace sdrk {

// Workgroups per CU an instantiation is built for: three (at most 168 VGPRs) where the compiler fits it without spilling —
// 158 (complex64), 132 (int16), 148 (int16 with the mixer) — and two for complex64 with the mixer, which needs 174.
template <class In, bool MIX>
constexpr int ols_wg_per_cu() { return (MIX && In::ELEM == 8) ? 2 : 3; }

struct OlsGeom {
    size_t n_in, n_out, n_blocks;
    int taps, L, log2d;
    unsigned shift_bins, phase0;   // both mod 4096
    unsigned run;                  // blocks per workgroup in contiguous runs; 0: grid-stride
};

template <class In, bool MIX>
__global__ __launch_bounds__(F4K_THREADS, (ols_wg_per_cu<In, MIX>())) void ols4096_kernel(
    const char* __restrict__ in, OlsGeom g, float2* __restrict__ out, const float2* __restrict__ H,
    const float2* __restrict__ tw4096) {
    __shared__ float2 lds[f4k_lds_elems(false)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;
    float2* __restrict__ tw1 = tw256 + 256;

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    __syncthreads();

    OlsC h[16];   // H_s[tid + 256 k2]
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const float2 t = H[ols_h_index(tid + 256 * k2, (int)g.shift_bins)];
        h[k2] = OlsC{t.x, t.y};
    }
    const int rel0 = tid - (g.taps - 1);                        // position p = tid + 256 k2 is output b L + rel0 + 256 k2
    const bool lane_kept = (rel0 & ((1 << g.log2d) - 1)) == 0;   // (two's complement: also right for rel0 < 0)
    const unsigned out_per_block = (unsigned)g.L >> g.log2d;

    size_t b, b_end, step;
    if (g.run) {
        b = (size_t)blockIdx.x * g.run;
        b_end = b + g.run < g.n_blocks ? b + g.run : g.n_blocks;
        step = 1;
    } else {
        b = blockIdx.x;
        b_end = g.n_blocks;
        step = gridDim.x;
    }
    if (b >= b_end) return;   // (the launcher starts no workgroup without a block)

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
        const bool more = b_next < b_end;
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
        if (lane_kept) {
            const size_t o0 = b * (size_t)out_per_block, left = g.n_out - o0;
            __amdgpu_buffer_rsrc_t w = frame_rsrc(out + o0, (unsigned)(left < out_per_block ? left : out_per_block) * 8);
            const size_t i0 = b * (size_t)g.L;
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) {
                const int rel = rel0 + 256 * k2;
                if ((unsigned)rel < (unsigned)g.L) {
                    const cf y = u[rev16(k2)];
                    OlsC o = ols_unscale(OlsC{y.x, y.y});
                    if (MIX) {
                        const float2 t = tw4096[ols_mix_index(g.phase0, g.shift_bins, i0 + (size_t)rel)];
                        o = ols_mix(o, OlsC{t.x, t.y});
                    }
                    const v2f ov = {o.x, o.y};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, ov), w, (rel >> g.log2d) * 8, 0, 0);
                }
            }
        }
        if (!more) break;
        b = b_next;
    }
}

template <class In>
static hipError_t launch_ols4096_of(const OlsArgs& a) {
    if (a.taps < 1 || a.taps > OLS_MAX_TAPS || a.n_in < (size_t)a.taps || !a.d_in || !a.d_out || !a.d_h || !a.d_twiddle)
        return hipErrorInvalidValue;
    if (a.decim < 1 || a.decim > OLS_MAX_DECIM || (a.decim & (a.decim - 1))) return hipErrorInvalidValue;
    if (a.shift_bins < -OLS_N / 2 || a.shift_bins >= OLS_N / 2) return hipErrorInvalidValue;
    OlsGeom g;
    g.n_in = a.n_in;
    g.n_out = ols_outputs(a.n_in, a.taps, a.decim);
    g.n_blocks = ols_blocks(a.n_in, a.taps);
    g.taps = a.taps;
    g.L = ols_block_len(a.taps);
    if (a.max_blocks && a.max_blocks < g.n_blocks) {
        g.n_blocks = a.max_blocks;
        const size_t cut = a.max_blocks * (size_t)(g.L / a.decim);
        if (cut < g.n_out) g.n_out = cut;
    }
    g.log2d = __builtin_ctz((unsigned)a.decim);
    g.shift_bins = (unsigned)a.shift_bins & (OLS_N - 1);
    g.phase0 = (unsigned)a.phase0 & (OLS_N - 1);
    const int wg_per_cu = a.shift_bins ? ols_wg_per_cu<In, true>() : ols_wg_per_cu<In, false>();
    unsigned grid = f4k_grid(a.num_cus, wg_per_cu, g.n_blocks);
    g.run = 0;
    if (a.assign == OLS_ASSIGN_RUNS) {
        const size_t run = (g.n_blocks + grid - 1) / grid;
        g.run = (unsigned)run;
        grid = (unsigned)((g.n_blocks + run - 1) / run);
    }
    const char* in = static_cast<const char*>(a.d_in);
    if (a.shift_bins)
        hipLaunchKernelGGL((ols4096_kernel<In, true>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, a.d_out, a.d_h, a.d_twiddle);
    else
        hipLaunchKernelGGL((ols4096_kernel<In, false>), dim3(grid), dim3(F4K_THREADS), 0, a.stream, in, g, a.d_out, a.d_h, a.d_twiddle);
    return hipGetLastError();
}

hipError_t launch_ols4096(const OlsArgs& a) { return launch_ols4096_of<OlsInC64>(a); }
hipError_t launch_ols4096_i16(const OlsArgs& a) { return launch_ols4096_of<OlsInI16>(a); }

}  // namespace sdrk

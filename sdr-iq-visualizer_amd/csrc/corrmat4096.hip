// corrmat4096.hip — the F-engine of the correlation-matrix calls at N = 4096: the flagship transform (fft4096.hip: window * x ->
// 4096-point FFT -> fftshift) run on every channel of a frame of C-channel elements, read DIRECTLY from the element stream, the
// shift-ordered complex64 spectra written to plan-owned staging for corrmat_rows.hip.  No split pass: 8 C bytes per element read
// from complex64 (4 C from int16, 2 C from 8-bit) and 8 C written, where de-interleaving first moves 16 C more.
//
// One workgroup takes a whole frame and runs its C channels one after the other, so the frame's cache lines — every one of them
// holds samples of all channels — are fetched from memory once and found in cache by the next channel.  Thread tid owns the
// samples tid + 256 j of the channel in hand and loads each as ONE sample-wide buffer load (8, 4 or 2 bytes) at
//     ((tid + 256 j) * C + channel) * sample bytes
// from the frame's start: that serves every C and the sample-only alignment of the stream.  The next channel's (or the next
// frame's first channel's) 16 loads per thread are issued before the current transform and stay in flight across it.  Persistent
// grid, frames taken grid-stride, buffer loads, LDS tables and window as in the other N = 4096 kernels; widening by the
// existing helpers (ci16_unpack, ci8_unpack with the format as a run-time argument).  The spectrum's bits are those of
// f4k_windowed_transform on the de-interleaved channel, which is what the plan's own EPI_COMPLEX launch and xspec4096.hip give.
//
// Built for three workgroups per CU: at most 168 VGPRs, 52.1 KiB of LDS with the window, no scratch (DESIGN.md 4.27 has the
// compiler's figures).
#include "fft4096_in_ci16.h"
#include "kernels_corrmat.h"

namespace sdrk {

constexpr int CM4K_WG_PER_CU = 3;

// Input policies of the N = 4096 reader: word = one sample of one channel as loaded.
struct CmInC64 {
    typedef v2u word;
    static constexpr int BYTES = 8;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv) {
        const v2f t = __builtin_bit_cast(v2f, w);
        return cf{t.x, t.y};
    }
};
struct CmInS16 {
    typedef unsigned word;
    static constexpr int BYTES = 4;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv) {
        float re, im;
        ci16_unpack(w, re, im);
        return cf{re, im};
    }
};
struct CmInB8 {
    typedef unsigned word;
    static constexpr int BYTES = 2;
    static __device__ __forceinline__ word load(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, F4K_NT);
    }
    static __device__ __forceinline__ cf widen(word w, Iq8Conv c) {
        float re, im;
        ci8_unpack(w, c, re, im);
        return cf{re, im};
    }
};

// iq: frame 0's first element; n_frames frames, frame_stride elements apart; spec: channel c's frame f at c * plane + f * 4096
template <class In, bool HAS_WINDOW>
__global__ __launch_bounds__(F4K_THREADS, CM4K_WG_PER_CU) void corrmat4096_spectra_kernel(
    const char* __restrict__ iq, size_t frame_stride, int channels, Iq8Conv conv, size_t n_frames, float2* __restrict__ spec,
    size_t plane, const float* __restrict__ window, const float2* __restrict__ tw4096, int shift) {
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
    const int elem = channels * In::BYTES;
    const int frame_bytes = F4K_N * elem;          // at most 256 KiB
    const int step = 256 * elem;                   // from sample tid + 256 j to tid + 256 (j + 1)
    const int voff_in = tid * elem;

    // the 16 samples of channel ch of frame fr that this thread owns: all inside the frame's own F4K_N elements
    auto issue = [&](typename In::word (&x)[16], size_t fr, int ch) {
        __amdgpu_buffer_rsrc_t r = frame_rsrc(iq + fr * frame_stride * (size_t)elem, (unsigned)frame_bytes);
        const int voff = voff_in + ch * In::BYTES;
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = In::load(r, voff, j * step);
    };

    size_t fr = blockIdx.x;   // (the launcher starts no more workgroups than there are frames)
    int ch = 0;
    typename In::word nxt[16];
    issue(nxt, fr, ch);
    for (;;) {
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j], conv);
        // what follows: the frame's next channel, or the first channel of this workgroup's next frame
        int n_ch = ch + 1;
        size_t n_fr = fr;
        if (n_ch == channels) {
            n_ch = 0;
            n_fr = fr + gridDim.x;
        }
        const bool more = n_fr < n_frames;
        issue(nxt, more ? n_fr : fr, more ? n_ch : ch);   // behind the last one: a harmless re-read of it
        f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
        __amdgpu_buffer_rsrc_t w = frame_rsrc(spec + (size_t)ch * plane + fr * (size_t)F4K_N, F4K_N * 8);
        f4k_store_row<EPI_COMPLEX>(v, w, tid * 8, xor_k2, 0.0f);
        if (!more) break;
        fr = n_fr;
        ch = n_ch;
    }
}

template <class In>
static hipError_t launch_corrmat4096_of(const IntegrateArgs& a, int fmt, int channels, float2* d_spec, size_t plane) {
    const size_t n_frames = a.f1 - a.f0;
    dim3 g(f4k_grid(a.num_cus, CM4K_WG_PER_CU, n_frames)), b(F4K_THREADS);
    const char* iq = static_cast<const char*>(a.d_in);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
    const Iq8Conv conv = iq8_conv(fmt == CM_B8_UNSIGNED ? IQ8_UNSIGNED : IQ8_SIGNED);
    if (a.d_window)
        hipLaunchKernelGGL((corrmat4096_spectra_kernel<In, true>), g, b, 0, a.stream, iq, a.in_stride, channels, conv, n_frames,
                           d_spec, plane, a.d_window, tw, a.shift);
    else
        hipLaunchKernelGGL((corrmat4096_spectra_kernel<In, false>), g, b, 0, a.stream, iq, a.in_stride, channels, conv, n_frames,
                           d_spec, plane, a.d_window, tw, a.shift);
    return hipGetLastError();
}

hipError_t launch_corrmat4096_spectra(const IntegrateArgs& a, int fmt, int channels, float2* d_spec, size_t plane) {
    if (a.f1 <= a.f0) return hipSuccess;
    if (channels < CM_MIN_CHANNELS || channels > CM_MAX_CHANNELS) return hipErrorInvalidValue;
    if (fmt == CM_C64) return launch_corrmat4096_of<CmInC64>(a, fmt, channels, d_spec, plane);
    if (fmt == CM_S16) return launch_corrmat4096_of<CmInS16>(a, fmt, channels, d_spec, plane);
    return launch_corrmat4096_of<CmInB8>(a, fmt, channels, d_spec, plane);
}

}  // namespace sdrk

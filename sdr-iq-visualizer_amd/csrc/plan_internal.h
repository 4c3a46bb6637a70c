// plan_internal.h — what the host translation units of the C ABI share: the plan object behind the opaque sdrk_plan and the
// entry points of sdrk_api.hip that the double-precision entry points (sdrk_f64.hip) build on.  Not installed; host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sdrk.h"

namespace sdrk_host {
constexpr int HOST_SLOTS = 3;
struct HostSlot {
    void *h_in = nullptr, *h_out = nullptr;   // pinned
    void *d_in = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;
    hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_done = nullptr;
    // the chunk in flight in this slot (busy == true): where its rows go once ev_done has fired
    // (user_out == nullptr: the rows were DMA'd straight into the caller's pinned array)
    bool busy = false;
    void* user_out = nullptr;
    size_t out_bytes = 0;
};
}  // namespace sdrk_host

struct sdrk_plan {
    int device = 0;
    int nfft = 0;
    size_t max_batch = 0;
    float eps = 1e-12f;
    int shift = 1;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float* d_window = nullptr;     // nfft floats, or nullptr for rectangular
    float2* d_twiddle = nullptr;   // W_min(nfft,4096)^m
    float2* d_scratch = nullptr;   // large plans
    size_t scratch_frames = 0;
    void* d_in = nullptr;          // whole-stream staging (Welch PSD, waterfall append from host IQ); only grows
    size_t in_cap = 0;
    void* d_out = nullptr;
    size_t out_cap = 0;
    void* d_feat = nullptr;          // per-row feature results of sdrk_frame_features_host (only grows)
    size_t feat_cap = 0;
    float2* d_tw_2p = nullptr;       // two-pass tiled plans (fft_tiled2.hip)
    bool tiled2 = false;
    // overlapped form of the two-pass plans: row pass of chunk i on stream2 beside the col pass of chunk i + 1
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_col[2] = {nullptr, nullptr}, ev_row[2] = {nullptr, nullptr}, ev_fork = nullptr;
    int col_cus = 0, row_cus = 0;    // 0: serial form
    // sdrk_exec_host pipeline: HOST_SLOTS chunks in flight, each with pinned host and device staging
    sdrk_host::HostSlot slot[sdrk_host::HOST_SLOTS];
    float staging_probe_ms[sdrk_host::HOST_SLOTS * 3] = {};   // SDRK_PLAN_TUNE_STAGING: the transform over each candidate pairing
    int staging_probe_n = 0;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    // non-power-of-two lengths (bluestein.hip): inner power-of-two plan of size blu_m
    sdrk_plan* blu_inner = nullptr;
    int blu_m = 0;
    float2* d_blu_chirp = nullptr;   // c[n] = exp(+i pi n^2 / N), n < N
    float2* d_blu_bspec = nullptr;   // FFT_M(b)
    float2* d_blu_a = nullptr;       // work buffers: blu_frames * M complex64 each
    float2* d_blu_b = nullptr;
    size_t blu_frames = 0;
    // small-call fast path of sdrk_exec_host: pinned, device-mapped staging the kernel reads and
    // writes directly over PCIe (no DMA-engine copies for a 32 KiB frame)
    void* h_small_in = nullptr;
    void* h_small_out = nullptr;
    uint32_t* h_small_flag = nullptr;   // completion word the stream writes behind a small call
    void* d_small_flag = nullptr;
    uint32_t small_seq = 0;
    // N = 65536 fused path (fft_fused64k.hip).  fused64k: every launch (SDRK_PLAN_FUSED64K); fused_auto: launches of at least
    // FUSED_AUTO_MIN_FRAMES frames (the default for nfft = 65536), until one reports a failed hand-over (fused_broken, latched).
    bool fused64k = false, fused_auto = false, fused_broken = false;
    void* d_fused_ring = nullptr;
    unsigned* d_fused_ctrl = nullptr;
    unsigned* h_fused_err = nullptr;   // pinned mailbox: error word of the last launches
    unsigned fused_launches = 0, fused_pending = 0;
    // double-precision plans (sdrk_plan_create_f64, sdrk_f64.hip): precision 64, and the fields below instead of the float32
    // window / tables / scratch above (which stay empty); every other plan has precision 32
    int precision = 32;
    double eps64 = 0.0;
    double* d_window64 = nullptr;   // nfft doubles, or nullptr for rectangular
    double* d_tw64 = nullptr;       // W_4096^m, m < 4096, complex128 (interleaved)
    void* d_scratch64 = nullptr;    // two-pass lengths: scratch_frames * nfft complex128
};

namespace sdrk_host {

// One transform of the plan: (plan, device input, frames, frame stride, device output, epilogue, stream) -> sdrk_status.
using LaunchFn = int (*)(sdrk_plan*, const void*, size_t, size_t, void*, int, hipStream_t);

// What the numpy boundary (exec_host) needs to know about one kind of transform.
struct HostIo {
    size_t in_elem = 0;            // bytes per input sample
    size_t out_elem = 0;           // bytes per output bin
    int epilogue = 0;              // handed to `launch`
    int precision = 32;            // the plan kind the entry point serves (32 / 64)
    int zero_copy_max_nfft = 0;    // longest frame whose kernel may read / write pinned host memory itself
    LaunchFn launch = nullptr;
};

int fail_text(int status, const char* msg);    // sets sdrk_last_error(), returns status
int check_device(int device);
// NULL plan, plan of another precision, NULL buffers, zero stride
int check_exec_args(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out, int precision);
// the small mapped call, the zero-copy chunks and the three-slot pipeline of sdrk_exec_host, for any element sizes
int exec_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out, const HostIo& io);

}  // namespace sdrk_host

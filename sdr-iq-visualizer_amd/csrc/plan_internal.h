// plan_internal.h — what the host translation units of the C ABI (sdrk_*.hip) share: the plan object behind the opaque
// sdrk_plan, error reporting, the argument checks, the launch dispatcher and the staging slots of the numpy boundary.  Each
// function is defined in exactly one .hip, named beside its declaration.  Not installed; host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/sdrk.h"
#include "kernels.h"

namespace sdrk_host {
constexpr int HOST_SLOTS = 3;
// What a chunk of a SlotPipe brings back, and how that reaches the caller's array `user` when the chunk's slot retires.
struct ChunkOut {
    enum Rows {
        None,     // nothing per chunk: ev_k ends the chunk, the D2H stream is not touched
        Pooled,   // D2H into h_out; at retire the helper threads copy h_out -> user
        Direct,   // D2H straight into the caller's pinned array; nothing at retire
        Kernel,   // the kernel wrote h_out itself (zero-copy): ev_done follows it on the plan's stream; then as Pooled
        Planes,   // D2H of `planes` packed planes into h_out; at retire a memcpy of each -> user + i * plane_stride bytes
    } rows = None;
    void* user = nullptr;
    size_t bytes = 0;   // of one plane; 0: no copy either way
    size_t planes = 1, plane_stride = 0;
};
struct HostSlot {
    void *h_in = nullptr, *h_out = nullptr;   // pinned
    void *d_in = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;
    hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_done = nullptr;
    bool busy = false;   // a chunk is in flight in this slot: `out` is what it brings back
    ChunkOut out;
};

// Plan-owned device staging that calls on any stream share: growing buffers under one ordering.  `ev` follows the last work
// enqueued on the buffers (on stream `last`; busy: there may be such work).  A call reserves what it needs, enters on its
// stream, enqueues its work and leaves; the buffers only grow, and never under work that still uses them.
struct Staging {
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool busy = false;
    struct Buf {
        void* d = nullptr;
        size_t cap = 0;
    } buf[2];                                 // (the integrated calls keep two under one ordering)
    int reserve(int i, size_t need);          // buf[i] of at least `need` bytes; the host waits for work in flight before it reallocates
    int wait();                               // the host waits for the work in flight
    int enter(hipStream_t stream);            // `stream` waits for the last user if that was another stream
    int leave(hipStream_t stream, int st);    // the event behind this call's work, also after a failed launch; -> st or the record's failure
    void release();                           // plan destruction
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
    // int16 input (ci16_api.hip) at the lengths without an int16-reading kernel: buf[0] = complex64 staging the frames are
    // widened into, at most 64 MiB
    sdrk_host::Staging ci16;
    // integrated spectra (integrate_api.hip): buf[0] = two carry rows + the partial rows of split groups; buf[1] = complex64
    // spectra of the lengths without a fused kernel, at most 64 MiB
    sdrk_host::Staging integ;
    // polyphase filter bank (pfb_api.hip): d_pfb_h = the prototype, pfb_taps * nfft float32 (sdrk_plan_set_pfb; 0 taps = none);
    // pfb_assign = pfb4096_kernel's frame assignment (kernels_pfb.h); pfb.buf[0] = folded complex64 frames of the lengths
    // without a folding transform, at most 64 MiB
    float* d_pfb_h = nullptr;
    int pfb_taps = 0;
    int pfb_assign = 0;
    sdrk_host::Staging pfb;
    // FIR filtering and channel extraction (fir_api.hip): d_fir_h = DFT_4096 of the zero-padded taps, 4096 complex64 in natural
    // bin order (sdrk_plan_set_fir; 0 taps = none); fir_assign = ols4096_kernel's block assignment (kernels_ols.h)
    float2* d_fir_h = nullptr;
    int fir_taps = 0;
    int fir_assign = 0;
    // filter-and-sum beamformer (fir_api.hip): d_beam_h = beam_channels x 4096 complex64, channel-major, row c = what
    // sdrk_plan_set_fir makes of channel c's taps (sdrk_plan_set_beam; 0 channels = none; allocated once, for 8 channels)
    float2* d_beam_h = nullptr;
    int beam_channels = 0;
    int beam_taps = 0;
    // N = 4096, frames dealt by ticket (f4k_ticket.h, fft4096_ticket_kernel): f4k_order = SDRK_F4K_ORDER at creation;
    // d_f4k_heads = the eight heads, never reset; f4k_bases = where they stand behind every launch enqueued so far.  Two
    // ticketed launches of a plan must not overlap: f4k_ev follows the last one (on f4k_last), and a call on another stream
    // waits for it.  f4k_parts: SDRK_F4K_PARTS, launches per call in either order (developer use; 0: f4k_ticket_parts / f4k_split_parts).
    int f4k_order = sdrk_host::F4K_ORDER_AUTO;
    sdrk_host::F4kTicketForm f4k_form = sdrk_host::F4K_TICKET_FORM;   // SDRK_F4K_TICKET_FORM (A/B work)
    unsigned* d_f4k_heads = nullptr;
    sdrk_host::F4kTicketBases f4k_bases = {};
    // the "rot H" order (f4k_rot.h): f4k_rot_heads = 2, 4 or 8 (SDRK_F4K_TICKET_FORM=rot<H>), 0 = f4k_form above;
    // d_f4k_rot = its heads and exit counter, zero between launches
    unsigned f4k_rot_heads = sdrk_host::F4K_ROT_DEFAULT_HEADS;
    unsigned* d_f4k_rot = nullptr;
    // its look-ahead (SDRK_F4K_ROT_AHEAD at creation): F4K_AHEAD_*
    int f4k_rot_ahead = sdrk_host::F4K_ROT_DEFAULT_AHEAD;
    hipEvent_t f4k_ev = nullptr;
    hipStream_t f4k_last = nullptr;
    bool f4k_recorded = false;
    size_t f4k_parts = 0;
    // real-sampled input (sdrk_exec_*_real, ci16_api.hip): d_real_win = the mode's own window, 2 * nfft float32
    // (sdrk_plan_set_real_window; nullptr = rectangular); d_real_tab = exp(-i pi k / nfft), k < nfft, built at the first call;
    // real.buf[0] = the windowed complex64 pairs and real.buf[1] = their transform, of the lengths without a fused kernel,
    // at most 64 MiB each
    float* d_real_win = nullptr;
    float2* d_real_tab = nullptr;
    sdrk_host::Staging real;
};

namespace sdrk_host {

constexpr size_t SMALL_IN_BYTES = 256 << 10;   // calls up to this much input take the zero-copy path
constexpr size_t HOST_CHUNK_BYTES = 16 << 20;  // target input bytes per pipelined chunk of sdrk_exec_host
constexpr size_t ZERO_COPY_MAX_BYTES = 32 << 20;  // calls up to this much input skip the DMA engines (see exec_host)
constexpr unsigned FUSED_MAILBOX = 64;   // entries of 8 words: error flag + debug record
// Below this many frames a launch of an auto plan takes the two tiled launches: the persistent launch costs about 30 us before
// its first row (control-block memset, role formation, the ramp of a set's pipeline, the mailbox copy) against 11-18 us, and
// the two forms cross between 384 and 512 frames, packed or half-overlapped (profiles/r06/fused64k_crossover.log).
constexpr size_t FUSED_AUTO_MIN_FRAMES = 512;

// ---- sdrk_api.hip: error text, devices, pinned ranges, growing device buffers ----
int fail(int status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // sets sdrk_last_error(), returns status

#define HIP_TRY(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t e__ = (expr);                                                                                        \
        if (e__ != hipSuccess)                                                                                          \
            return ::sdrk_host::fail(e__ == hipErrorOutOfMemory ? SDRK_ERR_NOMEM : SDRK_ERR_HIP,                        \
                                     "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__);       \
    } while (0)

int check_device(int device);
bool is_pow2(long long v);

// Pinned host ranges the library knows about (sdrk_host_alloc / sdrk_host_register): start -> (bytes, owned)
struct PinnedRanges {
    std::mutex m;
    std::map<uintptr_t, std::pair<size_t, bool>> r;
    bool covers(const void* p, size_t bytes) {
        if (!p || bytes == 0) return false;
        std::lock_guard<std::mutex> g(m);
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        auto it = r.upper_bound(a);
        if (it == r.begin()) return false;
        --it;
        return a >= it->first && a + bytes <= it->first + it->second.first;
    }
};
PinnedRanges& pinned_ranges();

int grow(int device, void** buf, size_t* cap, size_t need);   // device staging that only ever grows

inline int Staging::wait() {
    if (busy) {
        HIP_TRY(hipEventSynchronize(ev));
        busy = false;
    }
    return SDRK_OK;
}

inline int Staging::reserve(int i, size_t need) {
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    Buf& b = buf[i];
    if (need <= b.cap) return SDRK_OK;
    if (int st = wait(); st != SDRK_OK) return st;
    if (b.d) {
        HIP_TRY(hipFree(b.d));
        b.d = nullptr;
        b.cap = 0;
    }
    HIP_TRY(hipMalloc(&b.d, need));
    b.cap = need;
    return SDRK_OK;
}

inline int Staging::enter(hipStream_t stream) {
    if (busy && last != stream) HIP_TRY(hipStreamWaitEvent(stream, ev, 0));
    return SDRK_OK;
}

inline int Staging::leave(hipStream_t stream, int st) {
    const hipError_t e = hipEventRecord(ev, stream);
    last = stream;
    busy = true;
    if (st == SDRK_OK && e != hipSuccess) st = fail(SDRK_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    return st;
}

inline void Staging::release() {
    for (Buf& b : buf)
        if (b.d) (void)hipFree(b.d);
    if (ev) (void)hipEventDestroy(ev);
}

// ---- sdrk_plan.hip: argument checks, the launch dispatcher, the fused N = 65536 gate ----
int check_precision(const sdrk_plan* p, int precision);
// NULL plan, plan of another precision, NULL buffers, zero stride
int check_exec_args(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out, int precision = 32);
bool takes_fused(const sdrk_plan* p, size_t n_frames);   // the persistent N = 65536 kernel for a call of this many frames?
struct EpiArgs;   // chirp-z epilogues riding on an inner plan's row pass (sdrk_plan.hip)
// One float32 transform of the plan.  d_mip / mip_written: see LaunchArgs (kernels.h) — *mip_written tells whether the launch
// wrote the by-16 companion rows.  call_frames: when this launch is one chunk of a larger call, the frames of that call — the
// N = 65536 form is picked for the call (takes_fused), so that its chunks do not each fall under the threshold (0: n_frames).
int plan_launch(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, void* d_out, int epilogue,
                hipStream_t stream, float* d_mip = nullptr, bool* mip_written = nullptr, const EpiArgs* epi = nullptr,
                size_t call_frames = 0);
int fused_check(sdrk_plan* p);   // after a stream sync: the fused launches since the last check

// What every launcher of a float32 plan's own kernel takes from the plan, and the call's input, frames, stride, output,
// epilogue and stream (plan_launch adds its scratch, companion-row, epilogue-table and overlap fields).
inline sdrk::LaunchArgs plan_launch_args(const sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, void* d_out,
                                         int epilogue, hipStream_t stream) {
    sdrk::LaunchArgs a;
    a.d_iq = d_iq;
    a.frame_stride = frame_stride;
    a.d_out = d_out;
    a.n_frames = n_frames;
    a.nfft = p->nfft;
    a.d_window = p->d_window;
    a.d_twiddle = p->d_twiddle;
    a.eps = p->eps;
    a.shift = p->shift;
    a.epilogue = epilogue;
    a.stream = stream;
    a.num_cus = p->num_cus;
    return a;
}

// The body of the sdrk_exec_device*_timed_each entry points, behind their argument checks: `launches` times launch() (-> a
// sdrk_status) on the plan's stream with an event between consecutive ones, then the time of each in each_ms.  A failed launch
// ends the call with its status once the stream has drained.
template <class Launch>
int timed_each(sdrk_plan* p, int launches, float* each_ms, Launch launch) {
    HIP_TRY(hipSetDevice(p->device));
    std::vector<hipEvent_t> ev((size_t)launches + 1, nullptr);
    auto cleanup = [&] { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); };
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) { cleanup(); return fail(SDRK_ERR_HIP, "hipEventCreate failed"); }
    hipError_t e = hipEventRecord(ev[0], p->stream);
    for (int i = 0; i < launches && e == hipSuccess; ++i) {
        const int st = launch();
        if (st != SDRK_OK) { (void)hipStreamSynchronize(p->stream); cleanup(); return st; }
        e = hipEventRecord(ev[(size_t)i + 1], p->stream);
    }
    if (e == hipSuccess) e = hipEventSynchronize(ev[(size_t)launches]);
    for (int i = 0; i < launches && e == hipSuccess; ++i) e = hipEventElapsedTime(&each_ms[i], ev[i], ev[(size_t)i + 1]);
    cleanup();
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "timed launches failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

// ---- sdrk_probes.hip ----
int tune_staging(sdrk_plan* p);   // SDRK_PLAN_TUNE_STAGING, at plan creation

// ---- sdrk_host_pipeline.hip: the staging slots and the numpy boundary ----
// One transform of the plan: (plan, device input, frames, frame stride, device output, epilogue, stream) -> sdrk_status.
using LaunchFn = int (*)(sdrk_plan*, const void*, size_t, size_t, void*, int, hipStream_t);

// What the numpy boundary (exec_host) needs to know about one kind of transform.
struct HostIo {
    size_t in_elem = 0;            // bytes per input sample
    size_t out_elem = 0;           // bytes per output bin
    int epilogue = 0;              // handed to `launch`
    int precision = 32;            // the plan kind the entry point serves (32 / 64)
    int zero_copy_max_nfft = 0;    // longest frame whose kernel may read / write pinned host memory itself
    int zero_copy_min_nfft = 0;    // ... and the shortest
    size_t in_span = 0;            // input samples a frame reads from its start (0: nfft; pfb_api.hip: taps * nfft)
    size_t out_bins = 0;           // output bins per frame (0: nfft; the real-input spectra: nfft + 1, and then neither the
                                   // small mapped call nor the zero-copy branches are offered)
    LaunchFn launch = nullptr;
};

int slot_reserve(sdrk_plan* p, HostSlot& s, size_t in_bytes, size_t out_bytes);   // events and staging of at least these sizes
void slots_abandon(sdrk_plan* p);   // error path: nothing may still be writing into the staging buffers
// Where a copy engine (or, on the zero-copy branch, the kernel) reads a chunk of the caller's input: the caller's own array
// if it is pinned, else the slot's pinned h_in, filled by the helper threads.
const void* chunk_pinned_src(HostSlot& s, const void* src, size_t bytes, bool in_pinned);

// The chunks of one host call through the plan's HOST_SLOTS staging slots: the ordering every chunked entry point shares,
// written once.  Per chunk the caller runs acquire -> (fills or picks the pinned input) -> upload -> its launch on the plan's
// stream -> submit, and drain after the last chunk; how chunks are cut, what is launched and what comes back stay with the
// caller.  Every step that fails has abandoned the slots before it returns the status.
struct SlotPipe {
    sdrk_plan* p = nullptr;
    const char* what = nullptr;   // names the pipeline in a failure's text
    size_t n = 0;                 // chunks submitted so far: chunk n takes slot n % HOST_SLOTS
    // optional: called around a retire's wait (0 before, 1 after) and after its delivery (2) — exec_host's SDRK_HOST_TRACE
    void (*mark)(void* ctx, int point) = nullptr;
    void* mark_ctx = nullptr;

    int open(sdrk_plan* plan, const char* name);                   // s_h2d / s_d2h, created at the first chunked call
    // the next chunk's slot: waits for the chunk in flight there and delivers it, then staging of at least these sizes
    int acquire(size_t chunk_in, size_t chunk_out, HostSlot*& s);
    // the pinned chunk -> the slot's d_in on s_h2d; ev_in behind it, and the plan's stream waits for that
    int upload(HostSlot& s, const void* pinned_src, size_t bytes);
    // behind the caller's launch (launch_st: its status): ev_k on the plan's stream, then what `out` says — s_d2h waits for
    // ev_k, copies out.planes * out.bytes from d_out (no copy of 0 bytes) and records ev_done; ChunkOut::None stops at ev_k;
    // ChunkOut::Kernel records ev_done on the plan's stream and nothing else
    int submit(HostSlot& s, int launch_st, const ChunkOut& out);
    int drain();                                                   // retires the chunks in flight, in submission order

private:
    int retire(HostSlot& s);
    int hip_failed(hipError_t e);
};

// the small mapped call, the zero-copy chunks and the three-slot pipeline of sdrk_exec_host, for any element sizes
int exec_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out, const HostIo& io);

// The per-frame entry points of a mode (sample format x front end), behind their names — the shape integrate_call.h gives
// the integrated ones.  `check` is the mode's argument check, `launch` its transform.
using CheckFn = int (*)(const sdrk_plan*, const void* in, size_t n_frames, size_t frame_stride, const void* out);
int check_exec_f32(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out);   // check_exec_args, float32 (sdrk_plan.hip)
int launch_f32(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t s);   // plan_launch as a LaunchFn (sdrk_host_pipeline.hip)

inline int exec_device_frames(CheckFn check, LaunchFn launch, sdrk_plan* p, const void* d_in, size_t n_frames, size_t frame_stride,
                              float* d_out_db, void* stream) {
    int st = check(p, d_in, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK || n_frames == 0) return st;
    HIP_TRY(hipSetDevice(p->device));
    return launch(p, d_in, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, stream ? static_cast<hipStream_t>(stream) : p->stream);
}

inline int exec_device_frames_timed_each(CheckFn check, LaunchFn launch, sdrk_plan* p, const void* d_in, size_t n_frames,
                                         size_t frame_stride, float* d_out_db, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check(p, d_in, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    st = timed_each(p, launches, each_ms,
                    [&] { return launch(p, d_in, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, p->stream); });
    return st == SDRK_OK ? fused_check(p) : st;
}

// The HostIo of a float32 mode: samples of in_elem bytes, a frame reading in_span of them (0: nfft), float32 rows (EPI_LOGPSD)
// or complex64 out.  Through the copy engines unless the caller sets a zero-copy range.
inline HostIo frames_io(size_t in_elem, size_t in_span, LaunchFn launch, int epilogue) {
    HostIo io;
    io.in_elem = in_elem;
    io.out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    io.epilogue = epilogue;
    io.precision = 32;
    io.in_span = in_span;
    io.launch = launch;
    return io;
}

// ---- ci16_api.hip ----
// One transform of a float32 plan on int16 I,Q input (4 bytes per sample), the ci16 form of plan_launch: a LaunchFn.
int launch_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream);

// One transform of a float32 plan on 8-bit I,Q input (2 bytes per sample; fmt: SDRK_IQ8_SIGNED / _UNSIGNED), the LaunchFn
// that has a format bound into it, and the refusal every 8-bit entry point makes first: a format that is neither, a float64 plan
// (a NULL plan is left to the checks behind it).
int launch_ci8(sdrk_plan* p, const void* d_in, int fmt, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream);
LaunchFn launch_ci8_fn(int fmt);
int check_iq8_format(const sdrk_plan* p, int fmt);

// ---- pfb_api.hip ----
// One polyphase-filter-bank transform of a float32 plan on a raw complex64 stream (taps * nfft samples per frame), and the
// same on interleaved int16 I,Q (4 bytes per sample): LaunchFns.  N = 4096 is one launch; every other length folds chunks of
// frames into the plan's PFB staging, at most 64 MiB, and runs the plan's transform on that.
int launch_pfb(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream);
int launch_pfb_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream);
// The same on interleaved 8-bit I,Q (2 bytes per sample) of format fmt (SDRK_IQ8_*, checked by the caller): the LaunchFn with
// the format bound into it, as launch_ci8_fn.
LaunchFn launch_pfb_iq8_fn(int fmt);
// What every PFB entry point refuses: float64 or windowed plans; for any transform, per frame or integrated, also a plan
// with no prototype set (check_pfb_ready); and for a per-frame one zero frames, NULL pointers, stride 0 with more than one
// frame (the integrated calls leave those to integrate_call.h).
int check_pfb_plan(const sdrk_plan* p);
int check_pfb_ready(const sdrk_plan* p);
int check_pfb_exec(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out);

}  // namespace sdrk_host

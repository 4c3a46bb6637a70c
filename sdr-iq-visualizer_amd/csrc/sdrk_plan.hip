// sdrk_plan.hip — plans of include/sdrk.h (sdrk_plan_*, sdrk_exec_device*): creation and teardown, the tables a plan carries,
// and plan_launch, the one place that picks the kernel for a frame length (fft4096.hip, fft_lds.hip, fft_small.hip,
// fft_tiled2.hip, fft_fused64k.hip, bluestein.hip), with the one-at-a-time gate of the fused N = 65536 launch.  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <new>
#include <vector>

#include "f4k_split.h"
#include "kernels.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace sdrk_host {

// The chirp-z path's multiplies riding on an inner (power-of-two, two-pass) transform's row-pass stores: epilogue EPI_BLU_* with
// this table, row length, and the OUTER plan's eps / shift (kernels.h).
struct EpiArgs {
    const float2* tab = nullptr;
    int n_out = 0;
    float eps = 0.0f;
    int shift = 0;
    size_t in_valid = 0;   // samples that exist per input frame (0 = all): LaunchArgs::in_valid
};

namespace {

// exp(-2 pi i m / n) in double, rounded once to float32.
float2 twiddle(double m, double n) {
    const double a = -2.0 * M_PI * m / n;
    return make_float2((float)std::cos(a), (float)std::sin(a));
}

// Optional roctx ranges around every transform (SDRK_ROCTX=1; SURVEY.md §5 "tracing"): nfft, frames, stride, epilogue, so
// that a rocprofv3 --marker-trace names the calls the kernels belong to.  The library is dlopen'ed on first use — nothing is
// linked, and without the variable the cost is one load of a static.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* env = getenv("SDRK_ROCTX");
        if (!env || env[0] != '1') return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
struct RoctxRange {
    bool on = false;
    RoctxRange(const sdrk_plan* p, size_t n_frames, size_t stride, int epilogue);
    ~RoctxRange();
};
Roctx& roctx() {
    static Roctx r;
    return r;
}

// One fused N = 65536 launch at a time per device (see plan_launch_impl).  The events live for the life of the process.
struct FusedGate {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool recorded = false;
};
FusedGate& fused_gate(int device) {
    static FusedGate gates[64];
    FusedGate& g = gates[device >= 0 && device < 64 ? device : 0];
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.ev && hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) g.ev = nullptr;
    return g;
}

int plan_launch_impl(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, void* d_out,
                     int epilogue, hipStream_t stream, float* d_mip, bool* mip_written, const EpiArgs* epi, size_t call_frames);

}  // namespace

// Does a launch of n_frames frames of this plan take the persistent N = 65536 kernel?
bool takes_fused(const sdrk_plan* p, size_t n_frames) {
    return p->fused64k || (p->fused_auto && !p->fused_broken && n_frames >= FUSED_AUTO_MIN_FRAMES);
}

// d_mip / mip_written: see LaunchArgs (kernels.h) — *mip_written tells whether the launch wrote the by-16 companion rows.
int plan_launch(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, void* d_out,
                int epilogue, hipStream_t stream, float* d_mip, bool* mip_written, const EpiArgs* epi, size_t call_frames) {
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "float32 transform requested of a float64 plan");
    RoctxRange range(p, n_frames, frame_stride, epilogue);
    if (mip_written) *mip_written = false;
    return plan_launch_impl(p, d_iq, n_frames, frame_stride, d_out, epilogue, stream, d_mip, mip_written, epi,
                            call_frames > n_frames ? call_frames : n_frames);
}

namespace {

int plan_launch_impl(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, void* d_out,
                     int epilogue, hipStream_t stream, float* d_mip, bool* mip_written, const EpiArgs* epi, size_t call_frames) {
    sdrk::LaunchArgs a = plan_launch_args(p, d_iq, n_frames, frame_stride, d_out, epilogue, stream);
    a.d_mip = d_mip;
    a.mip_written = mip_written;
    a.d_scratch = p->d_scratch;
    a.scratch_frames = p->scratch_frames;
    a.d_twiddle_2p = p->d_tw_2p;
    if (epi) {
        if (!p->tiled2 || p->stream2 || epilogue < sdrk::EPI_BLU_MUL)
            return fail(SDRK_ERR_INVALID, "chirp-z epilogues need a serial two-pass inner plan");
        a.d_epi_tab = epi->tab;
        a.epi_n_out = epi->n_out;
        a.eps = epi->eps;
        a.shift = epi->shift;
        a.in_valid = epi->in_valid;
    } else if (epilogue >= sdrk::EPI_BLU_MUL) {
        return fail(SDRK_ERR_INVALID, "epilogue %d needs its table", epilogue);
    }
    if (p->col_cus > 0 && p->stream2) {
        a.stream2 = p->stream2;
        a.ev_fork = p->ev_fork;
        for (int h = 0; h < 2; ++h) { a.ev_col[h] = p->ev_col[h]; a.ev_row[h] = p->ev_row[h]; }
        a.col_cus = p->col_cus;
        a.row_cus = p->row_cus;
    }
    hipError_t e = hipSuccess;
    if (p->blu_inner) {
        const int N = p->nfft, M = p->blu_m;
        const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
        for (size_t f0 = 0; f0 < n_frames; f0 += p->blu_frames) {
            const size_t nf = n_frames - f0 < p->blu_frames ? n_frames - f0 : p->blu_frames;
            if (sdrk::blu_fused_supports(M)) {   // one kernel, one pass over HBM, instead of five
                e = sdrk::launch_blu_fused(static_cast<const float2*>(d_iq) + f0 * frame_stride, frame_stride, nf, N, M,
                                           p->d_window, p->d_blu_chirp, p->d_blu_bspec, p->blu_inner->d_twiddle,
                                           p->eps, p->shift, epilogue,
                                           static_cast<char*>(d_out) + f0 * (size_t)N * out_elem, p->num_cus, stream);
                if (e != hipSuccess) break;
                continue;
            }
            const bool fused_multiplies = p->blu_inner->tiled2 && !p->blu_inner->stream2;
            // (the pre-multiply writes only the N values that exist; the first col pass reads the padding as zeros by bounds check)
            e = sdrk::launch_blu_pre(static_cast<const float2*>(d_iq) + f0 * frame_stride, frame_stride, nf, N, M,
                                     p->d_window, p->d_blu_chirp, p->d_blu_a, p->num_cus, stream, fused_multiplies);
            if (e != hipSuccess) break;
            if (fused_multiplies) {
                // five launches instead of seven (round 6): the filter multiply (+ conjugation) rides on the stores of the first
                // inner transform's row pass, the post-multiply / crop to N / fftshift / log on the second one's, which writes the
                // caller's rows directly (fft_tiled2.hip, EPI_BLU_*): 16 M + 8 M + 12 N bytes per frame fewer through the fabric
                EpiArgs mul, post;
                mul.tab = p->d_blu_bspec;
                mul.in_valid = (size_t)N;
                post.tab = p->d_blu_chirp;
                post.n_out = N;
                post.eps = p->eps;
                post.shift = p->shift;
                int st = plan_launch(p->blu_inner, p->d_blu_a, nf, (size_t)M, p->d_blu_b, sdrk::EPI_BLU_MUL, stream, nullptr, nullptr, &mul);
                if (st != SDRK_OK) return st;
                st = plan_launch(p->blu_inner, p->d_blu_b, nf, (size_t)M, static_cast<char*>(d_out) + f0 * (size_t)N * out_elem,
                                 epilogue == sdrk::EPI_LOGPSD ? sdrk::EPI_BLU_POST_LOG : sdrk::EPI_BLU_POST_C64, stream, nullptr, nullptr, &post);
                if (st != SDRK_OK) return st;
                continue;
            }
            int st = plan_launch(p->blu_inner, p->d_blu_a, nf, (size_t)M, p->d_blu_b, sdrk::EPI_COMPLEX, stream);
            if (st != SDRK_OK) return st;
            e = sdrk::launch_blu_mul(p->d_blu_b, p->d_blu_bspec, nf, M, p->d_blu_a, p->num_cus, stream);
            if (e != hipSuccess) break;
            st = plan_launch(p->blu_inner, p->d_blu_a, nf, (size_t)M, p->d_blu_b, sdrk::EPI_COMPLEX, stream);
            if (st != SDRK_OK) return st;
            e = sdrk::launch_blu_post(p->d_blu_b, p->d_blu_chirp, nf, N, M, p->eps, p->shift, epilogue,
                                      static_cast<char*>(d_out) + f0 * (size_t)N * out_elem, p->num_cus, stream);
            if (e != hipSuccess) break;
        }
    } else if (p->nfft == 4096) {
        // A long call goes out as back-to-back launches of about F4K_SPLIT_FRAMES frames each (see there): the frames are
        // independent, so the rows are the same bits whichever launch computes them.
        // In the ticket order (f4k_ticket.h) the launches draw from the plan's heads, one launch after the other: a call on
        // another stream than the last one waits for it, and the host's bases move with every launch enqueued.
        const size_t max_blocks = sdrk::f4k_max_blocks(p->num_cus);
        const bool ticket = p->d_f4k_heads && f4k_ticket_takes(p->f4k_order, max_blocks, n_frames, F4K_TICKET_DEFAULT);
        size_t parts = p->f4k_parts ? p->f4k_parts : (ticket ? f4k_ticket_parts(n_frames) : f4k_split_parts(n_frames));
        if (p->f4k_parts && parts > n_frames) parts = n_frames ? n_frames : 1;
        const size_t per = (n_frames + parts - 1) / parts;
        const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
        if (ticket && p->f4k_recorded && p->f4k_last != stream) e = hipStreamWaitEvent(stream, p->f4k_ev, 0);
        for (size_t f0 = 0; f0 < n_frames && e == hipSuccess; f0 += per) {
            a.d_iq = static_cast<const float2*>(d_iq) + f0 * frame_stride;
            a.d_out = static_cast<char*>(d_out) + f0 * (size_t)4096 * out_elem;
            a.n_frames = n_frames - f0 < per ? n_frames - f0 : per;
            if (ticket) {
                const unsigned grid = f4k_ticket_grid(max_blocks, a.n_frames);
                if (p->f4k_rot_heads && p->f4k_rot_ahead == F4K_AHEAD_2FLOW) {
                    e = sdrk::launch_fft4096_flow2(a, p->d_f4k_rot, p->f4k_rot_heads, grid);
                } else if (p->f4k_rot_heads && p->f4k_rot_ahead == F4K_AHEAD_2TOP) {
                    e = sdrk::launch_fft4096_rot2(a, p->d_f4k_rot, p->f4k_rot_heads, grid);
                } else if (p->f4k_rot_heads) {
                    e = sdrk::launch_fft4096_rot(a, p->d_f4k_rot, p->f4k_rot_heads, grid);
                } else {
                    e = sdrk::launch_fft4096_ticket(a, p->d_f4k_heads, p->f4k_bases, p->f4k_form, grid);
                    if (e == hipSuccess) f4k_ticket_advance(p->f4k_form, p->f4k_bases, a.n_frames, grid);
                }
            } else {
                e = sdrk::launch_fft4096(a);
            }
        }
        if (ticket && e == hipSuccess) {
            e = hipEventRecord(p->f4k_ev, stream);
            p->f4k_last = stream;
            p->f4k_recorded = true;
        }
    } else if (sdrk::fft_lds_supports(p->nfft))
        e = sdrk::launch_fft_lds(a);
    else if (p->nfft < 4096)
        e = sdrk::launch_fft_small(a);
    else if (takes_fused(p, call_frames) && !d_mip && epilogue <= sdrk::EPI_COMPLEX) {
        // The persistent grid needs every one of its workgroups resident at the same time; two such grids on two streams could
        // each hold part of the device and wait for the rest.  One at a time per device: each launch waits for the one before.
        FusedGate& gate = fused_gate(p->device);
        std::lock_guard<std::mutex> lk(gate.mu);
        if (gate.ev && gate.last_stream != stream && gate.recorded) e = hipStreamWaitEvent(stream, gate.ev, 0);
        if (e == hipSuccess) e = sdrk::launch_fused64k(a, p->d_fused_ring, p->d_fused_ctrl);
        if (e == hipSuccess)   // error word, timeout record and the number of sets formed -> pinned mailbox
            e = hipMemcpyAsync(p->h_fused_err + 16 * (p->fused_launches++ % FUSED_MAILBOX), p->d_fused_ctrl,
                               16 * sizeof(unsigned), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && gate.ev) {
            e = hipEventRecord(gate.ev, stream);
            gate.last_stream = stream;
            gate.recorded = true;
        }
        ++p->fused_pending;
    } else if (p->tiled2)
        e = sdrk::launch_fft_tiled2(a);
    else
        return fail(SDRK_ERR_UNSUPPORTED, "no kernel for nfft=%d", p->nfft);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

RoctxRange::RoctxRange(const sdrk_plan* p, size_t n_frames, size_t stride, int epilogue) {
    Roctx& r = roctx();
    if (!r.push) return;
    char label[160];
    snprintf(label, sizeof label, "sdrk.plan_launch nfft=%d frames=%zu stride=%zu %s dev=%d", p->nfft, n_frames, stride,
             epilogue == sdrk::EPI_LOGPSD ? "logpsd" : (epilogue == sdrk::EPI_COMPLEX ? "complex" : "chirp-z stage"), p->device);
    r.push(label);
    on = true;
}
RoctxRange::~RoctxRange() {
    if (on) roctx().pop();
}

}  // namespace

// After a stream sync: did any fused N=65536 launch report an internal wait timeout?
int fused_check(sdrk_plan* p) {
    if (!p->h_fused_err || p->fused_pending == 0) return SDRK_OK;
    // mailbox entry: [0] sets formed + 1 (0 = unused entry), [1] error flag, [2..5] record of the first timeout
    const unsigned want = sdrk::fused64k_sets(p->num_cus);
    unsigned bad = 0, rec[16] = {0};
    const unsigned pending = p->fused_pending < FUSED_MAILBOX ? p->fused_pending : FUSED_MAILBOX;
    for (unsigned k = 0; k < pending; ++k) {            // the launches since the last check (older ones were overwritten)
        const unsigned* r = p->h_fused_err + 16 * ((p->fused_launches - 1 - k) % FUSED_MAILBOX);
        const unsigned code = r[1] ? r[1] : (r[0] != want ? 9u : 0u);
        if (code) { memcpy(rec, r, sizeof rec); bad = code; }
    }
    p->fused_pending = 0;
    if (bad && p->fused_auto) p->fused_broken = true;   // an auto plan takes the two tiled launches from here on
    if (bad)
        return fail(SDRK_ERR_HIP, "fused N=65536 kernel reported an internal synchronisation error (code %u; %u of %u sets formed; "
                    "word %u held %u, wanted %u, site %u)", bad, rec[0], want, rec[2], rec[3], rec[4], rec[5]);
    return SDRK_OK;
}

// A plan serves the entry points of its own precision only (sdrk_plan_create: float32; sdrk_plan_create_f64: float64).
int check_precision(const sdrk_plan* p, int precision) {
    if (p->precision == precision) return SDRK_OK;
    return fail(SDRK_ERR_INVALID, "this is a float%d plan (sdrk_plan_create%s) and the call is a float%d entry point%s",
                p->precision, p->precision == 64 ? "_f64" : "", precision,
                precision == 64 ? " (sdrk_*_f64)" : ": use the sdrk_*_f64 entry points");
}

int check_exec_args(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride,
                    const void* out, int precision) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (int st = check_precision(p, precision); st != SDRK_OK) return st;
    if (n_frames == 0) return SDRK_OK;
    if (!in || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (frame_stride == 0 && n_frames > 1)
        return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1 for more than one frame");
    return SDRK_OK;
}

int check_exec_f32(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out) {
    return check_exec_args(p, in, n_frames, frame_stride, out, 32);
}

}  // namespace sdrk_host

extern "C" {

int sdrk_plan_create(int device, int nfft, size_t max_batch, int window_kind, const float* window,
                     float eps, int shift, sdrk_plan** out) {
    return sdrk_plan_create_ex(device, nfft, max_batch, window_kind, window, eps, shift, 0u, out);
}

int sdrk_plan_create_ex(int device, int nfft, size_t max_batch, int window_kind, const float* window,
                        float eps, int shift, unsigned flags, sdrk_plan** out) {
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (flags & ~(unsigned)(SDRK_PLAN_FUSED64K | SDRK_PLAN_OVERLAP_PASSES | SDRK_PLAN_TUNE_STAGING | SDRK_PLAN_TILED64K))
        return fail(SDRK_ERR_INVALID, "unknown plan flags 0x%x", flags);
    if ((flags & SDRK_PLAN_TILED64K) && (flags & SDRK_PLAN_FUSED64K))
        return fail(SDRK_ERR_INVALID, "SDRK_PLAN_TILED64K and SDRK_PLAN_FUSED64K exclude each other");
    if ((flags & SDRK_PLAN_TILED64K) && nfft != 65536)
        return fail(SDRK_ERR_INVALID, "SDRK_PLAN_TILED64K applies to nfft = 65536 only (got %d)", nfft);
    if ((flags & SDRK_PLAN_OVERLAP_PASSES) && (!is_pow2(nfft) || nfft < (1 << 15)))
        return fail(SDRK_ERR_INVALID, "SDRK_PLAN_OVERLAP_PASSES applies to power-of-two nfft >= 32768 (got %d)", nfft);
    if ((flags & SDRK_PLAN_OVERLAP_PASSES) && (flags & SDRK_PLAN_FUSED64K))
        return fail(SDRK_ERR_INVALID, "SDRK_PLAN_OVERLAP_PASSES and SDRK_PLAN_FUSED64K exclude each other");
    if ((flags & SDRK_PLAN_FUSED64K) && nfft != 65536)
        return fail(SDRK_ERR_INVALID, "SDRK_PLAN_FUSED64K applies to nfft = 65536 only (got %d)", nfft);
    if (nfft < 2 || nfft > (1 << SDRK_MAX_LOG2_NFFT) || (!is_pow2(nfft) && nfft > (1 << (SDRK_MAX_LOG2_NFFT - 1))))
        return fail(SDRK_ERR_INVALID, "nfft=%d: must be in [2, 2^%d] (powers of two) or [2, 2^%d] (any other length)",
                    nfft, SDRK_MAX_LOG2_NFFT, SDRK_MAX_LOG2_NFFT - 1);
    if (max_batch == 0) return fail(SDRK_ERR_INVALID, "max_batch must be >= 1");
    if (window_kind < SDRK_WINDOW_RECT || window_kind > SDRK_WINDOW_CUSTOM)
        return fail(SDRK_ERR_INVALID, "unknown window_kind %d", window_kind);
    if (window_kind == SDRK_WINDOW_CUSTOM && !window)
        return fail(SDRK_ERR_INVALID, "SDRK_WINDOW_CUSTOM needs a window pointer");
    if (!(eps >= 0.0f)) return fail(SDRK_ERR_INVALID, "eps must be >= 0");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SDRK_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only",
                    device, prop.gcnArchName);

    sdrk_plan* p = new (std::nothrow) sdrk_plan();
    if (!p) return fail(SDRK_ERR_NOMEM, "out of host memory");
    p->device = device;
    p->nfft = nfft;
    p->max_batch = max_batch;
    p->eps = eps;
    p->shift = shift ? 1 : 0;
    p->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (const char* env = getenv("SDRK_NUM_CUS")) {   // size the persistent grids as for a smaller device (a partition
        long v = atol(env);                           // mode, or the tests of the grid-smaller-than-work paths); selects no kernel
        if (v >= 1 && v < p->num_cus) p->num_cus = (int)v;
    }

#define PLAN_TRY(expr)                                                                     \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            int s__ = fail(e__ == hipErrorOutOfMemory ? SDRK_ERR_NOMEM : SDRK_ERR_HIP,     \
                           "%s failed: %s", #expr, hipGetErrorString(e__));                \
            sdrk_plan_destroy(p);                                                          \
            return s__;                                                                    \
        }                                                                                  \
    } while (0)

    PLAN_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    PLAN_TRY(hipEventCreate(&p->ev0));
    PLAN_TRY(hipEventCreate(&p->ev1));

    // window
    if (window_kind != SDRK_WINDOW_RECT) {
        std::vector<float> w(nfft);
        if (window_kind == SDRK_WINDOW_HANN) {
            // numpy.hanning(M): 0.5 - 0.5 cos(2 pi n / (M-1)); M == 1 would be [1.0]
            for (int n = 0; n < nfft; ++n)
                w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)(nfft - 1)));
        } else {
            memcpy(w.data(), window, sizeof(float) * nfft);
        }
        PLAN_TRY(hipMalloc((void**)&p->d_window, sizeof(float) * nfft));
        PLAN_TRY(hipMemcpy(p->d_window, w.data(), sizeof(float) * nfft, hipMemcpyHostToDevice));
    }
    if (!is_pow2(nfft)) {
        // Bluestein: inner power-of-two plan of size M >= 2N-1, chirp table, spectrum of the chirp filter
        int M = 1;
        while (M < 2 * nfft - 1) M <<= 1;
        p->blu_m = M;
        // work buffers of the five-pass form: 128 MiB each; the one-kernel form (M <= 16384) needs none and takes any batch whole
        const bool one_kernel = sdrk::blu_fused_supports(M);
        size_t frames = ((size_t)128 << 20) / ((size_t)M * sizeof(float2));
        if (frames < 1) frames = 1;
        if (frames > max_batch || one_kernel) frames = max_batch;
        p->blu_frames = frames;
        int st2 = sdrk_plan_create(device, M, frames, SDRK_WINDOW_RECT, nullptr, 0.0f, 0, &p->blu_inner);
        if (st2 != SDRK_OK) { sdrk_plan_destroy(p); return st2; }
        std::vector<float2> c(nfft), b(M, make_float2(0.f, 0.f));
        for (long long n = 0; n < nfft; ++n) {
            const long long r = (n * n) % (2LL * nfft);          // n^2 mod 2N keeps the phase exact
            const double ang = M_PI * (double)r / (double)nfft;
            c[n] = make_float2((float)std::cos(ang), (float)std::sin(ang));
            b[n] = c[n];
            if (n) b[M - n] = c[n];
        }
        PLAN_TRY(hipMalloc((void**)&p->d_blu_chirp, sizeof(float2) * nfft));
        PLAN_TRY(hipMemcpy(p->d_blu_chirp, c.data(), sizeof(float2) * nfft, hipMemcpyHostToDevice));
        PLAN_TRY(hipMalloc((void**)&p->d_blu_a, (one_kernel ? 1 : frames) * (size_t)M * sizeof(float2)));   // (also carries b[] to its transform below)
        if (!one_kernel) PLAN_TRY(hipMalloc((void**)&p->d_blu_b, frames * (size_t)M * sizeof(float2)));
        PLAN_TRY(hipMalloc((void**)&p->d_blu_bspec, (size_t)M * sizeof(float2)));
        PLAN_TRY(hipMemcpy(p->d_blu_a, b.data(), sizeof(float2) * M, hipMemcpyHostToDevice));
        st2 = plan_launch(p->blu_inner, p->d_blu_a, 1, (size_t)M, p->d_blu_bspec, sdrk::EPI_COMPLEX, p->stream);
        if (st2 != SDRK_OK) { sdrk_plan_destroy(p); return st2; }
        PLAN_TRY(hipStreamSynchronize(p->stream));
        // window (if any) was uploaded above; nothing else of the power-of-two setup applies
        *out = p;
        return SDRK_OK;
    }
    // twiddles of the in-LDS transform: W_N for N <= 16384 (fft4096.hip, fft_lds.hip, fft_small.hip); the
    // two-pass plans carry their own tables below.  (N = 32768 also fits one CU — 32 points per thread, float-plane
    // LDS exchanges — and was built and measured in round 3: no faster than the two passes)
    if (nfft <= 16384) {
        std::vector<float2> t(nfft);
        for (int m = 0; m < nfft; ++m) t[m] = twiddle(m, nfft);
        PLAN_TRY(hipMalloc((void**)&p->d_twiddle, sizeof(float2) * nfft));
        PLAN_TRY(hipMemcpy(p->d_twiddle, t.data(), sizeof(float2) * nfft, hipMemcpyHostToDevice));
        if (nfft == 4096) {
            // The heads of the ticket order, one 128-byte line each.  They start a few hundred tickets short of the 32-bit
            // wrap: every plan that lives for more than a launch or two crosses it, so the wrap is no rare path.
            // SDRK_F4K_ORDER: "stride" / "ticket", either loop at any size (f4k_ticket_takes); SDRK_F4K_TICKET_FORM:
            // "<heads>x<frames per ticket>" or "rot<heads>" (f4k_rot.h), A/B work; SDRK_F4K_ROT_AHEAD: "3" / "2top" / "2flow", the rot
            // form's look-ahead
            const F4kChoice choice = f4k_choice(getenv("SDRK_F4K_ORDER"), getenv("SDRK_F4K_TICKET_FORM"), getenv("SDRK_F4K_ROT_AHEAD"));
            p->f4k_order = choice.order;
            p->f4k_form = choice.form;
            p->f4k_rot_heads = choice.rot_heads;
            p->f4k_rot_ahead = choice.rot_ahead;
            if (const char* env = getenv("SDRK_F4K_PARTS")) {   // launches per call, either order: developer use (tools/f4k_ticket_launches.py)
                long v = atol(env);
                if (v >= 1 && v <= 4096) p->f4k_parts = (size_t)v;
            }
            PLAN_TRY(hipMalloc((void**)&p->d_f4k_rot, F4K_ROT_WORDS * sizeof(uint32_t)));
            const std::vector<uint32_t> rot0(F4K_ROT_WORDS, 0u);
            PLAN_TRY(hipMemcpy(p->d_f4k_rot, rot0.data(), rot0.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            std::vector<uint32_t> h(F4K_TICKET_MAX_HEADS * F4K_TICKET_HEAD_WORDS, 0u);
            for (unsigned x = 0; x < F4K_TICKET_MAX_HEADS; ++x) h[x * F4K_TICKET_HEAD_WORDS] = p->f4k_bases.base[x] = 0xFFFFFE00u;
            PLAN_TRY(hipMalloc((void**)&p->d_f4k_heads, h.size() * sizeof(uint32_t)));
            PLAN_TRY(hipMemcpy(p->d_f4k_heads, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            PLAN_TRY(hipEventCreateWithFlags(&p->f4k_ev, hipEventDisableTiming));
        }
    } else {
        // scratch between the two passes: up to 192 MiB of complex64 frames.  It has to stay in the 256 MiB
        // Infinity Cache between the col pass that writes it and the row pass that reads it, and per-launch
        // costs favour few large chunks: measured on config 3 (N = 65536), 96 / 192 / 288 / 384 / 576 MiB give
        // 6.15 / 5.61 / 5.99 / 6.95 / 7.23 ms (the step past 256 MiB is the cache being outrun).
        size_t scratch_mb = 192;
        if (const char* env = getenv("SDRK_SCRATCH_MB")) {  // tuning knob (developer use)
            long v = atol(env);
            if (v >= 1 && v <= 65536) scratch_mb = (size_t)v;
        }
        size_t frames = (scratch_mb << 20) / ((size_t)nfft * sizeof(float2));
        if (frames < 1) frames = 1;
        if (frames > max_batch) frames = max_batch;
        p->scratch_frames = frames;
        PLAN_TRY(hipMalloc((void**)&p->d_scratch, frames * (size_t)nfft * sizeof(float2)));
        int la = 0, lm = 0;
        if (!sdrk::fft_tiled2_split(nfft, &la, &lm)) {
            sdrk_plan_destroy(p);
            return fail(SDRK_ERR_UNSUPPORTED, "no kernel for nfft=%d", nfft);
        }
        const int A = 1 << la, M = 1 << lm, TA = A / 16;
        std::vector<float2> t((size_t)4096 + (size_t)TA * M + (size_t)M * 16);
        for (int m = 0; m < A; ++m) t[m] = twiddle(m, A);
        for (int m = 0; m < M; ++m) t[2048 + m] = twiddle(m, M);
        for (int tau = 0; tau < TA; ++tau)
            for (int m = 0; m < M; ++m) t[4096 + (size_t)tau * M + m] = twiddle((double)m * tau, (double)nfft);
        for (int m = 0; m < M; ++m)
            for (int q = 0; q < 16; ++q)
                t[4096 + (size_t)TA * M + (size_t)m * 16 + q] = twiddle((double)m * TA * q, (double)nfft);
        PLAN_TRY(hipMalloc((void**)&p->d_tw_2p, sizeof(float2) * t.size()));
        PLAN_TRY(hipMemcpy(p->d_tw_2p, t.data(), sizeof(float2) * t.size(), hipMemcpyHostToDevice));
        p->tiled2 = true;
        if (flags & SDRK_PLAN_OVERLAP_PASSES) {
            // second stream, the events that chain the two, and the split of the CUs between the roles: 3/4 of
            // the device's CUs worth of col workgroups, 1/2 worth of row workgroups (the least slow of the splits
            // tried; SDRK_OVL_COL_CUS / SDRK_OVL_ROW_CUS override it for the sweep in tools/overlap_probe.py)
            PLAN_TRY(hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking));
            PLAN_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
            for (int h = 0; h < 2; ++h) {
                PLAN_TRY(hipEventCreateWithFlags(&p->ev_col[h], hipEventDisableTiming));
                PLAN_TRY(hipEventCreateWithFlags(&p->ev_row[h], hipEventDisableTiming));
            }
            p->col_cus = p->num_cus * 3 / 4 > 0 ? p->num_cus * 3 / 4 : 1;
            p->row_cus = p->num_cus / 2 > 0 ? p->num_cus / 2 : 1;
            if (const char* c = getenv("SDRK_OVL_COL_CUS")) { long v = atol(c); if (v >= 1 && v <= 4096) p->col_cus = (int)v; }
            if (const char* c = getenv("SDRK_OVL_ROW_CUS")) { long v = atol(c); if (v >= 1 && v <= 4096) p->row_cus = (int)v; }
        }
    }
    // Single-launch, XCD-resident form of N = 65536 (fft_fused64k.hip); shares the tables of the tiled path.  Forced by
    // SDRK_PLAN_FUSED64K; otherwise the default for launches of FUSED_AUTO_MIN_FRAMES frames or more, unless SDRK_PLAN_TILED64K
    // or SDRK_PLAN_OVERLAP_PASSES asks for the two launches or the device's CUs do not make whole sets (32 workgroups per XCD).
    // (A CU count that misdescribes the device — SDRK_NUM_CUS = 96 on eight XCDs — makes the first persistent launch fail its
    // set formation; the plan then falls back for good, which is how the suite tests the fall-back.)
    const bool fused_auto = nfft == 65536 && !(flags & (SDRK_PLAN_FUSED64K | SDRK_PLAN_TILED64K | SDRK_PLAN_OVERLAP_PASSES)) &&
                            p->num_cus >= 32 && p->num_cus % 32 == 0;
    if ((flags & SDRK_PLAN_FUSED64K) || fused_auto) {
        p->fused64k = (flags & SDRK_PLAN_FUSED64K) != 0;
        p->fused_auto = fused_auto;
        PLAN_TRY(hipMalloc(&p->d_fused_ring, sdrk::fused64k_ring_bytes()));
        PLAN_TRY(hipMalloc((void**)&p->d_fused_ctrl, sdrk::fused64k_ctrl_words() * sizeof(unsigned)));
        PLAN_TRY(hipHostMalloc((void**)&p->h_fused_err, FUSED_MAILBOX * 16 * sizeof(unsigned), hipHostMallocDefault));
        memset(p->h_fused_err, 0, FUSED_MAILBOX * 16 * sizeof(unsigned));
    }
#undef PLAN_TRY
    if (flags & SDRK_PLAN_TUNE_STAGING) {
        st = tune_staging(p);
        if (st != SDRK_OK) { sdrk_plan_destroy(p); return st; }
    }
    *out = p;
    return SDRK_OK;
}

int sdrk_plan_staging_probe(const sdrk_plan* p, float* probe_ms, int capacity, int* n) {
    if (!p || !n) return fail(SDRK_ERR_INVALID, "plan or n is NULL");
    *n = p->staging_probe_n;
    for (int i = 0; i < p->staging_probe_n && i < capacity && probe_ms; ++i) probe_ms[i] = p->staging_probe_ms[i];
    return SDRK_OK;
}

int sdrk_plan_fused_status(const sdrk_plan* p, unsigned* launches, int* fallen_back) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (launches) *launches = p->fused_launches;
    if (fallen_back) *fallen_back = p->fused_broken ? 1 : 0;
    return SDRK_OK;
}

int sdrk_plan_destroy(sdrk_plan* p) {
    if (!p) return SDRK_OK;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (p->stream2) { (void)hipStreamSynchronize(p->stream2); (void)hipStreamDestroy(p->stream2); }
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    for (int h = 0; h < 2; ++h) {
        if (p->ev_col[h]) (void)hipEventDestroy(p->ev_col[h]);
        if (p->ev_row[h]) (void)hipEventDestroy(p->ev_row[h]);
    }
    if (p->d_window) (void)hipFree(p->d_window);
    if (p->d_window64) (void)hipFree(p->d_window64);
    if (p->d_tw64) (void)hipFree(p->d_tw64);
    if (p->d_scratch64) (void)hipFree(p->d_scratch64);
    if (p->d_twiddle) (void)hipFree(p->d_twiddle);
    if (p->d_tw_2p) (void)hipFree(p->d_tw_2p);
    if (p->d_scratch) (void)hipFree(p->d_scratch);
    if (p->blu_inner) (void)sdrk_plan_destroy(p->blu_inner);
    if (p->d_blu_chirp) (void)hipFree(p->d_blu_chirp);
    if (p->d_blu_bspec) (void)hipFree(p->d_blu_bspec);
    if (p->d_blu_a) (void)hipFree(p->d_blu_a);
    if (p->d_blu_b) (void)hipFree(p->d_blu_b);
    if (p->h_small_in) (void)hipHostFree(p->h_small_in);
    if (p->h_small_out) (void)hipHostFree(p->h_small_out);
    if (p->h_small_flag) (void)hipHostFree(p->h_small_flag);
    if (p->d_fused_ring) (void)hipFree(p->d_fused_ring);
    if (p->d_fused_ctrl) (void)hipFree(p->d_fused_ctrl);
    if (p->h_fused_err) (void)hipHostFree(p->h_fused_err);
    if (p->d_in) (void)hipFree(p->d_in);
    if (p->d_out) (void)hipFree(p->d_out);
    if (p->d_feat) (void)hipFree(p->d_feat);
    p->ci16.release();
    p->integ.release();
    if (p->d_pfb_h) (void)hipFree(p->d_pfb_h);
    p->pfb.release();
    if (p->d_fir_h) (void)hipFree(p->d_fir_h);
    if (p->d_beam_h) (void)hipFree(p->d_beam_h);
    if (p->d_real_win) (void)hipFree(p->d_real_win);
    if (p->d_real_tab) (void)hipFree(p->d_real_tab);
    p->real.release();
    if (p->f4k_recorded) (void)hipEventSynchronize(p->f4k_ev);   // a ticketed launch on a caller's stream still draws from the heads
    if (p->d_f4k_heads) (void)hipFree(p->d_f4k_heads);
    if (p->d_f4k_rot) (void)hipFree(p->d_f4k_rot);
    if (p->f4k_ev) (void)hipEventDestroy(p->f4k_ev);
    if (p->s_h2d) (void)hipStreamSynchronize(p->s_h2d);
    if (p->s_d2h) (void)hipStreamSynchronize(p->s_d2h);
    for (auto& sl : p->slot) {
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.d_in) (void)hipFree(sl.d_in);
        if (sl.d_out) (void)hipFree(sl.d_out);
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_k) (void)hipEventDestroy(sl.ev_k);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (p->s_h2d) (void)hipStreamDestroy(p->s_h2d);
    if (p->s_d2h) (void)hipStreamDestroy(p->s_d2h);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return SDRK_OK;
}

int sdrk_plan_nfft(const sdrk_plan* p) { return p ? p->nfft : fail(SDRK_ERR_INVALID, "plan is NULL"); }
int sdrk_plan_device(const sdrk_plan* p) { return p ? p->device : fail(SDRK_ERR_INVALID, "plan is NULL"); }

int sdrk_exec_device(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride,
                     float* d_out_db, void* stream) {
    return exec_device_frames(check_exec_f32, launch_f32, p, d_iq, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_plan_sync(sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return fused_check(p);
}

int sdrk_exec_device_timed(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride,
                           float* d_out_db, int launches, float* elapsed_ms) {
    if (!elapsed_ms || launches < 1) return fail(SDRK_ERR_INVALID, "bad launches/elapsed_ms");
    int st = check_exec_args(p, d_iq, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    for (int i = 0; i < launches; ++i) {
        st = plan_launch(p, d_iq, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, p->stream);
        if (st != SDRK_OK) return st;
    }
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    HIP_TRY(hipEventSynchronize(p->ev1));
    HIP_TRY(hipEventElapsedTime(elapsed_ms, p->ev0, p->ev1));
    return fused_check(p);
}

int sdrk_exec_device_timed_each(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride,
                                float* d_out_db, int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_exec_f32, launch_f32, p, d_iq, n_frames, frame_stride, d_out_db, launches, each_ms);
}

}  // extern "C"

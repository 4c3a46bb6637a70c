// sdrk_probes.hip — the measuring entry points of include/sdrk.h: placement probes (sdrk_dev_alloc_stream_pair,
// sdrk_plan_tune_scratch, SDRK_PLAN_TUNE_STAGING), the streaming / copy / host-link ceilings, and the synthetic IQ fill they
// are fed with.  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace sdrk_host {
namespace {

// A placement probe's launch lambda maps a failed plan_launch to hipErrorUnknown; plan_launch has then already recorded the
// specific status and message on this thread — keep them instead of overwriting them with "unknown error".
thread_local int g_probe_status = SDRK_OK;
hipError_t probe_launch_result(int st) {
    if (st == SDRK_OK) return hipSuccess;
    g_probe_status = st;
    return hipErrorUnknown;
}
int probe_fail(hipError_t e, const char* what) {
    if (e == hipErrorUnknown && g_probe_status != SDRK_OK) {
        const int st = g_probe_status;
        g_probe_status = SDRK_OK;
        return st;                                     // sdrk_last_error() still holds plan_launch's own text
    }
    return fail(SDRK_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// ---- placement probes: warm first, then compare ---------------------------------------------------------------------
// An idle MI355X runs its shader clock near 1.0-1.4 GHz and needs tens of milliseconds of sustained load to reach the
// 1.85-2.0 GHz it holds afterwards (round 5, tools/cfg_steady.py: thirty back-to-back N = 2^20 transforms from idle take
// 1.53, 1.46, 1.46, 1.45, 1.42 ... 1.35 ms).  A probe that times candidate after candidate from a cold start therefore
// measures that ramp: every later candidate looks faster (round 4's sdrk_plan_tune_scratch records on config 5 were
// monotone in six runs of six, and "chose" the last candidate every time).  So every placement probe here (a) warms up BY
// TIME with the very launch it is going to time, and (b) times candidate 0 a second time after the last candidate: what a
// candidate gains is its time against that re-timed figure, and a gain under one per cent keeps what is already there.
struct PlacementReport {
    float warm_ms = 0.0f;            // wall time of the warm-up launches
    int warm_launches = 0;
    float first_ms = 0.0f;           // candidate 0 as first timed (after the warm-up)
    float retimed_first_ms = 0.0f;   // candidate 0 timed again after the last candidate
    float chosen_ms = 0.0f;          // the kept candidate's time
    int candidates = 0, chosen = 0;
};
thread_local PlacementReport g_placement;
constexpr double PLACEMENT_WARM_MS = 60.0;

template <typename Launch>
hipError_t placement_warm_up(hipStream_t s, Launch&& launch, PlacementReport& rep, int max_launches = 4000) {
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipSuccess;
    int n = 0;
    double ms = 0.0;
    while (e == hipSuccess && n < max_launches) {
        e = launch();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        ++n;
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms >= PLACEMENT_WARM_MS && n >= 2) break;
    }
    rep.warm_ms = (float)ms;
    rep.warm_launches = n;
    return e;
}

// one untimed launch, then the median of three isolated ones (event, launch, event, wait)
template <typename Launch>
hipError_t placement_time(hipStream_t s, hipEvent_t e0, hipEvent_t e1, Launch&& launch, float* median_ms) {
    float t[4] = {0, 0, 0, 0};
    hipError_t e = hipSuccess;
    for (int r = 0; r < 4 && e == hipSuccess; ++r) {
        e = hipEventRecord(e0, s);
        if (e == hipSuccess) e = launch();
        if (e == hipSuccess) e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t[r], e0, e1);
    }
    std::sort(t + 1, t + 4);
    *median_ms = t[2];
    return e;
}

// `launches` timed launches (after two untimed ones) of a probe kernel on a private stream
template <typename Launch>
int timed_probe(int device, int launches, float* each_ms, const char* what, Launch&& launch) {
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int i = -2; i < launches && e == hipSuccess; ++i) {     // two untimed warm-ups
        if (i >= 0) e = hipEventRecord(e0, s);
        if (e == hipSuccess) e = launch(prop.multiProcessorCount, s);
        if (i >= 0 && e == hipSuccess) e = hipEventRecord(e1, s);
        if (i >= 0 && e == hipSuccess) e = hipEventSynchronize(e1);
        if (i >= 0 && e == hipSuccess) e = hipEventElapsedTime(&each_ms[i], e0, e1);
    }
    (void)hipStreamSynchronize(s);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(s);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return SDRK_OK;
}

// The heads of one ceiling-probe call: its launches take their frames in the order a plan created now would (f4k_rot.h:
// f4k_choice), from heads of the call's own.  timed_probe waits for its launches, so they never overlap.
struct ProbeHeads {
    F4kProbeDeal deal;
    int status = SDRK_OK;
    explicit ProbeHeads(int device) {
        deal.choice = f4k_choice(getenv("SDRK_F4K_ORDER"), getenv("SDRK_F4K_TICKET_FORM"), getenv("SDRK_F4K_ROT_AHEAD"));
        if (deal.choice.order == F4K_ORDER_STRIDE) return;            // the grid-stride loops: no heads
        status = check_device(device);
        if (status != SDRK_OK) return;
        const std::vector<uint32_t> zero(F4K_ROT_WORDS, 0u);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void**)&deal.d_heads, zero.size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(deal.d_heads, zero.data(), zero.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) status = fail(SDRK_ERR_HIP, "probe heads: %s", hipGetErrorString(e));
    }
    ~ProbeHeads() {
        if (deal.d_heads) (void)hipFree(deal.d_heads);
    }
    ProbeHeads(const ProbeHeads&) = delete;
    ProbeHeads& operator=(const ProbeHeads&) = delete;
};

}  // namespace

// SDRK_PLAN_TUNE_STAGING: the numpy boundary's device staging (HOST_SLOTS chunk pairs of ~16 MiB in / 8 MiB out) allocated
// at plan creation, each slot's row buffer the fastest of three candidates under the plan's own transform over the
// chunk — the pairing effect of DESIGN.md §4.1 applied to the library's own buffers.  (Measured in round 4: the probe
// times of the candidates agree to the microsecond and B = 32768 does not move — a 24 MiB pair lives in the L2 /
// Infinity Cache, where placement levels do not exist, and the kernel is 1.5 % of a PCIe-bound call.  The flag stays
// for plans whose chunks are made larger.)
int tune_staging(sdrk_plan* p) {
    const size_t nfft = (size_t)p->nfft;
    if (p->blu_inner || p->max_batch * nfft * sizeof(float2) <= 2 * HOST_CHUNK_BYTES) return SDRK_OK;   // small plans: nothing staged in chunks
    size_t per = HOST_CHUNK_BYTES / (nfft * sizeof(float2));
    if (per < 1) per = 1;
    const size_t in_b = per * nfft * sizeof(float2), out_b = per * nfft * sizeof(float);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipError_t ee = hipEventCreate(&e1); ee != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(SDRK_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
    int st = SDRK_OK;
    PlacementReport rep;
    for (int i = 0; i < HOST_SLOTS && st == SDRK_OK; ++i) {
        HostSlot& s = p->slot[i];
        st = slot_reserve(p, s, in_b, 0);                        // events, pinned h_in, d_in
        if (st != SDRK_OK) break;
        if (hipHostMalloc(&s.h_out, out_b, hipHostMallocDefault) != hipSuccess) { st = fail(SDRK_ERR_NOMEM, "pinned staging"); break; }
        void* cand[3] = {nullptr, nullptr, nullptr};
        int best = 0;
        for (int c = 0; c < 3 && st == SDRK_OK; ++c) {           // earlier candidates stay allocated: each lands elsewhere
            if (hipMalloc(&cand[c], out_b) != hipSuccess) { st = fail(SDRK_ERR_NOMEM, "device staging"); break; }
            auto launch = [&]() -> hipError_t {
                return probe_launch_result(plan_launch(p, s.d_in, per, nfft, cand[c], sdrk::EPI_LOGPSD, p->stream));
            };
            hipError_t e = hipSuccess;
            if (i == 0 && c == 0) e = placement_warm_up(p->stream, launch, rep);   // (see "placement probes" above)
            float med = 0.0f;
            if (e == hipSuccess) e = placement_time(p->stream, e0, e1, launch, &med);
            if (e != hipSuccess) { st = probe_fail(e, "staging probe failed"); break; }
            p->staging_probe_ms[i * 3 + c] = med;
            if (med < p->staging_probe_ms[i * 3 + best]) best = c;
        }
        for (int c = 0; c < 3; ++c) {
            if (c == best && st == SDRK_OK) { s.d_out = cand[c]; s.out_cap = out_b; }
            else if (cand[c]) (void)hipFree(cand[c]);
        }
        if (st == SDRK_OK) p->staging_probe_n = (i + 1) * 3;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return st;
}

}  // namespace sdrk_host

extern "C" {

int sdrk_dev_alloc_stream_pair(int device, size_t in_bytes, size_t out_bytes, int candidates, sdrk_plan* plan,
                               void** d_in, void** d_out, float* probe_ms, int* chosen) {
    if (!d_in || !d_out) return fail(SDRK_ERR_INVALID, "d_in or d_out is NULL");
    *d_in = *d_out = nullptr;
    size_t plan_frames = 0;
    if (plan) {
        if (plan->device != device) return fail(SDRK_ERR_INVALID, "plan is on device %d, not %d", plan->device, device);
        if (int st = check_precision(plan, 32); st != SDRK_OK) return st;
        plan_frames = in_bytes / ((size_t)plan->nfft * sizeof(float2));
        if (plan_frames == 0 || out_bytes < plan_frames * (size_t)plan->nfft * sizeof(float))
            return fail(SDRK_ERR_INVALID, "buffers do not hold whole frames of the plan's length");
    }
    if (chosen) *chosen = 0;
    g_placement = PlacementReport();                  // whatever happens below, sdrk_placement_report never describes an older call
    if (candidates < 1) candidates = 1;
    if (candidates > 16) candidates = 16;
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    HIP_TRY(hipMalloc(d_in, in_bytes ? in_bytes : 1));
    // probe = the no-arithmetic streaming kernel with the spectrum path's 2:1 traffic shape over the pair (its
    // first 2^20 frame-equivalents: a short prefix mispredicts the intermediate levels); below 2^13
    // frame-equivalents the levels do not separate, and nothing is tuned
    size_t pf = in_bytes / 32768 < out_bytes / 16384 ? in_bytes / 32768 : out_bytes / 16384;
    if (pf > ((size_t)1 << 20)) pf = (size_t)1 << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        while (candidates > 1 && (size_t)candidates * out_bytes + ((size_t)1 << 30) > free_b) --candidates;
    }
    if (pf < ((size_t)1 << 13)) candidates = 1;
    if (plan && plan_frames > ((size_t)1 << 32) / (size_t)plan->nfft) plan_frames = ((size_t)1 << 32) / (size_t)plan->nfft;
    std::vector<void*> cand((size_t)candidates, nullptr);
    std::vector<float> ms((size_t)candidates, 0.0f);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t s = nullptr;
    hipError_t e = hipSuccess;
    if (candidates > 1) {
        e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    }
    int n_ok = 0;
    PlacementReport rep;
    auto launch_on = [&](void* out) {
        return [&, out]() -> hipError_t {
            if (plan)                                 // the plan's own transform over the pair: what will really run
                return probe_launch_result(plan_launch(plan, *d_in, plan_frames, (size_t)plan->nfft, out, sdrk::EPI_LOGPSD, s));
            return sdrk::launch_stream_mix(*d_in, out, pf, prop.multiProcessorCount, s);
        };
    };
    for (int c = 0; c < candidates && e == hipSuccess; ++c) {
        // earlier candidates stay allocated, so each new one lands somewhere else
        if (hipMalloc(&cand[(size_t)c], out_bytes ? out_bytes : 1) != hipSuccess) {
            (void)hipGetLastError();
            cand[(size_t)c] = nullptr;
            break;
        }
        ++n_ok;
        if (candidates == 1) break;
        if (c == 0) e = placement_warm_up(s, launch_on(cand[0]), rep);          // (see "placement probes" above)
        if (e == hipSuccess) e = placement_time(s, e0, e1, launch_on(cand[(size_t)c]), &ms[(size_t)c]);
    }
    if (e == hipSuccess && n_ok > 1) {                                            // candidate 0 again, after the last one
        rep.first_ms = ms[0];
        e = placement_time(s, e0, e1, launch_on(cand[0]), &rep.retimed_first_ms);
        if (e == hipSuccess) ms[0] = rep.retimed_first_ms < ms[0] ? rep.retimed_first_ms : ms[0];
    }
    if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    int best = 0;
    for (int c = 1; c < n_ok; ++c)
        if (ms[(size_t)c] < ms[(size_t)best]) best = c;
    if (e != hipSuccess || n_ok == 0) {
        for (void* p : cand) if (p) (void)hipFree(p);
        (void)hipFree(*d_in);
        *d_in = nullptr;
        if (e != hipSuccess) return probe_fail(e, "placement probe failed");
        return fail(SDRK_ERR_NOMEM, "could not allocate %zu bytes for the output buffer", out_bytes);
    }
    for (int c = 0; c < n_ok; ++c) {
        if (probe_ms) probe_ms[c] = (c == 0 && n_ok > 1) ? rep.first_ms : ms[(size_t)c];   // [0]: as first timed; re-timed: sdrk_placement_report
        if (c != best) (void)hipFree(cand[(size_t)c]);
    }
    if (probe_ms) for (int c = n_ok; c < candidates; ++c) probe_ms[c] = 0.0f;
    *d_out = cand[(size_t)best];
    if (chosen) *chosen = best;
    rep.candidates = n_ok;
    rep.chosen = best;
    rep.chosen_ms = ms[(size_t)best];
    g_placement = rep;
    return SDRK_OK;
}

int sdrk_plan_tune_scratch(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db,
                           int candidates, float* probe_ms, int* chosen) {
    if (chosen) *chosen = 0;
    int st = check_exec_args(p, d_iq, n_frames, frame_stride, d_out_db);
    if (st != SDRK_OK) return st;
    g_placement = PlacementReport();
    if (!p->d_scratch || p->scratch_frames == 0 || n_frames == 0 || takes_fused(p, n_frames)) {
        // no scratch on this workload's path (one-pass lengths; the persistent N = 65536 launch): nothing to place
        if (probe_ms) for (int c = 0; c < candidates; ++c) probe_ms[c] = 0.0f;
        return SDRK_OK;
    }
    if (candidates < 2) return SDRK_OK;
    if (candidates > 16) candidates = 16;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const size_t bytes = p->scratch_frames * (size_t)p->nfft * sizeof(float2);
    std::vector<float2*> cand((size_t)candidates, nullptr);
    std::vector<float> ms((size_t)candidates, 0.0f);
    cand[0] = p->d_scratch;                                               // candidate 0 = the plan's present scratch
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    PlacementReport rep;
    auto launch = [&]() -> hipError_t {
        return probe_launch_result(plan_launch(p, d_iq, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, p->stream));
    };
    if (e == hipSuccess) e = placement_warm_up(p->stream, launch, rep);    // (see "placement probes" above)
    int n_ok = 0;
    for (int c = 0; c < candidates && e == hipSuccess; ++c) {
        // earlier candidates stay allocated, so each new one lands somewhere else
        if (c > 0 && hipMalloc((void**)&cand[(size_t)c], bytes) != hipSuccess) {
            (void)hipGetLastError();
            cand[(size_t)c] = nullptr;
            break;
        }
        ++n_ok;
        p->d_scratch = cand[(size_t)c];
        e = placement_time(p->stream, e0, e1, launch, &ms[(size_t)c]);
    }
    if (e == hipSuccess && n_ok > 1) {                                     // candidate 0 again, after the last one
        p->d_scratch = cand[0];
        rep.first_ms = ms[0];
        e = placement_time(p->stream, e0, e1, launch, &rep.retimed_first_ms);
    }
    (void)hipStreamSynchronize(p->stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    // a candidate replaces the present scratch only if it beats BOTH timings of it by one per cent
    int best = 0;
    if (e == hipSuccess && n_ok > 1) {
        const float ref0 = rep.retimed_first_ms < ms[0] ? rep.retimed_first_ms : ms[0];
        float best_ms = ref0 * 0.99f;
        for (int c = 1; c < n_ok; ++c)
            if (ms[(size_t)c] < best_ms) { best = c; best_ms = ms[(size_t)c]; }
        rep.chosen_ms = best ? ms[(size_t)best] : ref0;
    }
    p->d_scratch = cand[(size_t)best];
    for (int c = 0; c < n_ok; ++c) {
        if (probe_ms) probe_ms[c] = ms[(size_t)c];
        if (c != best) (void)hipFree(cand[(size_t)c]);
    }
    if (probe_ms) for (int c = n_ok; c < candidates; ++c) probe_ms[c] = 0.0f;
    if (chosen) *chosen = best;
    rep.candidates = n_ok;
    rep.chosen = best;
    g_placement = rep;
    if (e != hipSuccess) return probe_fail(e, "scratch placement probe failed");
    return fused_check(p);
}

int sdrk_placement_report(float* warm_ms, int* warm_launches, float* first_ms, float* retimed_first_ms, float* chosen_ms) {
    const PlacementReport& r = g_placement;
    if (warm_ms) *warm_ms = r.warm_ms;
    if (warm_launches) *warm_launches = r.warm_launches;
    if (first_ms) *first_ms = r.first_ms;
    if (retimed_first_ms) *retimed_first_ms = r.retimed_first_ms;
    if (chosen_ms) *chosen_ms = r.chosen_ms;
    return r.candidates;
}

int sdrk_stream_ceiling_probe(int device, const void* d_in, void* d_out, size_t n_frames4096, int launches,
                              float* each_ms) {
    if (!d_in || !d_out || !each_ms || launches < 1 || launches > 4096 || n_frames4096 == 0)
        return fail(SDRK_ERR_INVALID, "bad argument");
    ProbeHeads heads(device);
    if (heads.status != SDRK_OK) return heads.status;
    return timed_probe(device, launches, each_ms, "stream ceiling probe", [&](int cus, hipStream_t s) {
        return sdrk::launch_stream_mix_dealt(d_in, d_out, n_frames4096, cus, s, heads.deal);
    });
}

int sdrk_copy_probe(int device, const void* d_in, void* d_out, size_t bytes, int launches, float* each_ms) {
    if (!d_in || !d_out || !each_ms || launches < 1 || launches > 4096 || bytes < 16)
        return fail(SDRK_ERR_INVALID, "bad argument");
    // the fastest of three grid sizes (by median): a ceiling should not depend on the probe's own launch shape
    std::vector<float> t((size_t)launches), best;
    float best_med = 0.0f;
    ProbeHeads heads(device);
    if (heads.status != SDRK_OK) return heads.status;
    for (int bpc : {3, 4, 16}) {
        int st = timed_probe(device, launches, t.data(), "copy probe", [&](int cus, hipStream_t s) {
            return sdrk::launch_copy_1to1_dealt(d_in, d_out, bytes, cus, bpc, s, heads.deal);
        });
        if (st != SDRK_OK) return st;
        std::vector<float> sorted = t;
        std::sort(sorted.begin(), sorted.end());
        const float med = sorted[sorted.size() / 2];
        if (best.empty() || med < best_med) { best = t; best_med = med; }
    }
    memcpy(each_ms, best.data(), sizeof(float) * (size_t)launches);
    return SDRK_OK;
}

int sdrk_host_link_probe(int device, size_t bytes, double* h2d_gbps, double* d2h_gbps, double* duplex_gbps) {
    if (!h2d_gbps || !d2h_gbps || !duplex_gbps || bytes < (1u << 20)) return fail(SDRK_ERR_INVALID, "bad argument");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    void *h_a = nullptr, *h_b = nullptr, *d_a = nullptr, *d_b = nullptr;
    hipStream_t s0 = nullptr, s1 = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    hipError_t e = hipHostMalloc(&h_a, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&h_b, bytes / 2, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&d_a, bytes);
    if (e == hipSuccess) e = hipMalloc(&d_b, bytes / 2);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s0, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s1, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventCreate(&e2);
    if (e == hipSuccess) memset(h_a, 1, bytes);
    float ms = 0.f;
    auto timed = [&](bool up, bool down, double* gbps, double moved) {
        for (int rep = 0; rep < 3 && e == hipSuccess; ++rep) {       // keep the last of three
            e = hipEventRecord(e0, s0);
            if (e == hipSuccess) e = hipStreamWaitEvent(s1, e0, 0);
            if (up && e == hipSuccess) e = hipMemcpyAsync(d_a, h_a, bytes, hipMemcpyHostToDevice, s0);
            if (down && e == hipSuccess) e = hipMemcpyAsync(h_b, d_b, bytes / 2, hipMemcpyDeviceToHost, s1);
            if (e == hipSuccess) e = hipEventRecord(e2, s1);
            if (e == hipSuccess) e = hipStreamWaitEvent(s0, e2, 0);
            if (e == hipSuccess) e = hipEventRecord(e1, s0);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        }
        if (e == hipSuccess) *gbps = moved / (ms * 1e-3) / 1e9;
    };
    timed(true, false, h2d_gbps, (double)bytes);
    timed(false, true, d2h_gbps, (double)(bytes / 2));
    // the spectrum path's mix: `bytes` up while bytes/2 come down; rate quoted on the upstream bytes
    timed(true, true, duplex_gbps, (double)bytes);
    if (s0) (void)hipStreamSynchronize(s0);
    if (s1) (void)hipStreamSynchronize(s1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e2) (void)hipEventDestroy(e2);
    if (s0) (void)hipStreamDestroy(s0);
    if (s1) (void)hipStreamDestroy(s1);
    if (h_a) (void)hipHostFree(h_a);
    if (h_b) (void)hipHostFree(h_b);
    if (d_a) (void)hipFree(d_a);
    if (d_b) (void)hipFree(d_b);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "host link probe failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

int sdrk_synth_fill(int device, uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft,
                    void* d_iq, void* stream) {
    if (n_frames == 0) return SDRK_OK;
    if (!d_iq) return fail(SDRK_ERR_INVALID, "d_iq is NULL");
    if (nfft < 2 || (nfft & 1)) return fail(SDRK_ERR_INVALID, "nfft must be even and >= 2");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = sdrk::launch_synth_fill(seed, first_frame, n_frames, nfft, d_iq, s);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "synth launch failed: %s", hipGetErrorString(e));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SDRK_OK;
}

}  // extern "C"

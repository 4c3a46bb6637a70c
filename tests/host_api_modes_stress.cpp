// tests/host_api_modes_stress.cpp — drives the host side of the int16, polyphase-filter-bank (PFB) and integrated entry points
// (csrc/ci16_api.hip, pfb_api.hip and integrate_api.hip on csrc/integrate_call.h and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels tests/fake_*_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_modes.py.  A program of its
// own: nothing is loaded into Python, nothing is preloaded.
//
//   host_api_modes_stress <leg> [threads] [iters]      leg: ci16 | integrate | integrate_ci16 | pfb | pfb_integrate | pfb_ci16
//
// C64, PFB, CI16 and PFB_CI16 below have the entry points of the four input modes (the seven symbols spectrum.py's _Mode names); the case bodies exist
// once, over the sample type; a leg is a mode, its plans and a table of cases.  Every leg runs its cases from several threads
// on their own plans at once and checks EVERY output element for equality with the stand-ins' definition (host_stress.h).
// Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

// ---- the four modes -----------------------------------------------------------------------------------------------------
template <class S> struct Mode {
    bool pfb;                  // the plan needs a prototype (sdrk_plan_set_pfb)
    const Mode<S>* plain;      // the mode of the same samples without the filter bank
    const Mode<float>* c64;    // int16 modes: the complex64 mode that defines them, on the widened samples
    decltype(&sdrk_exec_device) exec_device;
    decltype(&sdrk_exec_device_timed_each) exec_device_timed_each;
    decltype(&sdrk_exec_host) exec_host;
    decltype(&sdrk_exec_fft_host) exec_fft_host;
    decltype(&sdrk_exec_device_integrated) exec_device_integrated;
    decltype(&sdrk_exec_device_integrated_timed_each) exec_device_integrated_timed_each;
    decltype(&sdrk_exec_host_integrated) exec_host_integrated;
};
extern const Mode<float> C64, PFB;
extern const Mode<int16_t> CI16, PFB_CI16;
const Mode<float> C64{false, &C64, nullptr, sdrk_exec_device, sdrk_exec_device_timed_each, sdrk_exec_host, sdrk_exec_fft_host,
                      sdrk_exec_device_integrated, sdrk_exec_device_integrated_timed_each, sdrk_exec_host_integrated};
const Mode<float> PFB{true, &C64, nullptr, sdrk_exec_device_pfb, sdrk_exec_device_pfb_timed_each, sdrk_exec_host_pfb, sdrk_exec_fft_host_pfb,
                      sdrk_exec_device_pfb_integrated, sdrk_exec_device_pfb_integrated_timed_each, sdrk_exec_host_pfb_integrated};
const Mode<int16_t> CI16{false, &CI16, &C64, sdrk_exec_device_ci16, sdrk_exec_device_ci16_timed_each, sdrk_exec_host_ci16, sdrk_exec_fft_host_ci16,
                         sdrk_exec_device_integrated_ci16, sdrk_exec_device_integrated_ci16_timed_each, sdrk_exec_host_integrated_ci16};
const Mode<int16_t> PFB_CI16{true, &CI16, &PFB, sdrk_exec_device_pfb_ci16, sdrk_exec_device_pfb_ci16_timed_each, sdrk_exec_host_pfb_ci16,
                             sdrk_exec_fft_host_pfb_ci16, sdrk_exec_device_pfb_integrated_ci16, sdrk_exec_device_pfb_integrated_ci16_timed_each,
                             sdrk_exec_host_pfb_integrated_ci16};

// a Case (host_stress.h) through the device, the timed or the host entry: per frame (k == 0) or integrated
template <class S> int exec_device(const Mode<S>& m, sdrk_plan* p, const Case& c, const void* in, float* out, void* stream) {
    return c.k ? m.exec_device_integrated(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out, stream)
               : m.exec_device(p, in, c.groups, c.stride, out, stream);
}
template <class S> int exec_timed(const Mode<S>& m, sdrk_plan* p, const Case& c, const void* in, float* out, int launches, float* ms) {
    return c.k ? m.exec_device_integrated_timed_each(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out, launches, ms)
               : m.exec_device_timed_each(p, in, c.groups, c.stride, out, launches, ms);
}
template <class S> int exec_host(const Mode<S>& m, sdrk_plan* p, const Case& c, const void* in, float* out) {
    return c.k ? m.exec_host_integrated(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out) : m.exec_host(p, in, c.groups, c.stride, out);
}

// ---- a leg: a mode, its plans, its cases --------------------------------------------------------------------------------
enum PlanId { P4K, P1K, P128, P64K, P1000, PG, N_PLANS };
struct PlanSpec {   // nfft == 0: the leg has no such plan.  taps == 0: no prototype at creation
    int nfft;
    size_t max_batch;
    int window;
    float floor;
    int shift, taps;
    unsigned proto_seed;
};
struct Plan {
    sdrk_plan* p = nullptr;
    std::vector<float> h;   // the prototype set on it; empty (data() == nullptr: one block of ones) in the plain modes
};

enum Kind { FRAMES, FRAMES_VS_C64, DEVICE, HOST, CHIRPZ, GROWTH, STREAMS, SET_PFB };
enum : unsigned { PINNED = 1, TIMED = 2, VS_C64 = 4 };
struct Row {
    Kind kind;
    PlanId plan;
    Case c;
    unsigned seed;   // offset from the thread's and iteration's seed
    unsigned flags = 0;
};

enum Who { F64, WINDOWED, BARE, NO_PLAN, GOOD };   // a float64 plan, a Hann plan (PFB: refused), one without prototype, null, a good one
enum Defect { NONE, NO_IN, NO_OUT, NO_FRAMES, NO_K, HUGE_COUNTS, NO_STRIDE, FIVE_FRAMES, BAD_DET, BAD_FORM, NO_LAUNCHES, NO_MS };
enum : unsigned { E_DEVICE = 1, E_TIMED = 2, E_HOST = 4, E_FFT = 8, E_FRAMES = 15, I_DEVICE = 16, I_TIMED = 32, I_HOST = 64, I_ALL = 112 };
struct Refusal {
    Who who;
    Defect defect;
    unsigned entries;
};

template <class S> struct Leg;
template <class S> struct RefusalPlans {
    sdrk_plan *f64, *windowed, *bare, *good;
    S* in;
    float* out;
};
template <class S> struct Leg {
    const char* name;
    const Mode<S>* mode;
    void (*fill)(S*, size_t, unsigned);
    std::vector<float> (*proto)(int, int, unsigned);
    bool chirpz_via_c64;     // chirp-z reference of the integrated rows: the complex64 mode's spectra, not this mode's own
    PlanSpec plans[N_PLANS];
    std::vector<Row> rows;
    std::vector<Refusal> refusals;
    unsigned refusal_seed, refusal_proto_seed;
    Case works_frames, works_groups;                    // after the refusals the plan still works (groups == 0: not in this leg)
    void (*more_refusals)(const RefusalPlans<S>&);      // what only this leg has, or null
};

// ---- the case bodies ----------------------------------------------------------------------------------------------------
// the frames' complex spectra where the stand-in transforms give no closed form (chirp-z)
template <class S> std::vector<float> chirpz_spectra(const Leg<S>& L, sdrk_plan* p, const Case& c, const S* in) {
    std::vector<float> spec(2 * n_frames(c) * (size_t)c.nfft);
    if (L.chirpz_via_c64) {
        const std::vector<float> w = widen(in, in_samples(c));
        CHECK(L.mode->c64->exec_fft_host(p, w.data(), n_frames(c), c.stride, spec.data()) == SDRK_OK);
    } else {
        CHECK((!L.mode->c64 || c.stride == (size_t)c.nfft) && L.mode->exec_fft_host(p, in, n_frames(c), c.stride, spec.data()) == SDRK_OK);
    }
    return spec;
}

template <class S> int wrong(const Leg<S>& L, const Plan& pl, const Case& c, const S* in, const float* out) {
    if (!c.k) return wrong_frames(in, pl.h.data(), c, {out});
    if (!c.chirpz) return wrong_rows(in, pl.h.data(), c, out);
    return wrong_rows(in, pl.h.data(), c, out, chirpz_spectra(L, pl.p, c, in).data());
}

// The device entry point ("device" memory is host memory here): asynchronous, any number of frames, the stagings in chunks.
template <class S> void device_case(const Leg<S>& L, const Plan& pl, const Case& c, unsigned seed, bool timed) {
    std::vector<S> in(2 * in_samples(c));
    std::vector<float> out(n_out(c), -1.0f);
    L.fill(in.data(), in_samples(c), seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(exec_timed(*L.mode, pl.p, c, in.data(), out.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(exec_device(*L.mode, pl.p, c, in.data(), out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    }
    CHECK(wrong(L, pl, c, in.data(), out.data()) == 0);
}

// The host entry point, from pageable or pinned (library-allocated) arrays; per frame, the complex epilogue through the same
// pipeline as well; VS_C64: the complex64 entry of the same plan must agree on the widened samples.
// (the chirp-z stand-ins differ between the int16 and the complex64 route in how they chain, so only the rest is compared)
template <class S> void host_case(const Leg<S>& L, const Plan& pl, const Case& c, bool pinned, unsigned seed, bool vs_c64) {
    const Mode<S>& m = *L.mode;
    Buf<S> in(2 * in_samples(c), pinned);
    Buf<float> out(n_out(c), pinned), cx(c.k ? 0 : 2 * n_out(c), pinned && !c.k);
    if (!in.data() || !out.data() || (!c.k && !cx.data())) return;
    L.fill(in.data(), in_samples(c), seed);
    std::fill_n(out.data(), n_out(c), -1.0f);
    CHECK(exec_host(m, pl.p, c, in.data(), out.data()) == SDRK_OK);
    if (!c.k) {
        CHECK(m.exec_fft_host(pl.p, in.data(), c.groups, c.stride, cx.data()) == SDRK_OK);
        CHECK(wrong_frames(in.data(), pl.h.data(), c, {out.data()}, cx.data()) == 0);
    } else {
        CHECK(wrong(L, pl, c, in.data(), out.data()) == 0);
    }
    if (vs_c64 && !c.chirpz) {
        const std::vector<float> wide = widen(in.data(), in_samples(c));
        std::vector<float> ref(n_out(c), -2.0f);
        CHECK(exec_host(*m.c64, pl.p, c, wide.data(), ref.data()) == SDRK_OK);
        CHECK(same(out.data(), ref));
    }
}

// Every per-frame entry on one input: device (plain and timed), host dB rows, host complex spectra — every element against the fold.
template <class S> void frames_case(const Leg<S>& L, const Plan& pl, const Case& c, bool pinned, unsigned seed) {
    const Mode<S>& m = *L.mode;
    Buf<S> in(2 * in_samples(c), pinned);
    if (!in.data()) return;
    L.fill(in.data(), in_samples(c), seed);
    std::vector<float> dev(n_out(c), -1.0f), timed(n_out(c), -1.0f), host(n_out(c), -1.0f), spec(2 * n_out(c), -1.0f);
    float ms[2] = {0, 0};
    CHECK(m.exec_device(pl.p, in.data(), c.groups, c.stride, dev.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(m.exec_device_timed_each(pl.p, in.data(), c.groups, c.stride, timed.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    CHECK(m.exec_host(pl.p, in.data(), c.groups, c.stride, host.data()) == SDRK_OK);
    CHECK(m.exec_fft_host(pl.p, in.data(), c.groups, c.stride, spec.data()) == SDRK_OK);
    CHECK(wrong_frames(in.data(), pl.h.data(), c, {dev.data(), timed.data(), host.data()}, spec.data()) == 0);
}

// The same where the stand-in transforms give no closed form (chirp-z): every element against the complex64 entries of the
// same plan on the widened samples, which run none of the int16 code.
template <class S> void frames_case_vs_c64(const Leg<S>& L, const Plan& pl, const Case& c, unsigned seed) {
    const Mode<S>& m = *L.mode;
    std::vector<S> in(2 * in_samples(c));
    L.fill(in.data(), in_samples(c), seed);
    const std::vector<float> w = widen(in.data(), in_samples(c));
    std::vector<float> dev(n_out(c), -1.0f), timed(n_out(c), -1.0f), host(n_out(c), -1.0f), spec(2 * n_out(c), -1.0f);
    std::vector<float> want(n_out(c), -2.0f), want_spec(2 * n_out(c), -2.0f);
    float ms[2] = {0, 0};
    CHECK(m.c64->exec_host(pl.p, w.data(), c.groups, c.stride, want.data()) == SDRK_OK);
    CHECK(m.c64->exec_fft_host(pl.p, w.data(), c.groups, c.stride, want_spec.data()) == SDRK_OK);
    CHECK(m.exec_device(pl.p, in.data(), c.groups, c.stride, dev.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(m.exec_device_timed_each(pl.p, in.data(), c.groups, c.stride, timed.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    CHECK(m.exec_host(pl.p, in.data(), c.groups, c.stride, host.data()) == SDRK_OK);
    CHECK(m.exec_fft_host(pl.p, in.data(), c.groups, c.stride, spec.data()) == SDRK_OK);
    CHECK(same(dev.data(), want));
    CHECK(same(timed.data(), want));
    CHECK(same(host.data(), want));
    CHECK(same(spec.data(), want_spec));
}

// A chirp-z length, per frame (the stand-in kernels chain differently there): the mode's host call against the ordinary
// complex64 call on the folded frames (int16 without filter bank: on the widened samples).
template <class S> void chirpz_case(const Leg<S>& L, const Plan& pl, const Case& c, unsigned seed) {
    const size_t n = (size_t)c.nfft;
    std::vector<S> in(2 * in_samples(c));
    std::vector<float> y(2 * n_out(c)), a(n_out(c), -1.0f), b(n_out(c), -2.0f);
    L.fill(in.data(), in_samples(c), seed);
    for (size_t f = 0; f < c.groups; ++f)
        for (size_t k = 0; k < n; ++k) folded(in.data(), pl.h.data(), n, c.taps, f * c.stride, k, y[2 * (f * n + k)], y[2 * (f * n + k) + 1]);
    CHECK(L.mode->exec_host(pl.p, in.data(), c.groups, c.stride, a.data()) == SDRK_OK);
    CHECK(sdrk_exec_host(pl.p, y.data(), c.groups, n, b.data()) == SDRK_OK);
    CHECK(same(a.data(), b));
}

// A small call still in flight when a larger one makes the state and the stagings grow; then one on a stream of the caller's;
// int16 integrated: then the complex64 entry on the same plan's state, between two int16 calls.
template <class S> void growth_case(const Leg<S>& L, const Plan& pl, const Case& of, unsigned seed) {
    const Mode<S>& m = *L.mode;
    const size_t n = (size_t)of.nfft;
    const Case small = of.k ? Case{of.nfft, of.taps, 2, 3, n, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f} : Case{of.nfft, of.taps, 3, 0, n};
    const Case big = of.k ? Case{of.nfft, of.taps, 3, 40, n, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 0.5f}   // split: partial rows as well
                          : Case{of.nfft, of.taps, 40, 0, n};
    const bool and_c64 = of.k && m.c64;
    std::vector<S> a(2 * in_samples(small)), b(2 * in_samples(big));
    std::vector<float> ra(n_out(small)), rb(n_out(big)), rc(ra.size()), rd(ra.size());
    L.fill(a.data(), in_samples(small), seed);
    L.fill(b.data(), in_samples(big), seed + 1);
    const std::vector<float> wide = widen(a.data(), in_samples(small));
    CHECK(exec_device(m, pl.p, small, a.data(), ra.data(), nullptr) == SDRK_OK);
    CHECK(exec_device(m, pl.p, big, b.data(), rb.data(), nullptr) == SDRK_OK);    // grows: must wait for the first
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(wrong(L, pl, small, a.data(), ra.data()) == 0);
    CHECK(wrong(L, pl, big, b.data(), rb.data()) == 0);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(exec_device(m, pl.p, big, b.data(), rb.data(), nullptr) == SDRK_OK);    // plan's stream ...
    CHECK(exec_device(m, pl.p, small, a.data(), rc.data(), s) == SDRK_OK);        // ... then the caller's: same state and stagings
    if (and_c64) CHECK(exec_device(*m.c64, pl.p, small, wide.data(), rd.data(), nullptr) == SDRK_OK);   // ... and the complex64 entry
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(wrong(L, pl, small, a.data(), rc.data()) == 0);
    CHECK(wrong(L, pl, big, b.data(), rb.data()) == 0);
    if (and_c64) CHECK(same(rc.data(), rd));
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

// PFB, integrated.  A call on the plan's stream, then one on a stream of the caller's while the first may still be running:
// one state, one prototype and two stagings per plan.  Then another prototype (another T) with both still recorded on the plan.
template <class S> void streams_and_set_pfb(const Leg<S>& L, const Plan& pl, int nfft, unsigned seed) {
    const Mode<S>& m = *L.mode;
    const size_t n = (size_t)nfft;
    const Plan p3{pl.p, proto(nfft, 3, seed)}, p2{pl.p, proto(nfft, 2, seed + 1)};
    CHECK(sdrk_plan_set_pfb(pl.p, 3, p3.h.data()) == SDRK_OK);
    const Case big{nfft, 3, 3, 40, n, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 0.5f};   // split: partial rows as well
    const Case small{nfft, 3, 2, 3, n / 2 + 1, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f};
    std::vector<S> a(2 * in_samples(small)), b(2 * in_samples(big));
    std::vector<float> ra(n_out(small)), rb(n_out(big));
    L.fill(a.data(), in_samples(small), seed);
    L.fill(b.data(), in_samples(big), seed + 1);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(exec_device(m, pl.p, big, b.data(), rb.data(), nullptr) == SDRK_OK);
    CHECK(exec_device(m, pl.p, small, a.data(), ra.data(), s) == SDRK_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(wrong(L, p3, small, a.data(), ra.data()) == 0);
    CHECK(wrong(L, p3, big, b.data(), rb.data()) == 0);
    // work of the caller's stream still recorded on the plan when the prototype is replaced
    CHECK(exec_device(m, pl.p, small, a.data(), ra.data(), s) == SDRK_OK);
    CHECK(sdrk_plan_set_pfb(pl.p, 2, p2.h.data()) == SDRK_OK);
    CHECK(sdrk_plan_pfb_taps(pl.p) == 2);
    CHECK(wrong(L, p3, small, a.data(), ra.data()) == 0);   // (set_pfb waited for it)
    Case two = small;
    two.taps = 2;
    device_case(L, p2, two, seed + 2, false);
    // the per-frame PFB entry and the plain integrated entry of the same plan beside it (the int16 leg checks their rows too:
    // the plain integrated row is the PFB's with one tap of ones)
    const Case frames{nfft, 2, 2, 0, n}, plain{nfft, 1, 1, 2, n};
    const Plan ones{pl.p, {}};
    std::vector<float> rows(2 * n, -1.0f);
    CHECK(exec_host(m, pl.p, frames, a.data(), rows.data()) == SDRK_OK);
    if (m.c64) CHECK(wrong(L, p2, frames, a.data(), rows.data()) == 0);
    std::fill(rows.begin(), rows.end(), -1.0f);
    CHECK(exec_host(*m.plain, pl.p, plain, a.data(), rows.data()) == SDRK_OK);
    if (m.c64) CHECK(wrong(L, ones, plain, a.data(), rows.data()) == 0);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

// ---- the runner ---------------------------------------------------------------------------------------------------------
template <class S> void worker(const Leg<S>& L, int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        Plan plans[N_PLANS];
        for (const Row& r : L.rows) {
            Plan& pl = plans[r.plan];
            if (!pl.p) {   // first use
                const PlanSpec& ps = L.plans[r.plan];
                CHECK(ps.nfft == r.c.nfft && sdrk_plan_create(0, ps.nfft, ps.max_batch, ps.window, nullptr, ps.floor, ps.shift, &pl.p) == SDRK_OK);
                if (!pl.p) return;
                if (L.mode->pfb) CHECK(sdrk_plan_pfb_taps(pl.p) == 0);
                if (L.mode->pfb && ps.taps) {
                    pl.h = L.proto(ps.nfft, ps.taps, s + ps.proto_seed);
                    CHECK(sdrk_plan_set_pfb(pl.p, ps.taps, pl.h.data()) == SDRK_OK && sdrk_plan_pfb_taps(pl.p) == ps.taps);
                }
            }
            switch (r.kind) {
            case FRAMES: frames_case(L, pl, r.c, r.flags & PINNED, s + r.seed); break;
            case FRAMES_VS_C64: frames_case_vs_c64(L, pl, r.c, s + r.seed); break;
            case DEVICE: device_case(L, pl, r.c, s + r.seed, r.flags & TIMED); break;
            case HOST: host_case(L, pl, r.c, r.flags & PINNED, s + r.seed, r.flags & VS_C64); break;
            case CHIRPZ: chirpz_case(L, pl, r.c, s + r.seed); break;
            case GROWTH: growth_case(L, pl, r.c, s + r.seed); break;
            case STREAMS: streams_and_set_pfb(L, pl, r.c.nfft, s + r.seed); break;
            case SET_PFB:   // another T between calls
                pl.h = L.proto(r.c.nfft, r.c.taps, s + r.seed);
                CHECK(sdrk_plan_set_pfb(pl.p, r.c.taps, pl.h.data()) == SDRK_OK && sdrk_plan_pfb_taps(pl.p) == r.c.taps);
                break;
            }
        }
        for (Plan& pl : plans)
            if (pl.p) CHECK(sdrk_plan_destroy(pl.p) == SDRK_OK);
    }
}

// Every (plan, defect, entry) of the leg's table must be refused as invalid with a message, and the plan must still work after.
template <class S> void refusals(const Leg<S>& L) {
    const Mode<S>& m = *L.mode;
    sdrk_plan *f64 = nullptr, *windowed = nullptr, *bare = nullptr, *good = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_HANN, nullptr, 1e-12f, 1, &windowed) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &bare) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &good) == SDRK_OK);
    if (!f64 || !windowed || !bare || !good) return;
    const int taps = m.pfb ? 2 : 1;
    const Plan pl{good, m.pfb ? L.proto(4096, taps, L.refusal_proto_seed) : std::vector<float>()};
    if (m.pfb) CHECK(sdrk_plan_set_pfb(good, taps, pl.h.data()) == SDRK_OK);
    std::vector<S> in(2 * 10 * 4096);
    std::vector<float> out(2 * 8 * 4096);
    L.fill(in.data(), 10 * 4096, L.refusal_seed);
    float ms[2];
    for (const Refusal& r : L.refusals) {
        sdrk_plan* const p = r.who == F64 ? f64 : r.who == WINDOWED ? windowed : r.who == BARE ? bare : r.who == NO_PLAN ? nullptr : good;
        const void* const x = r.defect == NO_IN ? nullptr : in.data();
        float* const o = r.defect == NO_OUT ? nullptr : out.data();
        const size_t stride = r.defect == NO_STRIDE ? 0 : 4096;
        const int launches = r.defect == NO_LAUNCHES ? 0 : 2;
        float* const each = r.defect == NO_MS ? nullptr : ms;
        const size_t frames = r.defect == NO_FRAMES ? 0 : r.defect == FIVE_FRAMES ? 5 : 2;   // max_batch is 4
        const size_t groups = r.defect == NO_FRAMES ? 0 : r.defect == HUGE_COUNTS ? (size_t)1 << 40 : 4;
        const size_t k = r.defect == NO_K ? 0 : r.defect == HUGE_COUNTS ? (size_t)1 << 40 : 2;
        const int det = r.defect == BAD_DET ? 3 : 0, form = r.defect == BAD_FORM ? 2 : 0;
        if (r.entries & E_DEVICE) REFUSED(m.exec_device(p, x, frames, stride, o, nullptr));
        if (r.entries & E_TIMED) REFUSED(m.exec_device_timed_each(p, x, frames, stride, o, launches, each));
        if (r.entries & E_HOST) REFUSED(m.exec_host(p, x, frames, stride, o));
        if (r.entries & E_FFT) REFUSED(m.exec_fft_host(p, x, frames, stride, o));
        if (r.entries & I_DEVICE) REFUSED(m.exec_device_integrated(p, x, groups, k, stride, det, form, 1.0f, o, nullptr));
        if (r.entries & I_TIMED) REFUSED(m.exec_device_integrated_timed_each(p, x, groups, k, stride, det, form, 1.0f, o, launches, each));
        if (r.entries & I_HOST) REFUSED(m.exec_host_integrated(p, x, groups, k, stride, det, form, 1.0f, o));
        CHECK(sdrk_last_error()[0]);
    }
    if (L.more_refusals) L.more_refusals({f64, windowed, bare, good, in.data(), out.data()});
    // the refused plan still works: per frame, and integrated beyond its max_batch of 4
    for (const Case& c : {L.works_frames, L.works_groups}) {
        if (!c.groups) continue;
        CHECK(exec_host(m, good, c, in.data(), out.data()) == SDRK_OK);
        CHECK(wrong(L, pl, c, in.data(), out.data()) == 0);
    }
    for (sdrk_plan* p : {f64, windowed, bare, good}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

// ---- the legs -----------------------------------------------------------------------------------------------------------
static const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;
static const int RECT = SDRK_WINDOW_RECT, HANN = SDRK_WINDOW_HANN;
static const Case NO_CASE{4096, 1, 0, 0, 4096};
template <class T> std::vector<T> operator+(std::vector<T> a, const std::vector<T>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

// the int16 entry points alone refuse nothing at zero frames, and have a synthesiser of their own
static void ci16_more_refusals(const RefusalPlans<int16_t>& r) {
    CHECK(sdrk_exec_host_ci16(r.good, nullptr, 0, 4096, nullptr) == SDRK_OK);
    REFUSED(sdrk_synth_fill_ci16(0, 1, 0, 2, 4096, nullptr, nullptr));
    REFUSED(sdrk_synth_fill_ci16(0, 1, 0, 2, 4095, r.in, nullptr));
    CHECK(sdrk_synth_fill_ci16(7, 1, 0, 2, 4096, r.in, nullptr) == SDRK_ERR_NO_DEVICE);
    CHECK(sdrk_synth_fill_ci16(0, 5, 3, 2, 4096, r.in, nullptr) == SDRK_OK && r.in[0] == (int16_t)(8 - 2048) && r.in[3] == (int16_t)(1 - 2048));
}

// Every path with 4-byte samples — the mapped small call, the zero-copy chunks, the three-slot DMA pipeline from pageable and
// from pinned caller arrays with ragged last chunks, and for the lengths that are widened first the plan's staging: several
// chunks of it per call, overlapped frames with their halo, spaced frames, a staging that has to grow under work still in
// flight, two streams on one plan.
static const Leg<int16_t> CI16_LEG{
    "ci16", &CI16, fill_wide, proto, false,
    {{4096, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {1024, 1 << 20, HANN, 0.0f, 0, 1, 0}, {128, 1 << 20, RECT, 1e-12f, 1, 1, 0},
     {65536, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {1000, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {32768, 64, RECT, 1e-12f, 1, 1, 0}},
    {
        {HOST, P4K, {4096, 1, 1, 0, 4096}, 1},                // the live call: 16 KiB, the mapped small path
        {HOST, P128, {128, 1, 5, 0, 128}, 2},                 // small call of a widened length
        {HOST, P4K, {4096, 1, 3, 0, 4096}, 3, PINNED},        // small, pinned
        {HOST, P1K, {1024, 1, 1500, 0, 1024}, 4},             // 6 MiB of packed frames: zero-copy chunks
        {HOST, P128, {128, 1, 20000, 0, 128}, 5},             // the same size at a widened length: copy engines
        {HOST, P4K, {4096, 1, 2200, 0, 4096}, 6},             // 34 MiB: the DMA pipeline, ragged last chunk
        {HOST, P4K, {4096, 1, 3001, 0, 2049}, 7},             // overlapped frames at an odd hop, chunked
        {HOST, P4K, {4096, 1, 2200, 0, 4096}, 8, PINNED},     // pinned caller arrays, chunked
        {HOST, P4K, {4096, 1, 100, 0, 4096}, 9, PINNED},      // pinned both sides, one launch
        {HOST, P64K, {65536, 1, 37, 0, 65536}, 10},           // two-pass length through the staging
        {HOST, P64K, {65536, 1, 141, 0, 32769}, 11},          // ... overlapped, 18 MiB, ragged chunks
        {CHIRPZ, P1000, {1000, 1, 700, 0, 1000}, 12},
        {DEVICE, P64K, {65536, 1, 150, 0, 65536}, 13},        // 75 MiB of complex64: two staging chunks (128 + 22)
        {DEVICE, P64K, {65536, 1, 300, 0, 32769}, 14},        // overlapped, two chunks, each with its halo
        {DEVICE, P128, {128, 1, 3000, 0, 131}, 15},           // spaced frames, widened frame by frame
        {DEVICE, P128, {128, 1, 70000, 0, 128}, 16, TIMED},   // 68 MiB of complex64 at a short length, timed entry
        {DEVICE, P4K, {4096, 1, 777, 0, 4096}, 17, TIMED},
        {DEVICE, P1K, {1024, 1, 1, 0, 0}, 18},                // one frame, stride 0
        {DEVICE, P128, {128, 1, 1, 0, 0}, 19},
        {GROWTH, P128, {128, 1, 0, 0, 0}, 20},
        {GROWTH, PG, {32768, 1, 0, 0, 0}, 21},
    },
    {{F64, NONE, E_HOST | E_FFT | E_DEVICE | E_TIMED}, {NO_PLAN, NONE, E_HOST}, {GOOD, NO_IN, E_HOST}, {GOOD, NO_OUT, E_HOST},
     {GOOD, NO_STRIDE, E_HOST}, {GOOD, FIVE_FRAMES, E_HOST | E_FFT}, {GOOD, NO_IN, E_DEVICE}, {GOOD, NO_LAUNCHES, E_TIMED},
     {GOOD, NO_MS, E_TIMED}},
    77, 0, {4096, 1, 4, 0, 4096}, NO_CASE, ci16_more_refusals};

// Device and host entries, the fused length and the staged ones (chirp-z included), groups split into slices and not, chunks
// and staging boundaries that cut groups and slices (the carry rows), pageable and pinned caller arrays, state and staging
// that have to grow under work still in flight, two streams on one plan.
static const std::vector<Refusal> INTEGRATE_REFUSALS{
    {F64, NONE, I_ALL}, {NO_PLAN, NONE, I_HOST}, {GOOD, NO_IN, I_HOST}, {GOOD, NO_OUT, I_HOST}, {GOOD, NO_FRAMES, I_HOST}, {GOOD, NO_K, I_HOST},
    {GOOD, NO_STRIDE, I_HOST}, {GOOD, BAD_DET, I_HOST}, {GOOD, BAD_FORM, I_DEVICE}, {GOOD, NO_LAUNCHES, I_TIMED}, {GOOD, NO_MS, I_TIMED}};
static const Leg<float> INTEGRATE_LEG{
    "integrate", &C64, fill, proto, false,
    {{4096, 4, RECT, 1e-12f, 1, 1, 0} /* max_batch does not apply */, {1024, 1 << 20, HANN, 0.0f, 0, 1, 0}, {128, 1 << 20, RECT, 1e-12f, 1, 1, 0},
     {65536, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {1000, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {4096, 64, RECT, 1e-12f, 1, 1, 0}},
    {
        // device entry: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
        {DEVICE, P4K, {4096, 1, 5, 1, 4096, MEAN, DB, 1.0f}, 1},
        {DEVICE, P4K, {4096, 1, 30, 7, 4096, MEAN, POW, 0.25f}, 2},
        {DEVICE, P4K, {4096, 1, 2, 50, 2049, MEAN, DB, 1.0f}, 3},
        {DEVICE, P4K, {4096, 1, 1, 33, 4100, MAX, POW, 2.0f}, 4, TIMED},
        {DEVICE, P4K, {4096, 1, 3, 9, 4096, MIN, DB, 1.0f}, 5},
        // ... the staged lengths: 64 MiB of spectra is 65536 frames of 128 and 128 frames of 65536 — several staging chunks,
        // groups (unsplit) and slices (split) carried across their boundaries
        {DEVICE, P128, {128, 1, 700, 100, 128, MEAN, POW, 1.0f}, 6},          // 70000 frames, unsplit, 65536 % 100 != 0
        {DEVICE, P128, {128, 1, 3, 23000, 131, MEAN, DB, 1.0f}, 7, TIMED},    // 69000 frames, split
        {DEVICE, P128, {128, 1, 5, 14000, 128, MAX, DB, 1.0f}, 8},
        {DEVICE, P64K, {65536, 1, 2, 70, 65536, MEAN, POW, 0.125f}, 9},       // 140 frames: 128 + 12, split by bins
        {DEVICE, P64K, {65536, 1, 45, 3, 32769, MIN, DB, 1.0f}, 10},          // 135 frames, overlapped
        {DEVICE, P1K, {1024, 1, 1, 1, 1, MEAN, DB, 1.0f}, 11},
        {DEVICE, P1000, {1000, 1, 4, 25, 1000, MEAN, DB, 1.0f, true}, 12},    // chirp-z
        // host entry: one chunk, several chunks with groups and slices across their boundaries, pageable and pinned
        {HOST, P4K, {4096, 1, 3, 2, 4096, MEAN, DB, 1.0f}, 13},
        {HOST, P4K, {4096, 1, 12, 101, 4096, MEAN, POW, 0.5f}, 14},           // 1212 frames: three chunks of 512, split
        {HOST, P4K, {4096, 1, 12, 101, 4096, MAX, DB, 1.0f}, 15, PINNED},
        {HOST, P4K, {4096, 1, 400, 3, 4096, MEAN, DB, 1.0f}, 16},             // unsplit: rows leave chunk by chunk
        {HOST, P4K, {4096, 1, 400, 3, 2049, MIN, POW, 3.0f}, 17, PINNED},     // overlapped, pinned both sides
        {HOST, P4K, {4096, 1, 1, 1100, 4096, MEAN, POW, 1.0f}, 18},           // one group over three chunks
        {HOST, P128, {128, 1, 900, 40, 128, MEAN, DB, 1.0f}, 19},             // 36000 frames: two chunks of 16384
        {HOST, P128, {128, 1, 2, 17000, 128, MEAN, POW, 1.0f}, 20, PINNED},   // split, slices across chunks
        {HOST, P64K, {65536, 1, 9, 7, 65536, MEAN, DB, 1.0f}, 21},            // 63 frames: chunks of 32, 32 % 7 != 0
        {HOST, P1000, {1000, 1, 30, 100, 1000, MAX, DB, 1.0f, true}, 22},     // chirp-z, 24 MB: two chunks
        {HOST, P1K, {1024, 1, 5, 1, 1024, MEAN, DB, 1.0f}, 23, PINNED},
        {GROWTH, P1K, {1024, 1, 0, 1, 0}, 24},
        {GROWTH, PG, {4096, 1, 0, 1, 0}, 25},
    },
    INTEGRATE_REFUSALS, 77, 0, NO_CASE, {4096, 1, 4, 2, 4096}, nullptr};

// The same from int16 I,Q: the fused length and the staged ones (an int16-reading length, a widened one, a two-pass one,
// chirp-z).  The complex64 entry of the same plan must agree on the widened samples (VS_C64, and inside GROWTH).
static const Leg<int16_t> INTEGRATE_CI16_LEG{
    "integrate_ci16", &CI16, fill, proto, false,
    {{4096, 4, RECT, 1e-12f, 1, 1, 0} /* max_batch does not apply */, {1024, 1 << 20, HANN, 0.0f, 0, 1, 0}, {128, 1 << 20, RECT, 1e-12f, 1, 1, 0},
     {65536, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {1000, 1 << 20, RECT, 1e-12f, 1, 1, 0}, {4096, 64, RECT, 1e-12f, 1, 1, 0}},
    {
        // device entry at the fused length: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
        {DEVICE, P4K, {4096, 1, 5, 1, 4096, MEAN, DB, 1.0f}, 1},
        {DEVICE, P4K, {4096, 1, 30, 7, 4096, MEAN, POW, 0.25f}, 2},
        {DEVICE, P4K, {4096, 1, 2, 50, 2049, MEAN, DB, 1.0f}, 3},
        {DEVICE, P4K, {4096, 1, 1, 33, 4100, MAX, POW, 2.0f}, 4, TIMED},
        {DEVICE, P4K, {4096, 1, 3, 9, 1001, MIN, DB, 1.0f}, 5},               // frame starts 4-byte aligned only
        // ... the staged lengths: 64 MiB of spectra is 65536 frames of 128 and 128 frames of 65536 — several spectrum-staging
        // chunks (and, at the widened lengths, the int16 route's own staging inside each), groups and slices carried across
        {DEVICE, P128, {128, 1, 700, 100, 128, MEAN, POW, 1.0f}, 6},          // 70000 frames, unsplit, 65536 % 100 != 0
        {DEVICE, P128, {128, 1, 3, 23000, 131, MEAN, DB, 1.0f}, 7, TIMED},    // 69000 frames, split, spaced
        {DEVICE, P64K, {65536, 1, 2, 70, 65536, MEAN, POW, 0.125f}, 8},       // 140 frames: 128 + 12, split by bins
        {DEVICE, P64K, {65536, 1, 45, 3, 32769, MIN, DB, 1.0f}, 9},           // 135 frames, overlapped
        {DEVICE, P1K, {1024, 1, 40, 9, 1024, MAX, DB, 1.0f}, 10},             // a length that reads int16 itself
        {DEVICE, P1K, {1024, 1, 1, 1, 1, MEAN, DB, 1.0f}, 11},
        {DEVICE, P1000, {1000, 1, 4, 25, 1000, MEAN, DB, 1.0f, true}, 12},    // chirp-z
        // host entry: one chunk; several chunks of 1024 frames (4-byte samples) with groups and slices across their
        // boundaries, pageable and pinned
        {HOST, P4K, {4096, 1, 3, 2, 4096, MEAN, DB, 1.0f}, 13, VS_C64},
        {HOST, P4K, {4096, 1, 22, 101, 4096, MEAN, POW, 0.5f}, 14},           // 2222 frames: three chunks, split
        {HOST, P4K, {4096, 1, 22, 101, 4096, MAX, DB, 1.0f}, 15, PINNED},
        {HOST, P4K, {4096, 1, 700, 3, 4096, MEAN, DB, 1.0f}, 16, VS_C64},     // unsplit: rows leave chunk by chunk
        {HOST, P4K, {4096, 1, 700, 3, 2049, MIN, POW, 3.0f}, 17, PINNED},     // overlapped, pinned both sides
        {HOST, P4K, {4096, 1, 1, 2100, 4096, MEAN, POW, 1.0f}, 18},           // one group over three chunks
        {HOST, P128, {128, 1, 900, 80, 128, MEAN, DB, 1.0f}, 19, VS_C64},     // 72000 frames: three chunks of 32768
        {HOST, P128, {128, 1, 2, 34000, 128, MEAN, POW, 1.0f}, 20, PINNED},   // split, slices across chunks
        {HOST, P64K, {65536, 1, 9, 15, 65536, MEAN, DB, 1.0f}, 21},           // 135 frames: chunks of 64, 64 % 15 != 0
        {HOST, P1000, {1000, 1, 30, 200, 1000, MAX, DB, 1.0f, true}, 22},     // chirp-z, 24 MB: two chunks
        {HOST, P1K, {1024, 1, 5, 1, 1024, MEAN, DB, 1.0f}, 23, PINNED | VS_C64},
        {GROWTH, P1K, {1024, 1, 0, 1, 0}, 24},
        {GROWTH, P128, {128, 1, 0, 1, 0}, 25},
        {GROWTH, PG, {4096, 1, 0, 1, 0}, 26},
    },
    INTEGRATE_REFUSALS, 77, 0, NO_CASE, {4096, 1, 4, 2, 4096}, nullptr};

// set_pfb's own refusals, and the ordinary entry point of a plan with a prototype is still the ordinary one
static void pfb_more_refusals(const RefusalPlans<float>& r) {
    const std::vector<float> h = proto_random(4096, 2, 9);
    for (sdrk_plan* bad : {r.f64, r.windowed}) REFUSED(sdrk_plan_set_pfb(bad, 2, h.data()));
    REFUSED(sdrk_plan_set_pfb(r.bare, 0, h.data()));
    REFUSED(sdrk_plan_set_pfb(r.bare, 33, h.data()));
    REFUSED(sdrk_plan_set_pfb(r.bare, 2, nullptr));
    REFUSED(sdrk_plan_set_pfb(nullptr, 2, h.data()));
    REFUSED(sdrk_plan_pfb_taps(nullptr));
    const Case c{4096, 1, 2, 0, 4096};
    CHECK(sdrk_exec_host(r.good, r.in, 2, 4096, r.out) == SDRK_OK);
    CHECK(wrong_frames(r.in, (const float*)nullptr, c, {r.out}) == 0);
}

// The mapped small call, the three-slot pipeline with the (T - 1) * nfft samples of overlap every chunk carries, ragged last
// chunks, pageable and pinned arrays, N = 4096 and lengths folded into the plan's staging (several chunks of it, growth under
// work in flight, two streams on one plan), a chirp-z length, set_pfb between calls.
static const Leg<float> PFB_LEG{
    "pfb", &PFB, fill_wide, proto_random, false,
    {{4096, 1 << 20, RECT, 1e-12f, 1, 4, 50}, {1024, 1 << 20, RECT, 0.0f, 0, 3, 52}, {128, 1 << 20, RECT, 1e-12f, 1, 5, 53},
     {65536, 1 << 20, RECT, 1e-12f, 1, 2, 54}, {1000, 1 << 20, RECT, 1e-12f, 1, 3, 55}, {}},
    {
        {HOST, P4K, {4096, 4, 1, 0, 4096}, 1},                // one frame of four blocks: 128 KiB, the mapped small path
        {HOST, P128, {128, 5, 5, 0, 128}, 2},                 // small call of a staged length
        {HOST, P4K, {4096, 4, 3, 0, 4096}, 3, PINNED},        // pinned, small
        {HOST, P4K, {4096, 4, 600, 0, 4096}, 4},              // 19 MiB: four chunks, three blocks of overlap each
        {HOST, P4K, {4096, 4, 1201, 0, 2049}, 5},             // overlapped frames at an odd hop, ragged last chunk
        {HOST, P4K, {4096, 4, 600, 0, 4096}, 6, PINNED},      // pinned caller arrays, chunked
        {HOST, P1K, {1024, 3, 3000, 0, 700}, 7},              // staged length, chunked, hop < nfft
        {HOST, P64K, {65536, 2, 21, 0, 32769}, 8},            // two-pass length through the staging
        {CHIRPZ, P1000, {1000, 3, 300, 0, 777}, 9},
        {DEVICE, P1K, {1024, 3, 9000, 0, 512}, 10},           // 70 MiB of folded frames: two staging chunks
        {DEVICE, P128, {128, 5, 3000, 0, 131}, 11, TIMED},    // spaced frames, timed entry
        {DEVICE, P4K, {4096, 4, 300, 0, 4096}, 12, TIMED},
        {DEVICE, P1K, {1024, 3, 1, 0, 0}, 13},                // one frame, stride 0
        {GROWTH, P128, {128, 5, 0, 0, 0}, 14},
        {SET_PFB, P4K, {4096, 2, 0, 0, 0}, 51},               // another T between calls
        {HOST, P4K, {4096, 2, 300, 0, 4096}, 15},
        {DEVICE, P4K, {4096, 2, 40, 0, 1000}, 16},
    },
    {{F64, NONE, E_FRAMES}, {WINDOWED, NONE, E_FRAMES}, {BARE, NONE, E_HOST | E_DEVICE} /* no prototype set */, {NO_PLAN, NONE, E_HOST},
     {GOOD, NO_IN, E_HOST}, {GOOD, NO_OUT, E_HOST}, {GOOD, NO_STRIDE, E_HOST}, {GOOD, NO_FRAMES, E_HOST | E_FFT | E_DEVICE},
     {GOOD, FIVE_FRAMES, E_HOST}, {GOOD, NO_IN, E_DEVICE}, {GOOD, NO_LAUNCHES, E_TIMED}, {GOOD, NO_MS, E_TIMED}},
    3, 9, {4096, 2, 4, 0, 1024}, NO_CASE, pfb_more_refusals};

// PFB, integrated: device and host entries at N = 4096 (the fused stand-in), at a staged length and at a chirp-z length (fold ->
// transform -> rows through the two stagings); K that does not divide a chunk's frames, so that units are carried across chunks
// together with the T - 1 blocks of overlap; split calls with few groups; pageable and pinned arrays; two streams on one plan;
// set_pfb between calls.  The complex64 and the int16 leg run the same cases.
static const std::vector<Row> PFB_INTEGRATED_ROWS{
    // device entry, N = 4096: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
    {DEVICE, P4K, {4096, 4, 5, 1, 4096, MEAN, DB, 1.0f}, 1},
    {DEVICE, P4K, {4096, 4, 30, 7, 4096, MEAN, POW, 0.25f}, 2},
    {DEVICE, P4K, {4096, 4, 2, 50, 1025, MEAN, DB, 1.0f}, 3},
    {DEVICE, P4K, {4096, 4, 1, 33, 4100, MAX, POW, 2.0f}, 4, TIMED},
    {DEVICE, P4K, {4096, 4, 3, 9, 1, MIN, DB, 1.0f}, 5},
    // ... a staged length: 64 MiB is 65536 folded frames of 128 — two chunks of both stagings, groups (unsplit) and
    // slices (split) carried across the boundary
    {DEVICE, P128, {128, 3, 700, 100, 128, MEAN, POW, 1.0f}, 6},          // 70000 frames, 65536 % 100 != 0
    {DEVICE, P128, {128, 3, 3, 23000, 67, MEAN, DB, 1.0f}, 7, TIMED},     // 69000 frames, split
    {DEVICE, P1000, {1000, 2, 4, 25, 1000, MEAN, DB, 1.0f, true}, 8},     // chirp-z
    // host entry: one chunk; several chunks of 512 frames with K = 7 and K = 3 not dividing them (units carried across
    // chunks together with the 3 blocks of overlap); split calls with few groups; pageable and pinned
    {HOST, P4K, {4096, 4, 3, 2, 4096, MEAN, DB, 1.0f}, 9},
    {HOST, P4K, {4096, 4, 170, 7, 4096, MEAN, DB, 1.0f}, 10},             // 1190 frames: three chunks
    {HOST, P4K, {4096, 4, 400, 3, 2049, MIN, POW, 3.0f}, 11, PINNED},     // overlapped hop, pinned both sides
    {HOST, P4K, {4096, 4, 12, 101, 4096, MEAN, POW, 0.5f}, 12},           // 1212 frames, split
    {HOST, P4K, {4096, 4, 12, 101, 4096, MAX, DB, 1.0f}, 13, PINNED},
    {HOST, P4K, {4096, 4, 1, 1100, 4096, MEAN, POW, 1.0f}, 14},           // one group over three chunks
    {HOST, P128, {128, 3, 900, 40, 128, MEAN, DB, 1.0f}, 15},             // 36000 frames: chunks of 16384
    {HOST, P128, {128, 3, 2, 17000, 128, MAX, POW, 1.0f}, 16, PINNED},    // split, slices across chunks
    {HOST, P1000, {1000, 2, 30, 100, 1000, MAX, DB, 1.0f, true}, 17},     // chirp-z, 24 MB: two chunks
    {STREAMS, P128, {128, 3, 0, 0, 0}, 18},
    {STREAMS, PG, {4096, 0, 0, 0, 0}, 19},
};
static const std::vector<Refusal> PFB_INTEGRATED_REFUSALS{
    {F64, NONE, I_ALL}, {WINDOWED, NONE, I_ALL}, {BARE, NONE, I_ALL} /* no prototype set */, {NO_PLAN, NONE, I_ALL}, {GOOD, NO_IN, I_ALL},
    {GOOD, NO_OUT, I_ALL}, {GOOD, NO_FRAMES, I_ALL}, {GOOD, NO_K, I_ALL}, {GOOD, HUGE_COUNTS, I_ALL}, {GOOD, NO_STRIDE, I_ALL},
    {GOOD, BAD_DET, I_ALL}, {GOOD, BAD_FORM, I_ALL}, {GOOD, NO_LAUNCHES, I_TIMED}, {GOOD, NO_MS, I_TIMED}};
static const Leg<float> PFB_INTEGRATE_LEG{
    "pfb_integrate", &PFB, fill, proto, false,
    {{4096, 4, RECT, 1e-12f, 1, 4, 0} /* max_batch does not apply */, {}, {128, 1 << 20, RECT, 1e-12f, 1, 3, 1}, {},
     {1000, 1 << 20, RECT, 1e-12f, 0, 2, 2}, {4096, 64, RECT, 1e-12f, 1, 0, 0}},
    PFB_INTEGRATED_ROWS, PFB_INTEGRATED_REFUSALS, 77, 5, NO_CASE, {4096, 2, 4, 2, 4096}, nullptr};

// PFB from int16 I,Q: the per-frame entries (N = 4096: one chunk; 1190 frames = three chunks with their 3 blocks of overlap;
// overlapped hop, pinned; a staged length over two chunks of the PFB staging — 70000 folded frames of 128; an odd stride;
// chirp-z), then the integrated cases of the complex64 leg at 4 bytes per sample.  At the chirp-z length the reference is the
// complex64 PFB entry of the same plan on the widened samples — the definition of the int16 entries, and no int16 code.
static const Leg<int16_t> PFB_CI16_LEG{
    "pfb_ci16", &PFB_CI16, fill, proto, true,
    {{4096, 2048, RECT, 1e-12f, 1, 4, 0} /* the per-frame host entries keep to max_batch */, {}, {128, 1 << 20, RECT, 1e-12f, 1, 3, 1}, {},
     {1000, 1 << 20, RECT, 1e-12f, 0, 2, 2}, {4096, 64, RECT, 1e-12f, 1, 0, 0}},
    std::vector<Row>{
        {FRAMES, P4K, {4096, 4, 3, 0, 4096}, 20},
        {FRAMES, P4K, {4096, 4, 1190, 0, 4096}, 21},
        {FRAMES, P4K, {4096, 4, 900, 0, 2049}, 22, PINNED},
        {FRAMES, P128, {128, 3, 70000, 0, 128}, 23},
        {FRAMES, P128, {128, 3, 9, 0, 67}, 24, PINNED},
        {FRAMES_VS_C64, P1000, {1000, 2, 7, 0, 1000}, 25},    // chirp-z
        {FRAMES_VS_C64, P1000, {1000, 2, 5, 0, 333}, 26},
    } + PFB_INTEGRATED_ROWS,
    std::vector<Refusal>{{BARE, NONE, E_FRAMES} /* no prototype set */, {F64, NONE, E_FRAMES}, {WINDOWED, NONE, E_FRAMES}, {NO_PLAN, NONE, E_FRAMES},
                         {GOOD, NO_IN, E_FRAMES}, {GOOD, NO_OUT, E_FRAMES}, {GOOD, NO_FRAMES, E_FRAMES},
                         {GOOD, NO_STRIDE, E_FRAMES} /* stride 0 with more than one frame */, {GOOD, NO_LAUNCHES, E_TIMED}, {GOOD, NO_MS, E_TIMED}}
        + PFB_INTEGRATED_REFUSALS,
    77, 5, {4096, 2, 3, 0, 4096}, {4096, 2, 4, 2, 4096}, nullptr};

template <class S> int run(const Leg<S>& L, int threads, int iters) {
    return run_stress(L.name, threads, iters, [&] { refusals(L); }, [&](int t, int n) { worker(L, t, n); });
}

int main(int argc, char** argv) {
    const char* leg = argc > 1 ? argv[1] : "";
    const int threads = argc > 2 ? atoi(argv[2]) : 2, iters = argc > 3 ? atoi(argv[3]) : 1;
    for (const Leg<float>* L : {&INTEGRATE_LEG, &PFB_LEG, &PFB_INTEGRATE_LEG})
        if (!strcmp(leg, L->name)) return run(*L, threads, iters);
    for (const Leg<int16_t>* L : {&CI16_LEG, &INTEGRATE_CI16_LEG, &PFB_CI16_LEG})
        if (!strcmp(leg, L->name)) return run(*L, threads, iters);
    fprintf(stderr, "usage: %s ci16|integrate|integrate_ci16|pfb|pfb_integrate|pfb_ci16 [threads] [iters]\n", argv[0]);
    return 2;
}

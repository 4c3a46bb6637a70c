// tests/host_api_sk_stress.cpp — drives the host side of the spectral-kurtosis entry points (sdrk_exec_*_sk, _sk_ci16, _pfb_sk,
// _pfb_sk_ci16: csrc/integrate_api.hip on csrc/integrate_call.h and the staging slots of csrc/sdrk_host_pipeline.hip; built with
// the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp)
// for the sanitizer legs of tests/test_host_sanitizers_sk.py.  A program of its own: nothing is loaded into Python, nothing is
// preloaded.
//
//   host_api_sk_stress [threads] [iters]
//
// Every thread runs the cases of the four modes on plans of its own: the device, the timed and the host entries at N = 4096
// (the fused stand-in; behind the filter bank the staged route) and at a staged length, groups and slices carried across chunk
// and staging boundaries, pageable and pinned arrays, an existing integrated call between two SK calls on one plan — and checks
// EVERY element of both planes for equality.  Samples are -1 .. 1 and prototypes -2 .. 2, so S1 and S2 are exact in float32 for
// every K used here and each element has one right value however the call was cut.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

static const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;

template <class S> struct Mode {
    bool pfb;
    const Mode<float>* c64;   // int16 modes: the complex64 mode that defines them, on the widened samples
    decltype(&sdrk_exec_device_sk) device;
    decltype(&sdrk_exec_device_sk_timed_each) timed;
    decltype(&sdrk_exec_host_sk) host;
    decltype(&sdrk_exec_host_integrated) host_integrated;   // the existing call of the same mode
};
static const Mode<float> C64{false, nullptr, sdrk_exec_device_sk, sdrk_exec_device_sk_timed_each, sdrk_exec_host_sk, sdrk_exec_host_integrated};
static const Mode<float> PFB{true, nullptr, sdrk_exec_device_pfb_sk, sdrk_exec_device_pfb_sk_timed_each, sdrk_exec_host_pfb_sk,
                             sdrk_exec_host_pfb_integrated};
static const Mode<int16_t> CI16{false, &C64, sdrk_exec_device_sk_ci16, sdrk_exec_device_sk_ci16_timed_each, sdrk_exec_host_sk_ci16,
                                sdrk_exec_host_integrated_ci16};
static const Mode<int16_t> PFB_CI16{true, &PFB, sdrk_exec_device_pfb_sk_ci16, sdrk_exec_device_pfb_sk_ci16_timed_each,
                                    sdrk_exec_host_pfb_sk_ci16, sdrk_exec_host_pfb_integrated_ci16};

// -1 .. 1: the power is at most 8 without the filter bank and 50 behind two taps of -2 .. 2
template <class S> void fill_small(S* x, size_t n_samples, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (S)((int)((s >> 16) % 3u) - 1);
    }
}

// Wrong elements among the two planes of every group (Case of host_stress.h: det is not read).  The estimator is written out
// here on its own, in float32 and in the order of kernels_sk.h.
template <class S> int wrong_planes(const S* in, const float* h, const Case& c, const float* out) {
    const size_t n = (size_t)c.nfft;
    const float kf = (float)c.k;
    int bad = 0;
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < n; ++k) {
            double sum1 = 0, sum2 = 0;
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                double re = 1.0, im = -1.0;
                folded(in, h, n, c.taps, f * c.stride, k, re, im);
                const double pw = re * re + im * im;
                sum1 += pw;
                sum2 += pw * pw;
            }
            CHECK(sum2 < 16777216.0);   // (exact in float32: the case is a fair one)
            const float s1 = (float)sum1, s2 = (float)sum2;
            const float r = s1 * (1.0f / kf);
            const float want0 = c.form == SDRK_INT_OUT_POWER ? c.scale * r : 3.0f * r + (float)(k & 1023);
            const float d = s1 * s1, ratio = (kf + 1.0f) / (kf - 1.0f);
            const float want1 = d == 0.0f ? 0.0f : ratio * (kf * s2 / d - 1.0f);
            const float got0 = out[g * 2 * n + k], got1 = out[g * 2 * n + n + k];
            if ((got0 != want0 || got1 != want1) && bad++ == 0)
                fprintf(stderr, "nfft=%d taps=%d groups=%zu k=%zu stride=%zu form=%d: group %zu bin %zu is (%.9g, %.9g), not (%.9g, %.9g)\n",
                        c.nfft, c.taps, c.groups, c.k, c.stride, c.form, g, k, (double)got0, (double)got1, (double)want0, (double)want1);
        }
    g_compared += 2 * c.groups * n;
    return bad;
}

struct Plan {
    sdrk_plan* p = nullptr;
    std::vector<float> h;   // empty (data() == nullptr: one block of ones) in the plain modes
};

template <class S> Plan make_plan(const Mode<S>& m, int nfft, int taps, unsigned seed) {
    Plan pl;
    CHECK(sdrk_plan_create(0, nfft, 4 /* max_batch does not apply */, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &pl.p) == SDRK_OK);
    if (pl.p && m.pfb) {
        pl.h = proto(nfft, taps, seed);
        CHECK(sdrk_plan_set_pfb(pl.p, taps, pl.h.data()) == SDRK_OK);
    }
    return pl;
}

enum How { DEVICE, TIMED, HOST, HOST_PINNED };

template <class S> void run_case(const Mode<S>& m, const Plan& pl, const Case& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    Buf<S> in(2 * in_samples(c), pinned);
    Buf<float> out(2 * n_out(c), pinned);
    if (!in.data() || !out.data()) return;
    fill_small(in.data(), in_samples(c), seed);
    std::fill_n(out.data(), 2 * n_out(c), -1.0f);
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(m.device(pl.p, in.data(), c.groups, c.k, c.stride, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(m.timed(pl.p, in.data(), c.groups, c.k, c.stride, c.form, c.scale, out.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(m.host(pl.p, in.data(), c.groups, c.k, c.stride, c.form, c.scale, out.data()) == SDRK_OK);
    }
    CHECK(wrong_planes(in.data(), pl.h.data(), c, out.data()) == 0);
    if (m.c64 && how != TIMED) {   // the complex64 entry of the same plan agrees on the widened samples
        const std::vector<float> wide = widen(in.data(), in_samples(c));
        std::vector<float> ref(2 * n_out(c), -2.0f);
        CHECK(m.c64->host(pl.p, wide.data(), c.groups, c.k, c.stride, c.form, c.scale, ref.data()) == SDRK_OK);
        CHECK(same(out.data(), ref));
    }
}

// An existing integrated call between two SK calls on one plan: one state, one staging, both kinds of rows right.
template <class S> void between_case(const Mode<S>& m, const Plan& pl, int nfft, unsigned seed) {
    const size_t n = (size_t)nfft;
    const Case sk{nfft, pl.h.empty() ? 1 : 2, 3, 40, n, MEAN, POW, 0.5f};     // split: partial rows as well
    const Case mid{nfft, sk.taps, 2, 3, n, MAX, DB, 1.0f};
    std::vector<S> a(2 * in_samples(sk)), b(2 * in_samples(mid));
    std::vector<float> ra(2 * n_out(sk), -1.0f), rb(n_out(mid), -1.0f), rc(2 * n_out(sk), -1.0f);
    fill_small(a.data(), in_samples(sk), seed);
    fill_small(b.data(), in_samples(mid), seed + 1);
    CHECK(m.device(pl.p, a.data(), sk.groups, sk.k, sk.stride, sk.form, sk.scale, ra.data(), nullptr) == SDRK_OK);
    CHECK(m.host_integrated(pl.p, b.data(), mid.groups, mid.k, mid.stride, mid.det, mid.form, mid.scale, rb.data()) == SDRK_OK);
    CHECK(m.host(pl.p, a.data(), sk.groups, sk.k, sk.stride, sk.form, sk.scale, rc.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(pl.p) == SDRK_OK);
    CHECK(wrong_planes(a.data(), pl.h.data(), sk, ra.data()) == 0);
    CHECK(wrong_rows(b.data(), pl.h.data(), mid, rb.data()) == 0);
    CHECK(same(rc.data(), ra));
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s) {
    const int t = m.pfb ? 2 : 1;
    const Plan p4k = make_plan(m, 4096, t, s), p128 = make_plan(m, 128, t, s + 1);
    if (!p4k.p || !p128.p) return;
    // N = 4096, device entry: unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
    run_case(m, p4k, {4096, t, 30, 7, 4096, MEAN, POW, 0.25f}, DEVICE, s + 2);
    run_case(m, p4k, {4096, t, 2, 50, 2049, MEAN, DB, 1.0f}, DEVICE, s + 3);
    run_case(m, p4k, {4096, t, 1, 33, 4100, MEAN, POW, 2.0f}, TIMED, s + 4);
    run_case(m, p4k, {4096, t, 5, 2, 4096, MEAN, DB, 1.0f}, DEVICE, s + 5);                  // the smallest K
    // ... host entry: chunks of 512 frames (1024 of int16), groups and slices across their boundaries
    run_case(m, p4k, {4096, t, 22, 101, 4096, MEAN, POW, 0.5f}, HOST, s + 6);                // 2222 frames, split
    run_case(m, p4k, {4096, t, 700, 3, 2049, MEAN, DB, 1.0f}, HOST_PINNED, s + 7);           // unsplit: rows leave chunk by chunk
    run_case(m, p4k, {4096, t, 1, 2100, 4096, MEAN, POW, 1.0f}, HOST, s + 8);                // one group over the chunks
    // a staged length: 64 MiB of spectra is 65536 frames of 128 — two staging chunks, groups and slices carried across
    // (the int16 modes share the staging and the chunking with the complex64 ones: they run the two long cases once, split)
    if (!m.c64) run_case(m, p128, {128, t, 700, 100, 128, MEAN, POW, 1.0f}, DEVICE, s + 9);  // 70000 frames, 65536 % 100 != 0
    run_case(m, p128, {128, t, 3, 2300, 131, MEAN, DB, 1.0f}, TIMED, s + 10);                // split, spaced
    if (!m.c64) run_case(m, p128, {128, t, 900, 80, 128, MEAN, DB, 1.0f}, HOST, s + 11);     // 72000 frames: several chunks
    else run_case(m, p128, {128, t, 3, 23000, 128, MEAN, DB, 1.0f}, DEVICE, s + 11);         // 69000 frames, split
    run_case(m, p128, {128, t, 2, 3400, 128, MEAN, POW, 1.0f}, HOST_PINNED, s + 12);         // split, slices across chunks
    between_case(m, p4k, 4096, s + 13);
    between_case(m, p128, 128, s + 14);
    for (const Plan* pl : {&p4k, &p128}) CHECK(sdrk_plan_destroy(pl->p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        mode_cases(C64, s);
        mode_cases(CI16, s + 20);
        mode_cases(PFB, s + 40);
        mode_cases(PFB_CI16, s + 60);
    }
}

// Every refusal is SDRK_ERR_INVALID with a message, from all three entries, and the plan still works after.
template <class S> void mode_refusals(const Mode<S>& m) {
    sdrk_plan *f64 = nullptr, *windowed = nullptr, *bare = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_HANN, nullptr, 1e-12f, 1, &windowed) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &bare) == SDRK_OK);
    const Plan good = make_plan(m, 4096, 2, 5);
    if (!f64 || !windowed || !bare || !good.p) return;
    std::vector<S> in(2 * 10 * 4096);
    std::vector<float> out(2 * 4 * 4096);
    fill_small(in.data(), 10 * 4096, 77);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        size_t groups, k, stride;
        int form;
        float* out;
        int launches;
        float* ms;
    };
    const Args ok{good.p, in.data(), 4, 2, 4096, DB, out.data(), 2, ms};
    std::vector<Args> bad;
    auto with = [&](auto change) { Args a = ok; change(a); bad.push_back(a); };
    with([&](Args& a) { a.k = 1; });                          // the estimator divides by k_frames - 1
    with([&](Args& a) { a.k = 0; });
    with([&](Args& a) { a.groups = 0; });
    with([&](Args& a) { a.groups = a.k = (size_t)1 << 40; });
    with([&](Args& a) { a.stride = 0; });
    with([&](Args& a) { a.form = 2; });
    with([&](Args& a) { a.in = nullptr; });
    with([&](Args& a) { a.out = nullptr; });
    with([&](Args& a) { a.p = nullptr; });
    with([&](Args& a) { a.p = f64; });
    if (m.pfb) {
        with([&](Args& a) { a.p = windowed; });
        with([&](Args& a) { a.p = bare; });                   // no prototype set
    }
    for (const Args& a : bad) {
        REFUSED(m.device(a.p, a.in, a.groups, a.k, a.stride, a.form, 1.0f, a.out, nullptr));
        REFUSED(m.timed(a.p, a.in, a.groups, a.k, a.stride, a.form, 1.0f, a.out, a.launches, a.ms));
        REFUSED(m.host(a.p, a.in, a.groups, a.k, a.stride, a.form, 1.0f, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(m.timed(ok.p, ok.in, ok.groups, ok.k, ok.stride, ok.form, 1.0f, ok.out, 0, ms));
    REFUSED(m.timed(ok.p, ok.in, ok.groups, ok.k, ok.stride, ok.form, 1.0f, ok.out, 2, nullptr));
    // detector 3 stays refused by the existing call, with its present message
    REFUSED(m.host_integrated(good.p, in.data(), 4, 2, 4096, 3, DB, 1.0f, out.data()));
    CHECK(strstr(sdrk_last_error(), "SDRK_DET_MEAN"));
    // the refused plan still works, beyond its max_batch of 4
    const Case c{4096, m.pfb ? 2 : 1, 4, 2, 4096, MEAN, DB, 1.0f};
    CHECK(m.host(good.p, in.data(), c.groups, c.k, c.stride, c.form, c.scale, out.data()) == SDRK_OK);
    CHECK(wrong_planes(in.data(), good.h.data(), c, out.data()) == 0);
    for (sdrk_plan* p : {f64, windowed, bare, good.p}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("sk", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(CI16);
                          mode_refusals(PFB);
                          mode_refusals(PFB_CI16);
                      },
                      worker);
}

// tests/host_api_xspec_stress.cpp — drives the host side of the two-channel cross-spectrum entry points (sdrk_exec_*_xspec,
// _xspec_ci16: csrc/integrate_api.hip on csrc/integrate_call.h and the staging slots of csrc/sdrk_host_pipeline.hip; built with
// the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp)
// for the sanitizer legs of tests/test_host_sanitizers_xspec.py.  A program of its own: nothing is loaded into Python, nothing
// is preloaded.
//
//   host_api_xspec_stress [threads] [iters]
//
// Every thread runs the cases of both formats on plans of its own: the device, the timed and the host entries at N = 4096 (the
// fused stand-in) and at a staged length (split -> the stand-in transform once per channel -> columns), groups and slices
// carried across chunk and staging boundaries, pageable and pinned arrays, an existing integrated call between two
// cross-spectrum calls on one plan — and checks EVERY element of all four planes for equality.  Samples are -1 .. 1, so the
// four sums are exact in float32 for every K used here and each element has one right value however the call was cut.
// Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

static const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;

template <class S> struct Mode {
    const Mode<float>* c64;   // int16: the complex64 mode that defines it, on the widened elements
    decltype(&sdrk_exec_device_xspec) device;
    decltype(&sdrk_exec_device_xspec_timed_each) timed;
    decltype(&sdrk_exec_host_xspec) host;
};
static const Mode<float> C64{nullptr, sdrk_exec_device_xspec, sdrk_exec_device_xspec_timed_each, sdrk_exec_host_xspec};
static const Mode<int16_t> I16{&C64, sdrk_exec_device_xspec_ci16, sdrk_exec_device_xspec_ci16_timed_each, sdrk_exec_host_xspec_ci16};

// a Case of host_stress.h counts ELEMENTS here (taps = 1; det and form are not read): 4 values of S per element
inline size_t in_values(const Case& c) { return 4 * in_samples(c); }
inline size_t out_floats(const Case& c) { return 4 * n_out(c); }

template <class S> void fill_small(S* x, size_t n_values, unsigned seed) {   // -1 .. 1
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n_values; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (S)((int)((s >> 16) % 3u) - 1);
    }
}

// Wrong elements among the four planes of every group.  The stand-in spectrum of a channel's frame is (re + 1, im - 1) at
// position k; the sums are written out here on their own, in float64 (exact), the output in float32 as include/sdrk.h says.
template <class S> int wrong_planes(const S* in, const Case& c, const float* out) {
    const size_t n = (size_t)c.nfft;
    const float inv_k = 1.0f / (float)c.k;
    int bad = 0;
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < n; ++k) {
            double sum[4] = {0, 0, 0, 0};
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                const S* e = in + 4 * (f * c.stride + k);
                const double ar = (double)e[0] + 1, ai = (double)e[1] - 1, br = (double)e[2] + 1, bi = (double)e[3] - 1;
                sum[0] += ar * ar + ai * ai;
                sum[1] += br * br + bi * bi;
                sum[2] += ar * br + ai * bi;
                sum[3] += ai * br - ar * bi;
            }
            for (int pl = 0; pl < 4; ++pl) {
                CHECK(std::abs(sum[pl]) < 16777216.0);   // (exact in float32: the case is a fair one)
                const float want = c.scale * ((float)sum[pl] * inv_k), got = out[(g * 4 + pl) * n + k];
                if (got != want && bad++ == 0)
                    fprintf(stderr, "nfft=%d groups=%zu k=%zu stride=%zu: group %zu plane %d bin %zu is %.9g, not %.9g\n", c.nfft,
                            c.groups, c.k, c.stride, g, pl, k, (double)got, (double)want);
            }
        }
    g_compared += 4 * c.groups * n;
    return bad;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4 /* max_batch does not apply */, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

enum How { DEVICE, TIMED, HOST, HOST_PINNED };

template <class S> void run_case(const Mode<S>& m, sdrk_plan* p, const Case& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    Buf<S> in(in_values(c), pinned);
    Buf<float> out(out_floats(c), pinned);
    if (!in.data() || !out.data()) return;
    fill_small(in.data(), in_values(c), seed);
    std::fill_n(out.data(), out_floats(c), -1.0f);
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(m.device(p, in.data(), c.groups, c.k, c.stride, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(m.timed(p, in.data(), c.groups, c.k, c.stride, c.scale, out.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(m.host(p, in.data(), c.groups, c.k, c.stride, c.scale, out.data()) == SDRK_OK);
    }
    CHECK(wrong_planes(in.data(), c, out.data()) == 0);
    if (m.c64 && how != TIMED) {   // the complex64 entry of the same plan agrees on the widened elements
        std::vector<float> wide(in_values(c));
        for (size_t i = 0; i < wide.size(); ++i) wide[i] = (float)in[i];
        std::vector<float> ref(out_floats(c), -2.0f);
        CHECK(m.c64->host(p, wide.data(), c.groups, c.k, c.stride, c.scale, ref.data()) == SDRK_OK);
        CHECK(same(out.data(), ref));
    }
}

// An existing integrated call (float2 state rows, one staged spectrum) between two cross-spectrum calls (four-float state
// rows, two staged spectra and the split frames) on one plan: one state, one staging, both kinds of rows right.
template <class S> void between_case(const Mode<S>& m, sdrk_plan* p, int nfft, unsigned seed) {
    const size_t n = (size_t)nfft;
    const Case xs{nfft, 1, 3, 40, n, MEAN, POW, 0.5f};     // split: partial rows as well
    const Case mid{nfft, 1, 2, 3, n, MAX, DB, 1.0f};
    std::vector<S> a(in_values(xs));
    std::vector<float> b(2 * in_samples(mid));
    std::vector<float> ra(out_floats(xs), -1.0f), rb(n_out(mid), -1.0f), rc(out_floats(xs), -1.0f);
    fill_small(a.data(), a.size(), seed);
    fill_small(b.data(), b.size(), seed + 1);
    CHECK(m.device(p, a.data(), xs.groups, xs.k, xs.stride, xs.scale, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_host_integrated(p, b.data(), mid.groups, mid.k, mid.stride, mid.det, mid.form, mid.scale, rb.data()) == SDRK_OK);
    CHECK(m.host(p, a.data(), xs.groups, xs.k, xs.stride, xs.scale, rc.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_planes(a.data(), xs, ra.data()) == 0);
    CHECK(wrong_rows(b.data(), (const float*)nullptr, mid, rb.data()) == 0);
    CHECK(same(rc.data(), ra));
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s) {
    sdrk_plan *p4k = make_plan(4096), *p128 = make_plan(128);
    if (!p4k || !p128) return;
    // N = 4096, device entry: unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames, K = 1
    run_case(m, p4k, {4096, 1, 30, 7, 4096, MEAN, POW, 0.25f}, DEVICE, s + 2);
    run_case(m, p4k, {4096, 1, 2, 50, 2049, MEAN, POW, 1.0f}, DEVICE, s + 3);
    run_case(m, p4k, {4096, 1, 1, 33, 4100, MEAN, POW, 2.0f}, TIMED, s + 4);
    run_case(m, p4k, {4096, 1, 5, 1, 4096, MEAN, POW, 1.0f}, DEVICE, s + 5);
    // ... host entry: chunks of 256 frames (512 of int16), groups and slices across their boundaries
    run_case(m, p4k, {4096, 1, 11, 101, 4096, MEAN, POW, 0.5f}, HOST, s + 6);               // 1111 frames, split
    run_case(m, p4k, {4096, 1, 350, 3, 2049, MEAN, POW, 1.0f}, HOST_PINNED, s + 7);         // unsplit: rows leave chunk by chunk
    run_case(m, p4k, {4096, 1, 1, 1050, 4096, MEAN, POW, 1.0f}, HOST, s + 8);               // one group over the chunks
    // a staged length: 64 MiB of spectra is 32768 frames of 128 on both channels — two staging chunks, groups and slices carried
    // across (the int16 mode shares the staging and the chunking with the complex64 one: it runs the long cases once, split)
    if (!m.c64) run_case(m, p128, {128, 1, 350, 100, 128, MEAN, POW, 1.0f}, DEVICE, s + 9);  // 35000 frames, 32768 % 100 != 0
    run_case(m, p128, {128, 1, 3, 1200, 131, MEAN, POW, 1.0f}, TIMED, s + 10);               // split, spaced
    if (!m.c64) run_case(m, p128, {128, 1, 450, 80, 128, MEAN, POW, 0.5f}, HOST, s + 11);    // 36000 frames: several chunks
    else run_case(m, p128, {128, 1, 3, 11500, 128, MEAN, POW, 1.0f}, DEVICE, s + 11);        // 34500 frames, split
    run_case(m, p128, {128, 1, 2, 1700, 128, MEAN, POW, 1.0f}, HOST_PINNED, s + 12);         // split, slices across chunks
    between_case(m, p4k, 4096, s + 13);
    between_case(m, p128, 128, s + 14);
    for (sdrk_plan* p : {p4k, p128}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        mode_cases(C64, s);
        mode_cases(I16, s + 20);
    }
}

// Every refusal is SDRK_ERR_INVALID with a message, from all three entries, and the plan still works after.
template <class S> void mode_refusals(const Mode<S>& m) {
    sdrk_plan* f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    sdrk_plan* good = make_plan(4096);
    if (!f64 || !good) return;
    std::vector<S> in(4 * 10 * 4096);
    std::vector<float> out(4 * 4 * 4096);
    fill_small(in.data(), in.size(), 77);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        size_t groups, k, stride;
        float* out;
        int launches;
        float* ms;
    };
    const Args ok{good, in.data(), 4, 2, 4096, out.data(), 2, ms};
    std::vector<Args> bad;
    auto with = [&](auto change) { Args a = ok; change(a); bad.push_back(a); };
    with([&](Args& a) { a.k = 0; });
    with([&](Args& a) { a.groups = 0; });
    with([&](Args& a) { a.groups = a.k = (size_t)1 << 40; });
    with([&](Args& a) { a.stride = 0; });
    with([&](Args& a) { a.in = nullptr; });
    with([&](Args& a) { a.out = nullptr; });
    with([&](Args& a) { a.p = nullptr; });
    with([&](Args& a) { a.p = f64; });
    for (const Args& a : bad) {
        REFUSED(m.device(a.p, a.in, a.groups, a.k, a.stride, 1.0f, a.out, nullptr));
        REFUSED(m.timed(a.p, a.in, a.groups, a.k, a.stride, 1.0f, a.out, a.launches, a.ms));
        REFUSED(m.host(a.p, a.in, a.groups, a.k, a.stride, 1.0f, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(m.timed(ok.p, ok.in, ok.groups, ok.k, ok.stride, 1.0f, ok.out, 0, ms));
    REFUSED(m.timed(ok.p, ok.in, ok.groups, ok.k, ok.stride, 1.0f, ok.out, 2, nullptr));
    // the refused plan still works, beyond its max_batch of 4, and with K = 1
    for (size_t k : {(size_t)2, (size_t)1}) {
        const Case c{4096, 1, 4, k, 4096, MEAN, POW, 1.0f};
        CHECK(m.host(good, in.data(), c.groups, c.k, c.stride, c.scale, out.data()) == SDRK_OK);
        CHECK(wrong_planes(in.data(), c, out.data()) == 0);
    }
    for (sdrk_plan* p : {f64, good}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("xspec", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(I16);
                      },
                      worker);
}

// tests/host_api_corrmat_stress.cpp — drives the host side of the correlation-matrix entry points (sdrk_exec_*_corrmat,
// _corrmat_ci16, _corrmat_iq8: csrc/integrate_api.hip on csrc/integrate_call.h and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels tests/fake_*_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_corrmat.py.  A program of its
// own: nothing is loaded into Python, nothing is preloaded.
//
//   host_api_corrmat_stress [threads] [iters]
//
// Every thread runs the cases of all three formats (8-bit: signed and unsigned) at C = 2, 3 and 8 on plans of its own: the
// device, the timed and the host entries at N = 4096 (the spectra stand-in) and at a staged length (split -> the stand-in
// transform once per channel -> columns), groups and slices carried across chunk and staging boundaries, pageable and pinned
// arrays, an existing integrated call and a two-channel call between two correlation-matrix calls on one plan — and checks EVERY
// element of all C * C planes for equality.  Samples are small, so every sum is exact in float32 for every K used here and each
// element has one right value however the call was cut.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

static const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;

// One format: S the stored component type, `off` what widening takes off a component (cu8: 127.5), the three entries
template <class S> struct Mode {
    const char* name;
    double off;
    std::function<int(sdrk_plan*, const void*, int, size_t, size_t, size_t, float, float*)> device, host;
    std::function<int(sdrk_plan*, const void*, int, size_t, size_t, size_t, float, float*, int, float*)> timed;
};

static const Mode<float> C64{
    "c64", 0.0,
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_device_corrmat(p, x, c, g, k, s, sc, o, nullptr); },
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_host_corrmat(p, x, c, g, k, s, sc, o); },
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o, int n, float* ms) { return sdrk_exec_device_corrmat_timed_each(p, x, c, g, k, s, sc, o, n, ms); }};
static const Mode<int16_t> I16{
    "ci16", 0.0,
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_device_corrmat_ci16(p, x, c, g, k, s, sc, o, nullptr); },
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_host_corrmat_ci16(p, x, c, g, k, s, sc, o); },
    [](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o, int n, float* ms) { return sdrk_exec_device_corrmat_ci16_timed_each(p, x, c, g, k, s, sc, o, n, ms); }};
template <class S> Mode<S> iq8_mode(const char* name, int fmt, double off) {
    return Mode<S>{
        name, off,
        [fmt](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_device_corrmat_iq8(p, x, fmt, c, g, k, s, sc, o, nullptr); },
        [fmt](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o) { return sdrk_exec_host_corrmat_iq8(p, x, fmt, c, g, k, s, sc, o); },
        [fmt](sdrk_plan* p, const void* x, int c, size_t g, size_t k, size_t s, float sc, float* o, int n, float* ms) { return sdrk_exec_device_corrmat_iq8_timed_each(p, x, fmt, c, g, k, s, sc, o, n, ms); }};
}
static const Mode<int8_t> S8 = iq8_mode<int8_t>("ci8", SDRK_IQ8_SIGNED, 0.0);
static const Mode<uint8_t> U8 = iq8_mode<uint8_t>("cu8", SDRK_IQ8_UNSIGNED, 127.5);

// a Case of host_stress.h counts ELEMENTS here (taps = 1; det and form are not read): 2 C values of S per element
inline size_t in_values(const Case& c, int C) { return 2 * (size_t)C * in_samples(c); }
inline size_t out_floats(const Case& c, int C) { return (size_t)C * C * n_out(c); }

template <class S> void fill_small(S* x, size_t n_values, unsigned seed, double off) {   // -1 .. 1 (cu8: -1.5 .. 1.5) once widened
    uint32_t s = seed * 2654435761u + 12345u;
    const int mid = off != 0.0 ? 128 : 0;
    for (size_t i = 0; i < n_values; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (S)(mid + (int)((s >> 16) % (mid ? 4u : 3u)) - (mid ? 2 : 1));
    }
}

// Wrong elements among the C * C planes of every group.  The stand-in spectrum of a channel's frame is (re + 1, im - 1) at
// position k; the sums are written out here on their own, in float64 (exact), the output in float32 as include/sdrk.h says.
template <class S> int wrong_planes(const S* in, double off, int C, const Case& c, const float* out) {
    const size_t n = (size_t)c.nfft, Q = (size_t)C * C;
    const float inv_k = 1.0f / (float)c.k;
    int bad = 0;
    std::vector<double> sum(Q), xr(C), xi(C);
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < n; ++k) {
            std::fill(sum.begin(), sum.end(), 0.0);
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                const S* e = in + 2 * (size_t)C * (f * c.stride + k);
                for (int ch = 0; ch < C; ++ch) xr[ch] = (double)e[2 * ch] - off + 1, xi[ch] = (double)e[2 * ch + 1] - off - 1;
                size_t q = (size_t)C;
                for (int i = 0; i < C; ++i) {
                    sum[i] += xr[i] * xr[i] + xi[i] * xi[i];
                    for (int j = i + 1; j < C; ++j, q += 2) {
                        sum[q] += xr[i] * xr[j] + xi[i] * xi[j];
                        sum[q + 1] += xi[i] * xr[j] - xr[i] * xi[j];
                    }
                }
            }
            for (size_t q = 0; q < Q; ++q) {
                CHECK(std::abs(sum[q]) < 4194304.0);   // (exact in float32, quarters included: the case is a fair one)
                const float want = c.scale * ((float)sum[q] * inv_k), got = out[(g * Q + q) * n + k];
                if (got != want && bad++ == 0)
                    fprintf(stderr, "C=%d nfft=%d groups=%zu k=%zu stride=%zu: group %zu plane %zu bin %zu is %.9g, not %.9g\n", C,
                            c.nfft, c.groups, c.k, c.stride, g, q, k, (double)got, (double)want);
            }
        }
    g_compared += Q * c.groups * n;
    return bad;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4 /* max_batch does not apply */, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

enum How { DEVICE, TIMED, HOST, HOST_PINNED };

template <class S> void run_case(const Mode<S>& m, sdrk_plan* p, int C, const Case& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    // one spare sample in front: the stream starts a sample, not an element, into the buffer
    Buf<S> buf(in_values(c, C) + 2, pinned);
    Buf<float> out(out_floats(c, C), pinned);
    if (!buf.data() || !out.data()) return;
    S* in = buf.data() + 2;
    fill_small(in, in_values(c, C), seed, m.off);
    std::fill_n(out.data(), out_floats(c, C), -1.0f);
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(m.device(p, in, C, c.groups, c.k, c.stride, c.scale, out.data()) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(m.timed(p, in, C, c.groups, c.k, c.stride, c.scale, out.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(m.host(p, in, C, c.groups, c.k, c.stride, c.scale, out.data()) == SDRK_OK);
    }
    CHECK(wrong_planes(in, m.off, C, c, out.data()) == 0);
    if (std::strcmp(m.name, "c64") != 0 && how != TIMED) {   // the complex64 entry of the same plan agrees on the widened elements
        std::vector<float> wide(in_values(c, C));
        for (size_t i = 0; i < wide.size(); ++i) wide[i] = (float)in[i] - (float)m.off;
        std::vector<float> ref(out_floats(c, C), -2.0f);
        CHECK(C64.host(p, wide.data(), C, c.groups, c.k, c.stride, c.scale, ref.data()) == SDRK_OK);
        CHECK(same(out.data(), ref));
    }
}

// An existing integrated call (float2 state rows, one staged spectrum) and a two-channel call (four-float state rows) between
// two correlation-matrix calls (C * C planes of state, C staged spectra) on one plan: one state, one staging, every kind right.
template <class S> void between_case(const Mode<S>& m, sdrk_plan* p, int C, int nfft, unsigned seed) {
    const size_t n = (size_t)nfft;
    const Case cm{nfft, 1, 3, 40, n, MEAN, POW, 0.5f};     // split: partial rows as well
    const Case mid{nfft, 1, 2, 3, n, MAX, DB, 1.0f};
    std::vector<S> a(in_values(cm, C));
    std::vector<float> b(2 * in_samples(mid)), b2(4 * in_samples(mid));
    std::vector<float> ra(out_floats(cm, C), -1.0f), rb(n_out(mid), -1.0f), rc(out_floats(cm, C), -1.0f), rx(4 * n_out(mid)), ry(4 * n_out(mid));
    fill_small(a.data(), a.size(), seed, m.off);
    fill(b.data(), in_samples(mid), seed + 1);
    fill_small(b2.data(), b2.size(), seed + 2, 0.0);
    CHECK(sdrk_exec_host_xspec(p, b2.data(), mid.groups, mid.k, mid.stride, 1.0f, rx.data()) == SDRK_OK);
    CHECK(m.device(p, a.data(), C, cm.groups, cm.k, cm.stride, cm.scale, ra.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_integrated(p, b.data(), mid.groups, mid.k, mid.stride, mid.det, mid.form, mid.scale, rb.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_xspec(p, b2.data(), mid.groups, mid.k, mid.stride, 1.0f, ry.data()) == SDRK_OK);
    CHECK(m.host(p, a.data(), C, cm.groups, cm.k, cm.stride, cm.scale, rc.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_planes(a.data(), m.off, C, cm, ra.data()) == 0);
    CHECK(wrong_rows(b.data(), (const float*)nullptr, mid, rb.data()) == 0);
    CHECK(same(rc.data(), ra));
    CHECK(same(ry.data(), rx));
    if (C == 2 && m.off == 0.0 && std::strcmp(m.name, "c64") == 0) {   // two channels: the two-channel call's planes
        std::vector<float> r2(out_floats(cm, 2), -3.0f);
        CHECK(sdrk_exec_host_xspec(p, a.data(), cm.groups, cm.k, cm.stride, cm.scale, r2.data()) == SDRK_OK);
        CHECK(same(ra.data(), r2));
    }
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s, bool longs) {
    sdrk_plan *p4k = make_plan(4096), *p128 = make_plan(128);
    if (!p4k || !p128) return;
    // N = 4096, device entry: unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames, K = 1
    run_case(m, p4k, 3, {4096, 1, 30, 7, 4096, MEAN, POW, 0.25f}, DEVICE, s + 2);
    run_case(m, p4k, 8, {4096, 1, 2, 50, 2049, MEAN, POW, 1.0f}, DEVICE, s + 3);
    run_case(m, p4k, 2, {4096, 1, 1, 33, 4100, MEAN, POW, 2.0f}, TIMED, s + 4);
    run_case(m, p4k, 3, {4096, 1, 5, 1, 4096, MEAN, POW, 1.0f}, DEVICE, s + 5);
    // ... host entry: chunks of 16 MiB cut at element boundaries (24-, 12- and 6-byte elements do not divide them), groups and
    // slices across their boundaries
    if (longs) run_case(m, p4k, 3, {4096, 1, 11, 101, 4096, MEAN, POW, 0.5f}, HOST, s + 6);     // 1111 frames, split
    else run_case(m, p4k, 3, {4096, 1, 3, 101, 4096, MEAN, POW, 0.5f}, HOST, s + 6);            // 303 frames: two chunks of complex64
    if (longs) run_case(m, p4k, 8, {4096, 1, 150, 3, 2049, MEAN, POW, 1.0f}, HOST_PINNED, s + 7);   // unsplit: rows leave chunk by chunk
    if (longs) run_case(m, p4k, 2, {4096, 1, 1, 1050, 4096, MEAN, POW, 1.0f}, HOST, s + 8);     // one group over the chunks
    // a staged length: 64 MiB of spectra is 21845 frames of 128 on three channels, 8192 on eight — several staging chunks,
    // groups and slices carried across (the long cases run once per thread, from the format that has `longs`)
    if (longs) run_case(m, p128, 3, {128, 1, 350, 100, 128, MEAN, POW, 1.0f}, DEVICE, s + 9);   // 35000 frames, 21845 % 100 != 0
    run_case(m, p128, 8, {128, 1, 3, 1200, 131, MEAN, POW, 1.0f}, TIMED, s + 10);               // split, spaced
    if (longs) run_case(m, p128, 8, {128, 1, 3, 6000, 128, MEAN, POW, 1.0f}, DEVICE, s + 11);   // 18000 frames of 8: split, three staging chunks
    run_case(m, p128, 2, {128, 1, 2, 1700, 128, MEAN, POW, 1.0f}, HOST_PINNED, s + 12);         // split, slices across chunks
    if (longs) between_case(m, p4k, 3, 4096, s + 13);
    between_case(m, p128, 8, 128, s + 14);
    if (longs || m.off == 0.0) between_case(m, p128, 2, 128, s + 15);
    for (sdrk_plan* p : {p4k, p128}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        // (the long cases once per format among three threads: complex64 and cu8, int16, ci8)
        mode_cases(C64, s, t % 3 == 0);
        mode_cases(I16, s + 20, t % 3 == 1);
        mode_cases(S8, s + 40, t % 3 == 2);
        mode_cases(U8, s + 60, t % 3 == 0);
    }
}

// Every refusal is SDRK_ERR_INVALID with a message, from all three entries, and the plan still works after.
template <class S> void mode_refusals(const Mode<S>& m) {
    sdrk_plan* f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    sdrk_plan* good = make_plan(4096);
    if (!f64 || !good) return;
    const int C = 3;
    std::vector<S> in(2 * C * 10 * 4096);
    std::vector<float> out(C * C * 4 * 4096);
    fill_small(in.data(), in.size(), 77, m.off);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        int channels;
        size_t groups, k, stride;
        float* out;
        int launches;
        float* ms;
    };
    const Args ok{good, in.data(), C, 4, 2, 4096, out.data(), 2, ms};
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
    with([&](Args& a) { a.channels = 1; });
    with([&](Args& a) { a.channels = 9; });
    with([&](Args& a) { a.channels = -1; });
    with([&](Args& a) { a.groups = a.k = (size_t)1 << 20; a.stride = (size_t)1 << 30; });                       // elements overflow
    with([&](Args& a) { a.channels = 8; a.groups = a.k = a.stride = (size_t)1 << 20; });                      // their bytes do
    for (const Args& a : bad) {
        REFUSED(m.device(a.p, a.in, a.channels, a.groups, a.k, a.stride, 1.0f, a.out));
        REFUSED(m.timed(a.p, a.in, a.channels, a.groups, a.k, a.stride, 1.0f, a.out, a.launches, a.ms));
        REFUSED(m.host(a.p, a.in, a.channels, a.groups, a.k, a.stride, 1.0f, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(m.timed(ok.p, ok.in, C, ok.groups, ok.k, ok.stride, 1.0f, ok.out, 0, ms));
    REFUSED(m.timed(ok.p, ok.in, C, ok.groups, ok.k, ok.stride, 1.0f, ok.out, 2, nullptr));
    // the refused plan still works, beyond its max_batch of 4, and with K = 1
    for (size_t k : {(size_t)2, (size_t)1}) {
        const Case c{4096, 1, 4, k, 4096, MEAN, POW, 1.0f};
        CHECK(m.host(good, in.data(), C, c.groups, c.k, c.stride, c.scale, out.data()) == SDRK_OK);
        CHECK(wrong_planes(in.data(), m.off, C, c, out.data()) == 0);
    }
    for (sdrk_plan* p : {f64, good}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void format_refusals() {   // an 8-bit format that is neither
    sdrk_plan* good = make_plan(4096);
    if (!good) return;
    std::vector<uint8_t> in(2 * 3 * 2 * 4096, 128);
    std::vector<float> out(9 * 4096);
    float ms[2];
    for (int fmt : {2, -1, 100}) {
        REFUSED(sdrk_exec_device_corrmat_iq8(good, in.data(), fmt, 3, 1, 2, 4096, 1.0f, out.data(), nullptr));
        REFUSED(sdrk_exec_device_corrmat_iq8_timed_each(good, in.data(), fmt, 3, 1, 2, 4096, 1.0f, out.data(), 2, ms));
        REFUSED(sdrk_exec_host_corrmat_iq8(good, in.data(), fmt, 3, 1, 2, 4096, 1.0f, out.data()));
    }
    CHECK(sdrk_plan_destroy(good) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("corrmat", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(I16);
                          mode_refusals(S8);
                          mode_refusals(U8);
                          format_refusals();
                      },
                      worker);
}

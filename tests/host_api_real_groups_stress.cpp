// tests/host_api_real_groups_stress.cpp — drives the host side of the integrated real-input entry points
// (sdrk_exec_*_real_integrated: csrc/ci16_api.hip on the call machinery of csrc/integrate_call.h with rows of nfft + 1 bins;
// built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels
// tests/fake_*_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_real_groups.py.  A program of its own: nothing
// is loaded into Python, nothing is preloaded.
//
//   host_api_real_groups_stress [threads] [iters]
//
// Every thread runs a table of cases on plans of its own — N = 4096 (the fused stand-in) and N = 128 (the staged route) —
// over the four formats, the three detectors, both output forms, K in {1, 2, 3, 7}, the device, timed and host entries,
// pageable and pinned; a host call of more than two 16 MiB chunks whose boundaries cut groups (2048 ru8 frames of 8192 fill a
// chunk; 2048 is no multiple of 7); a staged call of more than one staging chunk; few long groups, which the library splits
// into slices; and a per-frame real call and a complex integrated call between two real-integrated calls on one plan.  EVERY
// output element is compared with the stand-ins' definition (fake_real_groups_kernels.cpp) evaluated here on the widened
// samples, bin N included.  Samples and coefficients are small integers (or halves): every value and sum is exact.
// Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

enum How { DEVICE, TIMED, HOST, HOST_PINNED };

template <class S> struct Fmt;
template <> struct Fmt<float> { static constexpr int code = SDRK_REAL_F32; };
template <> struct Fmt<int16_t> { static constexpr int code = SDRK_REAL_S16; };
template <> struct Fmt<int8_t> { static constexpr int code = SDRK_REAL_S8; };
template <> struct Fmt<uint8_t> { static constexpr int code = SDRK_REAL_U8; };

// the contract of include/sdrk.h, written out on its own
template <class S> float widen1(S v) { return (float)v; }
template <> float widen1<uint8_t>(uint8_t v) { return (float)v - 127.5f; }

// -6 .. 6 (uint8: those values modulo 256, so -133.5 .. 127.5 widened): powers and their sums over a group stay exact
template <class S> void fill_small(S* x, size_t n, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (S)((int)((s >> 16) % 13u) - 6);
    }
}

struct GCase {
    int nfft;
    size_t groups, k, stride;   // stride in REAL samples
    int det, form;
    float scale;
    bool window;
};
static size_t bins(const GCase& c) { return (size_t)c.nfft + 1; }
static size_t in_len(const GCase& c) { return (c.groups * c.k - 1) * c.stride + 2 * (size_t)c.nfft; }

static std::vector<float> window_of(int nfft, unsigned seed) {
    std::vector<float> w(2 * (size_t)nfft);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((int)((i * 5u + seed) % 5u) - 2);   // -2 .. 2, the two halves of a pair differ
    return w;
}

// wrong elements among the rows of one call; how the mean is rounded follows the cut the library makes
template <class S> int wrong_groups(const S* in, const float* w, const GCase& c, const float* out) {
    const size_t n = (size_t)c.nfft, nb = bins(c), ways = c.nfft == 4096 ? 1 : (n + 255) / 256;
    const bool split = sdrk::integrate_split(c.groups * ways, c.k, fakehip::cus()).slices > 1;
    int bad = 0;
    auto z = [&](size_t f, size_t m, double& re, double& im) {
        float a = widen1<S>(in[f * c.stride + 2 * m]), b = widen1<S>(in[f * c.stride + 2 * m + 1]);
        if (w) a *= w[2 * m], b *= w[2 * m + 1];
        re = (double)a + 1.0, im = (double)b - 1.0;
    };
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k <= n; ++k) {
            double sum = 0, hi = -1, lo = 1e30;
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                double kx, ky, mx, my;
                z(f, k % n, kx, ky);
                z(f, (n - k) % n, mx, my);
                const double re = kx + my, im = ky - mx, pw = re * re + im * im;
                sum += pw;
                hi = std::max(hi, pw);
                lo = std::min(lo, pw);
            }
            float r;
            if (c.det == SDRK_DET_MEAN) r = split ? (float)(sum * (1.0 / (double)c.k)) : (float)sum * (1.0f / (float)c.k);
            else r = (float)(c.det == SDRK_DET_MAX ? hi : lo);
            const float want = c.form == SDRK_INT_OUT_POWER ? c.scale * r : 3.0f * r + (float)(k & 1023);
            if (out[g * nb + k] != want && bad++ == 0)
                fprintf(stderr, "real groups nfft=%d groups=%zu k=%zu stride=%zu det=%d form=%d fmt=%d: group %zu bin %zu is %.9g, not %.9g\n",
                        c.nfft, c.groups, c.k, c.stride, c.det, c.form, Fmt<S>::code, g, k, (double)out[g * nb + k], (double)want);
        }
    g_compared += c.groups * nb;
    return bad;
}

static sdrk_plan* make_plan(int nfft, int window_kind = SDRK_WINDOW_RECT, size_t max_batch = 1 << 17) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, max_batch, window_kind, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

template <class S> void group_case(sdrk_plan* p, const GCase& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    const size_t out_n = c.groups * bins(c);
    Buf<S> in(in_len(c), pinned);
    Buf<float> out(out_n + 1, pinned);
    if (!in.data() || !out.data()) return;
    fill_small(in.data(), in_len(c), seed);
    const float pad = -77.0f;
    std::fill_n(out.data(), out_n + 1, pad);
    const std::vector<float> w = window_of(c.nfft, seed);
    CHECK(sdrk_plan_set_real_window(p, c.window ? w.data() : nullptr, c.window ? w.size() : 0) == SDRK_OK);
    const int fmt = Fmt<S>::code;
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(sdrk_exec_device_real_integrated(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(sdrk_exec_device_real_integrated_timed_each(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), 2, ms) == SDRK_OK &&
              ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_host_real_integrated(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data()) == SDRK_OK);
    }
    CHECK(wrong_groups(in.data(), c.window ? w.data() : nullptr, c, out.data()) == 0);
    CHECK(out[out_n] == pad);   // packed rows: nothing behind the last one
}

// A per-frame real call and a complex integrated call between two real-integrated calls on one plan (a windowed, shifting
// plan: the staged route switches both off around its transform and must put them back; the complex call uses the same carry
// rows and staging with rows of nfft): all four right.
static void between_case(sdrk_plan* p, int nfft, unsigned seed) {
    const GCase r{nfft, 5, 3, 2 * (size_t)nfft + 6, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, true};
    const Case c{nfft, 1, 4, 3, (size_t)nfft + 3};
    const size_t nb = bins(r), frames = r.groups * r.k;
    std::vector<int16_t> a(in_len(r));
    std::vector<float> b(2 * in_samples(c));
    std::vector<float> ra(r.groups * nb, -1.0f), rb(frames * nb, -1.0f), rc(n_out(c), -1.0f), rd(r.groups * nb, -1.0f);
    fill_small(a.data(), a.size(), seed);
    fill(b.data(), in_samples(c), seed + 1);
    const std::vector<float> w = window_of(nfft, seed);
    CHECK(sdrk_plan_set_real_window(p, w.data(), w.size()) == SDRK_OK);
    CHECK(sdrk_exec_device_real_integrated(p, a.data(), SDRK_REAL_S16, r.groups, r.k, r.stride, r.det, r.form, 1.0f, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_host_real(p, a.data(), SDRK_REAL_S16, frames, r.stride, rb.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_integrated(p, b.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, rc.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_real_integrated(p, a.data(), SDRK_REAL_S16, r.groups, r.k, r.stride, r.det, r.form, 1.0f, rd.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_groups(a.data(), w.data(), r, ra.data()) == 0);
    CHECK(wrong_groups(a.data(), w.data(), r, rd.data()) == 0);
    CHECK(wrong_rows(b.data(), nullptr, c, rc.data()) == 0);
    // the per-frame dB stand-in (fake_real_kernels.cpp): 3 zk.x - zk.y + 2 zm.x + (k & 1023)
    int bad = 0;
    const size_t n = (size_t)nfft;
    auto z = [&](size_t f, size_t m, float& re, float& im) {
        re = (float)a[f * r.stride + 2 * m] * w[2 * m] + 1.0f, im = (float)a[f * r.stride + 2 * m + 1] * w[2 * m + 1] - 1.0f;
    };
    for (size_t f = 0; f < frames; ++f)
        for (size_t k = 0; k <= n; ++k) {
            float kx, ky, mx, my;
            z(f, k % n, kx, ky);
            z(f, (n - k) % n, mx, my);
            bad += rb[f * nb + k] != 3.0f * kx - ky + 2.0f * mx + (float)(k & 1023);
        }
    g_compared += frames * nb;
    CHECK(bad == 0);
}

// the table of one format: detectors x forms x K over the entries, at both lengths
template <class S> void format_cases(sdrk_plan* p4k, sdrk_plan* p128, unsigned s) {
    static const size_t KS[4] = {1, 2, 3, 7};
    static const How HOWS[4] = {DEVICE, TIMED, HOST, HOST_PINNED};
    int i = 0;
    for (int det : {SDRK_DET_MEAN, SDRK_DET_MAX, SDRK_DET_MIN})
        for (int form : {SDRK_INT_OUT_DB, SDRK_INT_OUT_POWER}) {
            const size_t k = KS[i % 4];
            const How how = HOWS[(i + 1) % 4], how2 = HOWS[(i + 3) % 4];
            const size_t stride4k = i % 3 == 0 ? 8192 : i % 3 == 1 ? 4096 : 8198;
            group_case<S>(p4k, {4096, 30 / k + 1, k, stride4k, det, form, 0.5f, i % 2 == 0}, how, s + i);
            group_case<S>(p128, {128, 700 / k + 1, k, i % 2 ? (size_t)256 : (size_t)262, det, form, 0.25f, i % 2 == 1}, how2, s + 10 + i);
            ++i;
        }
    // few long groups: the library cuts them into slices and finalizes (8 stand-in CUs: 24 resident workgroups)
    group_case<S>(p4k, {4096, 2, 40, 8192, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, true}, DEVICE, s + 30);
    group_case<S>(p4k, {4096, 1, 33, 4096, SDRK_DET_MAX, SDRK_INT_OUT_POWER, 2.0f, false}, HOST, s + 31);
    group_case<S>(p128, {128, 3, 50, 256, SDRK_DET_MIN, SDRK_INT_OUT_POWER, 1.0f, false}, HOST_PINNED, s + 32);
    group_case<S>(p128, {128, 1, 64, 256, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, true}, TIMED, s + 33);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        sdrk_plan *p4k = make_plan(4096, SDRK_WINDOW_HANN), *p128 = make_plan(128, SDRK_WINDOW_HANN);
        if (!p4k || !p128) return;
        format_cases<float>(p4k, p128, s);
        format_cases<int16_t>(p4k, p128, s + 40);
        format_cases<int8_t>(p4k, p128, s + 80);
        format_cases<uint8_t>(p4k, p128, s + 120);
        // more than two 16 MiB host chunks: 2048 ru8 frames of 8192 fill one, and 2048 is no multiple of 7
        group_case<uint8_t>(p4k, {4096, 600, 7, 8192, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 1.0f, false}, t & 1 ? HOST_PINNED : HOST, s + 160);
        // the staged route: 64 MiB of staging is 65027 spectra of 129 bins — two staging chunks, the boundary inside a group
        group_case<uint8_t>(p128, {128, 22000, 3, 256, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f, true}, DEVICE, s + 161);
        group_case<int16_t>(p128, {128, 9500, 7, 256, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, false}, HOST, s + 162);
        between_case(p4k, 4096, s + 170);
        between_case(p128, 128, s + 171);
        CHECK(sdrk_plan_destroy(p4k) == SDRK_OK);
        CHECK(sdrk_plan_destroy(p128) == SDRK_OK);
    }
}

#define UNSUPPORTED(call)                                              \
    do {                                                               \
        if ((call) == SDRK_ERR_UNSUPPORTED) ++g_refused;               \
        else CHECK(!"unsupported: " #call);                            \
    } while (0)

// Every refusal has its status and a message, from every entry, nothing is written, and the plan still works after.
static void refusals() {
    sdrk_plan *f64 = nullptr, *good = make_plan(4096), *chirp = make_plan(1000, SDRK_WINDOW_RECT, 4), *big = make_plan(1 << 21, SDRK_WINDOW_RECT, 1);
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    if (!f64 || !good || !chirp || !big) return;
    std::vector<float> in(4 * 8192 + 8, 1.0f), out(2 * 4200, -5.0f);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        int fmt;
        size_t groups, k, stride;
        int det, form;
        float* out;
    };
    const Args ok{good, in.data(), SDRK_REAL_F32, 2, 2, 8192, SDRK_DET_MEAN, SDRK_INT_OUT_DB, out.data()};
    std::vector<Args> bad;
    auto with = [&](auto change) { Args a = ok; change(a); bad.push_back(a); };
    with([&](Args& a) { a.stride = 8193; });                                                        // odd stride
    with([&](Args& a) { a.in = reinterpret_cast<const char*>(in.data()) + 4; });                   // misaligned pairs
    with([&](Args& a) { a.fmt = SDRK_REAL_S16; a.in = reinterpret_cast<const char*>(in.data()) + 2; });
    with([&](Args& a) { a.fmt = SDRK_REAL_S8; a.in = reinterpret_cast<const char*>(in.data()) + 1; });
    with([&](Args& a) { a.fmt = 4; });
    with([&](Args& a) { a.fmt = -1; });
    with([&](Args& a) { a.det = 3; });
    with([&](Args& a) { a.det = -1; });
    with([&](Args& a) { a.form = 2; });
    with([&](Args& a) { a.k = 0; });
    with([&](Args& a) { a.groups = 0; });
    with([&](Args& a) { a.groups = ~(size_t)0 >> 2; a.k = 8; });                                   // groups * k out of range
    with([&](Args& a) { a.p = f64; });
    with([&](Args& a) { a.p = nullptr; });
    with([&](Args& a) { a.in = nullptr; });
    with([&](Args& a) { a.out = nullptr; });
    with([&](Args& a) { a.stride = 0; });
    for (const Args& a : bad) {
        REFUSED(sdrk_exec_device_real_integrated(a.p, a.in, a.fmt, a.groups, a.k, a.stride, a.det, a.form, 1.0f, a.out, nullptr));
        REFUSED(sdrk_exec_device_real_integrated_timed_each(a.p, a.in, a.fmt, a.groups, a.k, a.stride, a.det, a.form, 1.0f, a.out, 2, ms));
        REFUSED(sdrk_exec_host_real_integrated(a.p, a.in, a.fmt, a.groups, a.k, a.stride, a.det, a.form, 1.0f, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(sdrk_exec_device_real_integrated_timed_each(good, in.data(), ok.fmt, 2, 2, 8192, ok.det, ok.form, 1.0f, out.data(), 0, ms));
    REFUSED(sdrk_exec_device_real_integrated_timed_each(good, in.data(), ok.fmt, 2, 2, 8192, ok.det, ok.form, 1.0f, out.data(), 2, nullptr));
    REFUSED(sdrk_exec_device_real_integrated(good, in.data(), ok.fmt, 2, 2, 8193, ok.det, ok.form, 1.0f, out.data(), nullptr));
    CHECK(strstr(sdrk_last_error(), "odd"));
    REFUSED(sdrk_exec_device_real_integrated(good, in.data(), ok.fmt, 2, 2, 8192, 7, ok.form, 1.0f, out.data(), nullptr));
    CHECK(strstr(sdrk_last_error(), "detector"));
    REFUSED(sdrk_exec_host_real_integrated(f64, in.data(), ok.fmt, 2, 2, 8192, ok.det, ok.form, 1.0f, out.data()));
    CHECK(strstr(sdrk_last_error(), "float64"));
    UNSUPPORTED(sdrk_exec_device_real_integrated(chirp, in.data(), ok.fmt, 1, 1, 2000, ok.det, ok.form, 1.0f, out.data(), nullptr));
    CHECK(strstr(sdrk_last_error(), "chirp-z"));
    UNSUPPORTED(sdrk_exec_host_real_integrated(chirp, in.data(), ok.fmt, 1, 1, 2000, ok.det, ok.form, 1.0f, out.data()));
    UNSUPPORTED(sdrk_exec_device_real_integrated_timed_each(chirp, in.data(), ok.fmt, 1, 1, 2000, ok.det, ok.form, 1.0f, out.data(), 1, ms));
    UNSUPPORTED(sdrk_exec_device_real_integrated(big, in.data(), ok.fmt, 1, 1, 8192, ok.det, ok.form, 1.0f, out.data(), nullptr));
    CHECK(strstr(sdrk_last_error(), "2^20"));
    UNSUPPORTED(sdrk_exec_host_real_integrated(big, in.data(), ok.fmt, 1, 1, 8192, ok.det, ok.form, 1.0f, out.data()));
    CHECK(sdrk_plan_sync(good) == SDRK_OK);
    for (float v : out) CHECK(v == -5.0f);   // nothing was launched
    // the refused plan still works
    group_case<float>(good, {4096, 2, 2, 8192, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, true}, HOST, 5);
    group_case<uint8_t>(good, {4096, 3, 1, 8192, SDRK_DET_MIN, SDRK_INT_OUT_POWER, 3.0f, false}, DEVICE, 6);
    for (sdrk_plan* p : {f64, good, chirp, big}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("real_groups", threads, iters, refusals, worker);
}

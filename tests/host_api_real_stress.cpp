// tests/host_api_real_stress.cpp — drives the host side of the real-input entry points (sdrk_plan_set_real_window,
// sdrk_exec_*_real: csrc/ci16_api.hip on the staging slots of csrc/sdrk_host_pipeline.hip; built with the other host files by
// g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp) for the sanitizer legs
// of tests/test_host_sanitizers_real.py.  A program of its own: nothing is loaded into Python, nothing is preloaded.
//
//   host_api_real_stress [threads] [iters]
//
// Every thread runs the four formats on plans of its own — N = 4096 (the fused stand-in) and N = 128 (the staged route, with
// two staging chunks) — through the device, timed and host entries, both output forms, with and without a window, pageable
// and pinned, overlapped and spaced strides, packed and spaced rows, host calls of several chunks, and a plain complex64 call
// between two real calls; EVERY output element is compared with the stand-ins' definition (fake_real_kernels.cpp) evaluated
// here on the widened samples, bin N included.  Samples and coefficients are small integers: every value is exact.
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

template <class S> void fill_real(S* x, size_t n, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < n; ++i) {
        const unsigned r = rng();
        if (sizeof(S) == 1) x[i] = (S)(r & 0xFF);
        else if (sizeof(S) == 2) x[i] = (S)(int16_t)(r & 0xFFFF);
        else x[i] = (S)((int)(r & 0xFFF) - 2048);
    }
    if (n >= 4 && sizeof(S) <= 2) {   // the edges of the format
        x[0] = (S)(sizeof(S) == 1 ? 0x80 : 0x8000), x[1] = (S)(sizeof(S) == 1 ? 0x7F : 0x7FFF), x[2] = (S)0, x[3] = (S)0xFF;
    }
}

struct RCase {
    int nfft;
    size_t frames, stride;     // stride in REAL samples
    size_t out_stride;         // 0: packed
    bool window;
};
static size_t bins(const RCase& c) { return (size_t)c.nfft + 1; }
static size_t width(const RCase& c) { return c.out_stride ? c.out_stride : bins(c); }
static size_t in_len(const RCase& c) { return (c.frames - 1) * c.stride + 2 * (size_t)c.nfft; }

static std::vector<float> window_of(int nfft, unsigned seed) {
    std::vector<float> w(2 * (size_t)nfft);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((int)((i * 5u + seed) % 5u) - 2);   // -2 .. 2, the two halves of a pair differ
    return w;
}

// wrong elements among dB rows and complex rows (either may be null) of one call; what lies between rows must still be `pad`
template <class S> int wrong_real(const S* in, const float* w, const RCase& c, const float* db, const float* spec, float pad) {
    const size_t n = (size_t)c.nfft, wd = width(c);
    int bad = 0;
    auto z = [&](size_t f, size_t m, float& re, float& im) {
        re = widen1<S>(in[f * c.stride + 2 * m]), im = widen1<S>(in[f * c.stride + 2 * m + 1]);
        if (w) re *= w[2 * m], im *= w[2 * m + 1];
        re += 1.0f, im -= 1.0f;
    };
    for (size_t f = 0; f < c.frames; ++f) {
        for (size_t k = 0; k <= n; ++k) {
            float kx, ky, mx, my;
            z(f, k % n, kx, ky);
            z(f, (n - k) % n, mx, my);
            const float want = 3.0f * kx - ky + 2.0f * mx + (float)(k & 1023);
            const size_t i = f * wd + k;
            bool wrong = db && db[i] != want;
            wrong |= spec && (spec[2 * i] != kx + my || spec[2 * i + 1] != ky - mx);
            if (wrong && bad++ == 0)
                fprintf(stderr, "real nfft=%d frames=%zu stride=%zu out_stride=%zu fmt=%d: frame %zu bin %zu is wrong (dB wants %.9g)\n", c.nfft,
                        c.frames, c.stride, c.out_stride, Fmt<S>::code, f, k, (double)want);
        }
        for (size_t k = n + 1; k < wd; ++k) {
            if (db && db[f * wd + k] != pad) ++bad;
            if (spec && (spec[2 * (f * wd + k)] != pad || spec[2 * (f * wd + k) + 1] != pad)) ++bad;
        }
    }
    g_compared += ((db ? 1 : 0) + (spec ? 2 : 0)) * c.frames * wd;
    return bad;
}

static sdrk_plan* make_plan(int nfft, int window_kind = SDRK_WINDOW_RECT, size_t max_batch = 1 << 17) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, max_batch, window_kind, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

template <class S> void real_case(sdrk_plan* p, const RCase& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    const size_t out_n = c.frames * width(c);
    Buf<S> in(in_len(c), pinned);
    Buf<float> db(out_n, pinned), spec(2 * out_n, pinned);
    if (!in.data() || !db.data() || !spec.data()) return;
    fill_real(in.data(), in_len(c), seed);
    const float pad = -77.0f;
    std::fill_n(db.data(), out_n, pad);
    std::fill_n(spec.data(), 2 * out_n, pad);
    const std::vector<float> w = window_of(c.nfft, seed);
    CHECK(sdrk_plan_set_real_window(p, c.window ? w.data() : nullptr, c.window ? w.size() : 0) == SDRK_OK);
    const int fmt = Fmt<S>::code;
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(sdrk_exec_device_real(p, in.data(), fmt, c.frames, c.stride, SDRK_REAL_OUT_DB, db.data(), c.out_stride, nullptr) == SDRK_OK);
        CHECK(sdrk_exec_device_real(p, in.data(), fmt, c.frames, c.stride, SDRK_REAL_OUT_COMPLEX, spec.data(), c.out_stride, nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(sdrk_exec_device_real_timed_each(p, in.data(), fmt, c.frames, c.stride, SDRK_REAL_OUT_DB, db.data(), c.out_stride, 2, ms) == SDRK_OK &&
              ms[0] > 0 && ms[1] > 0);
        CHECK(sdrk_exec_device_real_timed_each(p, in.data(), fmt, c.frames, c.stride, SDRK_REAL_OUT_COMPLEX, spec.data(), c.out_stride, 1, ms) == SDRK_OK);
    } else {   // (the host entries write packed rows)
        CHECK(sdrk_exec_host_real(p, in.data(), fmt, c.frames, c.stride, db.data()) == SDRK_OK);
        CHECK(sdrk_exec_fft_host_real(p, in.data(), fmt, c.frames, c.stride, spec.data()) == SDRK_OK);
    }
    CHECK(wrong_real(in.data(), c.window ? w.data() : nullptr, c, db.data(), spec.data(), pad) == 0);
}

// A plain complex64 call between two real calls on one plan (a windowed, shifting plan: the staged route switches both off
// around its transform and must put them back): all three right.
static void between_case(sdrk_plan* p, int nfft, unsigned seed) {
    const RCase r{nfft, 9, 2 * (size_t)nfft + 6, 0, true};
    const Case c{nfft, 1, 9, 0, (size_t)nfft + 3};
    std::vector<int16_t> a(in_len(r));
    std::vector<float> b(2 * in_samples(c));
    std::vector<float> ra(r.frames * bins(r), -1.0f), rb(n_out(c), -1.0f), rc(2 * r.frames * bins(r), -1.0f);
    fill_real(a.data(), a.size(), seed);
    fill_wide(b.data(), in_samples(c), seed + 1);
    const std::vector<float> w = window_of(nfft, seed);
    CHECK(sdrk_plan_set_real_window(p, w.data(), w.size()) == SDRK_OK);
    CHECK(sdrk_exec_device_real(p, a.data(), SDRK_REAL_S16, r.frames, r.stride, SDRK_REAL_OUT_DB, ra.data(), 0, nullptr) == SDRK_OK);
    CHECK(sdrk_exec_host(p, b.data(), c.groups, c.stride, rb.data()) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_real(p, a.data(), SDRK_REAL_S16, r.frames, r.stride, rc.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_real(a.data(), w.data(), r, ra.data(), rc.data(), -1.0f) == 0);
    CHECK(wrong_frames(b.data(), nullptr, c, {rb.data()}) == 0);
}

template <class S> void format_cases(sdrk_plan* p4k, sdrk_plan* p128, unsigned s) {
    const size_t big = 2400000 / (8192 * sizeof(S)) + 8;   // > 2 MiB of input: several host chunks
    real_case<S>(p4k, {4096, 1, 8192, 0, false}, HOST, s + 1);
    real_case<S>(p4k, {4096, big, 8192, 0, true}, HOST, s + 2);
    real_case<S>(p4k, {4096, big / 2 + 3, 8198, 0, false}, HOST_PINNED, s + 3);   // gaps, a ragged last chunk
    real_case<S>(p4k, {4096, 40, 4096, 0, true}, HOST, s + 4);                    // overlapped
    real_case<S>(p4k, {4096, 13, 8192, 4100, true}, DEVICE, s + 5);
    real_case<S>(p4k, {4096, 3, 2, 0, false}, TIMED, s + 6);
    // the staged route: 64 MiB of staging is 65536 frames of 128 pairs — two staging chunks
    real_case<S>(p128, {128, 66000, 256, 0, false}, DEVICE, s + 7);
    real_case<S>(p128, {128, 5000, 200, 0, true}, HOST, s + 8);
    real_case<S>(p128, {128, 3000, 262, 131, true}, TIMED, s + 9);
    real_case<S>(p128, {128, 9000, 256, 0, true}, HOST_PINNED, s + 10);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        sdrk_plan *p4k = make_plan(4096, SDRK_WINDOW_HANN), *p128 = make_plan(128, SDRK_WINDOW_HANN);
        if (!p4k || !p128) return;
        format_cases<float>(p4k, p128, s);
        format_cases<int16_t>(p4k, p128, s + 20);
        format_cases<int8_t>(p4k, p128, s + 40);
        format_cases<uint8_t>(p4k, p128, s + 60);
        between_case(p4k, 4096, s + 80);
        between_case(p128, 128, s + 81);
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
    std::vector<float> in(4 * 8192 + 8, 1.0f), out(2 * 4 * 4200, -5.0f), w(8192 + 2, 1.0f);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        int fmt;
        size_t n, stride;
        int form;
        void* out;
        size_t out_stride;
    };
    const Args ok{good, in.data(), SDRK_REAL_F32, 4, 8192, SDRK_REAL_OUT_DB, out.data(), 0};
    std::vector<Args> bad;
    auto with = [&](auto change) { Args a = ok; change(a); bad.push_back(a); };
    with([&](Args& a) { a.stride = 8193; });                                                        // odd stride
    with([&](Args& a) { a.in = reinterpret_cast<const char*>(in.data()) + 4; });                   // misaligned pairs
    with([&](Args& a) { a.fmt = SDRK_REAL_S16; a.in = reinterpret_cast<const char*>(in.data()) + 2; });
    with([&](Args& a) { a.fmt = SDRK_REAL_S8; a.in = reinterpret_cast<const char*>(in.data()) + 1; });
    with([&](Args& a) { a.fmt = 4; });
    with([&](Args& a) { a.fmt = -1; });
    with([&](Args& a) { a.p = f64; });
    with([&](Args& a) { a.p = nullptr; });
    with([&](Args& a) { a.in = nullptr; });
    with([&](Args& a) { a.out = nullptr; });
    with([&](Args& a) { a.stride = 0; });
    for (const Args& a : bad) {
        REFUSED(sdrk_exec_device_real(a.p, a.in, a.fmt, a.n, a.stride, a.form, a.out, a.out_stride, nullptr));
        REFUSED(sdrk_exec_device_real_timed_each(a.p, a.in, a.fmt, a.n, a.stride, a.form, a.out, a.out_stride, 2, ms));
        REFUSED(sdrk_exec_host_real(a.p, a.in, a.fmt, a.n, a.stride, static_cast<float*>(a.out)));
        REFUSED(sdrk_exec_fft_host_real(a.p, a.in, a.fmt, a.n, a.stride, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(sdrk_exec_device_real(good, in.data(), ok.fmt, 4, 8192, 2, out.data(), 0, nullptr));            // unknown out_form
    REFUSED(sdrk_exec_device_real(good, in.data(), ok.fmt, 4, 8192, ok.form, out.data(), 4096, nullptr));   // out_stride < N + 1
    CHECK(strstr(sdrk_last_error(), "out_stride"));
    REFUSED(sdrk_exec_device_real_timed_each(good, in.data(), ok.fmt, 4, 8192, ok.form, out.data(), 0, 0, ms));
    REFUSED(sdrk_exec_device_real_timed_each(good, in.data(), ok.fmt, 4, 8192, ok.form, out.data(), 0, 2, nullptr));
    REFUSED(sdrk_exec_host_real(good, in.data(), ok.fmt, ((size_t)1 << 17) + 1, 2, out.data()));            // beyond max_batch
    REFUSED(sdrk_plan_set_real_window(good, w.data(), 8190));
    REFUSED(sdrk_plan_set_real_window(good, w.data(), 4096));
    CHECK(strstr(sdrk_last_error(), "2*nfft"));
    REFUSED(sdrk_plan_set_real_window(good, nullptr, 8192));
    REFUSED(sdrk_plan_set_real_window(f64, w.data(), 8192));
    CHECK(strstr(sdrk_last_error(), "float64"));
    REFUSED(sdrk_plan_set_real_window(nullptr, w.data(), 8192));
    UNSUPPORTED(sdrk_exec_device_real(chirp, in.data(), ok.fmt, 1, 2000, ok.form, out.data(), 0, nullptr));
    CHECK(strstr(sdrk_last_error(), "chirp-z"));
    UNSUPPORTED(sdrk_exec_host_real(chirp, in.data(), ok.fmt, 1, 2000, out.data()));
    UNSUPPORTED(sdrk_plan_set_real_window(chirp, w.data(), 2000));
    UNSUPPORTED(sdrk_exec_device_real(big, in.data(), ok.fmt, 0, 0, ok.form, out.data(), 0, nullptr));
    CHECK(strstr(sdrk_last_error(), "2^20"));
    UNSUPPORTED(sdrk_exec_fft_host_real(big, in.data(), ok.fmt, 0, 0, out.data()));
    CHECK(sdrk_plan_sync(good) == SDRK_OK);
    for (float v : out) CHECK(v == -5.0f);   // nothing was launched
    // the refused plan still works
    real_case<float>(good, {4096, 4, 8192, 0, true}, HOST, 5);
    real_case<uint8_t>(good, {4096, 4, 8192, 4099, false}, DEVICE, 6);
    for (sdrk_plan* p : {f64, good, chirp, big}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("real", threads, iters, refusals, worker);
}

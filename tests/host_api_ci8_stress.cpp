// tests/host_api_ci8_stress.cpp — drives the host side of the 8-bit entry points (sdrk_exec_*_ci8, sdrk_exec_*_integrated_ci8:
// csrc/ci16_api.hip and csrc/integrate_api.hip on the staging slots of csrc/sdrk_host_pipeline.hip; built with the other host
// files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp) for the
// sanitizer legs of tests/test_host_sanitizers_ci8.py.  A program of its own: nothing is loaded into Python, nothing is
// preloaded.
//
//   host_api_ci8_stress [threads] [iters]
//
// Every thread runs both formats on plans of its own: per-frame host calls (rows and spectra) of several chunks, pageable and
// pinned, the device and the timed entry, the unpack route of a length without an 8-bit kernel with two staging chunks, the
// integrated entries with groups and slices across chunk boundaries, an int16 call between two 8-bit calls on one plan — and
// checks EVERY output element for equality with the stand-ins' definition on the widened samples (host_stress.h).  Per-frame
// inputs cover the whole byte range; integrated inputs stay within 6.5 of zero, so every sum is exact.  Exit code 0 = every
// check passed.
#include "host_stress.h"

#include <cstring>

static const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;

// the contract of include/sdrk.h, written out on its own
static std::vector<float> widen8(const uint8_t* in, size_t n_samples, int fmt) {
    std::vector<float> w(2 * n_samples);
    for (size_t i = 0; i < 2 * n_samples; ++i)
        w[i] = fmt == SDRK_IQ8_SIGNED ? (float)(int8_t)in[i] : (float)in[i] - 127.5f;
    return w;
}

// bytes over the whole range, or (small) within 6.5 of the format's zero
static void fill8(uint8_t* x, size_t n_samples, int fmt, bool small, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        if (!small) x[i] = (uint8_t)(rng() & 0xFF);
        else if (fmt == SDRK_IQ8_SIGNED) x[i] = (uint8_t)(int8_t)((int)(rng() % 13u) - 6);
        else x[i] = (uint8_t)(121 + rng() % 14u);
    }
    if (!small && n_samples >= 2) x[0] = 0, x[1] = 127, x[2] = 128, x[3] = 255;
}

enum How { DEVICE, TIMED, HOST, HOST_PINNED };

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 1 << 17, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

// a per-frame call of c.groups frames: dB rows from the entry `how` names, and the complex spectra of the host entry
static void frames_case(sdrk_plan* p, int fmt, const Case& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    Buf<uint8_t> in(2 * in_samples(c), pinned);
    Buf<float> db(n_out(c), pinned), spec(2 * n_out(c), pinned);
    if (!in.data() || !db.data() || !spec.data()) return;
    fill8(in.data(), in_samples(c), fmt, false, seed);
    std::fill_n(db.data(), n_out(c), -1.0f);
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(sdrk_exec_device_ci8(p, in.data(), fmt, c.groups, c.stride, db.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(sdrk_exec_device_ci8_timed_each(p, in.data(), fmt, c.groups, c.stride, db.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_host_ci8(p, in.data(), fmt, c.groups, c.stride, db.data()) == SDRK_OK);
    }
    const std::vector<float> wide = widen8(in.data(), in_samples(c), fmt);
    if (how == HOST || how == HOST_PINNED) {
        CHECK(sdrk_exec_fft_host_ci8(p, in.data(), fmt, c.groups, c.stride, spec.data()) == SDRK_OK);
        CHECK(wrong_frames(wide.data(), nullptr, c, {db.data()}, spec.data()) == 0);
    } else {
        CHECK(wrong_frames(wide.data(), nullptr, c, {db.data()}) == 0);
    }
}

static void rows_case(sdrk_plan* p, int fmt, const Case& c, How how, unsigned seed) {
    const bool pinned = how == HOST_PINNED;
    Buf<uint8_t> in(2 * in_samples(c), pinned);
    Buf<float> out(n_out(c), pinned);
    if (!in.data() || !out.data()) return;
    fill8(in.data(), in_samples(c), fmt, true, seed);
    std::fill_n(out.data(), n_out(c), -1.0f);
    float ms[2] = {0, 0};
    if (how == DEVICE) {
        CHECK(sdrk_exec_device_integrated_ci8(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else if (how == TIMED) {
        CHECK(sdrk_exec_device_integrated_ci8_timed_each(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), 2, ms) == SDRK_OK &&
              ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_host_integrated_ci8(p, in.data(), fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data()) == SDRK_OK);
    }
    const std::vector<float> wide = widen8(in.data(), in_samples(c), fmt);
    CHECK(wrong_rows(wide.data(), nullptr, c, out.data()) == 0);
    if (how != TIMED) {   // the complex64 entry of the same plan agrees on the widened samples
        std::vector<float> ref(n_out(c), -2.0f);
        CHECK(sdrk_exec_host_integrated(p, wide.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, ref.data()) == SDRK_OK);
        CHECK(same(out.data(), ref));
    }
}

// An int16 call between two 8-bit calls on one plan (they share the unpack staging at the staged length): all three right.
static void between_case(sdrk_plan* p, int fmt, int nfft, unsigned seed) {
    const Case c{nfft, 1, 9, 0, (size_t)nfft + 3};
    std::vector<uint8_t> a(2 * in_samples(c));
    std::vector<int16_t> b(2 * in_samples(c));
    std::vector<float> ra(n_out(c), -1.0f), rb(n_out(c), -1.0f), rc(n_out(c), -1.0f);
    fill8(a.data(), in_samples(c), fmt, false, seed);
    fill_wide(b.data(), in_samples(c), seed + 1);
    CHECK(sdrk_exec_device_ci8(p, a.data(), fmt, c.groups, c.stride, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_host_ci16(p, b.data(), c.groups, c.stride, rb.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_ci8(p, a.data(), fmt, c.groups, c.stride, rc.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_frames(widen8(a.data(), in_samples(c), fmt).data(), nullptr, c, {ra.data(), rc.data()}) == 0);
    CHECK(wrong_frames(b.data(), nullptr, c, {rb.data()}) == 0);
}

static void format_cases(int fmt, unsigned s) {
    sdrk_plan *p4k = make_plan(4096), *p128 = make_plan(128);
    if (!p4k || !p128) return;
    // N = 4096 per frame: the small mapped call, chunks the stand-in kernel reads in place, the three-slot pipeline (pinned
    // arrays are not read in place), overlapped and odd strides
    frames_case(p4k, fmt, {4096, 1, 1, 0, 4096}, HOST, s + 1);
    frames_case(p4k, fmt, {4096, 1, 600, 0, 4096}, HOST, s + 2);            // 4.7 MiB: four chunks
    frames_case(p4k, fmt, {4096, 1, 777, 0, 4097}, HOST_PINNED, s + 3);     // odd sample offsets, a ragged last chunk
    frames_case(p4k, fmt, {4096, 1, 300, 0, 2048}, HOST, s + 4);            // overlapped: the copy engines
    frames_case(p4k, fmt, {4096, 1, 40, 0, 5000}, DEVICE, s + 5);
    frames_case(p4k, fmt, {4096, 1, 3, 0, 1}, TIMED, s + 6);
    // the unpack route: 64 MiB of staging is 65536 frames of 128 — two staging chunks; overlapped and spaced chunking
    frames_case(p128, fmt, {128, 1, 70000, 0, 128}, DEVICE, s + 7);
    frames_case(p128, fmt, {128, 1, 5000, 0, 100}, HOST, s + 8);
    frames_case(p128, fmt, {128, 1, 3000, 0, 131}, HOST_PINNED, s + 9);
    // integrated, N = 4096: chunks of 2048 frames, groups and slices across their boundaries
    rows_case(p4k, fmt, {4096, 1, 30, 7, 4096, MEAN, POW, 0.25f}, DEVICE, s + 10);
    rows_case(p4k, fmt, {4096, 1, 2, 50, 2049, MAX, DB, 1.0f}, TIMED, s + 11);
    rows_case(p4k, fmt, {4096, 1, 22, 101, 4096, MEAN, POW, 0.5f}, HOST, s + 12);          // 2222 frames, split
    rows_case(p4k, fmt, {4096, 1, 1400, 3, 2049, MIN, DB, 1.0f}, HOST_PINNED, s + 13);     // unsplit: rows leave chunk by chunk
    rows_case(p4k, fmt, {4096, 1, 1, 2100, 4097, MEAN, DB, 1.0f}, HOST, s + 14);           // one group over the chunks
    // ... and a staged length
    rows_case(p128, fmt, {128, 1, 3, 2300, 131, MEAN, DB, 1.0f}, DEVICE, s + 15);
    rows_case(p128, fmt, {128, 1, 900, 80, 128, MAX, POW, 2.0f}, HOST, s + 16);            // 72000 frames: two staging chunks
    between_case(p4k, fmt, 4096, s + 17);
    between_case(p128, fmt, 128, s + 18);
    CHECK(sdrk_plan_destroy(p4k) == SDRK_OK);
    CHECK(sdrk_plan_destroy(p128) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        format_cases(SDRK_IQ8_SIGNED, s);
        format_cases(SDRK_IQ8_UNSIGNED, s + 50);
    }
}

// Every refusal is SDRK_ERR_INVALID with a message, from all seven entries, and the plan still works after.
static void refusals() {
    sdrk_plan *f64 = nullptr, *good = make_plan(4096);
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    if (!f64 || !good) return;
    std::vector<uint8_t> in(2 * 10 * 4096);
    std::vector<float> out(2 * 10 * 4096);
    fill8(in.data(), 10 * 4096, SDRK_IQ8_UNSIGNED, true, 77);
    float ms[2];
    struct Args {
        sdrk_plan* p;
        const void* in;
        int fmt;
        size_t n, k, stride;
        int det, form;
        float* out;
    };
    const Args ok{good, in.data(), SDRK_IQ8_UNSIGNED, 4, 2, 4096, MEAN, DB, out.data()};
    std::vector<Args> frames, rows;   // refused by the per-frame entries and the integrated ones / by the integrated ones alone
    auto with = [&](std::vector<Args>& to, auto change) { Args a = ok; change(a); to.push_back(a); };
    with(frames, [&](Args& a) { a.fmt = 2; });
    with(frames, [&](Args& a) { a.fmt = -1; });
    with(frames, [&](Args& a) { a.p = f64; });
    with(frames, [&](Args& a) { a.p = nullptr; });
    with(frames, [&](Args& a) { a.in = nullptr; });
    with(frames, [&](Args& a) { a.out = nullptr; });
    with(frames, [&](Args& a) { a.stride = 0; });
    with(rows, [&](Args& a) { a.k = 0; });
    with(rows, [&](Args& a) { a.n = 0; });
    with(rows, [&](Args& a) { a.n = a.k = (size_t)1 << 40; });
    with(rows, [&](Args& a) { a.det = 3; });
    with(rows, [&](Args& a) { a.form = 2; });
    for (const Args& a : frames) {
        REFUSED(sdrk_exec_host_ci8(a.p, a.in, a.fmt, a.n, a.stride, a.out));
        REFUSED(sdrk_exec_fft_host_ci8(a.p, a.in, a.fmt, a.n, a.stride, a.out));
        REFUSED(sdrk_exec_device_ci8(a.p, a.in, a.fmt, a.n, a.stride, a.out, nullptr));
        REFUSED(sdrk_exec_device_ci8_timed_each(a.p, a.in, a.fmt, a.n, a.stride, a.out, 2, ms));
        CHECK(sdrk_last_error()[0]);
    }
    frames.insert(frames.end(), rows.begin(), rows.end());
    for (const Args& a : frames) {
        REFUSED(sdrk_exec_device_integrated_ci8(a.p, a.in, a.fmt, a.n, a.k, a.stride, a.det, a.form, 1.0f, a.out, nullptr));
        REFUSED(sdrk_exec_device_integrated_ci8_timed_each(a.p, a.in, a.fmt, a.n, a.k, a.stride, a.det, a.form, 1.0f, a.out, 2, ms));
        REFUSED(sdrk_exec_host_integrated_ci8(a.p, a.in, a.fmt, a.n, a.k, a.stride, a.det, a.form, 1.0f, a.out));
        CHECK(sdrk_last_error()[0]);
    }
    REFUSED(sdrk_exec_host_ci8(good, in.data(), ok.fmt, ((size_t)1 << 17) + 1, 1, out.data()));   // beyond max_batch
    REFUSED(sdrk_exec_device_ci8_timed_each(good, in.data(), ok.fmt, 4, 4096, out.data(), 0, ms));
    REFUSED(sdrk_exec_device_ci8_timed_each(good, in.data(), ok.fmt, 4, 4096, out.data(), 2, nullptr));
    REFUSED(sdrk_exec_device_integrated_ci8_timed_each(good, in.data(), ok.fmt, 4, 2, 4096, MEAN, DB, 1.0f, out.data(), 0, ms));
    REFUSED(sdrk_exec_device_ci8(good, in.data(), 7, 4, 4096, out.data(), nullptr));
    CHECK(strstr(sdrk_last_error(), "SDRK_IQ8_SIGNED"));
    REFUSED(sdrk_exec_host_integrated_ci8(f64, in.data(), ok.fmt, 4, 2, 4096, MEAN, DB, 1.0f, out.data()));
    CHECK(strstr(sdrk_last_error(), "float64"));
    // the refused plan still works
    rows_case(good, SDRK_IQ8_UNSIGNED, {4096, 1, 4, 2, 4096, MEAN, DB, 1.0f}, HOST, 5);
    frames_case(good, SDRK_IQ8_SIGNED, {4096, 1, 4, 0, 4096}, HOST, 6);
    CHECK(sdrk_plan_destroy(f64) == SDRK_OK);
    CHECK(sdrk_plan_destroy(good) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("ci8", threads, iters, refusals, worker);
}

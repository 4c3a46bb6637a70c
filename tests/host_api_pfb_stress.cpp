// tests/host_api_pfb_stress.cpp — drives the host side of the polyphase-filter-bank entry points (csrc/pfb_api.hip on top of
// csrc/sdrk_host_pipeline.hip's numpy boundary; built with the other host files by g++ against the stand-in runtime of
// tests/fake_hip and the stand-in kernels of tests/fake_pfb_kernels.cpp) for the sanitizer legs of
// tests/test_host_sanitizers_pfb.py.
//
// Samples and coefficients are small integers, so the fold is exact in float32 and every output element has one right value:
// 3 re(y) - im(y) + (k & 1023) for the dB epilogue, (re(y) + 1, im(y) - 1) for the complex one, y the folded frame.  Covered:
// the mapped small call, the three-slot pipeline with the (T - 1) * nfft samples of overlap every chunk carries, ragged last
// chunks, pageable and pinned arrays, N = 4096 and lengths folded into the plan's staging (several chunks of it, growth under
// work in flight, two streams on one plan), a chirp-z length, set_pfb between calls, and the refusals — several threads on their
// own plans at once.  Exit code 0 = every check passed.
#include "../include/sdrk.h"

#include <hip/hip_runtime.h>   // the stand-in runtime: a stream of the caller's own

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

static std::atomic<int> g_bad{0};
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            if (g_bad.fetch_add(1) < 20) fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, sdrk_last_error()); \
        }                                                                                    \
    } while (0)

static void fill(float* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (float)((int)(rng() & 0xFFF) - 2048);
}

static std::vector<float> taps_of(int nfft, int taps, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<float> h((size_t)taps * nfft);
    for (float& v : h) v = (float)((int)(rng() % 7) - 3);
    return h;
}

// folded sample k of frame f (exact: |sum| < 2^24)
static void folded(const float* in, const std::vector<float>& h, int nfft, int taps, size_t f, size_t stride, size_t k, float& re, float& im) {
    re = im = 0.0f;
    for (int t = 0; t < taps; ++t) {
        const size_t s = f * stride + (size_t)t * nfft + k;
        re += h[(size_t)t * nfft + k] * in[2 * s];
        im += h[(size_t)t * nfft + k] * in[2 * s + 1];
    }
}

static int wrong_rows(const float* in, const std::vector<float>& h, const float* db, int nfft, int taps, size_t n_frames, size_t stride) {
    int bad = 0;
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) {
            float re, im;
            folded(in, h, nfft, taps, f, stride, k, re, im);
            bad += db[f * nfft + k] != 3.0f * re - im + (float)(k & 1023);
        }
    return bad;
}

// One host call of each epilogue over (n_frames, stride), from pageable or pinned (library-allocated) arrays.
static void host_case(sdrk_plan* p, const std::vector<float>& h, int nfft, int taps, size_t n_frames, size_t stride, bool pinned, unsigned seed) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)taps * nfft, rows = n_frames * (size_t)nfft;
    std::vector<float> in_v, db_v, c_v;
    float *in = nullptr, *db = nullptr, *cx = nullptr;
    if (pinned) {
        void *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(sdrk_host_alloc(in_samples * 8, &a) == SDRK_OK);
        CHECK(sdrk_host_alloc(rows * 4, &b) == SDRK_OK);
        CHECK(sdrk_host_alloc(rows * 8, &c) == SDRK_OK);
        in = static_cast<float*>(a), db = static_cast<float*>(b), cx = static_cast<float*>(c);
        if (!in || !db || !cx) return;
    } else {
        in_v.resize(2 * in_samples), db_v.resize(rows), c_v.resize(2 * rows);
        in = in_v.data(), db = db_v.data(), cx = c_v.data();
    }
    fill(in, in_samples, seed);
    CHECK(sdrk_exec_host_pfb(p, in, n_frames, stride, db) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_pfb(p, in, n_frames, stride, cx) == SDRK_OK);
    int bad = wrong_rows(in, h, db, nfft, taps, n_frames, stride);
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) {
            float re, im;
            folded(in, h, nfft, taps, f, stride, k, re, im);
            bad += cx[2 * (f * nfft + k)] != re + 1.0f || cx[2 * (f * nfft + k) + 1] != im - 1.0f;
        }
    CHECK(bad == 0);
    if (pinned) {
        CHECK(sdrk_host_free(in) == SDRK_OK);
        CHECK(sdrk_host_free(db) == SDRK_OK);
        CHECK(sdrk_host_free(cx) == SDRK_OK);
    }
}

// A chirp-z length (the stand-in kernels chain differently there): the PFB call against the ordinary call on the folded frames.
static void chirpz_case(sdrk_plan* p, const std::vector<float>& h, int nfft, int taps, size_t n_frames, size_t stride, unsigned seed) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)taps * nfft;
    std::vector<float> in(2 * in_samples), y(2 * n_frames * (size_t)nfft), a(n_frames * (size_t)nfft, -1.0f), b(a.size(), -2.0f);
    fill(in.data(), in_samples, seed);
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) folded(in.data(), h, nfft, taps, f, stride, k, y[2 * (f * nfft + k)], y[2 * (f * nfft + k) + 1]);
    CHECK(sdrk_exec_host_pfb(p, in.data(), n_frames, stride, a.data()) == SDRK_OK);
    CHECK(sdrk_exec_host(p, y.data(), n_frames, nfft, b.data()) == SDRK_OK);
    CHECK(a == b);
}

// The device entry point ("device" memory is host memory here): asynchronous, any number of frames, the staging in chunks.
static void device_case(sdrk_plan* p, const std::vector<float>& h, int nfft, int taps, size_t n_frames, size_t stride, unsigned seed, bool timed = false) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)taps * nfft;
    std::vector<float> in(2 * in_samples), db(n_frames * (size_t)nfft, -1.0f);
    fill(in.data(), in_samples, seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(sdrk_exec_device_pfb_timed_each(p, in.data(), n_frames, stride, db.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_device_pfb(p, in.data(), n_frames, stride, db.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    }
    CHECK(wrong_rows(in.data(), h, db.data(), nfft, taps, n_frames, stride) == 0);
}

// A small call still in flight when a larger one makes the staging grow; then a third on a stream of the caller's.
static void growth_case(sdrk_plan* p, const std::vector<float>& h, int nfft, int taps, unsigned seed) {
    const size_t small_frames = 3, big_frames = 40, span = (size_t)taps * nfft;
    std::vector<float> a(2 * ((small_frames - 1) * nfft + span)), b(2 * ((big_frames - 1) * nfft + span));
    std::vector<float> ra(small_frames * (size_t)nfft), rb(big_frames * (size_t)nfft), rc(small_frames * (size_t)nfft);
    fill(a.data(), a.size() / 2, seed);
    fill(b.data(), b.size() / 2, seed + 1);
    CHECK(sdrk_exec_device_pfb(p, a.data(), small_frames, nfft, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb(p, b.data(), big_frames, nfft, rb.data(), nullptr) == SDRK_OK);    // grows: must wait for the first
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), h, ra.data(), nfft, taps, small_frames, nfft) == 0);
    CHECK(wrong_rows(b.data(), h, rb.data(), nfft, taps, big_frames, nfft) == 0);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(sdrk_exec_device_pfb(p, b.data(), big_frames, nfft, rb.data(), nullptr) == SDRK_OK);    // plan's stream ...
    CHECK(sdrk_exec_device_pfb(p, a.data(), small_frames, nfft, rc.data(), s) == SDRK_OK);         // ... then the caller's: same staging
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), h, rc.data(), nfft, taps, small_frames, nfft) == 0);
    CHECK(wrong_rows(b.data(), h, rb.data(), nfft, taps, big_frames, nfft) == 0);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p1k = nullptr, *p128 = nullptr, *p64k = nullptr, *p1000 = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p4k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1024, 1 << 20, SDRK_WINDOW_RECT, nullptr, 0.0f, 0, &p1k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 128, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p128) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 65536, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p64k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1000, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p1000) == SDRK_OK);
        if (!p4k || !p1k || !p128 || !p64k || !p1000) return;
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        const std::vector<float> h4k = taps_of(4096, 4, s + 50), h4k2 = taps_of(4096, 2, s + 51), h1k = taps_of(1024, 3, s + 52),
                                 h128 = taps_of(128, 5, s + 53), h64k = taps_of(65536, 2, s + 54), h1000 = taps_of(1000, 3, s + 55);
        CHECK(sdrk_plan_pfb_taps(p4k) == 0);
        CHECK(sdrk_plan_set_pfb(p4k, 4, h4k.data()) == SDRK_OK && sdrk_plan_pfb_taps(p4k) == 4);
        CHECK(sdrk_plan_set_pfb(p1k, 3, h1k.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p128, 5, h128.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p64k, 2, h64k.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p1000, 3, h1000.data()) == SDRK_OK);
        host_case(p4k, h4k, 4096, 4, 1, 4096, false, s + 1);         // one frame of four blocks: 128 KiB, the mapped small path
        host_case(p128, h128, 128, 5, 5, 128, false, s + 2);         // small call of a staged length
        host_case(p4k, h4k, 4096, 4, 3, 4096, true, s + 3);          // pinned, small
        host_case(p4k, h4k, 4096, 4, 600, 4096, false, s + 4);       // 19 MiB: four chunks, three blocks of overlap each
        host_case(p4k, h4k, 4096, 4, 1201, 2049, false, s + 5);      // overlapped frames at an odd hop, ragged last chunk
        host_case(p4k, h4k, 4096, 4, 600, 4096, true, s + 6);        // pinned caller arrays, chunked
        host_case(p1k, h1k, 1024, 3, 3000, 700, false, s + 7);       // staged length, chunked, hop < nfft
        host_case(p64k, h64k, 65536, 2, 21, 32769, false, s + 8);    // two-pass length through the staging
        chirpz_case(p1000, h1000, 1000, 3, 300, 777, s + 9);
        device_case(p1k, h1k, 1024, 3, 9000, 512, s + 10);           // 70 MiB of folded frames: two staging chunks
        device_case(p128, h128, 128, 5, 3000, 131, s + 11, true);    // spaced frames, timed entry
        device_case(p4k, h4k, 4096, 4, 300, 4096, s + 12, true);
        device_case(p1k, h1k, 1024, 3, 1, 0, s + 13);                // one frame, stride 0
        growth_case(p128, h128, 128, 5, s + 14);
        CHECK(sdrk_plan_set_pfb(p4k, 2, h4k2.data()) == SDRK_OK && sdrk_plan_pfb_taps(p4k) == 2);   // another T between calls
        host_case(p4k, h4k2, 4096, 2, 300, 4096, false, s + 15);
        device_case(p4k, h4k2, 4096, 2, 40, 1000, s + 16);
        for (sdrk_plan* p : {p4k, p1k, p128, p64k, p1000}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
    }
}

static void refusals() {
    sdrk_plan *p64 = nullptr, *p32 = nullptr, *pw = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p32) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_HANN, nullptr, 1e-12f, 1, &pw) == SDRK_OK);
    if (!p64 || !p32 || !pw) return;
    const std::vector<float> h = taps_of(4096, 2, 9);
    std::vector<float> in(2 * 8 * 4096), out(2 * 8 * 4096);
    fill(in.data(), 8 * 4096, 3);
    float ms[2];
    for (sdrk_plan* bad : {p64, pw}) {
        CHECK(sdrk_plan_set_pfb(bad, 2, h.data()) == SDRK_ERR_INVALID);
        CHECK(sdrk_exec_host_pfb(bad, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
        CHECK(sdrk_exec_fft_host_pfb(bad, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
        CHECK(sdrk_exec_device_pfb(bad, in.data(), 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
        CHECK(sdrk_exec_device_pfb_timed_each(bad, in.data(), 2, 4096, out.data(), 2, ms) == SDRK_ERR_INVALID);
    }
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);             // no prototype set
    CHECK(sdrk_exec_device_pfb(p32, in.data(), 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_set_pfb(p32, 0, h.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_set_pfb(p32, 33, h.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_set_pfb(p32, 2, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_set_pfb(nullptr, 2, h.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_pfb_taps(nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_plan_set_pfb(p32, 2, h.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_pfb(nullptr, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_pfb(p32, nullptr, 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 2, 4096, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 2, 0, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 0, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 5, 4096, out.data()) == SDRK_ERR_INVALID);          // max_batch is 4
    CHECK(sdrk_exec_fft_host_pfb(p32, in.data(), 0, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb(p32, nullptr, 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb(p32, in.data(), 0, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb_timed_each(p32, in.data(), 2, 4096, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb_timed_each(p32, in.data(), 2, 4096, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    // the refused plan still works, and its ordinary entry point is the ordinary one
    CHECK(sdrk_exec_host_pfb(p32, in.data(), 4, 1024, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), h, out.data(), 4096, 2, 4, 1024) == 0);
    const std::vector<float> one(4096, 1.0f);
    CHECK(sdrk_exec_host(p32, in.data(), 2, 4096, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), one, out.data(), 4096, 1, 2, 4096) == 0);
    for (sdrk_plan* p : {p64, p32, pw}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d pfb threads=%d bad=%d\n", sdrk_version(), threads, g_bad.load());
    return g_bad.load() ? 1 : 0;
}

// tests/host_api_ci16_stress.cpp — drives the host side of the int16 entry points (csrc/ci16_api.hip on top of
// csrc/sdrk_host_pipeline.hip's numpy boundary; built with the other host files by g++ against the stand-in runtime of
// tests/fake_hip and the stand-in kernels of tests/fake_ci16_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_ci16.py.
//
// Every path with 4-byte samples — the mapped small call, the zero-copy chunks, the three-slot DMA pipeline from pageable and
// from pinned caller arrays with ragged last chunks, and for the lengths that are widened first the plan's staging: several
// chunks of it per call, overlapped frames with their halo, spaced frames, a staging that has to grow under work still in
// flight, two streams on one plan — must deliver 3 I - Q + (k & 1023) for every element (complex epilogue: (I + 1, Q - 1)),
// from several threads on their own plans at once.  Exit code 0 = every check passed.
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

static void fill(int16_t* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (int16_t)((int)(rng() & 0xFFFF) - 32768);
}

static int wrong_rows(const int16_t* in, const float* db, int nfft, size_t n_frames, size_t stride) {
    int bad = 0;
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) {
            const float re = (float)in[2 * (f * stride + k)], im = (float)in[2 * (f * stride + k) + 1];
            bad += db[f * nfft + k] != 3.0f * re - im + (float)(k & 1023);
        }
    return bad;
}

// One host call of each epilogue over (n_frames, stride) of nfft, from pageable or pinned (library-allocated) arrays.
static void host_case(sdrk_plan* p, int nfft, size_t n_frames, size_t stride, bool pinned, unsigned seed) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)nfft, rows = n_frames * (size_t)nfft;
    std::vector<int16_t> in_v;
    std::vector<float> db_v, c_v;
    int16_t* in = nullptr;
    float *db = nullptr, *cx = nullptr;
    if (pinned) {
        void *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(sdrk_host_alloc(in_samples * 4, &a) == SDRK_OK);
        CHECK(sdrk_host_alloc(rows * 4, &b) == SDRK_OK);
        CHECK(sdrk_host_alloc(rows * 8, &c) == SDRK_OK);
        in = static_cast<int16_t*>(a), db = static_cast<float*>(b), cx = static_cast<float*>(c);
        if (!in || !db || !cx) return;
    } else {
        in_v.resize(2 * in_samples), db_v.resize(rows), c_v.resize(2 * rows);
        in = in_v.data(), db = db_v.data(), cx = c_v.data();
    }
    fill(in, in_samples, seed);
    CHECK(sdrk_exec_host_ci16(p, in, n_frames, stride, db) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_ci16(p, in, n_frames, stride, cx) == SDRK_OK);
    int bad = wrong_rows(in, db, nfft, n_frames, stride);
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) {
            const float re = (float)in[2 * (f * stride + k)], im = (float)in[2 * (f * stride + k) + 1];
            bad += cx[2 * (f * nfft + k)] != re + 1.0f || cx[2 * (f * nfft + k) + 1] != im - 1.0f;
        }
    CHECK(bad == 0);
    if (pinned) {
        CHECK(sdrk_host_free(in) == SDRK_OK);
        CHECK(sdrk_host_free(db) == SDRK_OK);
        CHECK(sdrk_host_free(cx) == SDRK_OK);
    }
}

// A chirp-z length (the stand-in kernels chain differently there): the int16 call against the complex64 call on the widened samples.
static void chirpz_case(sdrk_plan* p, int nfft, size_t n_frames, unsigned seed) {
    std::vector<int16_t> in(2 * n_frames * (size_t)nfft);
    std::vector<float> wide(in.size()), a(n_frames * (size_t)nfft, -1.0f), b(a.size(), -2.0f);
    fill(in.data(), n_frames * (size_t)nfft, seed);
    for (size_t i = 0; i < in.size(); ++i) wide[i] = (float)in[i];
    CHECK(sdrk_exec_host_ci16(p, in.data(), n_frames, nfft, a.data()) == SDRK_OK);
    CHECK(sdrk_exec_host(p, wide.data(), n_frames, nfft, b.data()) == SDRK_OK);
    CHECK(a == b);
}

// The device entry point ("device" memory is host memory here): asynchronous, any number of frames, the staging in chunks.
static void device_case(sdrk_plan* p, int nfft, size_t n_frames, size_t stride, unsigned seed, bool timed = false) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)nfft;
    std::vector<int16_t> in(2 * in_samples);
    std::vector<float> db(n_frames * (size_t)nfft, -1.0f);
    fill(in.data(), in_samples, seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(sdrk_exec_device_ci16_timed_each(p, in.data(), n_frames, stride, db.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_device_ci16(p, in.data(), n_frames, stride, db.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    }
    CHECK(wrong_rows(in.data(), db.data(), nfft, n_frames, stride) == 0);
}

// A small call still in flight when a larger one makes the staging grow; then a third on a stream of the caller's.
static void growth_case(sdrk_plan* p, int nfft, unsigned seed) {
    const size_t small_frames = 3, big_frames = 40;
    std::vector<int16_t> a(2 * small_frames * (size_t)nfft), b(2 * big_frames * (size_t)nfft);
    std::vector<float> ra(small_frames * (size_t)nfft), rb(big_frames * (size_t)nfft), rc(small_frames * (size_t)nfft);
    fill(a.data(), small_frames * (size_t)nfft, seed);
    fill(b.data(), big_frames * (size_t)nfft, seed + 1);
    CHECK(sdrk_exec_device_ci16(p, a.data(), small_frames, nfft, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_ci16(p, b.data(), big_frames, nfft, rb.data(), nullptr) == SDRK_OK);    // grows: must wait for the first
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), ra.data(), nfft, small_frames, nfft) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), nfft, big_frames, nfft) == 0);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(sdrk_exec_device_ci16(p, b.data(), big_frames, nfft, rb.data(), nullptr) == SDRK_OK);    // plan's stream ...
    CHECK(sdrk_exec_device_ci16(p, a.data(), small_frames, nfft, rc.data(), s) == SDRK_OK);         // ... then the caller's: same staging
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), rc.data(), nfft, small_frames, nfft) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), nfft, big_frames, nfft) == 0);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p1k = nullptr, *p128 = nullptr, *p64k = nullptr, *p1000 = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p4k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1024, 1 << 20, SDRK_WINDOW_HANN, nullptr, 0.0f, 0, &p1k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 128, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p128) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 65536, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p64k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1000, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p1000) == SDRK_OK);
        if (!p4k || !p1k || !p128 || !p64k || !p1000) return;
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        host_case(p4k, 4096, 1, 4096, false, s + 1);         // the live call: 16 KiB, the mapped small path
        host_case(p128, 128, 5, 128, false, s + 2);          // small call of a widened length
        host_case(p4k, 4096, 3, 4096, true, s + 3);          // small, pinned
        host_case(p1k, 1024, 1500, 1024, false, s + 4);      // 6 MiB of packed frames: zero-copy chunks
        host_case(p128, 128, 20000, 128, false, s + 5);      // the same size at a widened length: copy engines
        host_case(p4k, 4096, 2200, 4096, false, s + 6);      // 34 MiB: the DMA pipeline, ragged last chunk
        host_case(p4k, 4096, 3001, 2049, false, s + 7);      // overlapped frames at an odd hop, chunked
        host_case(p4k, 4096, 2200, 4096, true, s + 8);       // pinned caller arrays, chunked
        host_case(p4k, 4096, 100, 4096, true, s + 9);        // pinned both sides, one launch
        host_case(p64k, 65536, 37, 65536, false, s + 10);    // two-pass length through the staging
        host_case(p64k, 65536, 141, 32769, false, s + 11);   // ... overlapped, 18 MiB, ragged chunks
        chirpz_case(p1000, 1000, 700, s + 12);
        device_case(p64k, 65536, 150, 65536, s + 13);        // 75 MiB of complex64: two staging chunks (128 + 22)
        device_case(p64k, 65536, 300, 32769, s + 14);        // overlapped, two chunks, each with its halo
        device_case(p128, 128, 3000, 131, s + 15);           // spaced frames, widened frame by frame
        device_case(p128, 128, 70000, 128, s + 16, true);    // 68 MiB of complex64 at a short length, timed entry
        device_case(p4k, 4096, 777, 4096, s + 17, true);
        device_case(p1k, 1024, 1, 0, s + 18);                // one frame, stride 0
        device_case(p128, 128, 1, 0, s + 19);
        growth_case(p128, 128, s + 20);
        sdrk_plan* pg = nullptr;
        CHECK(sdrk_plan_create(0, 32768, 64, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &pg) == SDRK_OK);
        if (pg) growth_case(pg, 32768, s + 21);
        CHECK(sdrk_plan_destroy(pg) == SDRK_OK);
        for (sdrk_plan* p : {p4k, p1k, p128, p64k, p1000}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
    }
}

static void refusals() {
    sdrk_plan *p64 = nullptr, *p32 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p32) == SDRK_OK);
    if (!p64 || !p32) return;
    std::vector<int16_t> in(2 * 8 * 4096, 1);
    std::vector<float> out(2 * 8 * 4096);
    float ms[2];
    CHECK(sdrk_exec_host_ci16(p64, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_fft_host_ci16(p64, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_ci16(p64, in.data(), 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_ci16_timed_each(p64, in.data(), 2, 4096, out.data(), 2, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(nullptr, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(p32, nullptr, 2, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(p32, in.data(), 2, 4096, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(p32, in.data(), 2, 0, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(p32, in.data(), 5, 4096, out.data()) == SDRK_ERR_INVALID);          // max_batch is 4
    CHECK(sdrk_exec_fft_host_ci16(p32, in.data(), 5, 4096, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_ci16(p32, nullptr, 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_ci16_timed_each(p32, in.data(), 2, 4096, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_ci16_timed_each(p32, in.data(), 2, 4096, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_ci16(p32, nullptr, 0, 4096, nullptr) == SDRK_OK);
    CHECK(sdrk_synth_fill_ci16(0, 1, 0, 2, 4096, nullptr, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_synth_fill_ci16(0, 1, 0, 2, 4095, in.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_synth_fill_ci16(7, 1, 0, 2, 4096, in.data(), nullptr) == SDRK_ERR_NO_DEVICE);
    CHECK(sdrk_synth_fill_ci16(0, 5, 3, 2, 4096, in.data(), nullptr) == SDRK_OK && in[0] == (int16_t)(8 - 2048) && in[3] == (int16_t)(1 - 2048));
    // the refused plans still work
    CHECK(sdrk_exec_host_ci16(p32, in.data(), 4, 4096, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), out.data(), 4096, 4, 4096) == 0);
    CHECK(sdrk_plan_destroy(p64) == SDRK_OK);
    CHECK(sdrk_plan_destroy(p32) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d ci16 threads=%d bad=%d\n", sdrk_version(), threads, g_bad.load());
    return g_bad.load() ? 1 : 0;
}

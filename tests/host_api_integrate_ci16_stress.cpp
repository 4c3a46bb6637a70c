// tests/host_api_integrate_ci16_stress.cpp — drives the host side of the int16 integrated-spectrum entry points
// (csrc/integrate_api.hip on csrc/integrate_call.h, csrc/ci16_api.hip's launch_ci16 and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels of tests/fake_kgroup_ci16_kernels.cpp, fake_integrate_kernels.cpp and fake_ci16_kernels.cpp) for the
// sanitizer legs of tests/test_host_sanitizers_integrate_ci16.py.
//
// Device and host entries, the fused length and the staged ones (an int16-reading length, a widened one, a two-pass one,
// chirp-z), groups split into slices and not, chunks and staging boundaries that cut groups and slices (the carry rows),
// pageable and pinned caller arrays, two streams on one plan, the refusals — from several threads on their own plans at
// once.  Samples are small integers, so every sum is exact and EVERY output element is checked for equality with the
// stand-ins' definition: power (I + 1)^2 + (Q - 1)^2, rows 3 R + (k & 1023) (dB form) or scale * R.  The complex64 entry of
// the same plan must agree on the widened samples.  Exit code 0 = every check passed.
#include "../include/sdrk.h"
#include "../sdr-iq-visualizer_amd/csrc/integrate_split.h"

#include <hip/hip_runtime.h>   // the stand-in runtime: a stream of the caller's own, the stand-in device's CU count

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (int16_t)((int)((s >> 16) % 13u) - 6);
    }
}

struct Case {
    int nfft;
    size_t groups, k, stride;
    int det, form;
    float scale;
    bool chirpz;
};

// Every element of `out` against the definition; how the mean is rounded follows the cut the library makes.
// (chirp-z lengths: the stand-in transforms chain differently there, so the spectrum comes from the library's own int16 complex call)
static int wrong_rows(const int16_t* in, const float* out, const Case& c, sdrk_plan* p = nullptr) {
    std::vector<float> spec;
    if (c.chirpz) {
        spec.resize(2 * c.groups * c.k * (size_t)c.nfft);
        CHECK(p && c.stride == (size_t)c.nfft && sdrk_exec_fft_host_ci16(p, in, c.groups * c.k, c.stride, spec.data()) == SDRK_OK);
    }
    const bool fused = c.nfft == 4096 && !c.chirpz;
    const size_t ways = fused ? 1 : ((size_t)c.nfft + 255) / 256;
    const bool split = sdrk::integrate_split(c.groups * ways, c.k, fakehip::cus()).slices > 1;
    int bad = 0;
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < (size_t)c.nfft; ++k) {
            double sum = 0, hi = -1, lo = 1e30;
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                const double re = c.chirpz ? spec[2 * (f * c.nfft + k)] : in[2 * (f * c.stride + k)] + 1.0;
                const double im = c.chirpz ? spec[2 * (f * c.nfft + k) + 1] : in[2 * (f * c.stride + k) + 1] - 1.0;
                const double pw = re * re + im * im;
                sum += pw;
                hi = std::max(hi, pw);
                lo = std::min(lo, pw);
            }
            float r;
            if (c.det == SDRK_DET_MEAN) r = split ? (float)(sum * (1.0 / (double)c.k)) : (float)sum * (1.0f / (float)c.k);
            else r = (float)(c.det == SDRK_DET_MAX ? hi : lo);
            const float want = c.form == SDRK_INT_OUT_POWER ? c.scale * r : 3.0f * r + (float)(k & 1023);
            if (out[g * (size_t)c.nfft + k] != want && bad++ == 0)
                fprintf(stderr, "nfft=%d groups=%zu k=%zu stride=%zu det=%d form=%d: group %zu bin %zu is %.9g, not %.9g\n", c.nfft,
                        c.groups, c.k, c.stride, c.det, c.form, g, k, (double)out[g * (size_t)c.nfft + k], (double)want);
        }
    return bad;
}

static size_t in_samples(const Case& c) { return (c.groups * c.k - 1) * c.stride + (size_t)c.nfft; }

// (the chirp-z stand-ins differ between the int16 and the complex64 route in how they chain, so only the rest is compared)
static void check_against_c64(sdrk_plan* p, const int16_t* in, const float* out, const Case& c) {
    if (c.chirpz) return;
    const size_t n = in_samples(c);
    std::vector<float> wide(2 * n), ref(c.groups * (size_t)c.nfft, -2.0f);
    for (size_t i = 0; i < 2 * n; ++i) wide[i] = (float)in[i];
    CHECK(sdrk_exec_host_integrated(p, wide.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, ref.data()) == SDRK_OK);
    CHECK(std::equal(ref.begin(), ref.end(), out));
}

static void device_case(sdrk_plan* p, const Case& c, unsigned seed, bool timed = false) {
    std::vector<int16_t> in(2 * in_samples(c));
    std::vector<float> out(c.groups * (size_t)c.nfft, -1.0f);
    fill(in.data(), in_samples(c), seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(sdrk_exec_device_integrated_ci16_timed_each(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), 2, ms) == SDRK_OK
              && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_device_integrated_ci16(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    }
    CHECK(wrong_rows(in.data(), out.data(), c, p) == 0);
}

static void host_case(sdrk_plan* p, const Case& c, bool pinned, unsigned seed, bool against_c64 = false) {
    const size_t n_in = in_samples(c), n_out = c.groups * (size_t)c.nfft;
    std::vector<int16_t> in_v;
    std::vector<float> out_v;
    int16_t* in = nullptr;
    float* out = nullptr;
    if (pinned) {
        void *a = nullptr, *b = nullptr;
        CHECK(sdrk_host_alloc(n_in * 4, &a) == SDRK_OK);
        CHECK(sdrk_host_alloc(n_out * 4, &b) == SDRK_OK);
        in = static_cast<int16_t*>(a), out = static_cast<float*>(b);
        if (!in || !out) return;
    } else {
        in_v.resize(2 * n_in), out_v.resize(n_out);
        in = in_v.data(), out = out_v.data();
    }
    fill(in, n_in, seed);
    for (size_t i = 0; i < n_out; ++i) out[i] = -1.0f;
    CHECK(sdrk_exec_host_integrated_ci16(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out) == SDRK_OK);
    CHECK(wrong_rows(in, out, c, p) == 0);
    if (against_c64) check_against_c64(p, in, out, c);
    if (pinned) {
        CHECK(sdrk_host_free(in) == SDRK_OK);
        CHECK(sdrk_host_free(out) == SDRK_OK);
    }
}

// A small call still in flight when a larger one makes the state and the staging grow; then one on a stream of the caller's;
// then the complex64 entry on the same plan's state, between two int16 calls.
static void growth_case(sdrk_plan* p, int nfft, unsigned seed) {
    const Case small{nfft, 2, 3, (size_t)nfft, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f, false};
    const Case big{nfft, 3, 40, (size_t)nfft, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 0.5f, false};   // split: partial rows as well
    std::vector<int16_t> a(2 * in_samples(small)), b(2 * in_samples(big));
    std::vector<float> ra(small.groups * (size_t)nfft), rb(big.groups * (size_t)nfft), rc(ra.size()), rd(ra.size());
    fill(a.data(), in_samples(small), seed);
    fill(b.data(), in_samples(big), seed + 1);
    CHECK(sdrk_exec_device_integrated_ci16(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, ra.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_integrated_ci16(p, b.data(), big.groups, big.k, big.stride, big.det, big.form, 0.5f, rb.data(), nullptr) == SDRK_OK);   // grows
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), ra.data(), small) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), big) == 0);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    std::vector<float> wide(a.size());
    for (size_t i = 0; i < a.size(); ++i) wide[i] = (float)a[i];
    CHECK(sdrk_exec_device_integrated_ci16(p, b.data(), big.groups, big.k, big.stride, big.det, big.form, 0.5f, rb.data(), nullptr) == SDRK_OK);   // plan's stream ...
    CHECK(sdrk_exec_device_integrated_ci16(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, rc.data(), s) == SDRK_OK);   // ... then the caller's
    CHECK(sdrk_exec_device_integrated(p, wide.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, rd.data(), nullptr) == SDRK_OK);   // ... and the complex64 entry
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), rc.data(), small) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), big) == 0);
    CHECK(rc == rd);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

static void worker(int t, int iters) {
    const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p1k = nullptr, *p128 = nullptr, *p64k = nullptr, *p1000 = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p4k) == SDRK_OK);     // max_batch does not apply
        CHECK(sdrk_plan_create(0, 1024, 1 << 20, SDRK_WINDOW_HANN, nullptr, 0.0f, 0, &p1k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 128, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p128) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 65536, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p64k) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1000, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p1000) == SDRK_OK);
        if (!p4k || !p1k || !p128 || !p64k || !p1000) return;
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        // device entry at the fused length: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
        device_case(p4k, {4096, 5, 1, 4096, MEAN, DB, 1.0f, false}, s + 1);
        device_case(p4k, {4096, 30, 7, 4096, MEAN, POW, 0.25f, false}, s + 2);
        device_case(p4k, {4096, 2, 50, 2049, MEAN, DB, 1.0f, false}, s + 3);
        device_case(p4k, {4096, 1, 33, 4100, MAX, POW, 2.0f, false}, s + 4, true);
        device_case(p4k, {4096, 3, 9, 1001, MIN, DB, 1.0f, false}, s + 5);             // frame starts 4-byte aligned only
        // ... the staged lengths: 64 MiB of spectra is 65536 frames of 128 and 128 frames of 65536 — several spectrum-staging
        // chunks (and, at the widened lengths, the int16 route's own staging inside each), groups and slices carried across
        device_case(p128, {128, 700, 100, 128, MEAN, POW, 1.0f, false}, s + 6);        // 70000 frames, unsplit, 65536 % 100 != 0
        device_case(p128, {128, 3, 23000, 131, MEAN, DB, 1.0f, false}, s + 7, true);    // 69000 frames, split, spaced
        device_case(p64k, {65536, 2, 70, 65536, MEAN, POW, 0.125f, false}, s + 8);      // 140 frames: 128 + 12, split by bins
        device_case(p64k, {65536, 45, 3, 32769, MIN, DB, 1.0f, false}, s + 9);          // 135 frames, overlapped
        device_case(p1k, {1024, 40, 9, 1024, MAX, DB, 1.0f, false}, s + 10);            // a length that reads int16 itself
        device_case(p1k, {1024, 1, 1, 1, MEAN, DB, 1.0f, false}, s + 11);
        device_case(p1000, {1000, 4, 25, 1000, MEAN, DB, 1.0f, true}, s + 12);          // chirp-z
        // host entry: one chunk; several chunks of 1024 frames (4-byte samples) with groups and slices across their
        // boundaries, pageable and pinned
        host_case(p4k, {4096, 3, 2, 4096, MEAN, DB, 1.0f, false}, false, s + 13, true);
        host_case(p4k, {4096, 22, 101, 4096, MEAN, POW, 0.5f, false}, false, s + 14);    // 2222 frames: three chunks, split
        host_case(p4k, {4096, 22, 101, 4096, MAX, DB, 1.0f, false}, true, s + 15);
        host_case(p4k, {4096, 700, 3, 4096, MEAN, DB, 1.0f, false}, false, s + 16, true);   // unsplit: rows leave chunk by chunk
        host_case(p4k, {4096, 700, 3, 2049, MIN, POW, 3.0f, false}, true, s + 17);       // overlapped, pinned both sides
        host_case(p4k, {4096, 1, 2100, 4096, MEAN, POW, 1.0f, false}, false, s + 18);    // one group over three chunks
        host_case(p128, {128, 900, 80, 128, MEAN, DB, 1.0f, false}, false, s + 19, true);   // 72000 frames: three chunks of 32768
        host_case(p128, {128, 2, 34000, 128, MEAN, POW, 1.0f, false}, true, s + 20);     // split, slices across chunks
        host_case(p64k, {65536, 9, 15, 65536, MEAN, DB, 1.0f, false}, false, s + 21);    // 135 frames: chunks of 64, 64 % 15 != 0
        host_case(p1000, {1000, 30, 200, 1000, MAX, DB, 1.0f, true}, false, s + 22);     // chirp-z, 24 MB: two chunks
        host_case(p1k, {1024, 5, 1, 1024, MEAN, DB, 1.0f, false}, true, s + 23, true);
        growth_case(p1k, 1024, s + 24);
        growth_case(p128, 128, s + 25);
        sdrk_plan* pg = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 64, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &pg) == SDRK_OK);
        if (pg) growth_case(pg, 4096, s + 26);
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
    std::vector<float> out(8 * 4096);
    float ms[2];
    CHECK(sdrk_exec_device_integrated_ci16(p64, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p64, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_integrated_ci16_timed_each(p64, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data(), 2, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(nullptr, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, nullptr, 2, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 2, 2, 4096, 0, 0, 1.0f, nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 0, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 2, 0, 4096, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 2, 2, 0, 0, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 2, 2, 4096, 3, 0, 1.0f, out.data()) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_integrated_ci16(p32, in.data(), 2, 2, 4096, 0, 2, 1.0f, out.data(), nullptr) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_integrated_ci16_timed_each(p32, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_integrated_ci16_timed_each(p32, in.data(), 2, 2, 4096, 0, 0, 1.0f, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    // the refused plan still works, beyond its max_batch of 4
    const Case c{4096, 4, 2, 4096, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, false};
    fill(in.data(), 8 * 4096, 77);
    CHECK(sdrk_exec_host_integrated_ci16(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), out.data(), c) == 0);
    CHECK(sdrk_plan_destroy(p64) == SDRK_OK);
    CHECK(sdrk_plan_destroy(p32) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d integrate_ci16 threads=%d bad=%d\n", sdrk_version(), threads, g_bad.load());
    return g_bad.load() ? 1 : 0;
}

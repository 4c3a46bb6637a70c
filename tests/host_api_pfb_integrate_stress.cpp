// tests/host_api_pfb_integrate_stress.cpp — drives the host side of the integrated polyphase-filter-bank entry points
// (csrc/integrate_api.hip on top of csrc/integrate_call.h, csrc/pfb_api.hip and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels of tests/fake_pfb_groups_kernels.cpp, fake_pfb_kernels.cpp and fake_integrate_kernels.cpp) for the sanitizer
// legs of tests/test_host_sanitizers_pfb_integrate.py.
//
// Device and host entries at N = 4096 (the fused stand-in), at a staged length and at a chirp-z length (fold -> transform ->
// rows through the two stagings); K that does not divide a chunk's frames, so that units are carried across chunks together
// with the T - 1 blocks of overlap; split calls with few groups; pageable and pinned arrays; two streams on one plan; set_pfb
// between calls; the refusals — from several threads on their own plans at once.  Samples and coefficients are small
// integers, so every product and sum is exact and EVERY output element is checked for equality with the stand-ins'
// definition: power (re(y) + 1)^2 + (im(y) - 1)^2 of the folded sample y, rows 3 R + (k & 1023) (dB form) or scale * R.
// Exit code 0 = every check passed.
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

static void fill(float* x, size_t n_samples, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (float)((int)((s >> 16) % 13u) - 6);
    }
}

static std::vector<float> proto(int nfft, int taps, unsigned seed) {
    std::vector<float> h((size_t)taps * nfft);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    return h;
}

struct Case {
    int nfft, taps;
    size_t groups, k, stride;
    int det, form;
    float scale;
    bool chirpz;
};

static size_t in_samples(const Case& c) { return (c.groups * c.k - 1) * c.stride + (size_t)c.taps * c.nfft; }

// Every element of `out` against the definition; how the mean is rounded follows the cut the library makes.
// (chirp-z lengths: the stand-in transforms chain differently there, so the spectrum comes from the library's own complex call)
static int wrong_rows(const float* in, const float* out, const Case& c, const std::vector<float>& h, sdrk_plan* p = nullptr) {
    std::vector<float> spec;
    if (c.chirpz) {
        spec.resize(2 * c.groups * c.k * (size_t)c.nfft);
        CHECK(p && sdrk_exec_fft_host_pfb(p, in, c.groups * c.k, c.stride, spec.data()) == SDRK_OK);
    }
    const bool fused = c.nfft == 4096 && !c.chirpz;
    const size_t ways = fused ? 1 : ((size_t)c.nfft + 255) / 256;
    const bool split = sdrk::integrate_split(c.groups * ways, c.k, fakehip::cus()).slices > 1;
    const size_t n = (size_t)c.nfft;
    int bad = 0;
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < n; ++k) {
            double sum = 0, hi = -1, lo = 1e30;
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                double re, im;
                if (c.chirpz) {
                    re = spec[2 * (f * n + k)], im = spec[2 * (f * n + k) + 1];
                } else {
                    re = 1.0, im = -1.0;
                    for (int t = 0; t < c.taps; ++t) {
                        re += (double)in[2 * (f * c.stride + t * n + k)] * h[t * n + k];
                        im += (double)in[2 * (f * c.stride + t * n + k) + 1] * h[t * n + k];
                    }
                }
                const double pw = re * re + im * im;
                sum += pw;
                hi = std::max(hi, pw);
                lo = std::min(lo, pw);
            }
            float r;
            if (c.det == SDRK_DET_MEAN) r = split ? (float)(sum * (1.0 / (double)c.k)) : (float)sum * (1.0f / (float)c.k);
            else r = (float)(c.det == SDRK_DET_MAX ? hi : lo);
            const float want = c.form == SDRK_INT_OUT_POWER ? c.scale * r : 3.0f * r + (float)(k & 1023);
            if (out[g * n + k] != want && bad++ == 0)
                fprintf(stderr, "nfft=%d taps=%d groups=%zu k=%zu stride=%zu det=%d form=%d: group %zu bin %zu is %.9g, not %.9g\n",
                        c.nfft, c.taps, c.groups, c.k, c.stride, c.det, c.form, g, k, (double)out[g * n + k], (double)want);
        }
    return bad;
}

static void device_case(sdrk_plan* p, const Case& c, const std::vector<float>& h, unsigned seed, bool timed = false) {
    std::vector<float> in(2 * in_samples(c)), out(c.groups * (size_t)c.nfft, -1.0f);
    fill(in.data(), in_samples(c), seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(sdrk_exec_device_pfb_integrated_timed_each(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), 2, ms) == SDRK_OK
              && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_device_pfb_integrated(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    }
    CHECK(wrong_rows(in.data(), out.data(), c, h, p) == 0);
}

static void host_case(sdrk_plan* p, const Case& c, const std::vector<float>& h, bool pinned, unsigned seed) {
    const size_t n_in = in_samples(c), n_out = c.groups * (size_t)c.nfft;
    std::vector<float> in_v, out_v;
    float *in = nullptr, *out = nullptr;
    if (pinned) {
        void *a = nullptr, *b = nullptr;
        CHECK(sdrk_host_alloc(n_in * 8, &a) == SDRK_OK);
        CHECK(sdrk_host_alloc(n_out * 4, &b) == SDRK_OK);
        in = static_cast<float*>(a), out = static_cast<float*>(b);
        if (!in || !out) return;
    } else {
        in_v.resize(2 * n_in), out_v.resize(n_out);
        in = in_v.data(), out = out_v.data();
    }
    fill(in, n_in, seed);
    for (size_t i = 0; i < n_out; ++i) out[i] = -1.0f;
    CHECK(sdrk_exec_host_pfb_integrated(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out) == SDRK_OK);
    CHECK(wrong_rows(in, out, c, h, p) == 0);
    if (pinned) {
        CHECK(sdrk_host_free(in) == SDRK_OK);
        CHECK(sdrk_host_free(out) == SDRK_OK);
    }
}

// A call on the plan's stream, then one on a stream of the caller's while the first may still be running: one state, one
// prototype and two stagings per plan.  Then another prototype (another T) with both still recorded on the plan.
static void streams_and_set_pfb(sdrk_plan* p, int nfft, unsigned seed) {
    const std::vector<float> h3 = proto(nfft, 3, seed), h2 = proto(nfft, 2, seed + 1);
    CHECK(sdrk_plan_set_pfb(p, 3, h3.data()) == SDRK_OK);
    const Case big{nfft, 3, 3, 40, (size_t)nfft, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 0.5f, false};   // split: partial rows as well
    const Case small{nfft, 3, 2, 3, (size_t)nfft / 2 + 1, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f, false};
    std::vector<float> a(2 * in_samples(small)), b(2 * in_samples(big));
    std::vector<float> ra(small.groups * (size_t)nfft), rb(big.groups * (size_t)nfft);
    fill(a.data(), in_samples(small), seed);
    fill(b.data(), in_samples(big), seed + 1);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(sdrk_exec_device_pfb_integrated(p, b.data(), big.groups, big.k, big.stride, big.det, big.form, 0.5f, rb.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_integrated(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, ra.data(), s) == SDRK_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), ra.data(), small, h3) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), big, h3) == 0);
    // work of the caller's stream still recorded on the plan when the prototype is replaced
    CHECK(sdrk_exec_device_pfb_integrated(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, ra.data(), s) == SDRK_OK);
    CHECK(sdrk_plan_set_pfb(p, 2, h2.data()) == SDRK_OK);
    CHECK(sdrk_plan_pfb_taps(p) == 2);
    CHECK(wrong_rows(a.data(), ra.data(), small, h3) == 0);   // (set_pfb waited for it)
    Case two = small;
    two.taps = 2;
    device_case(p, two, h2, seed + 2);
    // the per-frame PFB entry and the plain integrated entry of the same plan beside it
    std::vector<float> rows(2 * (size_t)nfft);
    CHECK(sdrk_exec_host_pfb(p, a.data(), 2, (size_t)nfft, rows.data()) == SDRK_OK);
    CHECK(sdrk_exec_host_integrated(p, a.data(), 1, 2, (size_t)nfft, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, rows.data()) == SDRK_OK);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

static void worker(int t, int iters) {
    const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p128 = nullptr, *p1000 = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p4k) == SDRK_OK);     // max_batch does not apply
        CHECK(sdrk_plan_create(0, 128, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p128) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1000, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 0, &p1000) == SDRK_OK);
        if (!p4k || !p128 || !p1000) return;
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        const std::vector<float> h4k = proto(4096, 4, s), h128 = proto(128, 3, s + 1), h1000 = proto(1000, 2, s + 2);
        CHECK(sdrk_plan_set_pfb(p4k, 4, h4k.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p128, 3, h128.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p1000, 2, h1000.data()) == SDRK_OK);
        // device entry, N = 4096: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
        device_case(p4k, {4096, 4, 5, 1, 4096, MEAN, DB, 1.0f, false}, h4k, s + 1);
        device_case(p4k, {4096, 4, 30, 7, 4096, MEAN, POW, 0.25f, false}, h4k, s + 2);
        device_case(p4k, {4096, 4, 2, 50, 1025, MEAN, DB, 1.0f, false}, h4k, s + 3);
        device_case(p4k, {4096, 4, 1, 33, 4100, MAX, POW, 2.0f, false}, h4k, s + 4, true);
        device_case(p4k, {4096, 4, 3, 9, 1, MIN, DB, 1.0f, false}, h4k, s + 5);
        // ... a staged length: 64 MiB is 65536 folded frames of 128 — two chunks of both stagings, groups (unsplit) and
        // slices (split) carried across the boundary
        device_case(p128, {128, 3, 700, 100, 128, MEAN, POW, 1.0f, false}, h128, s + 6);      // 70000 frames, 65536 % 100 != 0
        device_case(p128, {128, 3, 3, 23000, 67, MEAN, DB, 1.0f, false}, h128, s + 7, true);  // 69000 frames, split
        device_case(p1000, {1000, 2, 4, 25, 1000, MEAN, DB, 1.0f, true}, h1000, s + 8);       // chirp-z
        // host entry: one chunk; several chunks of 512 frames with K = 7 and K = 3 not dividing them (units carried across
        // chunks together with the 3 blocks of overlap); split calls with few groups; pageable and pinned
        host_case(p4k, {4096, 4, 3, 2, 4096, MEAN, DB, 1.0f, false}, h4k, false, s + 9);
        host_case(p4k, {4096, 4, 170, 7, 4096, MEAN, DB, 1.0f, false}, h4k, false, s + 10);      // 1190 frames: three chunks
        host_case(p4k, {4096, 4, 400, 3, 2049, MIN, POW, 3.0f, false}, h4k, true, s + 11);       // overlapped hop, pinned both sides
        host_case(p4k, {4096, 4, 12, 101, 4096, MEAN, POW, 0.5f, false}, h4k, false, s + 12);    // 1212 frames, split
        host_case(p4k, {4096, 4, 12, 101, 4096, MAX, DB, 1.0f, false}, h4k, true, s + 13);
        host_case(p4k, {4096, 4, 1, 1100, 4096, MEAN, POW, 1.0f, false}, h4k, false, s + 14);    // one group over three chunks
        host_case(p128, {128, 3, 900, 40, 128, MEAN, DB, 1.0f, false}, h128, false, s + 15);     // 36000 frames: chunks of 16384
        host_case(p128, {128, 3, 2, 17000, 128, MAX, POW, 1.0f, false}, h128, true, s + 16);     // split, slices across chunks
        host_case(p1000, {1000, 2, 30, 100, 1000, MAX, DB, 1.0f, true}, h1000, false, s + 17);   // chirp-z, 24 MB: two chunks
        streams_and_set_pfb(p128, 128, s + 18);
        sdrk_plan* pg = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 64, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &pg) == SDRK_OK);
        if (pg) streams_and_set_pfb(pg, 4096, s + 19);
        CHECK(sdrk_plan_destroy(pg) == SDRK_OK);
        for (sdrk_plan* p : {p4k, p128, p1000}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
    }
}

static void refusals() {
    sdrk_plan *p64 = nullptr, *pw = nullptr, *p32 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_HANN, nullptr, 1e-12f, 1, &pw) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p32) == SDRK_OK);
    if (!p64 || !pw || !p32) return;
    const std::vector<float> h = proto(4096, 2, 5);
    const Case c{4096, 2, 4, 2, 4096, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, false};
    std::vector<float> in(2 * in_samples(c)), out(c.groups * 4096);
    fill(in.data(), in_samples(c), 77);
    float ms[2];
    auto every = [&](sdrk_plan* p, const float* x, size_t g, size_t k, size_t stride, int det, int form, float* o) {
        CHECK(sdrk_exec_device_pfb_integrated(p, x, g, k, stride, det, form, 1.0f, o, nullptr) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_device_pfb_integrated_timed_each(p, x, g, k, stride, det, form, 1.0f, o, 2, ms) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_host_pfb_integrated(p, x, g, k, stride, det, form, 1.0f, o) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
    };
    every(p64, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(pw, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 0, out.data());      // no prototype set
    CHECK(sdrk_plan_set_pfb(p32, 2, h.data()) == SDRK_OK);
    every(nullptr, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(p32, nullptr, 4, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 0, nullptr);
    every(p32, in.data(), 0, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 0, 4096, 0, 0, out.data());
    every(p32, in.data(), (size_t)1 << 40, (size_t)1 << 40, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 0, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 3, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 2, out.data());
    CHECK(sdrk_exec_device_pfb_integrated_timed_each(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb_integrated_timed_each(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    // the refused plan still works, beyond its max_batch of 4
    CHECK(sdrk_exec_host_pfb_integrated(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), out.data(), c, h) == 0);
    for (sdrk_plan* p : {p64, pw, p32}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d pfb_integrate threads=%d bad=%d\n", sdrk_version(), threads, g_bad.load());
    return g_bad.load() ? 1 : 0;
}

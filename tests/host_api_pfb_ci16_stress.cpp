// tests/host_api_pfb_ci16_stress.cpp — drives the host side of the int16 polyphase-filter-bank entry points
// (csrc/pfb_api.hip and csrc/integrate_api.hip on top of csrc/integrate_call.h and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels of tests/fake_pfb_ci16_kernels.cpp beside the existing ones) for the sanitizer legs of
// tests/test_host_sanitizers_pfb_ci16.py.  A program of its own: nothing is loaded into Python, nothing is preloaded.
//
// The per-frame entries (device, timed, host dB, host complex) and the integrated entries (device, timed, host) at N = 4096
// (the fused stand-ins), at a staged length and at a chirp-z length (int16 fold -> transform [-> rows] through the stagings);
// K that does not divide a chunk's frames, so that units are carried across chunks together with the T - 1 blocks of overlap
// at 4 bytes per sample; split calls with few groups; pageable and pinned arrays; two streams on one plan; set_pfb between
// calls; the refusals of every entry — from several threads on their own plans at once.  Samples are small int16 values and coefficients
// small integers, so every product and sum is exact and EVERY output element is checked for equality with the stand-ins'
// definition: per frame 3 re(y) - im(y) + (k & 1023) of the folded sample y (dB form) or (re + 1, im - 1); integrated, the
// power (re(y) + 1)^2 + (im(y) - 1)^2 reduced to rows 3 R + (k & 1023) (dB form) or scale * R.
// At the chirp-z length, where the stand-in transforms give no closed form, the reference is the complex64 PFB entry of the
// same plan on the widened samples.
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

static void fill(int16_t* x, size_t n_samples, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (int16_t)((int)((s >> 16) % 13u) - 6);
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
static std::vector<float> widen(const int16_t* in, size_t n_samples) {
    std::vector<float> w(2 * n_samples);
    for (size_t i = 0; i < 2 * n_samples; ++i) w[i] = (float)in[i];
    return w;
}

// (chirp-z lengths: the stand-in transforms chain differently there, so the spectrum comes from the complex64 PFB call of the
// same plan on the widened samples — the definition of the int16 entries, and no int16 code)
static int wrong_rows(const int16_t* in, const float* out, const Case& c, const std::vector<float>& h, sdrk_plan* p = nullptr) {
    std::vector<float> spec;
    if (c.chirpz) {
        spec.resize(2 * c.groups * c.k * (size_t)c.nfft);
        const std::vector<float> w = widen(in, in_samples(c));
        CHECK(p && sdrk_exec_fft_host_pfb(p, w.data(), c.groups * c.k, c.stride, spec.data()) == SDRK_OK);
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

// dB rows of the per-frame entries against the fold: 3 re(y) - im(y) + (k & 1023)
static int wrong_frames(const int16_t* in, const float* rows, int nfft, int taps, size_t frames, size_t stride, const std::vector<float>& h) {
    const size_t n = (size_t)nfft;
    int bad = 0;
    for (size_t f = 0; f < frames; ++f)
        for (size_t k = 0; k < n; ++k) {
            float re = 0, im = 0;
            for (int t = 0; t < taps; ++t) {
                re += (float)in[2 * (f * stride + t * n + k)] * h[t * n + k];
                im += (float)in[2 * (f * stride + t * n + k) + 1] * h[t * n + k];
            }
            if (rows[f * n + k] != 3.0f * re - im + (float)(k & 1023)) ++bad;
        }
    return bad;
}

static void device_case(sdrk_plan* p, const Case& c, const std::vector<float>& h, unsigned seed, bool timed = false) {
    std::vector<int16_t> in(2 * in_samples(c));
    std::vector<float> out(c.groups * (size_t)c.nfft, -1.0f);
    fill(in.data(), in_samples(c), seed);
    if (timed) {
        float ms[2] = {0, 0};
        CHECK(sdrk_exec_device_pfb_integrated_ci16_timed_each(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), 2, ms) == SDRK_OK
              && ms[0] > 0 && ms[1] > 0);
    } else {
        CHECK(sdrk_exec_device_pfb_integrated_ci16(p, in.data(), c.groups, c.k, c.stride, c.det, c.form, c.scale, out.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    }
    CHECK(wrong_rows(in.data(), out.data(), c, h, p) == 0);
}

static void host_case(sdrk_plan* p, const Case& c, const std::vector<float>& h, bool pinned, unsigned seed) {
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
    CHECK(sdrk_exec_host_pfb_integrated_ci16(p, in, c.groups, c.k, c.stride, c.det, c.form, c.scale, out) == SDRK_OK);
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
    std::vector<int16_t> a(2 * in_samples(small)), b(2 * in_samples(big));
    std::vector<float> ra(small.groups * (size_t)nfft), rb(big.groups * (size_t)nfft);
    fill(a.data(), in_samples(small), seed);
    fill(b.data(), in_samples(big), seed + 1);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(sdrk_exec_device_pfb_integrated_ci16(p, b.data(), big.groups, big.k, big.stride, big.det, big.form, 0.5f, rb.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_integrated_ci16(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, ra.data(), s) == SDRK_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(wrong_rows(a.data(), ra.data(), small, h3) == 0);
    CHECK(wrong_rows(b.data(), rb.data(), big, h3) == 0);
    // work of the caller's stream still recorded on the plan when the prototype is replaced
    CHECK(sdrk_exec_device_pfb_integrated_ci16(p, a.data(), small.groups, small.k, small.stride, small.det, small.form, 1.0f, ra.data(), s) == SDRK_OK);
    CHECK(sdrk_plan_set_pfb(p, 2, h2.data()) == SDRK_OK);
    CHECK(sdrk_plan_pfb_taps(p) == 2);
    CHECK(wrong_rows(a.data(), ra.data(), small, h3) == 0);   // (set_pfb waited for it)
    Case two = small;
    two.taps = 2;
    device_case(p, two, h2, seed + 2);
    // the per-frame PFB entry and the plain integrated entry of the same plan beside it
    std::vector<float> rows(2 * (size_t)nfft, -1.0f);
    CHECK(sdrk_exec_host_pfb_ci16(p, a.data(), 2, (size_t)nfft, rows.data()) == SDRK_OK);
    CHECK(wrong_frames(a.data(), rows.data(), nfft, 2, 2, (size_t)nfft, h2) == 0);
    // (the plain integrated row is the PFB's with one tap of ones)
    const std::vector<float> ones((size_t)nfft, 1.0f);
    const Case plain{nfft, 1, 1, 2, (size_t)nfft, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, false};
    std::fill(rows.begin(), rows.end(), -1.0f);
    CHECK(sdrk_exec_host_integrated_ci16(p, a.data(), 1, 2, (size_t)nfft, SDRK_DET_MEAN, SDRK_INT_OUT_DB, 1.0f, rows.data()) == SDRK_OK);
    CHECK(wrong_rows(a.data(), rows.data(), plain, ones) == 0);
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

// The per-frame entries: device (plain or timed), host dB rows, host complex spectra — every element against the fold.
static void frames_case(sdrk_plan* p, int nfft, int taps, size_t frames, size_t stride, const std::vector<float>& h, bool pinned,
                        unsigned seed) {
    const size_t n = (size_t)nfft, n_in = (frames - 1) * stride + (size_t)taps * n;
    std::vector<int16_t> in_v;
    int16_t* in = nullptr;
    void* a = nullptr;
    if (pinned) {
        CHECK(sdrk_host_alloc(n_in * 4, &a) == SDRK_OK);
        in = static_cast<int16_t*>(a);
        if (!in) return;
    } else {
        in_v.resize(2 * n_in);
        in = in_v.data();
    }
    fill(in, n_in, seed);
    std::vector<float> dev(frames * n, -1.0f), timed(frames * n, -1.0f), host(frames * n, -1.0f), spec(2 * frames * n, -1.0f);
    float ms[2] = {0, 0};
    CHECK(sdrk_exec_device_pfb_ci16(p, in, frames, stride, dev.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_ci16_timed_each(p, in, frames, stride, timed.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    CHECK(sdrk_exec_host_pfb_ci16(p, in, frames, stride, host.data()) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_pfb_ci16(p, in, frames, stride, spec.data()) == SDRK_OK);
    int bad = 0;
    for (size_t f = 0; f < frames; ++f)
        for (size_t k = 0; k < n; ++k) {
            float re = 0, im = 0;
            for (int t = 0; t < taps; ++t) {
                re += (float)in[2 * (f * stride + t * n + k)] * h[t * n + k];
                im += (float)in[2 * (f * stride + t * n + k) + 1] * h[t * n + k];
            }
            const float want = 3.0f * re - im + (float)(k & 1023);
            const size_t i = f * n + k;
            if ((dev[i] != want || timed[i] != want || host[i] != want || spec[2 * i] != re + 1.0f || spec[2 * i + 1] != im - 1.0f) && bad++ == 0)
                fprintf(stderr, "nfft=%d taps=%d frames=%zu stride=%zu: frame %zu bin %zu is %.9g / %.9g / %.9g / (%.9g, %.9g), not %.9g / (%.9g, %.9g)\n",
                        nfft, taps, frames, stride, f, k, (double)dev[i], (double)timed[i], (double)host[i], (double)spec[2 * i],
                        (double)spec[2 * i + 1], (double)want, (double)re + 1.0, (double)im - 1.0);
        }
    CHECK(bad == 0);
    if (pinned) CHECK(sdrk_host_free(a) == SDRK_OK);
}

// The per-frame entries where the stand-in transforms give no closed form (chirp-z): every element against the complex64 PFB
// entries of the same plan on the widened samples, which run none of the int16 code.
static void frames_case_vs_c64(sdrk_plan* p, int nfft, int taps, size_t frames, size_t stride, unsigned seed) {
    const size_t n = (size_t)nfft, n_in = (frames - 1) * stride + (size_t)taps * n;
    std::vector<int16_t> in(2 * n_in);
    fill(in.data(), n_in, seed);
    const std::vector<float> w = widen(in.data(), n_in);
    std::vector<float> dev(frames * n, -1.0f), timed(frames * n, -1.0f), host(frames * n, -1.0f), spec(2 * frames * n, -1.0f);
    std::vector<float> want(frames * n, -2.0f), want_spec(2 * frames * n, -2.0f);
    float ms[2] = {0, 0};
    CHECK(sdrk_exec_host_pfb(p, w.data(), frames, stride, want.data()) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_pfb(p, w.data(), frames, stride, want_spec.data()) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_ci16(p, in.data(), frames, stride, dev.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_ci16_timed_each(p, in.data(), frames, stride, timed.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
    CHECK(sdrk_exec_host_pfb_ci16(p, in.data(), frames, stride, host.data()) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_pfb_ci16(p, in.data(), frames, stride, spec.data()) == SDRK_OK);
    CHECK(dev == want && timed == want && host == want && spec == want_spec);
}

static void worker(int t, int iters) {
    const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p128 = nullptr, *p1000 = nullptr;
        CHECK(sdrk_plan_create(0, 4096, 2048, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p4k) == SDRK_OK);  // (the per-frame host entries keep to max_batch)
        CHECK(sdrk_plan_create(0, 128, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p128) == SDRK_OK);
        CHECK(sdrk_plan_create(0, 1000, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12f, 0, &p1000) == SDRK_OK);
        if (!p4k || !p128 || !p1000) return;
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        const std::vector<float> h4k = proto(4096, 4, s), h128 = proto(128, 3, s + 1), h1000 = proto(1000, 2, s + 2);
        CHECK(sdrk_plan_set_pfb(p4k, 4, h4k.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p128, 3, h128.data()) == SDRK_OK);
        CHECK(sdrk_plan_set_pfb(p1000, 2, h1000.data()) == SDRK_OK);
        // per frame: N = 4096 (one chunk; 1190 frames = three chunks with their 3 blocks of overlap; overlapped hop, pinned),
        // a staged length over two chunks of the PFB staging (70000 folded frames of 128), an odd stride
        frames_case(p4k, 4096, 4, 3, 4096, h4k, false, s + 20);
        frames_case(p4k, 4096, 4, 1190, 4096, h4k, false, s + 21);
        frames_case(p4k, 4096, 4, 900, 2049, h4k, true, s + 22);
        frames_case(p128, 128, 3, 70000, 128, h128, false, s + 23);
        frames_case(p128, 128, 3, 9, 67, h128, true, s + 24);
        frames_case_vs_c64(p1000, 1000, 2, 7, 1000, s + 25);       // chirp-z
        frames_case_vs_c64(p1000, 1000, 2, 5, 333, s + 26);
        // integrated.  device entry, N = 4096: K = 1, unsplit (>= 24 groups on the 8-CU stand-in), split, overlapped and spaced frames
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
    std::vector<int16_t> in(2 * in_samples(c));
    std::vector<float> out(c.groups * 4096);
    fill(in.data(), in_samples(c), 77);
    float ms[2];
    auto every = [&](sdrk_plan* p, const int16_t* x, size_t g, size_t k, size_t stride, int det, int form, float* o) {
        CHECK(sdrk_exec_device_pfb_integrated_ci16(p, x, g, k, stride, det, form, 1.0f, o, nullptr) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_device_pfb_integrated_ci16_timed_each(p, x, g, k, stride, det, form, 1.0f, o, 2, ms) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_host_pfb_integrated_ci16(p, x, g, k, stride, det, form, 1.0f, o) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
    };
    every(p64, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(pw, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 0, out.data());      // no prototype set
    {
        float ms2[2];
        CHECK(sdrk_exec_device_pfb_ci16(p32, in.data(), 2, 4096, out.data(), nullptr) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_device_pfb_ci16_timed_each(p32, in.data(), 2, 4096, out.data(), 2, ms2) == SDRK_ERR_INVALID);
        CHECK(sdrk_exec_host_pfb_ci16(p32, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_fft_host_pfb_ci16(p32, in.data(), 2, 4096, out.data()) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
    }
    CHECK(sdrk_plan_set_pfb(p32, 2, h.data()) == SDRK_OK);
    auto every_frame = [&](sdrk_plan* p, const int16_t* x, size_t frames, size_t stride, float* o) {
        CHECK(sdrk_exec_device_pfb_ci16(p, x, frames, stride, o, nullptr) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_device_pfb_ci16_timed_each(p, x, frames, stride, o, 2, ms) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_host_pfb_ci16(p, x, frames, stride, o) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
        CHECK(sdrk_exec_fft_host_pfb_ci16(p, x, frames, stride, o) == SDRK_ERR_INVALID && sdrk_last_error()[0]);
    };
    every_frame(p64, in.data(), 2, 4096, out.data());
    every_frame(pw, in.data(), 2, 4096, out.data());
    every_frame(nullptr, in.data(), 2, 4096, out.data());
    every_frame(p32, nullptr, 2, 4096, out.data());
    every_frame(p32, in.data(), 2, 4096, nullptr);
    every_frame(p32, in.data(), 0, 4096, out.data());
    every_frame(p32, in.data(), 2, 0, out.data());            // stride 0 with more than one frame
    CHECK(sdrk_exec_device_pfb_ci16_timed_each(p32, in.data(), 2, 4096, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb_ci16_timed_each(p32, in.data(), 2, 4096, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    every(nullptr, in.data(), 4, 2, 4096, 0, 0, out.data());
    every(p32, nullptr, 4, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 0, nullptr);
    every(p32, in.data(), 0, 2, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 0, 4096, 0, 0, out.data());
    every(p32, in.data(), (size_t)1 << 40, (size_t)1 << 40, 4096, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 0, 0, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 3, 0, out.data());
    every(p32, in.data(), 4, 2, 4096, 0, 2, out.data());
    CHECK(sdrk_exec_device_pfb_integrated_ci16_timed_each(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data(), 0, ms) == SDRK_ERR_INVALID);
    CHECK(sdrk_exec_device_pfb_integrated_ci16_timed_each(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data(), 2, nullptr) == SDRK_ERR_INVALID);
    // the refused plan still works: per frame, and integrated beyond its max_batch of 4
    CHECK(sdrk_exec_host_pfb_ci16(p32, in.data(), 3, 4096, out.data()) == SDRK_OK);
    CHECK(wrong_frames(in.data(), out.data(), 4096, 2, 3, 4096, h) == 0);
    CHECK(sdrk_exec_host_pfb_integrated_ci16(p32, in.data(), 4, 2, 4096, 0, 0, 1.0f, out.data()) == SDRK_OK);
    CHECK(wrong_rows(in.data(), out.data(), c, h) == 0);
    for (sdrk_plan* p : {p64, pw, p32}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d pfb_ci16 threads=%d bad=%d\n", sdrk_version(), threads, g_bad.load());
    return g_bad.load() ? 1 : 0;
}

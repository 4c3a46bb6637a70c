// tests/host_stress.h — what the stand-alone host stress programs (tests/host_api_*_stress.cpp) share: the CHECK macro and
// its counters, the input generators, a buffer that is pageable or pinned, the references of the stand-in kernels
// (tests/fake_hip, tests/fake_*_kernels.cpp) written once over the sample type, and the skeleton of main.  For programs with
// a main of their own only: built by g++ with the host files, run directly, nothing loaded into Python.
//
// The stand-ins' definition, with y the folded frame (sum over `taps` blocks of h * x; the plain corners are taps = 1, h = 1, given as no h):
//   per frame    dB rows 3 re(y) - im(y) + (k & 1023), complex spectra (re(y) + 1, im(y) - 1);
//   integrated   the power (re(y) + 1)^2 + (im(y) - 1)^2 reduced over K frames to R, rows 3 R + (k & 1023) (dB form) or scale * R.
// Samples and coefficients are small integers, so every sum is exact and every output element has one right value.
#pragma once
#include "../include/sdrk.h"
#include "../sdr-iq-visualizer_amd/csrc/integrate_split.h"

#include <hip/hip_runtime.h>   // the stand-in runtime: a stream of the caller's own, the stand-in device's CU count

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <random>
#include <thread>
#include <vector>

inline std::atomic<int> g_bad{0};
inline std::atomic<int> g_refused{0};             // calls that had to return SDRK_ERR_INVALID and did
inline std::atomic<size_t> g_compared{0};         // output elements (floats) compared with a reference
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            if (g_bad.fetch_add(1) < 20) fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, sdrk_last_error()); \
        }                                                                                    \
    } while (0)
// a call that has to be refused as invalid
#define REFUSED(call)                                                \
    do {                                                             \
        if ((call) == SDRK_ERR_INVALID) ++g_refused;                 \
        else CHECK(!"refused: " #call);                              \
    } while (0)

// ---- inputs -------------------------------------------------------------------------------------------------------------
// small values (-6 .. 6): products with a prototype and sums over thousands of frames stay exact
template <class S> void fill(S* x, size_t n_samples, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = (S)((int)((s >> 16) % 13u) - 6);
    }
}
// the whole range of the format (12 bits for the floating-point ones): for the per-frame rows, which are linear in the samples
inline void fill_wide(float* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (float)((int)(rng() & 0xFFF) - 2048);
}
inline void fill_wide(double* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (double)((int)(rng() & 0xFFF) - 2048) + 0.25;
}
inline void fill_wide(int16_t* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (int16_t)((int)(rng() & 0xFFFF) - 32768);
}

// prototypes of `taps` blocks of nfft coefficients: -2 .. 2 by position, or -3 .. 3 at random
inline std::vector<float> proto(int nfft, int taps, unsigned seed) {
    std::vector<float> h((size_t)taps * nfft);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    return h;
}
inline std::vector<float> proto_random(int nfft, int taps, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<float> h((size_t)taps * nfft);
    for (float& v : h) v = (float)((int)(rng() % 7) - 3);
    return h;
}

template <class S> std::vector<float> widen(const S* in, size_t n_samples) {
    std::vector<float> w(2 * n_samples);
    for (size_t i = 0; i < 2 * n_samples; ++i) w[i] = (float)in[i];
    return w;
}

// n elements the caller hands to the library: pageable (a vector) or pinned (sdrk_host_alloc); null if that failed
template <class T> class Buf {
public:
    Buf(size_t n, bool pinned) : pinned_(pinned) {
        if (pinned) {
            void* p = nullptr;
            CHECK(sdrk_host_alloc(n * sizeof(T), &p) == SDRK_OK);
            ptr_ = static_cast<T*>(p);
        } else {
            v_.resize(n);
            ptr_ = v_.data();
        }
    }
    ~Buf() {
        if (pinned_ && ptr_) CHECK(sdrk_host_free(ptr_) == SDRK_OK);
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    T* data() const { return ptr_; }
    T& operator[](size_t i) const { return ptr_[i]; }

private:
    bool pinned_;
    std::vector<T> v_;
    T* ptr_ = nullptr;
};

// ---- references ---------------------------------------------------------------------------------------------------------
// sample k of the folded frame that starts at sample `at`, added to (re, im); h == nullptr: the plain corners' one block of ones
template <class A, class S> void folded(const S* in, const float* h, size_t n, int taps, size_t at, size_t k, A& re, A& im) {
    for (int t = 0; t < taps; ++t) {
        const A c = h ? (A)h[t * n + k] : (A)1;
        re += (A)in[2 * (at + t * n + k)] * c;
        im += (A)in[2 * (at + t * n + k) + 1] * c;
    }
}

// One call: `groups` rows, each of K frames reduced by (det, form, scale); k == 0 is a per-frame call of `groups` frames.
struct Case {
    int nfft, taps;
    size_t groups, k, stride;
    int det = SDRK_DET_MEAN, form = SDRK_INT_OUT_DB;
    float scale = 1.0f;
    bool chirpz = false;
};
inline size_t n_frames(const Case& c) { return c.groups * std::max<size_t>(c.k, 1); }
inline size_t in_samples(const Case& c) { return (n_frames(c) - 1) * c.stride + (size_t)c.taps * c.nfft; }
inline size_t n_out(const Case& c) { return c.groups * (size_t)c.nfft; }

// wrong elements among the dB rows of a per-frame call, as every array of `dbs` has them, and (if given) its complex spectra
template <class S> int wrong_frames(const S* in, const float* h, const Case& c, std::initializer_list<const float*> dbs, const float* spec = nullptr) {
    const size_t n = (size_t)c.nfft;
    int bad = 0;
    for (size_t f = 0; f < c.groups; ++f)
        for (size_t k = 0; k < n; ++k) {
            float re = 0, im = 0;
            folded(in, h, n, c.taps, f * c.stride, k, re, im);
            const size_t i = f * n + k;
            const float want = 3.0f * re - im + (float)(k & 1023);
            bool wrong = spec && (spec[2 * i] != re + 1.0f || spec[2 * i + 1] != im - 1.0f);
            for (const float* db : dbs) wrong |= db[i] != want;
            if (wrong && bad++ == 0)
                fprintf(stderr, "nfft=%d taps=%d frames=%zu stride=%zu: frame %zu bin %zu is %.9g, not %.9g (spectrum of (%.9g, %.9g))\n",
                        c.nfft, c.taps, c.groups, c.stride, f, k, (double)(*dbs.begin())[i], (double)want, (double)re, (double)im);
        }
    g_compared += (dbs.size() + (spec ? 2 : 0)) * c.groups * n;
    return bad;
}

// Wrong elements among the rows of an integrated call; how the mean is rounded follows the cut the library makes.
// (chirp-z lengths: the stand-in transforms chain differently there, so `spec` has the frames' spectra from the library's own
// per-frame complex call; everywhere else it is null)
template <class S> int wrong_rows(const S* in, const float* h, const Case& c, const float* out, const float* spec = nullptr) {
    const bool fused = c.nfft == 4096 && !c.chirpz;
    const size_t n = (size_t)c.nfft, ways = fused ? 1 : (n + 255) / 256;
    const bool split = sdrk::integrate_split(c.groups * ways, c.k, fakehip::cus()).slices > 1;
    int bad = 0;
    for (size_t g = 0; g < c.groups; ++g)
        for (size_t k = 0; k < n; ++k) {
            double sum = 0, hi = -1, lo = 1e30;
            for (size_t f = g * c.k; f < (g + 1) * c.k; ++f) {
                double re = 1.0, im = -1.0;
                if (spec) re = spec[2 * (f * n + k)], im = spec[2 * (f * n + k) + 1];
                else folded(in, h, n, c.taps, f * c.stride, k, re, im);
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
    g_compared += c.groups * n;
    return bad;
}

// `got` against what another entry of the same plan delivered (the complex64 one on the widened samples, as a rule)
inline bool same(const float* got, const std::vector<float>& want) {
    g_compared += want.size();
    return std::equal(want.begin(), want.end(), got);
}

// ---- main ---------------------------------------------------------------------------------------------------------------
// refusals on the main thread, then `threads` workers (thread number, iterations) at once, then the line the tests look for
inline int run_stress(const char* name, int threads, int iters, const std::function<void()>& refusals, const std::function<void(int, int)>& worker) {
    refusals();
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t) ts.emplace_back(worker, t, iters);
    for (auto& t : ts) t.join();
    printf("sdrk %d %s threads=%d bad=%d compared=%zu refused=%d\n", sdrk_version(), name, threads, g_bad.load(), g_compared.load(), g_refused.load());
    return g_bad.load() ? 1 : 0;
}

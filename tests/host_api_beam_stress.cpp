// tests/host_api_beam_stress.cpp — drives the host side of the filter-and-sum beamformer's entry points (sdrk_plan_set_beam,
// sdrk_exec_device_beam*, sdrk_exec_host_beam*: csrc/fir_api.hip and the staging slots of csrc/sdrk_host_pipeline.hip; built with
// the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp) for
// the sanitizer legs of tests/test_host_sanitizers_beam.py.  A program of its own: nothing is loaded into Python, nothing is
// preloaded.
//
//   host_api_beam_stress [threads] [iters]        (SDRK_FIR_CHUNK_BLOCKS=3 in the environment: several chunks per host call)
//
// Every thread runs C = 1, 3 and 8 in all three formats (both byte types) on plans of its own.  What is compared, element for
// element and bit for bit (the stand-ins run one transform per block and channel and the shared arithmetic of csrc/kernels_beam.h):
//   device   C = 1 against sdrk_exec_device_ddc* on the same plan with sdrk_plan_set_fir(h_0); the integer formats against the
//            complex64 entry on the widened elements; the elements behind n_out untouched;
//   timed    against the device entry;
//   host     against the device entry on prefix || iq with index0 = sample0 — chunks of three blocks with D = 7, so chunk
//            boundaries are no multiples of D, sample0 near 2^40, with a prefix and without (cu8: bytes of 0x80);
// then a DDC call between two beam calls on one plan, and every refusal.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

static const float SENTINEL = -77.0f;
static const uint64_t FAR = (1ull << 40) + 3;
static const uint32_t FINE = 0x12345678u;
static const int M = 257, D = 7;                    // L = 3840
static const size_t L = 3840, N_IQ = 7 * L + 321;   // the host call: eight blocks, chunks of 3 + 3 + 2
enum Fmt { C64, S16, I8, U8 };

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

static std::vector<float> int_taps(int rows, int m, unsigned seed) {   // complex taps with parts in -2 .. 2, every row's first non-zero
    std::vector<float> h(2 * (size_t)rows * m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    for (int r = 0; r < rows; ++r) h[2 * (size_t)r * m] = 1.0f;
    return h;
}

static size_t sample_bytes(Fmt f) { return f == C64 ? 8 : f == S16 ? 4 : 2; }

// n elements of c samples in format f, as bytes; and the same widened to complex64 as the library widens
static std::vector<unsigned char> elements(Fmt f, size_t n, int c, unsigned seed, std::vector<float>& wide) {
    const size_t vals = 2 * n * (size_t)c;
    std::vector<unsigned char> raw(vals * sample_bytes(f) / 2);
    wide.resize(vals);
    uint32_t s = seed * 2654435761u + 99u;
    for (size_t i = 0; i < vals; ++i) {
        s = s * 1664525u + 1013904223u;
        const int v = (int)((s >> 16) % 255u) - 127;
        if (f == C64) reinterpret_cast<float*>(raw.data())[i] = wide[i] = (float)v;
        else if (f == S16) reinterpret_cast<int16_t*>(raw.data())[i] = (int16_t)(v * 100), wide[i] = (float)(v * 100);
        else if (f == I8) reinterpret_cast<int8_t*>(raw.data())[i] = (int8_t)v, wide[i] = (float)v;
        else raw[i] = (unsigned char)(v + 128), wide[i] = (float)(v + 128) - 127.5f;
    }
    return raw;
}

static int device_call(Fmt f, sdrk_plan* p, const void* in, size_t n, uint32_t word, int d, uint64_t i0, void* out) {
    if (f == C64) return sdrk_exec_device_beam(p, in, n, word, d, i0, out, nullptr);
    if (f == S16) return sdrk_exec_device_beam_ci16(p, in, n, word, d, i0, out, nullptr);
    return sdrk_exec_device_beam_iq8(p, in, f == U8 ? SDRK_IQ8_UNSIGNED : SDRK_IQ8_SIGNED, n, word, d, i0, out, nullptr);
}
static int timed_call(Fmt f, sdrk_plan* p, const void* in, size_t n, uint32_t word, int d, uint64_t i0, void* out, float* ms) {
    if (f == C64) return sdrk_exec_device_beam_timed_each(p, in, n, word, d, i0, out, 2, ms);
    if (f == S16) return sdrk_exec_device_beam_ci16_timed_each(p, in, n, word, d, i0, out, 2, ms);
    return sdrk_exec_device_beam_iq8_timed_each(p, in, f == U8 ? SDRK_IQ8_UNSIGNED : SDRK_IQ8_SIGNED, n, word, d, i0, out, 2, ms);
}
static int host_call(Fmt f, sdrk_plan* p, const void* pre, const void* iq, size_t n, uint32_t word, int d, uint64_t s0, void* out, size_t* n_out) {
    if (f == C64) return sdrk_exec_host_beam(p, pre, iq, n, word, d, s0, out, n_out);
    if (f == S16) return sdrk_exec_host_beam_ci16(p, pre, iq, n, word, d, s0, out, n_out);
    return sdrk_exec_host_beam_iq8(p, pre, iq, f == U8 ? SDRK_IQ8_UNSIGNED : SDRK_IQ8_SIGNED, n, word, d, s0, out, n_out);
}
static int ddc_call(Fmt f, sdrk_plan* p, const void* in, size_t n, uint32_t word, int d, uint64_t i0, void* out) {
    if (f == C64) return sdrk_exec_device_ddc(p, in, n, word, d, i0, out, nullptr);
    if (f == S16) return sdrk_exec_device_ddc_ci16(p, in, n, word, d, i0, out, nullptr);
    return sdrk_exec_device_downconv_iq8(p, in, f == U8 ? SDRK_IQ8_UNSIGNED : SDRK_IQ8_SIGNED, n, word, d, i0, out, nullptr);
}

// the device entry -> its outputs, the GUARD behind them checked
static std::vector<float> device_out(Fmt f, sdrk_plan* p, const void* in, size_t n, uint32_t word, int d, uint64_t i0) {
    const size_t n_out = sdrk_ddc_outputs(n, M, d, i0), room = n_out + 16;
    std::vector<float> out(2 * room, SENTINEL);
    CHECK(device_call(f, p, in, n, word, d, i0, out.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    for (size_t i = 2 * n_out; i < 2 * room; ++i) CHECK(out[i] == SENTINEL);
    out.resize(2 * n_out);
    return out;
}

static void one_format(sdrk_plan* p, Fmt f, int c, unsigned seed, bool pinned) {
    const size_t n_all = N_IQ + M - 1, eb = (size_t)c * sample_bytes(f);
    std::vector<float> wide;
    const std::vector<unsigned char> raw = elements(f, n_all, c, seed, wide);
    for (const uint32_t word : {0u, FINE}) {
        const std::vector<float> dev = device_out(f, p, raw.data(), n_all, word, D, FAR);
        CHECK(!dev.empty());
        if (f != C64) CHECK(same(dev.data(), device_out(C64, p, wide.data(), n_all, word, D, FAR)));   // the widened elements
        if (c == 1) {                                                                                  // the down-converter
            std::vector<float> ref(dev.size(), SENTINEL);
            CHECK(ddc_call(f, p, raw.data(), n_all, word, D, FAR, ref.data()) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK);
            CHECK(same(dev.data(), ref));
        }
        float ms[2] = {-1.0f, -1.0f};
        std::vector<float> timed(dev.size(), SENTINEL);
        CHECK(timed_call(f, p, raw.data(), n_all, word, D, FAR, timed.data(), ms) == SDRK_OK && ms[0] >= 0.0f && ms[1] >= 0.0f);
        CHECK(same(timed.data(), dev));
        // host: prefix || iq, chunked
        Buf<unsigned char> iq(N_IQ * eb, pinned);
        Buf<float> out(2 * ((N_IQ + D - 1) / D), pinned);
        if (!iq.data() || !out.data()) return;
        memcpy(iq.data(), raw.data() + (M - 1) * eb, N_IQ * eb);
        size_t n_out = 0;
        CHECK(host_call(f, p, raw.data(), iq.data(), N_IQ, word, D, FAR, out.data(), &n_out) == SDRK_OK);
        CHECK(2 * n_out == dev.size() && same(out.data(), dev));
    }
    // a NULL prefix: elements of byte 0 (cu8: 0x80)
    std::vector<unsigned char> silent(raw);
    memset(silent.data(), f == U8 ? 0x80 : 0, (M - 1) * eb);
    const std::vector<float> want = device_out(f, p, silent.data(), n_all, FINE, D, 5);
    std::vector<float> out(2 * ((N_IQ + D - 1) / D), SENTINEL);
    size_t n_out = 0;
    CHECK(host_call(f, p, nullptr, raw.data() + (M - 1) * eb, N_IQ, FINE, D, 5, out.data(), &n_out) == SDRK_OK);
    CHECK(2 * n_out == want.size() && same(out.data(), want));
}

static void worker(int t, int iters) {
    sdrk_plan* p = make_plan(4096);
    if (!p) return;
    for (int it = 0; it < iters; ++it)
        for (const int c : {1, 3, 8}) {
            const std::vector<float> h = int_taps(c, M, (unsigned)(t + c));
            CHECK(sdrk_plan_set_beam(p, c, M, h.data()) == SDRK_OK);
            CHECK(sdrk_plan_set_fir(p, M, h.data()) == SDRK_OK);      // h_0: separate state, for the C = 1 identity and below
            CHECK(sdrk_plan_beam_channels(p) == c && sdrk_plan_beam_taps(p) == M && sdrk_plan_fir_taps(p) == M);
            for (const Fmt f : {C64, S16, I8, U8}) one_format(p, f, c, (unsigned)(100 * t + 10 * c + f), (t + c) % 2 == 1);
            // a DDC call between two beam calls on one plan
            std::vector<float> wide, w1;
            const std::vector<unsigned char> raw = elements(C64, 2 * L + M, c, 7u + (unsigned)t, wide);
            const std::vector<unsigned char> one = elements(C64, 2 * L + M, 1, 8u + (unsigned)t, w1);
            const std::vector<float> first = device_out(C64, p, raw.data(), 2 * L + M, FINE, D, 1);
            std::vector<float> mid(2 * sdrk_ddc_outputs(2 * L + M, M, D, 1), SENTINEL);
            CHECK(sdrk_exec_device_ddc(p, one.data(), 2 * L + M, FINE, D, 1, mid.data(), nullptr) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK && mid[0] != SENTINEL);
            CHECK(same(device_out(C64, p, raw.data(), 2 * L + M, FINE, D, 1).data(), first));
        }
    CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void refusals() {
    sdrk_plan *good = make_plan(4096), *small = make_plan(1024), *f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    const std::vector<float> h = int_taps(3, M, 1);
    std::vector<float> x(2 * 3 * 4096, 1.0f), out(2 * 4096);
    float ms[2];
    size_t n_out = 0;
    CHECK(sdrk_plan_beam_channels(good) == 0 && sdrk_plan_beam_taps(good) == 0);
    REFUSED(sdrk_exec_device_beam(good, x.data(), 4096, FINE, D, 0, out.data(), nullptr));          // no beam set
    CHECK(strstr(sdrk_last_error(), "sdrk_plan_set_beam") != nullptr);
    REFUSED(sdrk_exec_host_beam(good, nullptr, x.data(), 4096, FINE, D, 0, out.data(), &n_out));
    REFUSED(sdrk_plan_set_beam(nullptr, 3, M, h.data()));
    REFUSED(sdrk_plan_set_beam(good, 0, M, h.data()));
    REFUSED(sdrk_plan_set_beam(good, 9, M, h.data()));
    REFUSED(sdrk_plan_set_beam(good, 3, 0, h.data()));
    REFUSED(sdrk_plan_set_beam(good, 3, 2050, h.data()));
    REFUSED(sdrk_plan_set_beam(good, 3, M, nullptr));
    REFUSED(sdrk_plan_set_beam(f64, 3, M, h.data()));
    CHECK(sdrk_plan_set_beam(small, 3, M, h.data()) == SDRK_ERR_UNSUPPORTED);
    CHECK(sdrk_plan_set_beam(good, 3, M, h.data()) == SDRK_OK);
    for (const int d : {0, 257}) {
        REFUSED(sdrk_exec_device_beam(good, x.data(), 4096, FINE, d, 0, out.data(), nullptr));
        REFUSED(sdrk_exec_device_beam_ci16(good, x.data(), 4096, FINE, d, 0, out.data(), nullptr));
        REFUSED(sdrk_exec_host_beam(good, nullptr, x.data(), 4096, FINE, d, 0, out.data(), &n_out));
    }
    REFUSED(sdrk_exec_device_beam(good, x.data(), M - 1, FINE, D, 0, out.data(), nullptr));         // n_in < M
    REFUSED(sdrk_exec_device_beam(good, nullptr, 4096, FINE, D, 0, out.data(), nullptr));
    REFUSED(sdrk_exec_device_beam(good, x.data(), 4096, FINE, D, 0, nullptr, nullptr));
    REFUSED(sdrk_exec_device_beam_iq8(good, x.data(), 2, 4096, FINE, D, 0, out.data(), nullptr));   // format
    CHECK(strstr(sdrk_last_error(), "iq8_format 2 is neither") != nullptr);
    REFUSED(sdrk_exec_device_beam_iq8_timed_each(good, x.data(), -1, 4096, FINE, D, 0, out.data(), 2, ms));
    REFUSED(sdrk_exec_host_beam_iq8(good, nullptr, x.data(), 3, 4096, FINE, D, 0, out.data(), &n_out));
    REFUSED(sdrk_exec_device_beam_timed_each(good, x.data(), 4096, FINE, D, 0, out.data(), 0, ms));   // launches < 1
    REFUSED(sdrk_exec_device_beam_timed_each(good, x.data(), 4096, FINE, D, 0, out.data(), 2, nullptr));
    REFUSED(sdrk_exec_host_beam(good, nullptr, x.data(), 4096, FINE, D, 0, out.data(), nullptr));
    REFUSED(sdrk_exec_host_beam(good, nullptr, nullptr, 4096, FINE, D, 0, out.data(), &n_out));
    REFUSED(sdrk_exec_host_beam_ci16(good, nullptr, x.data(), 4096, FINE, D, 0, nullptr, &n_out));
    // the plan that has refused all this still works
    CHECK(sdrk_exec_host_beam(good, nullptr, x.data(), 4096, FINE, D, 0, out.data(), &n_out) == SDRK_OK && n_out == (4096 + D - 1) / D);
    for (sdrk_plan* p : {f64, good, small}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("beam", threads, iters, refusals, worker);
}

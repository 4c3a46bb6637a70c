// tests/host_api_downconv_iq8_stress.cpp — drives the host side of the 8-bit down-converter's entry points
// (sdrk_exec_*_downconv_iq8, sdrk_exec_*_downconvbank_iq8: csrc/fir_api.hip and the staging slots of csrc/sdrk_host_pipeline.hip;
// built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels
// tests/fake_*_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_downconv_iq8.py.  A program of its own: nothing
// is loaded into Python, nothing is preloaded.
//
//   host_api_downconv_iq8_stress [threads] [iters]   (SDRK_FIR_CHUNK_BLOCKS=3 in the environment: several chunks per host call)
//
// Every thread runs the cases of both formats (ci8, cu8) on plans of its own, on bytes over the whole range.  What is compared,
// element for element and bit for bit, is every output with the complex64 entry of the same plan on the widened samples
// (tests/fake_ddc_kernels.cpp: the same transform and the shared arithmetic of csrc/kernels_ols.h and csrc/kernels_ddc.h):
//   device   the bank, C = 1, 3 and 64, packed and padded planes, against sdrk_exec_device_ddcbank; the single call against
//            sdrk_exec_device_ddc and the bank's plane; the elements behind n_out untouched; a final block shorter than 4096
//            (the positions past n_in count as +0.0, not as byte 0);
//   timed    against the device entries;
//   host     chunks of three blocks with D = 7 (chunk boundaries that are no multiples of D), sample0 near 2^40, with a given
//            prefix and with NULL — NULL against the complex64 host entry GIVEN the widened bytes 0 / 0x80 as its prefix — and
//            against the 8-bit device entry on prefix || iq;
// then the refusals.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

static const float SENTINEL = -77.0f;
static const uint64_t FAR = (1ull << 40) + 3;

static std::vector<float> int_taps(int m, unsigned seed) {   // complex taps with parts in -2 .. 2, the first one non-zero
    std::vector<float> h(2 * (size_t)m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    h[0] = 1.0f;
    return h;
}

// channel 0 runs no mixer, 1 sits on a bin, 2 and 3 are fine words of both signs, the rest are spread by the seed
static std::vector<uint32_t> words_of(int n_chan, unsigned seed) {
    std::vector<uint32_t> w((size_t)n_chan);
    for (int c = 0; c < n_chan; ++c)
        w[c] = c == 0 ? 0u : c == 1 ? 0x80000000u : c == 2 ? 0x12345678u : c == 3 ? 0xFEDCBA98u : (uint32_t)c * 2654435761u + seed * 97u;
    return w;
}

static void fill_bytes(uint8_t* x, size_t n_samples, unsigned seed) {   // all 256 values
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (uint8_t)(rng() & 0xFFu);
}

// the widening of include/sdrk.h, exact in float32
static std::vector<float> widen8(const uint8_t* x, size_t n_samples, int fmt) {
    std::vector<float> w(2 * n_samples);
    for (size_t i = 0; i < 2 * n_samples; ++i) w[i] = fmt == SDRK_IQ8_SIGNED ? (float)(int8_t)x[i] : (float)x[i] - 127.5f;
    return w;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

// n_out elements of `plane` equal to `ref`, the `room - n_out` behind them untouched
static bool plane_ok(const float* plane, size_t room, const float* ref, size_t n_out) {
    bool ok = same(plane, std::vector<float>(ref, ref + 2 * n_out));
    for (size_t i = 2 * n_out; i < 2 * room; ++i) ok &= plane[i] == SENTINEL;
    return ok;
}

struct Shape {
    int taps, decim;
    size_t n;            // samples of the piece (device entry: n_in)
    uint64_t index0;     // device: index0; host: sample0
    bool prefix;         // host entry: a given prefix (else NULL)
};

static void device_case(int fmt, sdrk_plan* p, const Shape& c, int n_chan, size_t pad, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK);
    std::vector<uint8_t> in(2 * c.n);
    fill_bytes(in.data(), c.n, seed + 1);
    const std::vector<float> wide = widen8(in.data(), c.n, fmt);
    const std::vector<uint32_t> words = words_of(n_chan, seed);
    const size_t n_out = sdrk_ddc_outputs(c.n, c.taps, c.decim, c.index0), stride = n_out + pad;
    std::vector<float> bank(2 * stride * (size_t)n_chan + 2, SENTINEL), ref(bank.size(), SENTINEL);
    CHECK(sdrk_exec_device_downconvbank_iq8(p, in.data(), fmt, c.n, n_chan, words.data(), c.decim, c.index0, bank.data(), stride, nullptr) == SDRK_OK);
    CHECK(sdrk_exec_device_ddcbank(p, wide.data(), c.n, n_chan, words.data(), c.decim, c.index0, ref.data(), stride, nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(same(bank.data(), ref));   // the sentinels behind n_out and between the planes included
    float ms[2] = {0, 0};
    for (int ch = 0; ch < n_chan; ++ch) {
        if (ch > 4 && ch % 9) continue;   // (C = 64: every ninth plane against the single calls)
        std::vector<float> one(2 * (n_out + 3), SENTINEL), one_ref(one.size(), SENTINEL), timed(one.size(), SENTINEL);
        CHECK(sdrk_exec_device_downconv_iq8(p, in.data(), fmt, c.n, words[ch], c.decim, c.index0, one.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_exec_device_ddc(p, wide.data(), c.n, words[ch], c.decim, c.index0, one_ref.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
        CHECK(same(one.data(), one_ref) && plane_ok(one.data(), n_out + 3, bank.data() + 2 * stride * (size_t)ch, n_out));
        CHECK(sdrk_exec_device_downconv_iq8_timed_each(p, in.data(), fmt, c.n, words[ch], c.decim, c.index0, timed.data(), 2, ms) == SDRK_OK);
        CHECK(same(timed.data(), one));
    }
    std::vector<float> timed(bank.size(), SENTINEL);
    CHECK(sdrk_exec_device_downconvbank_iq8_timed_each(p, in.data(), fmt, c.n, n_chan, words.data(), c.decim, c.index0, timed.data(), stride,
                                                       2, ms) == SDRK_OK && (n_out == 0 || (ms[0] > 0 && ms[1] > 0)));
    CHECK(same(timed.data(), bank));
}

static void host_case(int fmt, sdrk_plan* p, const Shape& c, int n_chan, size_t pad, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK && sdrk_plan_fir_taps(p) == c.taps);
    const size_t M = (size_t)c.taps, D = (size_t)c.decim;
    // prefix || iq: a NULL prefix stands for bytes 0 (signed) / 0x80 (unsigned)
    std::vector<uint8_t> virt(2 * (M - 1 + c.n), (uint8_t)(fmt == SDRK_IQ8_UNSIGNED ? 0x80 : 0));
    if (c.prefix) fill_bytes(virt.data(), M - 1, seed + 2);
    uint8_t* in = virt.data() + 2 * (M - 1);
    fill_bytes(in, c.n, seed + 1);
    const uint8_t* prefix = c.prefix && M > 1 ? virt.data() : nullptr;
    const std::vector<float> wide = widen8(virt.data(), M - 1 + c.n, fmt);   // the complex64 call is GIVEN the widened prefix
    if (!c.prefix && M > 1) CHECK(wide[0] == (fmt == SDRK_IQ8_UNSIGNED ? 0.5f : 0.0f) && wide[1] == wide[0]);
    const std::vector<uint32_t> words = words_of(n_chan, seed);
    const size_t want = sdrk_ddc_outputs(c.n + M - 1, c.taps, c.decim, c.index0), stride = (c.n + D - 1) / D + pad;
    std::vector<float> out(2 * stride * (size_t)n_chan + 2, SENTINEL), ref(out.size(), SENTINEL), dev(out.size(), SENTINEL);
    size_t n_out = 12345, n_ref = 12345;
    CHECK(sdrk_exec_host_downconvbank_iq8(p, prefix, in, fmt, c.n, n_chan, words.data(), c.decim, c.index0, out.data(), stride, &n_out) == SDRK_OK);
    CHECK(sdrk_exec_host_ddcbank(p, M > 1 ? wide.data() : nullptr, wide.data() + 2 * (M - 1), c.n, n_chan, words.data(), c.decim, c.index0,
                                 ref.data(), stride, &n_ref) == SDRK_OK);
    CHECK(n_out == want && n_ref == want && want <= stride && same(out.data(), ref));
    CHECK(sdrk_exec_device_downconvbank_iq8(p, virt.data(), fmt, M - 1 + c.n, n_chan, words.data(), c.decim, c.index0, dev.data(), stride,
                                            nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(same(out.data(), dev));
    for (int ch = 0; ch < n_chan; ++ch) {
        if (ch > 4 && ch % 9) continue;
        std::vector<float> one(2 * stride + 2, SENTINEL);
        size_t n_one = 0;
        CHECK(sdrk_exec_host_downconv_iq8(p, prefix, in, fmt, c.n, words[ch], c.decim, c.index0, one.data(), &n_one) == SDRK_OK && n_one == want);
        CHECK(plane_ok(one.data(), stride, out.data() + 2 * stride * (size_t)ch, want));
    }
}

static void format_cases(int fmt, unsigned s) {
    sdrk_plan* p = make_plan(4096);
    if (!p) return;
    const size_t L5 = 3840, L300 = 3584, L2049 = 2048;
    device_case(fmt, p, {5, 7, 2 * L5 + 100, 0, false}, 1, 0, s + 1);                  // C = 1, packed; the last block 104 samples
    device_case(fmt, p, {300, 50, 2 * L300 + 1234 + 299, 1, false}, 3, 7, s + 2);      // C = 3, padded planes, index0 % D != 0
    device_case(fmt, p, {2049, 200, L2049 + 2049, FAR, false}, 64, 0, s + 3);          // C = 64 at the tap limit, two blocks
    device_case(fmt, p, {5, 255, 5, 3, false}, 3, 1, s + 4);                           // n_in = M: one output, not kept: n_out = 0
    device_case(fmt, p, {5, 255, 5, 255, false}, 3, 1, s + 4);                         // ... kept: n_out = 1
    // host entry, 3 blocks per chunk, D = 7: chunk boundaries that are no multiples of D, with a prefix and without
    host_case(fmt, p, {300, 7, 7 * L300 + 5, 13, true}, 3, 3, s + 8);
    host_case(fmt, p, {300, 7, 10 * L300 + 5, FAR, false}, 3, 0, s + 9);               // four chunks, a NULL prefix
    host_case(fmt, p, {5, 7, 4 * L5, FAR, false}, 1, 0, s + 10);
    host_case(fmt, p, {2049, 50, 3 * L2049 + 9, 12345, false}, 64, 0, s + 11);         // C = 64 over two chunks, a NULL prefix of 2048
    host_case(fmt, p, {1, 7, 5000, 3, false}, 3, 0, s + 12);                           // M = 1: no prefix at all
    host_case(fmt, p, {2, 256, 200, 100, true}, 3, 2, s + 13);                         // one output a plane: stream index 256
    host_case(fmt, p, {2, 256, 100, 100, true}, 3, 2, s + 14);                         // none
    CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        format_cases(SDRK_IQ8_SIGNED, s);
        format_cases(SDRK_IQ8_UNSIGNED, s + 20);
    }
}

// Every refusal comes with its status and a message, from the device, the timed and the host entries; the plans still work after.
static void refusals() {
    sdrk_plan* f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    sdrk_plan *good = make_plan(4096), *small = make_plan(1024);
    if (!f64 || !good || !small) return;
    const std::vector<float> h = int_taps(9, 3);
    const size_t n = 5000, n_out = n - 9 + 1;
    std::vector<uint8_t> in(2 * n);
    std::vector<float> out(2 * 3 * n);
    fill_bytes(in.data(), n, 77);
    const uint32_t w3[3] = {0, 0x12345678u, 0xFFF00000u};
    std::vector<uint32_t> many(65, 1u << 20);
    float ms[2];
    size_t got = 0;
#define ONE_DEVICE(plan, src, fmt, len, decim, dst) sdrk_exec_device_downconv_iq8(plan, src, fmt, len, w3[1], decim, 0, dst, nullptr)
#define ONE_TIMED(plan, src, fmt, len, decim, dst, k, each) sdrk_exec_device_downconv_iq8_timed_each(plan, src, fmt, len, w3[1], decim, 0, dst, k, each)
#define ONE_HOST(plan, src, fmt, len, decim, dst, cnt) sdrk_exec_host_downconv_iq8(plan, nullptr, src, fmt, len, w3[1], decim, 0, dst, cnt)
#define BANK_DEVICE(plan, src, fmt, len, chans, w, decim, dst, stride) \
    sdrk_exec_device_downconvbank_iq8(plan, src, fmt, len, chans, w, decim, 0, dst, stride, nullptr)
#define BANK_TIMED(plan, src, fmt, len, chans, w, decim, dst, stride, k, each) \
    sdrk_exec_device_downconvbank_iq8_timed_each(plan, src, fmt, len, chans, w, decim, 0, dst, stride, k, each)
#define BANK_HOST(plan, src, fmt, len, chans, w, decim, dst, stride, cnt) \
    sdrk_exec_host_downconvbank_iq8(plan, nullptr, src, fmt, len, chans, w, decim, 0, dst, stride, cnt)
    CHECK(sdrk_plan_set_fir(good, 9, h.data()) == SDRK_OK);
    // the format: the two values, nothing else, from every entry, with the text of the 8-bit spectra
    for (int fmt : {2, -1, 255}) {
        REFUSED(ONE_DEVICE(good, in.data(), fmt, n, 1, out.data()));
        CHECK(strstr(sdrk_last_error(), "is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED") != nullptr);
        REFUSED(ONE_TIMED(good, in.data(), fmt, n, 1, out.data(), 2, ms));
        REFUSED(ONE_HOST(good, in.data(), fmt, n, 1, out.data(), &got));
        REFUSED(BANK_DEVICE(good, in.data(), fmt, n, 3, w3, 1, out.data(), n));
        REFUSED(BANK_TIMED(good, in.data(), fmt, n, 3, w3, 1, out.data(), n, 2, ms));
        REFUSED(BANK_HOST(good, in.data(), fmt, n, 3, w3, 1, out.data(), n, &got));
        CHECK(strstr(sdrk_last_error(), "iq8_format") != nullptr);
    }
    CHECK(sdrk_plan_destroy(good) == SDRK_OK);
    good = make_plan(4096);
    if (!good) return;
    for (int fmt : {SDRK_IQ8_SIGNED, SDRK_IQ8_UNSIGNED}) {
        // another length: unsupported; a float64 plan, no plan
        CHECK(ONE_DEVICE(small, in.data(), fmt, n, 1, out.data()) == SDRK_ERR_UNSUPPORTED && sdrk_last_error()[0]);
        CHECK(BANK_HOST(small, in.data(), fmt, n, 3, w3, 1, out.data(), n, &got) == SDRK_ERR_UNSUPPORTED);
        REFUSED(ONE_DEVICE(f64, in.data(), fmt, n, 1, out.data()));
        REFUSED(BANK_HOST(f64, in.data(), fmt, n, 3, w3, 1, out.data(), n, &got));
        REFUSED(ONE_DEVICE(nullptr, in.data(), fmt, n, 1, out.data()));
        REFUSED(BANK_DEVICE(nullptr, in.data(), fmt, n, 3, w3, 1, out.data(), n));
    }
    // no filter set
    REFUSED(ONE_DEVICE(good, in.data(), 0, n, 1, out.data()));
    CHECK(strstr(sdrk_last_error(), "sdrk_plan_set_fir") != nullptr);
    REFUSED(ONE_HOST(good, in.data(), 1, n, 1, out.data(), &got));
    REFUSED(ONE_TIMED(good, in.data(), 0, n, 1, out.data(), 2, ms));
    REFUSED(BANK_DEVICE(good, in.data(), 1, n, 3, w3, 1, out.data(), n));
    REFUSED(BANK_HOST(good, in.data(), 0, n, 3, w3, 1, out.data(), n, &got));
    REFUSED(BANK_TIMED(good, in.data(), 1, n, 3, w3, 1, out.data(), n, 2, ms));
    CHECK(sdrk_plan_set_fir(good, 9, h.data()) == SDRK_OK);
    // the decimation: any integer in 1 .. 256, nothing else
    for (int decim : {0, 257, -2}) {
        REFUSED(ONE_DEVICE(good, in.data(), 1, n, decim, out.data()));
        CHECK(strstr(sdrk_last_error(), "decim") != nullptr);
        REFUSED(ONE_HOST(good, in.data(), 0, n, decim, out.data(), &got));
        REFUSED(ONE_TIMED(good, in.data(), 1, n, decim, out.data(), 2, ms));
        REFUSED(BANK_DEVICE(good, in.data(), 0, n, 3, w3, decim, out.data(), n));
        REFUSED(BANK_HOST(good, in.data(), 1, n, 3, w3, decim, out.data(), n, &got));
        REFUSED(BANK_TIMED(good, in.data(), 0, n, 3, w3, decim, out.data(), n, 2, ms));
    }
    // the channel count, the words, the stride
    for (int chans : {0, -1, 65}) {
        REFUSED(BANK_DEVICE(good, in.data(), 1, n, chans, many.data(), 1, out.data(), n));
        CHECK(strstr(sdrk_last_error(), "n_chan") != nullptr);
        REFUSED(BANK_HOST(good, in.data(), 0, n, chans, many.data(), 1, out.data(), n, &got));
        REFUSED(BANK_TIMED(good, in.data(), 1, n, chans, many.data(), 1, out.data(), n, 2, ms));
    }
    REFUSED(BANK_DEVICE(good, in.data(), 1, n, 3, nullptr, 1, out.data(), n));
    CHECK(strstr(sdrk_last_error(), "freq_word") != nullptr);
    REFUSED(BANK_HOST(good, in.data(), 1, n, 3, nullptr, 1, out.data(), n, &got));
    REFUSED(BANK_DEVICE(good, in.data(), 1, n, 3, w3, 1, out.data(), n_out - 1));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    REFUSED(BANK_TIMED(good, in.data(), 0, n, 3, w3, 1, out.data(), n_out - 1, 2, ms));
    REFUSED(BANK_HOST(good, in.data(), 1, n, 3, w3, 7, out.data(), (n + 6) / 7 - 1, &got));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    // pointers, lengths, the timed entries' own arguments
    REFUSED(ONE_DEVICE(good, nullptr, 1, n, 1, out.data()));
    REFUSED(ONE_DEVICE(good, in.data(), 0, n, 1, nullptr));
    REFUSED(ONE_DEVICE(good, in.data(), 1, 8, 1, out.data()));                             // n_in < M
    REFUSED(BANK_DEVICE(good, nullptr, 0, n, 3, w3, 1, out.data(), n));
    REFUSED(BANK_DEVICE(good, in.data(), 1, n, 3, w3, 1, nullptr, n));
    REFUSED(ONE_HOST(good, in.data(), 1, n, 1, out.data(), nullptr));
    REFUSED(ONE_HOST(good, (const uint8_t*)nullptr, 0, n, 1, out.data(), &got));
    REFUSED(ONE_HOST(good, in.data(), 1, n, 1, nullptr, &got));
    REFUSED(BANK_HOST(good, in.data(), 0, n, 3, w3, 1, out.data(), n, nullptr));
    REFUSED(ONE_TIMED(good, in.data(), 1, n, 1, out.data(), 0, ms));
    REFUSED(ONE_TIMED(good, in.data(), 0, n, 1, out.data(), 2, nullptr));
    REFUSED(BANK_TIMED(good, in.data(), 1, n, 3, w3, 1, out.data(), n, 0, ms));
    CHECK(sdrk_last_error()[0]);
    got = 7;
    CHECK(BANK_HOST(good, in.data(), 1, 0, 3, w3, 7, out.data(), 0, &got) == SDRK_OK && got == 0);   // an empty piece
#undef ONE_DEVICE
#undef ONE_TIMED
#undef ONE_HOST
#undef BANK_DEVICE
#undef BANK_TIMED
#undef BANK_HOST
    // the refused plans still work
    host_case(SDRK_IQ8_UNSIGNED, good, {9, 7, n, 3, true}, 3, 1, 5);
    for (sdrk_plan* p : {f64, good, small}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("downconv_iq8", threads, iters, refusals, worker);
}

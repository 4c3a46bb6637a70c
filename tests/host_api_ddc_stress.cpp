// tests/host_api_ddc_stress.cpp — drives the host side of the digital down-converter's entry points (sdrk_ddc_outputs,
// sdrk_exec_device_ddc*, sdrk_exec_host_ddc*, sdrk_exec_*_ddcbank*: csrc/fir_api.hip and the staging slots of
// csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against the stand-in runtime of tests/fake_hip and the
// stand-in kernels tests/fake_*_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_ddc.py.  A program of its own:
// nothing is loaded into Python, nothing is preloaded.
//
//   host_api_ddc_stress [threads] [iters]         (SDRK_FIR_CHUNK_BLOCKS=3 in the environment: several chunks per host call)
//
// Every thread runs the cases of both formats on plans of its own.  What is compared, element for element and bit for bit (the
// stand-ins run one transform and the shared arithmetic of csrc/kernels_ols.h and csrc/kernels_ddc.h):
//   device   D = d against D = 1: out_d[m] == out_1[i_first + m d]; the count against sdrk_ddc_outputs and a brute-force count;
//            the elements behind n_out untouched; a word s << 20 with a power-of-two D against sdrk_exec_device_fir;
//   timed    against the device entry;
//   host     against the device entry on prefix || iq with index0 = sample0 — chunks of three blocks with D = 7, so chunk
//            boundaries are no multiples of D, sample0 near 2^40; int16 against complex64 on the widened samples;
//   bank     C = 1, 3 and 64, packed and padded planes: plane c against the single call with freq_word[c];
// then the refusals, and an existing FIR call between DDC calls on one plan.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

template <class S> struct Mode {
    const Mode<float>* c64;   // int16: the complex64 mode that defines it, on the widened samples
    decltype(&sdrk_exec_device_ddc) device;
    decltype(&sdrk_exec_host_ddc) host;
    decltype(&sdrk_exec_device_ddcbank) bank_device;
    decltype(&sdrk_exec_host_ddcbank) bank_host;
    decltype(&sdrk_exec_device_fir) fir_device;
};
static const Mode<float> C64{nullptr, sdrk_exec_device_ddc, sdrk_exec_host_ddc, sdrk_exec_device_ddcbank, sdrk_exec_host_ddcbank,
                             sdrk_exec_device_fir};
static const Mode<int16_t> I16{&C64, sdrk_exec_device_ddc_ci16, sdrk_exec_host_ddc_ci16, sdrk_exec_device_ddcbank_ci16,
                               sdrk_exec_host_ddcbank_ci16, sdrk_exec_device_fir_ci16};

static const float SENTINEL = -77.0f;
static const uint64_t FAR = (1ull << 40) + 3;

static std::vector<float> int_taps(int m, unsigned seed) {   // complex taps with parts in -2 .. 2, the first one non-zero
    std::vector<float> h(2 * (size_t)m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    h[0] = 1.0f;
    return h;
}

// channel 0 runs no mixer, 1 sits on a bin, 2 and 3 are fine words of both signs, 4 repeats 3, the rest are spread by the seed
static std::vector<uint32_t> words_of(int n_chan, unsigned seed) {
    std::vector<uint32_t> w((size_t)n_chan);
    for (int c = 0; c < n_chan; ++c)
        w[c] = c == 0 ? 0u : c == 1 ? 0x80000000u : c == 2 ? 0x12345678u : c == 3 ? 0xFEDCBA98u : (uint32_t)c * 2654435761u + seed * 97u;
    if (n_chan > 4) w[4] = w[3];
    return w;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

static size_t brute_count(size_t n_in, int taps, int decim, uint64_t index0) {
    size_t k = 0;
    for (size_t i = 0; i + (size_t)taps <= n_in; ++i) k += (index0 + i) % (uint64_t)decim == 0;
    return k;
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
    bool prefix;         // host entry: a non-zero prefix
};

// the device entry of one word -> its outputs; checked against D = 1 and the counts
template <class S> std::vector<float> device_one(const Mode<S>& m, sdrk_plan* p, const Shape& c, const S* in, uint32_t word) {
    const size_t M = (size_t)c.taps, D = (size_t)c.decim, n_all = c.n - M + 1;
    const size_t n_out = sdrk_ddc_outputs(c.n, c.taps, c.decim, c.index0);
    CHECK(n_out == brute_count(c.n, c.taps, c.decim, c.index0));
    std::vector<float> out(2 * (n_out + 3), SENTINEL), all(2 * n_all, SENTINEL);
    CHECK(m.device(p, in, c.n, word, c.decim, c.index0, out.data(), nullptr) == SDRK_OK);
    CHECK(m.device(p, in, c.n, word, 1, c.index0, all.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    const size_t i_first = (size_t)((D - c.index0 % D) % D);
    std::vector<float> picked(2 * n_out);
    for (size_t k = 0; k < n_out; ++k) picked[2 * k] = all[2 * (i_first + k * D)], picked[2 * k + 1] = all[2 * (i_first + k * D) + 1];
    CHECK(plane_ok(out.data(), n_out + 3, picked.data(), n_out));
    out.resize(2 * n_out);
    return out;
}

template <class S> void device_case(const Mode<S>& m, sdrk_plan* p, const Shape& c, int n_chan, size_t pad, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK);
    std::vector<S> in(2 * c.n);
    fill(in.data(), c.n, seed + 1);
    const std::vector<uint32_t> words = words_of(n_chan, seed);
    const size_t n_out = sdrk_ddc_outputs(c.n, c.taps, c.decim, c.index0), stride = n_out + pad;
    std::vector<float> bank(2 * stride * (size_t)n_chan + 2, SENTINEL);
    CHECK(m.bank_device(p, in.data(), c.n, n_chan, words.data(), c.decim, c.index0, bank.data(), stride, nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    for (int ch = 0; ch < n_chan; ++ch) {
        if (ch > 5 && ch % 9) continue;   // (C = 64: every ninth plane against the single call, all of them against each other below)
        const std::vector<float> one = device_one(m, p, c, in.data(), words[ch]);
        CHECK(plane_ok(bank.data() + 2 * stride * (size_t)ch, stride, one.data(), n_out));
    }
    if (n_chan > 4) CHECK(same(bank.data() + 2 * stride * 4, std::vector<float>(bank.begin() + 2 * stride * 3, bank.begin() + 2 * stride * 3 + 2 * n_out)));
    if (!m.c64) {   // the timed entries: the bits of the device entries
        float ms[2] = {0, 0};
        std::vector<float> timed(bank.size(), SENTINEL), t1(2 * n_out + 2, SENTINEL);
        CHECK(sdrk_exec_device_ddcbank_timed_each(p, in.data(), c.n, n_chan, words.data(), c.decim, c.index0, timed.data(), stride, 2, ms) ==
                  SDRK_OK && (n_out == 0 || (ms[0] > 0 && ms[1] > 0)));
        CHECK(same(timed.data(), bank));
        const uint32_t w = words[n_chan > 2 ? 2 : 0];
        CHECK(sdrk_exec_device_ddc_timed_each(p, in.data(), c.n, w, c.decim, c.index0, t1.data(), 2, ms) == SDRK_OK);
        CHECK(plane_ok(t1.data(), n_out + 1, device_one(m, p, c, in.data(), w).data(), n_out));
    }
}

// a word on a bin, a power-of-two D, index0 a multiple of D: the stand-in FIR launch's elements
template <class S> void fir_case(const Mode<S>& m, sdrk_plan* p, int taps, int decim, size_t n, uint64_t index0, int s, unsigned seed) {
    const std::vector<float> h = int_taps(taps, seed);
    CHECK(sdrk_plan_set_fir(p, taps, h.data()) == SDRK_OK);
    std::vector<S> in(2 * n);
    fill(in.data(), n, seed + 1);
    const size_t n_out = (n - (size_t)taps) / (size_t)decim + 1;
    CHECK(index0 % (uint64_t)decim == 0 && sdrk_ddc_outputs(n, taps, decim, index0) == n_out);
    std::vector<float> a(2 * n_out, SENTINEL), b(2 * n_out, SENTINEL);
    const int phase0 = (int)(((uint64_t)(unsigned)(s & 4095) * (index0 & 4095)) & 4095);
    CHECK(m.device(p, in.data(), n, (uint32_t)s << 20, decim, index0, a.data(), nullptr) == SDRK_OK);
    CHECK(m.fir_device(p, in.data(), n, decim, s, phase0, b.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(same(a.data(), b));
}

// the host entries against the device entries on prefix || iq; -> the bank's output (for the callers that compare two calls)
template <class S> std::vector<float> host_case(const Mode<S>& m, sdrk_plan* p, const Shape& c, int n_chan, size_t pad, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK && sdrk_plan_fir_taps(p) == c.taps);
    const size_t M = (size_t)c.taps, D = (size_t)c.decim;
    std::vector<S> virt(2 * (M - 1 + c.n), (S)0);   // prefix || iq
    if (c.prefix) fill(virt.data(), M - 1, seed + 2);
    S* in = virt.data() + 2 * (M - 1);
    fill(in, c.n, seed + 1);
    const S* prefix = c.prefix && M > 1 ? virt.data() : nullptr;
    const std::vector<uint32_t> words = words_of(n_chan, seed);
    const size_t want = brute_count(c.n + M - 1, c.taps, c.decim, c.index0), stride = (c.n + D - 1) / D + pad;
    std::vector<float> out(2 * stride * (size_t)n_chan + 2, SENTINEL), one(2 * stride + 2, SENTINEL), dev(2 * want + 2, SENTINEL);
    size_t n_out = 12345;
    CHECK(m.bank_host(p, prefix, in, c.n, n_chan, words.data(), c.decim, c.index0, out.data(), stride, &n_out) == SDRK_OK);
    CHECK(n_out == want && want <= stride);
    for (int ch = 0; ch < n_chan; ++ch) {
        if (ch > 5 && ch % 9) continue;
        size_t n_one = 0;
        CHECK(m.device(p, virt.data(), M - 1 + c.n, words[ch], c.decim, c.index0, dev.data(), nullptr) == SDRK_OK);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
        CHECK(plane_ok(out.data() + 2 * stride * (size_t)ch, stride, dev.data(), want));
        std::fill(one.begin(), one.end(), SENTINEL);
        CHECK(m.host(p, prefix, in, c.n, words[ch], c.decim, c.index0, one.data(), &n_one) == SDRK_OK && n_one == want);
        CHECK(plane_ok(one.data(), stride, dev.data(), want));
    }
    if (m.c64) {   // the complex64 entry of the same plan agrees on the widened samples, bit for bit
        const std::vector<float> wide = widen(virt.data(), M - 1 + c.n);
        std::vector<float> other(out.size(), SENTINEL);
        size_t n_other = 0;
        CHECK(m.c64->bank_host(p, prefix ? wide.data() : nullptr, wide.data() + 2 * (M - 1), c.n, n_chan, words.data(), c.decim, c.index0,
                               other.data(), stride, &n_other) == SDRK_OK);
        CHECK(n_other == want && same(out.data(), other));
    }
    return out;
}

// An existing FIR call between two DDC calls on one plan: every output right, the second DDC call the bits of the first.
template <class S> void between_case(const Mode<S>& m, sdrk_plan* p, unsigned seed) {
    const Shape c{33, 7, 3 * 4096 + 11, FAR, true};
    const std::vector<float> first = host_case(m, p, c, 3, 5, seed);
    fir_case(m, p, 33, 4, 9000, 4096, -7, seed);   // (sdrk_exec_device_fir*, and the DDC against it)
    CHECK(same(host_case(m, p, c, 3, 5, seed).data(), first));
    CHECK(sdrk_plan_fir_taps(p) == 33);
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s) {
    sdrk_plan* p = make_plan(4096);
    if (!p) return;
    const size_t L5 = 3840, L300 = 3584, L2049 = 2048;
    device_case(m, p, {5, 7, 2 * L5 + 100, 0, false}, 1, 0, s + 1);                  // C = 1, packed
    device_case(m, p, {300, 50, 2 * L300 + 17, 1, false}, 3, 7, s + 2);              // C = 3, padded planes, index0 % D != 0
    device_case(m, p, {2049, 200, L2049 + 2049, FAR, false}, 64, 0, s + 3);          // C = 64 at the tap limit, two blocks, D > L / 16
    device_case(m, p, {5, 255, 5, 3, false}, 3, 1, s + 4);                           // n_in = M: one output, not kept: n_out = 0
    device_case(m, p, {5, 255, 5, 255, false}, 3, 1, s + 4);                         // ... kept: n_out = 1
    for (int sh : {0, 1, -7, 2047, -2048}) fir_case(m, p, 300, 16, 2 * L300 + 17, (1ull << 40) + 16, sh, s + 5);
    fir_case(m, p, 5, 1, L5 + 9, 0, 100, s + 6);
    fir_case(m, p, 2049, 256, 3 * L2049, 512, -1000, s + 7);
    // host entry, 3 blocks per chunk, D = 7: chunk boundaries that are no multiples of D, with a prefix and without
    host_case(m, p, {300, 7, 7 * L300 + 5, 13, true}, 3, 3, s + 8);
    host_case(m, p, {300, 7, 10 * L300 + 5, FAR, true}, 3, 0, s + 9);                // four chunks: the first slot's planes leave before it is reused
    host_case(m, p, {5, 7, 4 * L5, FAR, false}, 1, 0, s + 10);
    host_case(m, p, {2049, 50, 3 * L2049 + 9, 12345, false}, 64, 0, s + 11);         // C = 64 over two chunks
    host_case(m, p, {2, 256, 200, 100, true}, 3, 2, s + 12);                         // one output a plane: stream index 256
    host_case(m, p, {2, 256, 100, 100, true}, 3, 2, s + 13);                         // none
    between_case(m, p, s + 14);
    CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        mode_cases(C64, s);
        mode_cases(I16, s + 20);
    }
}

// Every refusal comes with its status and a message, from the device, the timed and the host entries; the plans still work after.
template <class S> void mode_refusals(const Mode<S>& m) {
    sdrk_plan* f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    sdrk_plan *good = make_plan(4096), *small = make_plan(1024);
    if (!f64 || !good || !small) return;
    const std::vector<float> h = int_taps(9, 3);
    const size_t n = 5000, n_out = n - 9 + 1;
    std::vector<S> in(2 * n);
    std::vector<float> out(2 * 3 * n);
    fill(in.data(), n, 77);
    const uint32_t w3[3] = {0, 0x12345678u, 0xFFF00000u};
    std::vector<uint32_t> many(65, 1u << 20);
    float ms[2];
    size_t got = 0;
#define ONE_DEVICE(plan, src, len, decim, dst) m.device(plan, src, len, w3[1], decim, 0, dst, nullptr)
#define ONE_TIMED(plan, src, len, decim, dst, k, each) sdrk_exec_device_ddc_timed_each(plan, src, len, w3[1], decim, 0, dst, k, each)
#define ONE_HOST(plan, src, len, decim, dst, cnt) m.host(plan, nullptr, src, len, w3[1], decim, 0, dst, cnt)
#define BANK_DEVICE(plan, src, len, chans, w, decim, dst, stride) m.bank_device(plan, src, len, chans, w, decim, 0, dst, stride, nullptr)
#define BANK_TIMED(plan, src, len, chans, w, decim, dst, stride, k, each) \
    sdrk_exec_device_ddcbank_timed_each(plan, src, len, chans, w, decim, 0, dst, stride, k, each)
#define BANK_HOST(plan, src, len, chans, w, decim, dst, stride, cnt) m.bank_host(plan, nullptr, src, len, chans, w, decim, 0, dst, stride, cnt)
    // another length: unsupported, from every entry
    CHECK(ONE_DEVICE(small, in.data(), n, 1, out.data()) == SDRK_ERR_UNSUPPORTED && sdrk_last_error()[0]);
    CHECK(ONE_HOST(small, in.data(), n, 1, out.data(), &got) == SDRK_ERR_UNSUPPORTED);
    CHECK(BANK_DEVICE(small, in.data(), n, 3, w3, 1, out.data(), n) == SDRK_ERR_UNSUPPORTED);
    CHECK(BANK_HOST(small, in.data(), n, 3, w3, 1, out.data(), n, &got) == SDRK_ERR_UNSUPPORTED);
    REFUSED(ONE_DEVICE(f64, in.data(), n, 1, out.data()));
    REFUSED(ONE_HOST(f64, in.data(), n, 1, out.data(), &got));
    REFUSED(BANK_DEVICE(f64, in.data(), n, 3, w3, 1, out.data(), n));
    REFUSED(BANK_HOST(f64, in.data(), n, 3, w3, 1, out.data(), n, &got));
    REFUSED(ONE_DEVICE(nullptr, in.data(), n, 1, out.data()));
    REFUSED(BANK_DEVICE(nullptr, in.data(), n, 3, w3, 1, out.data(), n));
    // no filter set
    REFUSED(ONE_DEVICE(good, in.data(), n, 1, out.data()));
    CHECK(strstr(sdrk_last_error(), "sdrk_plan_set_fir") != nullptr);
    REFUSED(ONE_HOST(good, in.data(), n, 1, out.data(), &got));
    REFUSED(ONE_TIMED(good, in.data(), n, 1, out.data(), 2, ms));
    REFUSED(BANK_DEVICE(good, in.data(), n, 3, w3, 1, out.data(), n));
    REFUSED(BANK_HOST(good, in.data(), n, 3, w3, 1, out.data(), n, &got));
    REFUSED(BANK_TIMED(good, in.data(), n, 3, w3, 1, out.data(), n, 2, ms));
    CHECK(sdrk_plan_set_fir(good, 9, h.data()) == SDRK_OK);
    // the decimation: any integer in 1 .. 256, nothing else
    for (int decim : {0, 257, 512, -2}) {
        REFUSED(ONE_DEVICE(good, in.data(), n, decim, out.data()));
        CHECK(strstr(sdrk_last_error(), "decim") != nullptr);
        REFUSED(ONE_HOST(good, in.data(), n, decim, out.data(), &got));
        REFUSED(ONE_TIMED(good, in.data(), n, decim, out.data(), 2, ms));
        REFUSED(BANK_DEVICE(good, in.data(), n, 3, w3, decim, out.data(), n));
        REFUSED(BANK_HOST(good, in.data(), n, 3, w3, decim, out.data(), n, &got));
        REFUSED(BANK_TIMED(good, in.data(), n, 3, w3, decim, out.data(), n, 2, ms));
        CHECK(sdrk_ddc_outputs(n, 9, decim, 0) == 0);
    }
    // the channel count, the words, the stride
    for (int chans : {0, -1, 65}) {
        REFUSED(BANK_DEVICE(good, in.data(), n, chans, many.data(), 1, out.data(), n));
        CHECK(strstr(sdrk_last_error(), "n_chan") != nullptr);
        REFUSED(BANK_HOST(good, in.data(), n, chans, many.data(), 1, out.data(), n, &got));
        REFUSED(BANK_TIMED(good, in.data(), n, chans, many.data(), 1, out.data(), n, 2, ms));
    }
    REFUSED(BANK_DEVICE(good, in.data(), n, 3, nullptr, 1, out.data(), n));
    CHECK(strstr(sdrk_last_error(), "freq_word") != nullptr);
    REFUSED(BANK_HOST(good, in.data(), n, 3, nullptr, 1, out.data(), n, &got));
    REFUSED(BANK_TIMED(good, in.data(), n, 3, nullptr, 1, out.data(), n, 2, ms));
    REFUSED(BANK_DEVICE(good, in.data(), n, 3, w3, 1, out.data(), n_out - 1));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    REFUSED(BANK_TIMED(good, in.data(), n, 3, w3, 1, out.data(), n_out - 1, 2, ms));
    REFUSED(BANK_HOST(good, in.data(), n, 3, w3, 1, out.data(), n - 1, &got));
    REFUSED(BANK_HOST(good, in.data(), n, 3, w3, 7, out.data(), (n + 6) / 7 - 1, &got));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    // pointers, lengths, the timed entries' own arguments
    REFUSED(ONE_DEVICE(good, nullptr, n, 1, out.data()));
    REFUSED(ONE_DEVICE(good, in.data(), n, 1, nullptr));
    REFUSED(ONE_DEVICE(good, in.data(), 8, 1, out.data()));                             // n_in < M
    REFUSED(BANK_DEVICE(good, nullptr, n, 3, w3, 1, out.data(), n));
    REFUSED(BANK_DEVICE(good, in.data(), n, 3, w3, 1, nullptr, n));
    REFUSED(BANK_DEVICE(good, in.data(), 8, 3, w3, 1, out.data(), n));
    REFUSED(ONE_HOST(good, in.data(), n, 1, out.data(), nullptr));
    REFUSED(ONE_HOST(good, (const S*)nullptr, n, 1, out.data(), &got));
    REFUSED(ONE_HOST(good, in.data(), n, 1, nullptr, &got));
    REFUSED(BANK_HOST(good, in.data(), n, 3, w3, 1, out.data(), n, nullptr));
    REFUSED(ONE_TIMED(good, in.data(), n, 1, out.data(), 0, ms));
    REFUSED(ONE_TIMED(good, in.data(), n, 1, out.data(), 2, nullptr));
    REFUSED(BANK_TIMED(good, in.data(), n, 3, w3, 1, out.data(), n, 0, ms));
    CHECK(sdrk_last_error()[0]);
    got = 7;
    CHECK(BANK_HOST(good, in.data(), 0, 3, w3, 7, out.data(), 0, &got) == SDRK_OK && got == 0);   // an empty piece
    CHECK(sdrk_ddc_outputs(8, 9, 1, 0) == 0 && sdrk_ddc_outputs(9, 0, 1, 0) == 0 && sdrk_ddc_outputs(9, 9, 1, 0) == 1);
#undef ONE_DEVICE
#undef ONE_TIMED
#undef ONE_HOST
#undef BANK_DEVICE
#undef BANK_TIMED
#undef BANK_HOST
    // the refused plans still work
    host_case(m, good, {9, 7, n, 3, true}, 3, 1, 5);
    std::vector<float> x(2 * 1024), row(1024);
    fill(x.data(), 1024, 9);
    const Case one{1024, 1, 1, 0, 1024};
    CHECK(sdrk_exec_host(small, x.data(), 1, 1024, row.data()) == SDRK_OK);
    CHECK(wrong_frames(x.data(), (const float*)nullptr, one, {row.data()}) == 0);
    for (sdrk_plan* p : {f64, good, small}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("ddc", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(I16);
                      },
                      worker);
}

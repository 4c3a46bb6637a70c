// tests/host_api_bank_stress.cpp — drives the host side of the channel-bank entry points (sdrk_exec_device_chanbank*,
// sdrk_exec_host_chanbank*: csrc/fir_api.hip and the staging slots of csrc/sdrk_host_pipeline.hip; built with the other host
// files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp) for the sanitizer
// legs of tests/test_host_sanitizers_bank.py.  A program of its own: nothing is loaded into Python, nothing is preloaded.
//
//   host_api_bank_stress [threads] [iters]         (SDRK_FIR_CHUNK_BLOCKS=3 in the environment: several chunks per host call)
//
// Every thread runs the cases of both formats on plans of its own: the device, the timed and the host entries, C = 1, 3 and 64,
// chunk boundaries with a prefix and without, planes packed and padded — and compares EVERY output element of EVERY channel with
// the single-channel call of the same plan on the same input (sdrk_exec_device_fir* / sdrk_exec_host_fir*, which
// host_api_ols_stress.cpp holds to a float64 convolution): equal bits, since the stand-ins of both run the same transform and
// the shared arithmetic of csrc/kernels_ols.h.  A single-channel call and a PFB call run between bank calls on one plan.
// Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

template <class S> struct Mode {
    const Mode<float>* c64;   // int16: the complex64 mode that defines it, on the widened samples
    decltype(&sdrk_exec_device_chanbank) device;
    decltype(&sdrk_exec_host_chanbank) host;
    decltype(&sdrk_exec_device_fir) one_device;
    decltype(&sdrk_exec_host_fir) one_host;
};
static const Mode<float> C64{nullptr, sdrk_exec_device_chanbank, sdrk_exec_host_chanbank, sdrk_exec_device_fir, sdrk_exec_host_fir};
static const Mode<int16_t> I16{&C64, sdrk_exec_device_chanbank_ci16, sdrk_exec_host_chanbank_ci16, sdrk_exec_device_fir_ci16,
                               sdrk_exec_host_fir_ci16};

struct Bank {
    int taps, decim, n_chan;
    size_t n;            // samples of the piece (device entry: n_in)
    uint64_t sample0;    // host entry
    bool prefix;         // host entry: a non-zero prefix
    size_t pad;          // complex64 between the end of a plane and the next one
};

static const float SENTINEL = -77.0f;

static std::vector<float> int_taps(int m, unsigned seed) {   // complex taps with parts in -2 .. 2, the first one non-zero
    std::vector<float> h(2 * (size_t)m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    h[0] = 1.0f;
    return h;
}

// channel 0 runs no mixer, 1 and 2 sit on the limits, 4 repeats 3, the rest are spread by the seed
static std::vector<int> shifts_of(int n_chan, unsigned seed) {
    std::vector<int> s((size_t)n_chan);
    for (int c = 0; c < n_chan; ++c) s[c] = c == 0 ? 0 : c == 1 ? -2048 : c == 2 ? 2047 : (int)((c * 331u + seed * 17u) % 4096u) - 2048;
    if (n_chan > 4) s[4] = s[3];
    return s;
}
static std::vector<int> phases_of(int n_chan) {
    std::vector<int> ph((size_t)n_chan);
    for (int c = 0; c < n_chan; ++c) ph[c] = 1000 * c - 3000;   // negative ones and ones beyond 4096 among them
    return ph;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

// plane c of `out` (planes `stride` complex64 apart): n_out elements equal to `ref`, the rest of the plane untouched
static bool plane_ok(const std::vector<float>& out, size_t stride, int c, const std::vector<float>& ref, size_t n_out) {
    const float* plane = out.data() + 2 * stride * (size_t)c;
    bool ok = same(plane, std::vector<float>(ref.begin(), ref.begin() + 2 * n_out));
    for (size_t i = 2 * n_out; i < 2 * stride; ++i) ok &= plane[i] == SENTINEL;
    return ok;
}

enum How { DEVICE, TIMED, HOST };

// -> the bank's output (for the callers that compare two bank calls)
template <class S> std::vector<float> run_case(const Mode<S>& m, sdrk_plan* p, const Bank& c, How how, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK && sdrk_plan_fir_taps(p) == c.taps);
    const size_t M = (size_t)c.taps, D = (size_t)c.decim;
    const std::vector<int> shift = shifts_of(c.n_chan, seed), phase = phases_of(c.n_chan);
    std::vector<S> in(2 * c.n), pre(2 * (M - 1) + 2);
    fill(in.data(), c.n, seed + 1);
    fill(pre.data(), M - 1, seed + 2);
    if (how != HOST) {
        const size_t n_out = (c.n - M) / D + 1, stride = n_out + c.pad;
        std::vector<float> out(2 * stride * (size_t)c.n_chan, SENTINEL), ref(2 * n_out);
        const std::vector<float> wide = widen(in.data(), c.n);
        if (how == DEVICE) {
            CHECK(m.device(p, in.data(), c.n, c.decim, c.n_chan, shift.data(), phase.data(), out.data(), stride, nullptr) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK);
        } else {
            float ms[2] = {0, 0};
            CHECK(sdrk_exec_device_chanbank_timed_each(p, wide.data(), c.n, c.decim, c.n_chan, shift.data(), phase.data(), out.data(),
                                                       stride, 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
        }
        for (int ch = 0; ch < c.n_chan; ++ch) {
            if (how == DEVICE) CHECK(m.one_device(p, in.data(), c.n, c.decim, shift[ch], phase[ch], ref.data(), nullptr) == SDRK_OK);
            else CHECK(sdrk_exec_device_fir(p, wide.data(), c.n, c.decim, shift[ch], phase[ch], ref.data(), nullptr) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK);
            CHECK(plane_ok(out, stride, ch, ref, n_out));
        }
        if (how == DEVICE && c.n_chan <= 3) {   // phase0 = NULL: zeros
            std::vector<float> zero(out.size(), SENTINEL);
            CHECK(m.device(p, in.data(), c.n, c.decim, c.n_chan, shift.data(), nullptr, zero.data(), stride, nullptr) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK);
            for (int ch = 0; ch < c.n_chan; ++ch) {
                CHECK(m.one_device(p, in.data(), c.n, c.decim, shift[ch], 0, ref.data(), nullptr) == SDRK_OK);
                CHECK(sdrk_plan_sync(p) == SDRK_OK);
                CHECK(plane_ok(zero, stride, ch, ref, n_out));
            }
        }
        return out;
    }
    const size_t j0 = (size_t)((D - c.sample0 % D) % D);
    const size_t want_out = c.n > j0 ? (c.n - j0 - 1) / D + 1 : 0, stride = (c.n + D - 1) / D + c.pad;
    std::vector<float> out(2 * stride * (size_t)c.n_chan, SENTINEL), ref(2 * stride);
    size_t n_out = 12345;
    const S* prefix = c.prefix && M > 1 ? pre.data() : nullptr;
    CHECK(m.host(p, prefix, in.data(), c.n, c.decim, c.n_chan, shift.data(), c.sample0, out.data(), stride, &n_out) == SDRK_OK);
    CHECK(n_out == want_out);
    for (int ch = 0; ch < c.n_chan; ++ch) {
        size_t n_ref = 0;
        CHECK(m.one_host(p, prefix, in.data(), c.n, c.decim, shift[ch], c.sample0, ref.data(), &n_ref) == SDRK_OK && n_ref == want_out);
        CHECK(plane_ok(out, stride, ch, ref, want_out));
    }
    if (m.c64) {   // the complex64 entry of the same plan agrees on the widened samples, bit for bit
        std::vector<float> wide = widen(in.data(), c.n), wpre = widen(pre.data(), M - 1 + 1), other(out.size(), SENTINEL);
        size_t n_other = 0;
        CHECK(m.c64->host(p, prefix ? wpre.data() : nullptr, wide.data(), c.n, c.decim, c.n_chan, shift.data(), c.sample0, other.data(),
                          stride, &n_other) == SDRK_OK);
        CHECK(n_other == want_out && same(out.data(), other));
    }
    return out;
}

// A single-channel call and a PFB call between two bank calls on one plan: filter and prototype live side by side, every kind
// of output right, the second bank call the bits of the first.
template <class S> void between_case(const Mode<S>& m, sdrk_plan* p, unsigned seed) {
    const Bank c{33, 4, 3, 3 * 4096 + 11, 6, true, 5};
    const Case pf{4096, 2, 3, 0, 4096};
    const std::vector<float> proto_h = proto(4096, 2, seed);
    CHECK(sdrk_plan_set_pfb(p, 2, proto_h.data()) == SDRK_OK);
    const std::vector<float> first = run_case(m, p, c, HOST, seed);   // (ends with single-channel calls of its own)
    std::vector<float> x(2 * in_samples(pf)), rows(n_out(pf), -1.0f);
    fill(x.data(), in_samples(pf), seed + 5);
    CHECK(sdrk_exec_host_pfb(p, x.data(), pf.groups, pf.stride, rows.data()) == SDRK_OK);
    CHECK(wrong_frames(x.data(), proto_h.data(), pf, {rows.data()}) == 0);
    CHECK(same(run_case(m, p, c, HOST, seed).data(), first));
    CHECK(sdrk_plan_pfb_taps(p) == 2 && sdrk_plan_fir_taps(p) == 33);
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s) {
    sdrk_plan* p = make_plan(4096);
    if (!p) return;
    const size_t L5 = 3840, L300 = 3584, L2049 = 2048;
    run_case(m, p, {5, 1, 1, 2 * L5 + 100, 0, false, 0}, DEVICE, s + 1);                // C = 1, packed
    run_case(m, p, {300, 4, 3, 2 * L300 + 17, 0, false, 7}, DEVICE, s + 2);             // C = 3, padded planes
    run_case(m, p, {2049, 64, 64, L2049 + 2049, 0, false, 0}, DEVICE, s + 3);           // C = 64 at the tap limit, two blocks, packed
    if (!m.c64) run_case(m, p, {5, 8, 3, 300, 0, false, 1}, TIMED, s + 4);
    // host entry, 3 blocks per chunk: chunk boundaries with a prefix and without, the first kept sample inside the piece
    run_case(m, p, {300, 8, 3, 7 * L300 + 5, 13, true, 3}, HOST, s + 5);
    run_case(m, p, {300, 8, 3, 10 * L300 + 5, 2, true, 3}, HOST, s + 11);               // four chunks: the first slot's planes leave before it is reused
    run_case(m, p, {5, 1, 1, 4 * L5, 1u << 20, false, 0}, HOST, s + 6);
    run_case(m, p, {2049, 64, 64, 3 * L2049 + 9, 0, false, 0}, HOST, s + 7);            // C = 64 over two chunks
    run_case(m, p, {2, 256, 3, 200, 100, true, 2}, HOST, s + 8);                        // one output a plane: stream index 256
    run_case(m, p, {2, 256, 3, 100, 100, true, 2}, HOST, s + 9);                        // none
    between_case(m, p, s + 10);
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
    const int ok3[3] = {0, 5, -5}, low[3] = {0, -2049, 5}, high[3] = {0, 5, 2048};
    std::vector<int> many(65, 1);
    float ms[2];
    size_t got = 0;
#define DEVICE_CALL(plan, src, len, decim, chans, sh, dst, stride) m.device(plan, src, len, decim, chans, sh, nullptr, dst, stride, nullptr)
#define TIMED_CALL(plan, src, len, decim, chans, sh, dst, stride, k, each) \
    sdrk_exec_device_chanbank_timed_each(plan, src, len, decim, chans, sh, nullptr, dst, stride, k, each)
#define HOST_CALL(plan, src, len, decim, chans, sh, dst, stride, cnt) m.host(plan, nullptr, src, len, decim, chans, sh, 0, dst, stride, cnt)
    // another length: unsupported, from every entry
    CHECK(DEVICE_CALL(small, in.data(), n, 1, 3, ok3, out.data(), n) == SDRK_ERR_UNSUPPORTED && sdrk_last_error()[0]);
    CHECK(HOST_CALL(small, in.data(), n, 1, 3, ok3, out.data(), n, &got) == SDRK_ERR_UNSUPPORTED);
    REFUSED(DEVICE_CALL(f64, in.data(), n, 1, 3, ok3, out.data(), n));
    REFUSED(HOST_CALL(f64, in.data(), n, 1, 3, ok3, out.data(), n, &got));
    REFUSED(DEVICE_CALL(nullptr, in.data(), n, 1, 3, ok3, out.data(), n));
    // no filter set
    REFUSED(DEVICE_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n));
    REFUSED(HOST_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n, &got));
    REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n, 2, ms));
    CHECK(sdrk_plan_set_fir(good, 9, h.data()) == SDRK_OK);
    // the channel count, the shifts, the stride
    for (int chans : {0, -1, 65}) {
        REFUSED(DEVICE_CALL(good, in.data(), n, 1, chans, many.data(), out.data(), n));
        CHECK(strstr(sdrk_last_error(), "n_chan") != nullptr);
        REFUSED(HOST_CALL(good, in.data(), n, 1, chans, many.data(), out.data(), n, &got));
        REFUSED(TIMED_CALL(good, in.data(), n, 1, chans, many.data(), out.data(), n, 2, ms));
    }
    REFUSED(DEVICE_CALL(good, in.data(), n, 1, 3, nullptr, out.data(), n));
    CHECK(strstr(sdrk_last_error(), "shift_bins") != nullptr);
    REFUSED(HOST_CALL(good, in.data(), n, 1, 3, nullptr, out.data(), n, &got));
    REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, nullptr, out.data(), n, 2, ms));
    for (const int* bad : {low, high}) {
        REFUSED(DEVICE_CALL(good, in.data(), n, 1, 3, bad, out.data(), n));
        CHECK(strstr(sdrk_last_error(), "shift_bins[") != nullptr);
        REFUSED(HOST_CALL(good, in.data(), n, 1, 3, bad, out.data(), n, &got));
        REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, bad, out.data(), n, 2, ms));
    }
    REFUSED(DEVICE_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n_out - 1));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n_out - 1, 2, ms));
    REFUSED(HOST_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n - 1, &got));
    REFUSED(HOST_CALL(good, in.data(), n, 4, 3, ok3, out.data(), (n + 3) / 4 - 1, &got));
    CHECK(strstr(sdrk_last_error(), "out_stride") != nullptr);
    // what the single call refuses
    REFUSED(DEVICE_CALL(good, nullptr, n, 1, 3, ok3, out.data(), n));
    REFUSED(DEVICE_CALL(good, in.data(), n, 1, 3, ok3, nullptr, n));
    REFUSED(DEVICE_CALL(good, in.data(), 8, 1, 3, ok3, out.data(), n));                 // n_in < M
    for (int decim : {0, 3, 512, -2}) {
        REFUSED(DEVICE_CALL(good, in.data(), n, decim, 3, ok3, out.data(), n));
        REFUSED(HOST_CALL(good, in.data(), n, decim, 3, ok3, out.data(), n, &got));
        REFUSED(TIMED_CALL(good, in.data(), n, decim, 3, ok3, out.data(), n, 2, ms));
    }
    REFUSED(HOST_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n, nullptr));
    REFUSED(HOST_CALL(good, (const S*)nullptr, n, 1, 3, ok3, out.data(), n, &got));
    REFUSED(HOST_CALL(good, in.data(), n, 1, 3, ok3, nullptr, n, &got));
    REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n, 0, ms));
    REFUSED(TIMED_CALL(good, in.data(), n, 1, 3, ok3, out.data(), n, 2, nullptr));
    CHECK(sdrk_last_error()[0]);
    got = 7;
    CHECK(HOST_CALL(good, in.data(), 0, 1, 3, ok3, out.data(), 0, &got) == SDRK_OK && got == 0);   // an empty piece
#undef DEVICE_CALL
#undef TIMED_CALL
#undef HOST_CALL
    // the refused plans still work
    run_case(m, good, {9, 2, 3, n, 3, true, 1}, HOST, 5);
    std::vector<float> x(2 * 1024), row(1024);
    fill(x.data(), 1024, 9);
    const Case one{1024, 1, 1, 0, 1024};
    CHECK(sdrk_exec_host(small, x.data(), 1, 1024, row.data()) == SDRK_OK);
    CHECK(wrong_frames(x.data(), (const float*)nullptr, one, {row.data()}) == 0);
    for (sdrk_plan* p : {f64, good, small}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("bank", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(I16);
                      },
                      worker);
}

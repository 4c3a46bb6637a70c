// tests/host_api_iq8_modes_stress.cpp — drives the host side of the 8-bit filter-bank and spectral-kurtosis entry points
// (sdrk_exec_*_pfb_iq8, _pfb_integrated_iq8, _kurtosis_iq8, _pfb_kurtosis_iq8: csrc/pfb_api.hip, csrc/integrate_api.hip,
// csrc/integrate_call.h and the staging slots of csrc/sdrk_host_pipeline.hip; built with the other host files by g++ against
// the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp, fake_iq8_modes_kernels.cpp among
// them) for the sanitizer legs of tests/test_host_sanitizers_iq8_modes.py.  A program of its own: nothing is loaded into
// Python, nothing is preloaded.
//
//   host_api_iq8_modes_stress [threads] [iters]
//
// Every thread runs the cases of both formats (ci8, cu8) on plans of its own.  What is compared, element for element and bit
// for bit, is every output with the complex64 entry of the same plan on the widened samples — whose values the other drivers
// check against the stand-ins' definition — so what is under test is what the 8-bit entries add: 2-byte samples in every byte
// offset (chunks of the host pipeline with the (T - 1) * nfft samples of overlap each carries, chunks of the 64 MiB stagings,
// strides, odd sample offsets), the format bound into the launchers, the carry of groups and slices across chunks.
//   per frame    device, timed, host (dB rows) and host (spectra), N = 4096 and folded lengths, pageable and pinned;
//   integrated   every detector and both forms; groups that divide no chunk; one group over several chunks (slices);
//   kurtosis     plain (N = 4096 fused with and without a window, staged lengths, chirp-z) and behind the filter bank;
//   one plan     a call on the plan's stream and one on a stream of the caller's in flight together, both formats, an int16
//                call between them;
// then the refusals.  Exit code 0 = every check passed.
#include "host_stress.h"

#include <cstring>

// per-frame rows are linear in the samples: all 256 byte values
static void fill_bytes(uint8_t* x, size_t n_samples, unsigned seed) {
    std::mt19937 rng(seed);
    for (size_t i = 0; i < 2 * n_samples; ++i) x[i] = (uint8_t)(rng() & 0xFFu);
}
// sums of powers over thousands of frames stay exact: values -6 .. 6 (signed), -5.5 .. 5.5 (unsigned: bytes 122 .. 133)
static void fill_small(uint8_t* x, size_t n_samples, int fmt, unsigned seed) {
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < 2 * n_samples; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i] = fmt == SDRK_IQ8_SIGNED ? (uint8_t)(int8_t)((int)((s >> 16) % 13u) - 6) : (uint8_t)(122u + (s >> 16) % 12u);
    }
}
// the widening of include/sdrk.h, exact in float32
static std::vector<float> widen8(const uint8_t* x, size_t n_samples, int fmt) {
    std::vector<float> w(2 * n_samples);
    for (size_t i = 0; i < 2 * n_samples; ++i) w[i] = fmt == SDRK_IQ8_SIGNED ? (float)(int8_t)x[i] : (float)x[i] - 127.5f;
    return w;
}

static sdrk_plan* make_plan(int nfft, int window = SDRK_WINDOW_RECT, int shift = 1) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, (size_t)1 << 20, window, nullptr, 1e-12f, shift, &p) == SDRK_OK);
    return p;
}

enum Entry { DEVICE, TIMED, HOST, HOST_PINNED };

// ---- per frame ----------------------------------------------------------------------------------------------------------
static void frames_case(int fmt, sdrk_plan* p, int nfft, int taps, size_t frames, size_t stride, Entry e, unsigned seed) {
    const std::vector<float> h = proto_random(nfft, taps, seed);
    CHECK(sdrk_plan_set_pfb(p, taps, h.data()) == SDRK_OK && sdrk_plan_pfb_taps(p) == taps);
    const Case c{nfft, taps, frames, 0, stride};
    const size_t ns = in_samples(c), no = n_out(c);
    const bool pinned = e == HOST_PINNED;
    Buf<uint8_t> in(2 * ns + 2, pinned);   // (one sample of slack: the odd-offset variant below starts at byte 2)
    Buf<float> out(no + 1, pinned);
    if (!in.data() || !out.data()) return;
    fill_bytes(in.data(), ns + 1, seed + 1);
    const uint8_t* x = in.data() + 2 * (seed & 1u);   // every other case: the first sample at byte 2
    const std::vector<float> wide = widen8(x, ns, fmt);
    std::vector<float> ref(no + 1, -3.0f);
    out[no] = -3.0f;
    float ms[2] = {0, 0};
    if (e == DEVICE || e == TIMED) {
        CHECK(sdrk_exec_device_pfb(p, wide.data(), frames, stride, ref.data(), nullptr) == SDRK_OK);
        if (e == DEVICE) CHECK(sdrk_exec_device_pfb_iq8(p, x, fmt, frames, stride, out.data(), nullptr) == SDRK_OK);
        else CHECK(sdrk_exec_device_pfb_iq8_timed_each(p, x, fmt, frames, stride, out.data(), 2, ms) == SDRK_OK && ms[0] > 0 && ms[1] > 0);
        CHECK(sdrk_plan_sync(p) == SDRK_OK);
    } else {
        CHECK(sdrk_exec_host_pfb(p, wide.data(), frames, stride, ref.data()) == SDRK_OK);
        CHECK(sdrk_exec_host_pfb_iq8(p, x, fmt, frames, stride, out.data()) == SDRK_OK);
    }
    CHECK(same(out.data(), ref));   // (the element behind the rows included)
    if (e == HOST) {                // the spectra of the same call
        std::vector<float> spec(2 * no + 1, -3.0f), spec_ref(2 * no + 1, -3.0f);
        CHECK(sdrk_exec_fft_host_pfb(p, wide.data(), frames, stride, spec_ref.data()) == SDRK_OK);
        CHECK(sdrk_exec_fft_host_pfb_iq8(p, x, fmt, frames, stride, spec.data()) == SDRK_OK);
        CHECK(same(spec.data(), spec_ref));
    }
}

// ---- one row (kurtosis: two) per K frames -------------------------------------------------------------------------------
enum Kind { PFB_INT, KURT, PFB_KURT };

static int call8(Kind kind, Entry e, sdrk_plan* p, const uint8_t* x, int fmt, const Case& c, float* out, hipStream_t s = nullptr) {
    float ms[2] = {0, 0};
    int st;
    switch (kind) {
    case PFB_INT:
        if (e == DEVICE) return sdrk_exec_device_pfb_integrated_iq8(p, x, fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out, s);
        if (e == TIMED) st = sdrk_exec_device_pfb_integrated_iq8_timed_each(p, x, fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out, 2, ms);
        else return sdrk_exec_host_pfb_integrated_iq8(p, x, fmt, c.groups, c.k, c.stride, c.det, c.form, c.scale, out);
        break;
    case KURT:
        if (e == DEVICE) return sdrk_exec_device_kurtosis_iq8(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out, s);
        if (e == TIMED) st = sdrk_exec_device_kurtosis_iq8_timed_each(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out, 2, ms);
        else return sdrk_exec_host_kurtosis_iq8(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out);
        break;
    default:
        if (e == DEVICE) return sdrk_exec_device_pfb_kurtosis_iq8(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out, s);
        if (e == TIMED) st = sdrk_exec_device_pfb_kurtosis_iq8_timed_each(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out, 2, ms);
        else return sdrk_exec_host_pfb_kurtosis_iq8(p, x, fmt, c.groups, c.k, c.stride, c.form, c.scale, out);
    }
    CHECK(st != SDRK_OK || (ms[0] > 0 && ms[1] > 0));
    return st;
}

static int call64(Kind kind, bool host, sdrk_plan* p, const float* x, const Case& c, float* out) {
    switch (kind) {
    case PFB_INT:
        return host ? sdrk_exec_host_pfb_integrated(p, x, c.groups, c.k, c.stride, c.det, c.form, c.scale, out)
                    : sdrk_exec_device_pfb_integrated(p, x, c.groups, c.k, c.stride, c.det, c.form, c.scale, out, nullptr);
    case KURT:
        return host ? sdrk_exec_host_sk(p, x, c.groups, c.k, c.stride, c.form, c.scale, out)
                    : sdrk_exec_device_sk(p, x, c.groups, c.k, c.stride, c.form, c.scale, out, nullptr);
    default:
        return host ? sdrk_exec_host_pfb_sk(p, x, c.groups, c.k, c.stride, c.form, c.scale, out)
                    : sdrk_exec_device_pfb_sk(p, x, c.groups, c.k, c.stride, c.form, c.scale, out, nullptr);
    }
}

static void groups_case(Kind kind, int fmt, sdrk_plan* p, const Case& c, Entry e, unsigned seed) {
    std::vector<float> h;
    if (kind != KURT) {
        h = proto(c.nfft, c.taps, seed);
        CHECK(sdrk_plan_set_pfb(p, c.taps, h.data()) == SDRK_OK);
    }
    const size_t ns = in_samples(c), no = n_out(c) * (kind == PFB_INT ? 1 : 2);
    const bool pinned = e == HOST_PINNED, host = e == HOST || e == HOST_PINNED;
    Buf<uint8_t> in(2 * ns + 2, pinned);
    Buf<float> out(no + 1, pinned);
    if (!in.data() || !out.data()) return;
    fill_small(in.data(), ns + 1, fmt, seed + 1);
    const uint8_t* x = in.data() + 2 * (seed & 1u);
    const std::vector<float> wide = widen8(x, ns, fmt);
    std::vector<float> ref(no + 1, -3.0f);
    out[no] = -3.0f;
    CHECK(call64(kind, host, p, wide.data(), c, ref.data()) == SDRK_OK);
    CHECK(call8(kind, e, p, x, fmt, c, out.data()) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(same(out.data(), ref));
}

// A call on the plan's stream and one on a stream of the caller's in flight together, one of each format, an int16 call of
// the same plan between them: one prototype, one state and two stagings per plan.
static void one_plan(sdrk_plan* p, int nfft, unsigned seed) {
    const size_t n = (size_t)nfft;
    const std::vector<float> h = proto(nfft, 3, seed);
    CHECK(sdrk_plan_set_pfb(p, 3, h.data()) == SDRK_OK);
    const Case big{nfft, 3, 3, 40, n, SDRK_DET_MEAN, SDRK_INT_OUT_POWER, 0.5f};   // split: partial rows as well
    const Case small{nfft, 3, 2, 3, n / 2 + 1, SDRK_DET_MAX, SDRK_INT_OUT_DB, 1.0f};
    const Case frames{nfft, 3, 6, 0, n / 2 + 1};   // (the frames of `small`)
    std::vector<uint8_t> a(2 * in_samples(small)), b(2 * in_samples(big));
    fill_small(a.data(), in_samples(small), SDRK_IQ8_UNSIGNED, seed);
    fill_small(b.data(), in_samples(big), SDRK_IQ8_SIGNED, seed + 1);
    std::vector<int16_t> a16(2 * in_samples(small));
    fill(a16.data(), in_samples(small), seed + 2);
    const std::vector<float> wa = widen8(a.data(), in_samples(small), SDRK_IQ8_UNSIGNED), wb = widen8(b.data(), in_samples(big), SDRK_IQ8_SIGNED),
                             w16 = widen(a16.data(), in_samples(small));
    std::vector<float> ra(n_out(small)), rb(n_out(big)), r16(n_out(small)), rk(2 * n_out(small)), rf(n_out(frames));
    std::vector<float> ea(ra.size()), eb(rb.size()), e16(r16.size()), ek(rk.size()), ef(rf.size());
    CHECK(call64(PFB_INT, false, p, wa.data(), small, ea.data()) == SDRK_OK);
    CHECK(call64(PFB_INT, false, p, wb.data(), big, eb.data()) == SDRK_OK);
    CHECK(call64(PFB_INT, false, p, w16.data(), small, e16.data()) == SDRK_OK);
    CHECK(call64(PFB_KURT, false, p, wa.data(), small, ek.data()) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb(p, wa.data(), frames.groups, frames.stride, ef.data(), nullptr) == SDRK_OK);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    hipStream_t s = nullptr;
    CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
    CHECK(call8(PFB_INT, DEVICE, p, b.data(), SDRK_IQ8_SIGNED, big, rb.data()) == SDRK_OK);            // the plan's stream ...
    CHECK(call8(PFB_INT, DEVICE, p, a.data(), SDRK_IQ8_UNSIGNED, small, ra.data(), s) == SDRK_OK);     // ... then the caller's
    CHECK(sdrk_exec_device_pfb_integrated_ci16(p, a16.data(), small.groups, small.k, small.stride, small.det, small.form, small.scale,
                                               r16.data(), nullptr) == SDRK_OK);
    CHECK(call8(PFB_KURT, DEVICE, p, a.data(), SDRK_IQ8_UNSIGNED, small, rk.data(), s) == SDRK_OK);
    CHECK(sdrk_exec_device_pfb_iq8(p, a.data(), SDRK_IQ8_UNSIGNED, frames.groups, frames.stride, rf.data(), nullptr) == SDRK_OK);
    CHECK(hipStreamSynchronize(s) == hipSuccess);
    CHECK(sdrk_plan_sync(p) == SDRK_OK);
    CHECK(same(ra.data(), ea) && same(rb.data(), eb) && same(r16.data(), e16) && same(rk.data(), ek) && same(rf.data(), ef));
    // work of the caller's stream still recorded on the plan when the prototype is replaced
    CHECK(call8(PFB_INT, DEVICE, p, a.data(), SDRK_IQ8_UNSIGNED, small, ra.data(), s) == SDRK_OK);
    const std::vector<float> h2 = proto(nfft, 2, seed + 3);
    CHECK(sdrk_plan_set_pfb(p, 2, h2.data()) == SDRK_OK && sdrk_plan_pfb_taps(p) == 2);
    CHECK(same(ra.data(), ea));   // (set_pfb waited for it)
    CHECK(hipStreamDestroy(s) == hipSuccess);
}

static void format_cases(int fmt, unsigned s) {
    const int MEAN = SDRK_DET_MEAN, MAX = SDRK_DET_MAX, MIN = SDRK_DET_MIN, DB = SDRK_INT_OUT_DB, POW = SDRK_INT_OUT_POWER;
    sdrk_plan *p4k = make_plan(4096), *hann = make_plan(4096, SDRK_WINDOW_HANN, 0), *p1k = make_plan(1024), *p128 = make_plan(128, SDRK_WINDOW_RECT, 0),
              *p1000 = make_plan(1000);
    if (!p4k || !hann || !p1k || !p128 || !p1000) return;
    // per frame
    frames_case(fmt, p4k, 4096, 4, 600, 4096, HOST, s + 1);           // 4.9 MB of bytes: four chunks, each with 3 * 4096 samples of overlap
    frames_case(fmt, p4k, 4096, 2, 701, 2049, HOST_PINNED, s + 2);    // overlapped at an odd hop, pinned both sides
    frames_case(fmt, p4k, 4096, 1, 3, 4096, HOST, s + 3);             // the small call
    frames_case(fmt, p4k, 4096, 3, 9, 1001, DEVICE, s + 4);           // odd sample offsets
    frames_case(fmt, p4k, 4096, 32, 3, 1, TIMED, s + 5);              // the tap limit, hop 1
    frames_case(fmt, p128, 128, 5, 9000, 128, HOST, s + 6);           // a folded length through the host pipeline, three chunks
    frames_case(fmt, p1k, 1024, 3, 600, 1024, DEVICE, s + 7);         // a folded length on the device (two staging chunks: the integrated case below)
    frames_case(fmt, p1000, 1000, 3, 7, 1500, TIMED, s + 8);          // chirp-z, spaced frames
    // integrated behind the filter bank
    groups_case(PFB_INT, fmt, p4k, {4096, 3, 330, 7, 4096, MEAN, DB, 1.0f}, HOST, s + 10);           // 2310 frames: chunks of 2048, 2048 % 7 != 0
    groups_case(PFB_INT, fmt, p4k, {4096, 2, 1, 2100, 4096, MEAN, POW, 0.5f}, HOST_PINNED, s + 11);  // one group over two chunks: slices
    groups_case(PFB_INT, fmt, p4k, {4096, 4, 40, 16, 1024, MIN, POW, 2.0f}, DEVICE, s + 12);
    groups_case(PFB_INT, fmt, p4k, {4096, 5, 2, 100, 1, MAX, DB, 1.0f}, TIMED, s + 13);
    groups_case(PFB_INT, fmt, p1k, {1024, 2, 2750, 3, 512, MAX, DB, 1.0f}, DEVICE, s + 14);          // 8250 frames: two chunks of the staging, a carried unit
    groups_case(PFB_INT, fmt, p1k, {1024, 2, 1180, 7, 1024, MEAN, POW, 1.0f}, HOST, s + 15);         // 8260 frames: two chunks of 8192
    // spectral kurtosis
    groups_case(KURT, fmt, p4k, {4096, 1, 330, 7, 4096, MEAN, DB, 1.0f}, HOST, s + 20);
    groups_case(KURT, fmt, p4k, {4096, 1, 1, 2100, 4096, MEAN, POW, 0.25f}, HOST, s + 21);           // slices, partials, finalize
    groups_case(KURT, fmt, hann, {4096, 1, 2, 33, 1001, MEAN, DB, 1.0f}, DEVICE, s + 22);            // windowed, odd sample offsets
    groups_case(KURT, fmt, hann, {4096, 1, 40, 5, 4096, MEAN, POW, 1.0f}, TIMED, s + 23);
    groups_case(KURT, fmt, p1k, {1024, 1, 400, 9, 512, MEAN, DB, 1.0f}, HOST_PINNED, s + 24);        // the widening route
    groups_case(KURT, fmt, p1000, {1000, 1, 3, 4, 1000, MEAN, DB, 1.0f, true}, DEVICE, s + 25);      // chirp-z
    // ... behind the filter bank (staged at every length)
    groups_case(PFB_KURT, fmt, p4k, {4096, 4, 420, 5, 4096, MEAN, DB, 1.0f}, HOST, s + 30);          // 2100 frames: two chunks
    groups_case(PFB_KURT, fmt, p4k, {4096, 4, 6, 5, 4096, MEAN, POW, 3.0f}, DEVICE, s + 31);
    groups_case(PFB_KURT, fmt, p1k, {1024, 4, 5, 6, 512, MEAN, DB, 1.0f}, TIMED, s + 32);
    groups_case(PFB_KURT, fmt, p1000, {1000, 3, 4, 3, 1000, MEAN, DB, 1.0f, true}, HOST, s + 33);
    one_plan(p4k, 4096, s + 40);
    one_plan(p1k, 1024, s + 41);
    for (sdrk_plan* p : {p4k, hann, p1k, p128, p1000}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        const unsigned s = 1000u * (unsigned)t + 100u * (unsigned)it;
        format_cases(SDRK_IQ8_SIGNED, s);
        format_cases(SDRK_IQ8_UNSIGNED, s + 50);
    }
}

// Every refusal comes with its status and a message, from the device, the timed and the host entries; the plans still work after.
static void refusals() {
    sdrk_plan* f64 = nullptr;
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &f64) == SDRK_OK);
    sdrk_plan *good = make_plan(4096), *bare = make_plan(4096), *windowed = make_plan(4096, SDRK_WINDOW_HANN);
    if (!f64 || !good || !bare || !windowed) return;
    const std::vector<float> h = proto(4096, 2, 3);
    CHECK(sdrk_plan_set_pfb(good, 2, h.data()) == SDRK_OK);
    const size_t n = 6 * 4096;
    std::vector<uint8_t> in(2 * n);
    std::vector<float> out(2 * 4 * 4096);
    fill_bytes(in.data(), n, 77);
    float ms[2];
    const uint8_t* x = in.data();
    float* o = out.data();
#define PF_DEVICE(p, src, fmt, frames, stride, dst) sdrk_exec_device_pfb_iq8(p, src, fmt, frames, stride, dst, nullptr)
#define PF_TIMED(p, src, fmt, frames, stride, dst, k, each) sdrk_exec_device_pfb_iq8_timed_each(p, src, fmt, frames, stride, dst, k, each)
#define PF_HOST(p, src, fmt, frames, stride, dst) sdrk_exec_host_pfb_iq8(p, src, fmt, frames, stride, dst)
#define PF_FFT(p, src, fmt, frames, stride, dst) sdrk_exec_fft_host_pfb_iq8(p, src, fmt, frames, stride, dst)
#define PI_DEVICE(p, src, fmt, g, k, stride, det, form, dst) sdrk_exec_device_pfb_integrated_iq8(p, src, fmt, g, k, stride, det, form, 1.0f, dst, nullptr)
#define PI_TIMED(p, src, fmt, g, k, stride, det, form, dst, l, each) \
    sdrk_exec_device_pfb_integrated_iq8_timed_each(p, src, fmt, g, k, stride, det, form, 1.0f, dst, l, each)
#define PI_HOST(p, src, fmt, g, k, stride, det, form, dst) sdrk_exec_host_pfb_integrated_iq8(p, src, fmt, g, k, stride, det, form, 1.0f, dst)
#define KU_DEVICE(p, src, fmt, g, k, stride, form, dst) sdrk_exec_device_kurtosis_iq8(p, src, fmt, g, k, stride, form, 1.0f, dst, nullptr)
#define KU_TIMED(p, src, fmt, g, k, stride, form, dst, l, each) sdrk_exec_device_kurtosis_iq8_timed_each(p, src, fmt, g, k, stride, form, 1.0f, dst, l, each)
#define KU_HOST(p, src, fmt, g, k, stride, form, dst) sdrk_exec_host_kurtosis_iq8(p, src, fmt, g, k, stride, form, 1.0f, dst)
#define PK_DEVICE(p, src, fmt, g, k, stride, form, dst) sdrk_exec_device_pfb_kurtosis_iq8(p, src, fmt, g, k, stride, form, 1.0f, dst, nullptr)
#define PK_TIMED(p, src, fmt, g, k, stride, form, dst, l, each) \
    sdrk_exec_device_pfb_kurtosis_iq8_timed_each(p, src, fmt, g, k, stride, form, 1.0f, dst, l, each)
#define PK_HOST(p, src, fmt, g, k, stride, form, dst) sdrk_exec_host_pfb_kurtosis_iq8(p, src, fmt, g, k, stride, form, 1.0f, dst)
    // the format: the two values, nothing else, from every entry, with the text of the 8-bit spectra
    for (int fmt : {2, -1, 255}) {
        REFUSED(PF_DEVICE(good, x, fmt, 2, 4096, o));
        CHECK(strstr(sdrk_last_error(), "is neither SDRK_IQ8_SIGNED nor SDRK_IQ8_UNSIGNED") != nullptr);
        REFUSED(PF_TIMED(good, x, fmt, 2, 4096, o, 2, ms));
        REFUSED(PF_HOST(good, x, fmt, 2, 4096, o));
        REFUSED(PF_FFT(good, x, fmt, 2, 4096, o));
        REFUSED(PI_DEVICE(good, x, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(PI_TIMED(good, x, fmt, 2, 2, 4096, 0, 0, o, 2, ms));
        REFUSED(PI_HOST(good, x, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(KU_DEVICE(good, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(KU_TIMED(good, x, fmt, 2, 2, 4096, 0, o, 2, ms));
        REFUSED(KU_HOST(good, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(PK_DEVICE(good, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(PK_TIMED(good, x, fmt, 2, 2, 4096, 0, o, 2, ms));
        REFUSED(PK_HOST(good, x, fmt, 2, 2, 4096, 0, o));
        CHECK(strstr(sdrk_last_error(), "iq8_format") != nullptr);
    }
    for (int fmt : {SDRK_IQ8_SIGNED, SDRK_IQ8_UNSIGNED}) {
        // the filter bank's own, in the twins' words: a float64 plan, a windowed plan, no prototype, no plan
        REFUSED(PF_DEVICE(f64, x, fmt, 2, 4096, o));
        CHECK(strstr(sdrk_last_error(), "the polyphase filter bank serves float32 plans only") != nullptr);
        REFUSED(PF_HOST(f64, x, fmt, 2, 4096, o));
        REFUSED(PI_HOST(f64, x, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(PK_DEVICE(f64, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(KU_HOST(f64, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(KU_TIMED(f64, x, fmt, 2, 2, 4096, 0, o, 2, ms));
        REFUSED(PF_FFT(windowed, x, fmt, 2, 4096, o));
        CHECK(strstr(sdrk_last_error(), "SDRK_WINDOW_RECT") != nullptr);
        REFUSED(PI_DEVICE(windowed, x, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(PK_HOST(windowed, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(PF_TIMED(bare, x, fmt, 2, 4096, o, 2, ms));
        CHECK(strstr(sdrk_last_error(), "sdrk_plan_set_pfb") != nullptr);
        REFUSED(PI_TIMED(bare, x, fmt, 2, 2, 4096, 0, 0, o, 2, ms));
        REFUSED(PK_TIMED(bare, x, fmt, 2, 2, 4096, 0, o, 2, ms));
        REFUSED(PF_DEVICE(nullptr, x, fmt, 2, 4096, o));
        REFUSED(PI_HOST(nullptr, x, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(KU_DEVICE(nullptr, x, fmt, 2, 2, 4096, 0, o));
        REFUSED(PK_HOST(nullptr, x, fmt, 2, 2, 4096, 0, o));
        // per frame: frames, pointers, the stride, the timed entries' own arguments
        REFUSED(PF_DEVICE(good, x, fmt, 0, 4096, o));
        REFUSED(PF_HOST(good, nullptr, fmt, 2, 4096, o));
        REFUSED(PF_FFT(good, x, fmt, 2, 4096, nullptr));
        REFUSED(PF_HOST(good, x, fmt, 2, 0, o));
        REFUSED(PF_TIMED(good, x, fmt, 2, 4096, o, 0, ms));
        REFUSED(PF_TIMED(good, x, fmt, 2, 4096, o, 2, nullptr));
        // integrated: groups, K, stride, detector, form, pointers
        REFUSED(PI_HOST(good, x, fmt, 0, 2, 4096, 0, 0, o));
        REFUSED(PI_DEVICE(good, x, fmt, 2, 0, 4096, 0, 0, o));
        REFUSED(PI_HOST(good, x, fmt, 2, 2, 0, 0, 0, o));
        REFUSED(PI_DEVICE(good, x, fmt, 2, 2, 4096, 3, 0, o));
        REFUSED(PI_HOST(good, x, fmt, 2, 2, 4096, 0, 2, o));
        REFUSED(PI_DEVICE(good, nullptr, fmt, 2, 2, 4096, 0, 0, o));
        REFUSED(PI_HOST(good, x, fmt, 2, 2, 4096, 0, 0, nullptr));
        REFUSED(PI_TIMED(good, x, fmt, 2, 2, 4096, 0, 0, o, 0, ms));
        REFUSED(PI_TIMED(good, x, fmt, 2, 2, 4096, 0, 0, o, 2, nullptr));
        // kurtosis: K < 2 as well
        REFUSED(KU_DEVICE(good, x, fmt, 2, 1, 4096, 0, o));
        REFUSED(KU_HOST(good, x, fmt, 2, 1, 4096, 0, o));
        REFUSED(PK_DEVICE(good, x, fmt, 2, 1, 4096, 0, o));
        REFUSED(PK_HOST(good, x, fmt, 2, 0, 4096, 0, o));
        REFUSED(KU_HOST(good, x, fmt, 0, 2, 4096, 0, o));
        REFUSED(KU_DEVICE(good, x, fmt, 2, 2, 0, 0, o));
        REFUSED(KU_HOST(good, x, fmt, 2, 2, 4096, 2, o));
        REFUSED(PK_DEVICE(good, x, fmt, 2, 2, 4096, -1, o));
        REFUSED(KU_DEVICE(good, nullptr, fmt, 2, 2, 4096, 0, o));
        REFUSED(PK_HOST(good, x, fmt, 2, 2, 4096, 0, nullptr));
        REFUSED(KU_TIMED(good, x, fmt, 2, 2, 4096, 0, o, 0, ms));
        REFUSED(PK_TIMED(good, x, fmt, 2, 2, 4096, 0, o, 2, nullptr));
        CHECK(sdrk_last_error()[0]);
    }
#undef PF_DEVICE
#undef PF_TIMED
#undef PF_HOST
#undef PF_FFT
#undef PI_DEVICE
#undef PI_TIMED
#undef PI_HOST
#undef KU_DEVICE
#undef KU_TIMED
#undef KU_HOST
#undef PK_DEVICE
#undef PK_TIMED
#undef PK_HOST
    // the refused plans still work
    frames_case(SDRK_IQ8_UNSIGNED, good, 4096, 2, 5, 4096, HOST, 5);
    groups_case(PFB_INT, SDRK_IQ8_SIGNED, good, {4096, 2, 2, 2, 4096}, DEVICE, 6);
    groups_case(KURT, SDRK_IQ8_UNSIGNED, windowed, {4096, 1, 2, 2, 4096}, HOST, 7);
    groups_case(PFB_KURT, SDRK_IQ8_SIGNED, bare, {4096, 2, 2, 2, 4096}, HOST, 8);   // (sets a prototype first)
    for (sdrk_plan* p : {f64, good, bare, windowed}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("iq8_modes", threads, iters, refusals, worker);
}

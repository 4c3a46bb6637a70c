// tests/host_api_ols_stress.cpp — drives the host side of the FIR filtering / channel extraction entry points (sdrk_plan_set_fir,
// sdrk_exec_device_fir*, sdrk_exec_host_fir*: csrc/fir_api.hip and the staging slots of csrc/sdrk_host_pipeline.hip; built with
// the other host files by g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp)
// for the sanitizer legs of tests/test_host_sanitizers_ols.py.  A program of its own: nothing is loaded into Python, nothing is
// preloaded.
//
//   host_api_ols_stress [threads] [iters]          (SDRK_FIR_CHUNK_BLOCKS=3 in the environment: several chunks per host call)
//
// Every thread runs the cases of both formats on plans of its own: the device, the timed and the host entries, chunk boundaries
// with a prefix and without, decimation phases that start inside the piece, a PFB call between two FIR calls on one plan — and
// checks EVERY output element against a direct convolution in float64.  The stand-in launcher (tests/fake_ols_kernels.cpp) runs
// the real block geometry and the shared arithmetic of csrc/kernels_ols.h around a float64 transform, so with samples of
// -6 .. 6 and integer taps every element is within the GPU tests' bound, 1e-5 ||h||_1 max|x|, however the call was chunked.
// Exit code 0 = every check passed.
#include "host_stress.h"

#include <cmath>
#include <complex>
#include <cstring>

typedef std::complex<double> cd;
static const double PI = 3.14159265358979323846;

template <class S> struct Mode {
    const Mode<float>* c64;   // int16: the complex64 mode that defines it, on the widened samples
    decltype(&sdrk_exec_device_fir) device;
    decltype(&sdrk_exec_host_fir) host;
};
static const Mode<float> C64{nullptr, sdrk_exec_device_fir, sdrk_exec_host_fir};
static const Mode<int16_t> I16{&C64, sdrk_exec_device_fir_ci16, sdrk_exec_host_fir_ci16};

struct Fir {
    int taps, decim, shift;
    size_t n;            // samples of the piece (device entry: n_in)
    long phase0;         // device entry
    uint64_t sample0;    // host entry
    bool prefix;         // host entry: a non-zero prefix
};

static std::vector<float> int_taps(int m, unsigned seed) {   // complex taps with parts in -2 .. 2, the first one non-zero
    std::vector<float> h(2 * (size_t)m);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((int)((i * 7u + seed) % 5u) - 2);
    h[0] = 1.0f;
    return h;
}

static sdrk_plan* make_plan(int nfft) {
    sdrk_plan* p = nullptr;
    CHECK(sdrk_plan_create(0, nfft, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p) == SDRK_OK);
    return p;
}

// Wrong elements of out[0 .. n_out): out[m] = v[i] exp(-2 pi i ((phase + s i) mod 4096) / 4096) at i = first + m D, with
// v[i] = sum_t h[t] exp(2 pi i s t / 4096) x[i + M - 1 - t] over the (virtual) stream x.
static int wrong_fir(const std::vector<cd>& x, const std::vector<float>& h, const Fir& c, size_t first, long phase, const float* out,
                     size_t n_out) {
    const size_t M = (size_t)c.taps;
    std::vector<cd> hs(M);
    double l1 = 0, peak = 0;
    for (size_t t = 0; t < M; ++t) {
        hs[t] = cd(h[2 * t], h[2 * t + 1]) * std::polar(1.0, 2 * PI * (double)(((long)c.shift * (long)t) % 4096) / 4096.0);
        l1 += std::abs(hs[t]);
    }
    for (const cd& v : x) peak = std::max(peak, std::abs(v));
    const double tol = 1e-5 * l1 * peak;
    int bad = 0;
    for (size_t m = 0; m < n_out; ++m) {
        const size_t i = first + m * (size_t)c.decim;
        cd v = 0;
        for (size_t t = 0; t < M; ++t) v += hs[t] * x[i + M - 1 - t];
        const long q = (((phase + (long)c.shift * (long)(i % 4096)) % 4096) + 4096) % 4096;
        v *= std::polar(1.0, -2 * PI * (double)q / 4096.0);
        if (!(std::abs(cd(out[2 * m], out[2 * m + 1]) - v) <= tol) && bad++ == 0)
            fprintf(stderr, "taps=%d decim=%d shift=%d n=%zu: output %zu is (%.9g, %.9g), not (%.9g, %.9g)\n", c.taps, c.decim, c.shift,
                    c.n, m, (double)out[2 * m], (double)out[2 * m + 1], v.real(), v.imag());
    }
    g_compared += 2 * n_out;
    return bad;
}

template <class S> std::vector<cd> as_cd(const S* x, size_t n) {
    std::vector<cd> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = cd((double)x[2 * i], (double)x[2 * i + 1]);
    return v;
}

enum How { DEVICE, TIMED, HOST };

template <class S> void run_case(const Mode<S>& m, sdrk_plan* p, const Fir& c, How how, unsigned seed) {
    const std::vector<float> h = int_taps(c.taps, seed);
    CHECK(sdrk_plan_set_fir(p, c.taps, h.data()) == SDRK_OK && sdrk_plan_fir_taps(p) == c.taps);
    const size_t M = (size_t)c.taps, D = (size_t)c.decim;
    std::vector<S> in(2 * c.n), pre(2 * (M - 1) + 2);
    fill(in.data(), c.n, seed + 1);
    fill(pre.data(), M - 1, seed + 2);
    if (how != HOST) {
        const size_t n_out = (c.n - M) / D + 1;
        std::vector<float> out(2 * n_out + 2, -1.0f);
        float ms[2] = {0, 0};
        if (how == DEVICE) {
            CHECK(m.device(p, in.data(), c.n, c.decim, c.shift, (int)c.phase0, out.data(), nullptr) == SDRK_OK);
            CHECK(sdrk_plan_sync(p) == SDRK_OK);
        } else {
            std::vector<float> wide = widen(in.data(), c.n);
            CHECK(sdrk_exec_device_fir_timed_each(p, wide.data(), c.n, c.decim, c.shift, (int)c.phase0, out.data(), 2, ms) == SDRK_OK &&
                  ms[0] > 0 && ms[1] > 0);
        }
        CHECK(wrong_fir(as_cd(in.data(), c.n), h, c, 0, c.phase0, out.data(), n_out) == 0);
        CHECK(out[2 * n_out] == -1.0f && out[2 * n_out + 1] == -1.0f);   // nothing past n_out
        return;
    }
    const size_t j0 = (size_t)((D - c.sample0 % D) % D);
    const size_t want_out = c.n > j0 ? (c.n - j0 - 1) / D + 1 : 0;
    std::vector<float> out(2 * ((c.n + D - 1) / D) + 2, -1.0f);
    size_t n_out = 12345;
    const S* prefix = c.prefix && M > 1 ? pre.data() : nullptr;
    CHECK(m.host(p, prefix, in.data(), c.n, c.decim, c.shift, c.sample0, out.data(), &n_out) == SDRK_OK);
    CHECK(n_out == want_out);
    std::vector<cd> virt(M - 1 + c.n);
    for (size_t i = 0; i + 1 < M; ++i) virt[i] = prefix ? cd((double)pre[2 * i], (double)pre[2 * i + 1]) : cd(0, 0);
    for (size_t i = 0; i < c.n; ++i) virt[M - 1 + i] = cd((double)in[2 * i], (double)in[2 * i + 1]);
    const long phase = (long)(((uint64_t)(c.shift & 4095) * (c.sample0 % 4096)) % 4096);
    CHECK(wrong_fir(virt, h, c, j0, phase, out.data(), n_out) == 0);
    CHECK(out[2 * want_out] == -1.0f);
    if (m.c64) {   // the complex64 entry of the same plan agrees on the widened samples, bit for bit
        std::vector<float> wide = widen(in.data(), c.n), wpre = widen(pre.data(), M - 1 + 1), ref(2 * want_out + 2, -2.0f);
        size_t n_ref = 0;
        CHECK(m.c64->host(p, prefix ? wpre.data() : nullptr, wide.data(), c.n, c.decim, c.shift, c.sample0, ref.data(), &n_ref) == SDRK_OK);
        ref.resize(2 * want_out);
        CHECK(n_ref == want_out && same(out.data(), ref));
    }
}

// A PFB call between two FIR calls on one plan: filter and prototype live side by side, both kinds of output right.
template <class S> void between_case(const Mode<S>& m, sdrk_plan* p, unsigned seed) {
    const Fir c{33, 4, 100, 3 * 4096 + 11, 0, 6, true};
    const Case pf{4096, 2, 3, 0, 4096};
    const std::vector<float> proto_h = proto(4096, 2, seed);
    CHECK(sdrk_plan_set_pfb(p, 2, proto_h.data()) == SDRK_OK);
    run_case(m, p, c, HOST, seed);
    std::vector<float> x(2 * in_samples(pf)), rows(n_out(pf), -1.0f);
    fill(x.data(), in_samples(pf), seed + 5);
    CHECK(sdrk_exec_host_pfb(p, x.data(), pf.groups, pf.stride, rows.data()) == SDRK_OK);
    CHECK(wrong_frames(x.data(), proto_h.data(), pf, {rows.data()}) == 0);
    run_case(m, p, c, HOST, seed);
    CHECK(sdrk_plan_pfb_taps(p) == 2 && sdrk_plan_fir_taps(p) == 33);
}

template <class S> void mode_cases(const Mode<S>& m, unsigned s) {
    sdrk_plan* p = make_plan(4096);
    if (!p) return;
    const size_t L5 = 3840, L300 = 3584, L2049 = 2048;
    run_case(m, p, {5, 1, 0, 3 * L5 + 100, 0, 0, false}, DEVICE, s + 1);
    run_case(m, p, {300, 4, -37, 2 * L300 + 17, 77, 0, false}, DEVICE, s + 2);
    run_case(m, p, {1, 2, 5, 4096 + 1, -5000, 0, false}, DEVICE, s + 3);               // one tap, a negative phase0
    if (!m.c64) run_case(m, p, {5, 8, 2047, 300, 4095, 0, false}, TIMED, s + 4);
    // host entry, 3 blocks per chunk: chunk boundaries with a prefix and without, the first kept sample inside the piece
    run_case(m, p, {300, 8, 611, 7 * L300 + 5, 0, 13, true}, HOST, s + 5);
    run_case(m, p, {5, 1, -2048, 10 * L5, 0, 1u << 20, false}, HOST, s + 6);
    run_case(m, p, {2049, 64, 0, 4 * L2049 + 9, 0, 0, false}, HOST, s + 7);            // the tap limit, lfilter
    run_case(m, p, {2, 256, 3, 200, 0, 100, true}, HOST, s + 8);                       // one output: stream index 256
    run_case(m, p, {2, 256, 3, 100, 0, 100, true}, HOST, s + 9);                       // none
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
    std::vector<S> in(2 * 5000);
    std::vector<float> out(2 * 5000);
    fill(in.data(), 5000, 77);
    float ms[2];
    size_t n_out = 0;
    // another length: unsupported, from every entry
    CHECK(sdrk_plan_set_fir(small, 9, h.data()) == SDRK_ERR_UNSUPPORTED && sdrk_last_error()[0]);
    CHECK(m.device(small, in.data(), 5000, 1, 0, 0, out.data(), nullptr) == SDRK_ERR_UNSUPPORTED);
    CHECK(m.host(small, nullptr, in.data(), 5000, 1, 0, 0, out.data(), &n_out) == SDRK_ERR_UNSUPPORTED);
    CHECK(sdrk_plan_fir_taps(small) == 0);
    REFUSED(sdrk_plan_set_fir(f64, 9, h.data()));
    REFUSED(m.device(f64, in.data(), 5000, 1, 0, 0, out.data(), nullptr));
    // no filter set
    REFUSED(m.device(good, in.data(), 5000, 1, 0, 0, out.data(), nullptr));
    REFUSED(m.host(good, nullptr, in.data(), 5000, 1, 0, 0, out.data(), &n_out));
    REFUSED(sdrk_exec_device_fir_timed_each(good, in.data(), 5000, 1, 0, 0, out.data(), 2, ms));
    REFUSED(sdrk_plan_set_fir(good, 0, h.data()));
    REFUSED(sdrk_plan_set_fir(good, 2050, h.data()));
    REFUSED(sdrk_plan_set_fir(good, 9, nullptr));
    REFUSED(sdrk_plan_set_fir(nullptr, 9, h.data()));
    CHECK(sdrk_plan_set_fir(good, 9, h.data()) == SDRK_OK);
    REFUSED(m.device(good, nullptr, 5000, 1, 0, 0, out.data(), nullptr));
    REFUSED(m.device(good, in.data(), 5000, 1, 0, 0, nullptr, nullptr));
    REFUSED(m.device(good, in.data(), 8, 1, 0, 0, out.data(), nullptr));               // n_in < M
    REFUSED(m.device(nullptr, in.data(), 5000, 1, 0, 0, out.data(), nullptr));
    for (int decim : {0, 3, 512, -2}) {
        REFUSED(m.device(good, in.data(), 5000, decim, 0, 0, out.data(), nullptr));
        REFUSED(m.host(good, nullptr, in.data(), 5000, decim, 0, 0, out.data(), &n_out));
        REFUSED(sdrk_exec_device_fir_timed_each(good, in.data(), 5000, decim, 0, 0, out.data(), 2, ms));
    }
    for (int shift : {-2049, 2048}) {
        REFUSED(m.device(good, in.data(), 5000, 1, shift, 0, out.data(), nullptr));
        REFUSED(m.host(good, nullptr, in.data(), 5000, 1, shift, 0, out.data(), &n_out));
    }
    REFUSED(m.host(good, nullptr, in.data(), 5000, 1, 0, 0, out.data(), nullptr));
    REFUSED(m.host(good, nullptr, nullptr, 5000, 1, 0, 0, out.data(), &n_out));
    REFUSED(m.host(good, nullptr, in.data(), 5000, 1, 0, 0, nullptr, &n_out));
    REFUSED(sdrk_exec_device_fir_timed_each(good, in.data(), 5000, 1, 0, 0, out.data(), 0, ms));
    REFUSED(sdrk_exec_device_fir_timed_each(good, in.data(), 5000, 1, 0, 0, out.data(), 2, nullptr));
    CHECK(sdrk_last_error()[0]);
    n_out = 7;
    CHECK(m.host(good, nullptr, in.data(), 0, 1, 0, 0, out.data(), &n_out) == SDRK_OK && n_out == 0);   // an empty piece
    // the refused plans still work
    run_case(m, good, {9, 2, -7, 5000, 0, 3, true}, HOST, 5);
    std::vector<float> x(2 * 1024), row(1024);
    fill(x.data(), 1024, 9);
    const Case one{1024, 1, 1, 0, 1024};
    CHECK(sdrk_exec_host(small, x.data(), 1, 1024, row.data()) == SDRK_OK);
    CHECK(wrong_frames(x.data(), (const float*)nullptr, one, {row.data()}) == 0);
    for (sdrk_plan* p : {f64, good, small}) CHECK(sdrk_plan_destroy(p) == SDRK_OK);
}

int main(int argc, char** argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 2, iters = argc > 2 ? atoi(argv[2]) : 1;
    return run_stress("ols", threads, iters,
                      [] {
                          mode_refusals(C64);
                          mode_refusals(I16);
                      },
                      worker);
}

// tests/host_api_f64_stress.cpp — drives the host side of the double-precision entry points (csrc/sdrk_f64.hip on top of
// csrc/sdrk_host_pipeline.hip's numpy boundary; all host files csrc/sdrk_*.hip built with g++ against the stand-in runtime
// of tests/fake_hip and the stand-in launcher of tests/fake_f64_kernels.cpp) for the sanitizer legs of tests/test_host_sanitizers_f64.py.
//
// Every path of sdrk_exec_host_f64 with 16-byte samples — the mapped small call, the zero-copy chunks, the three-slot DMA
// pipeline from pageable and from pinned caller arrays, overlapped frames, ragged last chunks, the two-pass lengths' scratch —
// must deliver 3 re - im + (k & 1023) for every element (complex epilogue: (re + 1, im - 1)), from two threads on two plans at
// once; and plans of one precision must be refused by the other precision's entry points.  Exit code 0 = every check passed.
#include "host_stress.h"

// One call of each epilogue over (n_frames, stride) of nfft, from pageable or pinned (library-allocated) arrays.
static void one_case(sdrk_plan* p, int nfft, size_t n_frames, size_t stride, bool pinned, unsigned seed) {
    const size_t in_samples = (n_frames - 1) * stride + (size_t)nfft, rows = n_frames * (size_t)nfft;
    Buf<double> in(2 * in_samples, pinned), db(rows, pinned), cx(2 * rows, pinned);
    if (!in.data() || !db.data() || !cx.data()) return;
    fill_wide(in.data(), in_samples, seed);
    CHECK(sdrk_exec_host_f64(p, in.data(), n_frames, stride, db.data()) == SDRK_OK);
    CHECK(sdrk_exec_fft_host_f64(p, in.data(), n_frames, stride, cx.data()) == SDRK_OK);
    int bad = 0;
    for (size_t f = 0; f < n_frames; ++f)
        for (size_t k = 0; k < (size_t)nfft; ++k) {
            const double re = in[2 * (f * stride + k)], im = in[2 * (f * stride + k) + 1];
            bad += db[f * nfft + k] != 3.0 * re - im + (double)(k & 1023);
            bad += cx[2 * (f * nfft + k)] != re + 1.0 || cx[2 * (f * nfft + k) + 1] != im - 1.0;
        }
    g_compared += 3 * rows;
    CHECK(bad == 0);
}

static void worker(int t, int iters) {
    for (int it = 0; it < iters; ++it) {
        sdrk_plan *p4k = nullptr, *p1k = nullptr, *p64k = nullptr;
        CHECK(sdrk_plan_create_f64(0, 4096, 1 << 20, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p4k) == SDRK_OK);
        CHECK(sdrk_plan_create_f64(0, 1024, 1 << 20, SDRK_WINDOW_HANN, nullptr, 0.0, 0, &p1k) == SDRK_OK);
        CHECK(sdrk_plan_create_f64(0, 65536, 40, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p64k) == SDRK_OK);
        if (!p4k || !p1k || !p64k) return;
        CHECK(sdrk_plan_precision(p4k) == 64 && sdrk_plan_nfft(p4k) == 4096 && sdrk_plan_device(p4k) == 0);
        const unsigned s = 1000u * (unsigned)t + (unsigned)it;
        one_case(p4k, 4096, 1, 4096, false, s + 1);        // the live call: 64 KiB, the mapped small path
        one_case(p4k, 4096, 3, 4096, true, s + 2);         // small, pinned
        one_case(p1k, 1024, 1500, 1024, false, s + 3);     // 24 MiB of packed frames: zero-copy chunks
        one_case(p4k, 4096, 700, 4096, false, s + 4);      // 44 MiB: the DMA pipeline, ragged last chunk
        one_case(p4k, 4096, 900, 2048, false, s + 5);      // overlapped frames
        one_case(p4k, 4096, 700, 4096, true, s + 6);       // pinned caller arrays, chunked
        one_case(p4k, 4096, 100, 4096, true, s + 7);       // pinned both sides, one launch
        one_case(p64k, 65536, 37, 65536, false, s + 8);    // two-pass length, scratch sized by max_batch
        CHECK(sdrk_plan_sync(p64k) == SDRK_OK);
        CHECK(sdrk_plan_destroy(p4k) == SDRK_OK);
        CHECK(sdrk_plan_destroy(p1k) == SDRK_OK);
        CHECK(sdrk_plan_destroy(p64k) == SDRK_OK);
    }
}

static void refusals() {
    sdrk_plan *p64 = nullptr, *p32 = nullptr, *q = nullptr;
    CHECK(sdrk_plan_create_f64(0, 1000, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &q) == SDRK_ERR_UNSUPPORTED && !q);
    CHECK(sdrk_plan_create_f64(0, 1 << 23, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &q) == SDRK_ERR_INVALID && !q);
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_CUSTOM, nullptr, 1e-12, 1, &q) == SDRK_ERR_INVALID && !q);
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, -1.0, 1, &q) == SDRK_ERR_INVALID && !q);
    CHECK(sdrk_plan_create_f64(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12, 1, &p64) == SDRK_OK);
    CHECK(sdrk_plan_create(0, 4096, 4, SDRK_WINDOW_RECT, nullptr, 1e-12f, 1, &p32) == SDRK_OK);
    if (!p64 || !p32) return;
    CHECK(sdrk_plan_precision(p32) == 32);
    std::vector<double> in(2 * 4 * 4096, 1.0), out(2 * 4 * 4096);
    std::vector<float> out32(4 * 4096);
    REFUSED(sdrk_exec_host(p64, in.data(), 2, 4096, out32.data()));
    REFUSED(sdrk_exec_fft_host(p64, in.data(), 2, 4096, out.data()));
    REFUSED(sdrk_exec_device(p64, in.data(), 2, 4096, out32.data(), nullptr));
    REFUSED(sdrk_welch_psd_host(p64, in.data(), 2, 4096, 1.0f, out32.data()));
    float ms[2];
    REFUSED(sdrk_exec_device_timed_each(p64, in.data(), 2, 4096, out32.data(), 2, ms));
    REFUSED(sdrk_exec_host_f64(p32, in.data(), 2, 4096, out.data()));
    REFUSED(sdrk_exec_fft_host_f64(p32, in.data(), 2, 4096, out.data()));
    REFUSED(sdrk_exec_device_f64(p32, in.data(), 2, 4096, out.data(), nullptr));
    REFUSED(sdrk_exec_device_f64_timed_each(p32, in.data(), 2, 4096, out.data(), 2, ms));
    sdrk_waterfall* wf = nullptr;
    CHECK(sdrk_waterfall_create(0, 4096, 4, &wf) == SDRK_OK);
    REFUSED(sdrk_waterfall_append_iq(wf, p64, in.data(), 2, 4096));
    REFUSED(sdrk_waterfall_append_iq_device(wf, p64, in.data(), 2, 4096));
    CHECK(sdrk_waterfall_destroy(wf) == SDRK_OK);
    // the refused plans still work
    CHECK(sdrk_exec_host_f64(p64, in.data(), 2, 4096, out.data()) == SDRK_OK && out[5] == 3.0 - 1.0 + 5.0);
    CHECK(sdrk_plan_destroy(p64) == SDRK_OK);
    CHECK(sdrk_plan_destroy(p32) == SDRK_OK);
}

int main(int argc, char** argv) {
    return run_stress("f64", argc > 1 ? atoi(argv[1]) : 2, argc > 2 ? atoi(argv[2]) : 1, refusals, worker);
}

// tests/fake_f64_kernels.cpp — stand-in for the double-precision launcher of csrc/kernels_f64.h, for the host-only sanitizer
// build of csrc/sdrk_f64.hip (with the stand-in runtime of tests/fake_hip).  Like fake_kernels.cpp, the "launch" enqueues a
// host function on the stream it was given, and the "transform" is not a spectrum but a function of the input that lets the
// driver check every element: row[f][k] = 3 re(x[f][k]) - im(x[f][k]) + (k & 1023) (dB epilogue) or (re + 1, im - 1) (complex).
// Two-pass lengths also write every element of the scratch frames they are given, so that a scratch sized too small is an
// out-of-bounds write under AddressSanitizer.
#include "../sdr-iq-visualizer_amd/csrc/kernels_f64.h"

#include <algorithm>

namespace sdrk {

bool fft_f64_split(int nfft, int* l_col, int* l_row) {
    int l = 0;
    while ((1 << l) < nfft) ++l;
    if (nfft < 2 || (1 << l) != nfft || l > 22) return false;
    *l_col = l <= 12 ? 0 : l / 2;
    *l_row = l <= 12 ? l : l - l / 2;
    return true;
}

hipError_t launch_fft_f64(const F64Args& a) {
    int lc = 0, lr = 0;
    if (!fft_f64_split(a.nfft, &lc, &lr) || a.n_frames == 0 || !a.d_twiddle) return hipErrorInvalidValue;
    if (lc && (!a.d_scratch || a.scratch_frames == 0)) return hipErrorInvalidValue;
    F64Args c = a;
    fakehip::of(a.stream).push([c, lc] {
        const size_t N = (size_t)c.nfft;
        const double* x = static_cast<const double*>(c.d_iq);
        if (lc) {
            double* s = static_cast<double*>(c.d_scratch);
            std::fill(s, s + 2 * N * std::min(c.n_frames, c.scratch_frames), 0.0);
        }
        for (size_t f = 0; f < c.n_frames; ++f)
            for (size_t k = 0; k < N; ++k) {
                const double re = x[2 * (f * c.frame_stride + k)], im = x[2 * (f * c.frame_stride + k) + 1];
                if (c.epilogue == EPI64_DB) {
                    static_cast<double*>(c.d_out)[f * N + k] = 3.0 * re - im + (double)(k & 1023);
                } else {
                    static_cast<double*>(c.d_out)[2 * (f * N + k)] = re + 1.0;
                    static_cast<double*>(c.d_out)[2 * (f * N + k) + 1] = im - 1.0;
                }
            }
    });
    return hipSuccess;
}

}  // namespace sdrk

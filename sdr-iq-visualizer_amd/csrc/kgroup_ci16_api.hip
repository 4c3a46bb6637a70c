// kgroup_ci16_api.hip — the int16 integrated-spectrum entry points of include/sdrk.h (sdrk_exec_*_integrated_ci16): one row per
// group of K consecutive frames — mean, maximum or minimum of |fft(w x_f)|^2 per bin — from interleaved little-endian int16
// I,Q, 4 bytes per sample.  x[n] = float32(I[n]) + i float32(Q[n]) exactly, then the bits sdrk_exec_*_integrated returns for
// those widened samples: every length of a float32 plan, every detector, form, K, group count and stride, device entry and
// host entry alike.
//
// The call is integrate_call.h's, with 4-byte samples and the int16 launchers: N = 4096 runs fft4096_kgroup_ci16.hip on the
// caller's samples (4 + 4/K bytes per sample through HBM); every other length runs the plan's own int16 transform (launch_ci16,
// ci16_api.hip: the int16-reading fft_lds forms at 256 ... 16384, widen-then-transform in chunks of at most 64 MiB elsewhere)
// with EPI_COMPLEX into the plan's spectrum staging, then integrate_rows.hip — the same carry rows, partial rows and finalize.
// Host code only (not named sdrk_*.hip: tests/host_sources.py globs those for the stand-in kernel builds).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include "integrate_call.h"
#include "kernels_kgroup_ci16.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

IntIo ci16_int_io() {
    IntIo io;
    io.in_elem = 4;
    io.fused = sdrk::launch_fft4096_kgroup_ci16;
    io.transform = launch_ci16;
    return io;
}

}  // namespace

extern "C" {

int sdrk_exec_device_integrated_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                     int detector, int out_form, float scale, float* d_out, void* stream) {
    return exec_device_integrated(ci16_int_io(), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale,
                                  d_out, stream);
}

int sdrk_exec_device_integrated_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                int launches, float* each_ms) {
    return exec_device_integrated_timed_each(ci16_int_io(), p, d_iq_ci16, n_groups, k_frames, frame_stride, detector, out_form,
                                             scale, d_out, launches, each_ms);
}

int sdrk_exec_host_integrated_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                   int detector, int out_form, float scale, float* out) {
    return exec_host_integrated(ci16_int_io(), p, iq_ci16, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

}  // extern "C"

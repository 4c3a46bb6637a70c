// integrate_api.hip — the complex64 integrated-spectrum entry points of include/sdrk.h (sdrk_exec_*_integrated): per group of
// K consecutive frames ONE row — the mean, maximum or minimum over the frames of |fft(w x_f)|^2 per bin — as dB or as scaled
// linear power.  Video averaging / Welch, peak hold and noise-floor hold inside the transform.
//
// The call itself — the N = 4096 kernel on the caller's samples, every other length through the plan's own transform and at
// most 64 MiB of staging, carry rows across chunks, slices and their finalize, the numpy boundary through the three staging
// slots — is integrate_call.h, shared with the int16 form (kgroup_ci16_api.hip).  This file gives it the complex64 launchers:
// fft4096_integrate.hip and plan_launch.
// Host code only (not named sdrk_*.hip: tests/host_sources.py globs those for the stand-in kernel builds).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include "integrate_call.h"
#include "kernels_integrate.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

int transform_c64(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return plan_launch(p, d_in, n_frames, stride, d_out, epilogue, stream);
}

IntIo c64_io() {
    IntIo io;
    io.in_elem = sizeof(float2);
    io.fused = sdrk::launch_fft4096_integrate;
    io.transform = transform_c64;
    return io;
}

}  // namespace

extern "C" {

int sdrk_exec_device_integrated(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                int detector, int out_form, float scale, float* d_out, void* stream) {
    return exec_device_integrated(c64_io(), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                  stream);
}

int sdrk_exec_device_integrated_timed_each(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                           size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                           int launches, float* each_ms) {
    return exec_device_integrated_timed_each(c64_io(), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale,
                                             d_out, launches, each_ms);
}

int sdrk_exec_host_integrated(sdrk_plan* p, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                              int detector, int out_form, float scale, float* out) {
    return exec_host_integrated(c64_io(), p, iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

}  // extern "C"

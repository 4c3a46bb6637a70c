// pfb_groups_api.hip — the integrated polyphase-filter-bank entry points of include/sdrk.h (sdrk_exec_*_pfb_integrated): the
// spectrometer form of the filter bank — fold T blocks under the plan's prototype, transform, |.|^2, and ONE row per K
// consecutive folded frames (mean, maximum or minimum per bin), as dB or as scaled linear power.  The row is, bit for bit,
// what sdrk_exec_device_integrated returns for the packed folded frames (kernels_pfb.h has the fold's arithmetic).
//
// The call itself is integrate_call.h — units, slices and their finalize, carry rows across chunks, the numpy boundary through
// the three staging slots — with an input span of T * nfft samples per frame, so that a chunk carries its (T - 1) * nfft
// samples of overlap.  This file gives it the launchers: pfb4096_groups.hip at N = 4096 (fold, transform and reduction in one
// kernel on the caller's samples), and for every other length pfb_api.hip's launch_pfb with EPI_COMPLEX — the fold into the PFB
// staging, then the plan's transform into the integrate staging, each at most 64 MiB — in front of integrate_rows.hip.  Both
// stagings keep their own stream and event ordering (ev_pfb / ev_int).
// Host code only (not named sdrk_*.hip, and not part of pfb_api.hip: tests/test_host_sanitizers_pfb.py links that file without
// stand-ins for the integrate kernels).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include "integrate_call.h"
#include "kernels_integrate.h"
#include "kernels_pfb.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

IntIo pfb_groups_io(const sdrk_plan* p) {
    IntIo io;
    io.in_elem = sizeof(float2);
    io.fused = sdrk::launch_pfb4096_groups;
    io.transform = launch_pfb;
    io.in_span = (size_t)p->pfb_taps * (size_t)p->nfft;
    return io;
}

}  // namespace

extern "C" {

int sdrk_exec_device_pfb_integrated(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                    int detector, int out_form, float scale, float* d_out, void* stream) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated(pfb_groups_io(p), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                                  stream);
}

int sdrk_exec_device_pfb_integrated_timed_each(sdrk_plan* p, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                               size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                               int launches, float* each_ms) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_device_integrated_timed_each(pfb_groups_io(p), p, d_iq_c64, n_groups, k_frames, frame_stride, detector, out_form,
                                             scale, d_out, launches, each_ms);
}

int sdrk_exec_host_pfb_integrated(sdrk_plan* p, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                  int detector, int out_form, float scale, float* out) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    return exec_host_integrated(pfb_groups_io(p), p, iq_c64, n_groups, k_frames, frame_stride, detector, out_form, scale, out);
}

}  // extern "C"

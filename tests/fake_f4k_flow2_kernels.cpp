// tests/fake_f4k_flow2_kernels.cpp — stand-in for the launcher of fft4096_flow2_kernel (csrc/fft4096.hip, kernels.h: look-ahead
// two with the row stores left in flight, what a plan takes unasked), for the host-only sanitizer build of csrc/sdrk_plan.hip:
// the "rot H" stand-in of fake_f4k_rot_kernels.cpp — the real launcher's argument checks, the heads found at zero, moved and
// left at zero — which neither the look-ahead nor the loop's waits change.
#include "../sdr-iq-visualizer_amd/csrc/kernels.h"

namespace sdrk {

hipError_t launch_fft4096_flow2(const LaunchArgs& a, unsigned* d_heads, unsigned n_heads, unsigned grid) {
    return launch_fft4096_rot(a, d_heads, n_heads, grid);
}

}  // namespace sdrk

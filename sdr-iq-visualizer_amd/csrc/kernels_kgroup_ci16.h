// kernels_kgroup_ci16.h — interface between integrate_api.hip and fft4096_kgroup_ci16.hip: the N = 4096 transform reading
// int16 I,Q with the reduction over K frames in its registers.  IntegrateArgs is kernels_integrate.h's, with d_in pointing at
// int16 pairs (4 bytes per sample) and in_stride counting samples; carry rows, partial rows and the finalize are those of the
// complex64 kernels.
#pragma once
#include "kernels_integrate.h"

namespace sdrk {

hipError_t launch_fft4096_kgroup_ci16(const IntegrateArgs& a);

}  // namespace sdrk

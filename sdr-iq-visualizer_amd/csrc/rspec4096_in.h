// rspec4096_in.h — what the two N = 4096 real-input kernels share (rspec4096.hip: a row per frame; rspec4096_groups.hip: a row
// per K frames): the input policy of a pair format with its widening, and the compile-time half of the split's twiddle.
#pragma once
#include "fft4096_in_ci16.h"
#include "fft4096_in_ci8.h"
#include "kernels_real.h"

namespace sdrk {

namespace {

// The input policy of a pair format (RFMT: 0 float32, 1 int16, 2 bytes) and its widening with the 8-bit conversion's arguments.
template <int RFMT> struct RspecIn;
template <> struct RspecIn<0> {
    typedef F4kInC64 In;
    static __device__ __forceinline__ cf widen(In::word w, Iq8Conv) { return In::widen(w); }
};
template <> struct RspecIn<1> {
    typedef F4kInCi16<false> In;
    static __device__ __forceinline__ cf widen(In::word w, Iq8Conv) { return In::widen(w); }
};
template <> struct RspecIn<2> {
    typedef F4kInCi8 In;
    static __device__ __forceinline__ cf widen(In::word w, Iq8Conv c) { return In::widen(w, c); }
};

// exp(-i pi k2 / 16) = (RS_C[k2], -RS_S[k2])
__device__ constexpr float RS_C[16] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
                                        0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f,
                                        0.19509032201612826785f, 0.0f, -0.19509032201612826785f, -0.38268343236508977173f,
                                        -0.55557023301960222474f, -0.70710678118654752440f, -0.83146961230254523708f,
                                        -0.92387953251128675613f, -0.98078528040323044913f};
__device__ constexpr float RS_S[16] = {0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f,
                                        0.70710678118654752440f, 0.83146961230254523708f, 0.92387953251128675613f,
                                        0.98078528040323044913f, 1.0f, 0.98078528040323044913f, 0.92387953251128675613f,
                                        0.83146961230254523708f, 0.70710678118654752440f, 0.55557023301960222474f,
                                        0.38268343236508977173f, 0.19509032201612826785f};

}  // namespace

}  // namespace sdrk

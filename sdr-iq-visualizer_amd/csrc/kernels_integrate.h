// kernels_integrate.h — interface between integrate_api.hip and the integrated-spectrum kernels (fft4096_integrate.hip: the
// N = 4096 transform with the reduction over frames in its registers; integrate_rows.hip: the reduction over complex spectra
// of any length, and the finalize of split groups).  See integrate_split.h for groups, slices and units.
#pragma once
#include "integrate_split.h"
#include "kernels.h"

namespace sdrk {

enum IntDetector : int { INT_DET_MEAN = 0, INT_DET_MAX = 1, INT_DET_MIN = 2 };
enum IntOutForm : int { INT_OUT_DB = 0, INT_OUT_POWER = 1 };

// One launch covers the frames [f0, f1) of a call.  Unit state is a float2 per bin: MEAN {Kahan sum, compensation},
// MAX / MIN {value, 0}; rows, partials and carries are all indexed by output position (the plan's shift order).
struct IntegrateArgs {
    const void* d_in = nullptr;      // frame f0: complex64 samples (fft4096_integrate) or a complex64 spectrum (integrate_rows)
    size_t in_stride = 0;            // complex64 elements between consecutive frames
    size_t f0 = 0, f1 = 0;
    size_t k = 1;                    // frames per group
    size_t slices = 1, slice_len = 1;
    int detector = INT_DET_MEAN;
    int out_form = INT_OUT_DB;
    float scale = 1.0f;              // INT_OUT_POWER
    float eps = 1e-12f;              // INT_OUT_DB
    float* d_out = nullptr;          // slices == 1: the row of group g at d_out + (g - out_row0) * nfft
    size_t out_row0 = 0;
    float2* d_partials = nullptr;    // slices > 1: [unit][nfft]
    const float2* d_carry_in = nullptr;   // state of the unit that began before f0
    float2* d_carry_out = nullptr;        // state of the unit that goes on behind f1 (never the same row as d_carry_in)
    int nfft = 0;
    const float* d_window = nullptr;
    const void* d_twiddle = nullptr;
    int shift = 1;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    // polyphase filter bank in front (pfb4096_groups.hip): the plan's prototype, pfb_taps * nfft float32; d_in is then the raw
    // stream and a frame covers pfb_taps * nfft samples from its start
    const float* d_pfb_h = nullptr;
    int pfb_taps = 0;
    // real-sampled input (rspec4096_groups.hip): d_in is then the stream of pairs in format real_fmt (a REAL_* value of
    // kernels_real.h), in_stride counts pairs, nfft is the row length 4097, and the rows are not shifted; the mode's own window
    // (2 * 4096 floats or nullptr) and the split's table exp(-i pi k / 4096)
    const float* d_real_window = nullptr;
    const float2* d_real_tab = nullptr;
    int real_fmt = 0;
};

hipError_t launch_fft4096_integrate(const IntegrateArgs& a);
hipError_t launch_integrate_rows(const IntegrateArgs& a);
// slices > 1: out[g][pos] = epilogue(combine of partials[g * slices + s][pos], s ascending), g < n_groups
hipError_t launch_integrate_finalize(const float2* d_partials, size_t n_groups, size_t k, size_t slices, int nfft, int detector,
                                     int out_form, float scale, float eps, float* d_out, int num_cus, hipStream_t stream);

#ifdef __HIPCC__
// What a kernel needs of IntegrateArgs, by value.
struct IntUnits {
    size_t f0, f1, k, slice_len, u_first, u_last, out_row0;
    unsigned slices;
    int out_form;
    float scale, eps, inv_k;
};

// ... of a launch's arguments (f1 > f0); a launcher that fixes the output form overrides out_form and eps behind it
inline IntUnits int_units(const IntegrateArgs& a) {
    IntUnits c;
    const IntSplit sp{a.slices, a.slice_len};
    c.f0 = a.f0;
    c.f1 = a.f1;
    c.k = a.k;
    c.slice_len = a.slice_len;
    c.slices = (unsigned)a.slices;
    c.u_first = integrate_unit_of(a.f0, a.k, sp);
    c.u_last = integrate_unit_of(a.f1 - 1, a.k, sp);
    c.out_row0 = a.out_row0;
    c.out_form = a.out_form;
    c.scale = a.scale;
    c.eps = a.eps;
    c.inv_k = 1.0f / (float)a.k;
    return c;
}

struct IntUnit {
    size_t g, fb, fe;     // group; frames [fb, fe) of the unit that this launch covers
    bool starts, ends;    // the unit begins / is complete within this launch
};

// (slices > 1 only when the groups are fewer than the resident grid: unit numbers then fit 32 bits)
__device__ __forceinline__ IntUnit int_unit(const IntUnits& c, size_t u) {
    IntUnit r;
    unsigned s = 0;
    if (c.slices == 1) {
        r.g = u;
    } else {
        const unsigned uu = (unsigned)u, g = uu / c.slices;
        r.g = g;
        s = uu - g * c.slices;
    }
    const size_t off = (size_t)s * c.slice_len, rem = c.k - off;
    const size_t ub = r.g * c.k + off, ue = ub + (rem < c.slice_len ? rem : c.slice_len);
    r.fb = ub > c.f0 ? ub : c.f0;
    r.fe = ue < c.f1 ? ue : c.f1;
    r.starts = r.fb == ub;
    r.ends = r.fe == ue;
    return r;
}

template <int DET>
__device__ __forceinline__ void int_init(float& acc, float& cmp) {
    acc = DET == INT_DET_MEAN ? 0.0f : (DET == INT_DET_MAX ? -__builtin_huge_valf() : __builtin_huge_valf());
    cmp = 0.0f;
}

// One more frame's power.  MEAN: Kahan — the accumulation's error stays at the rounding of one term however many frames
// a group has (plain float32 summation of 4096 equal terms is off by more than the parity bound allows).
template <int DET>
__device__ __forceinline__ void int_accumulate(float& acc, float& cmp, float p) {
    if (DET == INT_DET_MEAN) {
        const float y = p - cmp, t = acc + y;
        cmp = (t - acc) - y;
        acc = t;
    } else if (DET == INT_DET_MAX) {
        acc = fmaxf(acc, p);
    } else {
        acc = fminf(acc, p);
    }
}

// 20*log10(sqrt(R) + eps) — logpsd_db (kernels.h) from the power on — or scale * R.
__device__ __forceinline__ float int_epilogue(float r, int out_form, float scale, float eps) {
    if (out_form == INT_OUT_POWER) return scale * r;
    const float mag = __builtin_amdgcn_sqrtf(r);
    return __builtin_amdgcn_logf(mag + eps) * 6.02059991327962390427f;
}

template <int DET>
__device__ __forceinline__ float int_reduced(float acc, float cmp, float inv_k) {
    return DET == INT_DET_MEAN ? (acc - cmp) * inv_k : acc;
}
#endif  // __HIPCC__

}  // namespace sdrk

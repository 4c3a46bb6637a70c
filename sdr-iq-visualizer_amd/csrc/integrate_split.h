// integrate_split.h — how the integrated-spectrum entry points (integrate_api.hip) cut a call into work units.  Plain C++ with
// no HIP in it: the kernels, the host file and tests/test_integrate_host.py (through g++) all compile this one definition.
//
// A call is n_groups groups of k consecutive frames.  A group is cut into `slices` runs of `len` frames (the last one may be
// shorter, none is empty); unit u = group * slices + slice covers the call's frames
//     [group * k + slice * len,  group * k + min(k, (slice + 1) * len)).
// With slices == 1 a unit is a group and its reduced row is final; otherwise every unit leaves a partial row and a finalize
// kernel combines a group's partials in slice order.  The cut depends on (n_groups, k, num_cus) only, never on how a call
// is chunked: a chunk boundary inside a unit is bridged by carrying the unit's accumulator state, so the device entry and the
// chunked host entry add the same numbers in the same order.
#pragma once
#include <stddef.h>

namespace sdrk {

constexpr size_t INT_WG_PER_CU = 3;      // the resident grid the cut fills: F4K_WAVES workgroups per CU
constexpr size_t INT_MIN_SLICE = 4;      // frames: a shorter slice costs more in partial rows than it gains in parallelism

struct IntSplit {
    size_t slices;   // per group
    size_t len;      // frames per slice
};

inline IntSplit integrate_split(size_t n_groups, size_t k, int num_cus) {
    const size_t grid = (size_t)(num_cus > 0 ? num_cus : 1) * INT_WG_PER_CU;
    IntSplit r{1, k ? k : 1};
    if (n_groups == 0 || n_groups >= grid || k < 2 * INT_MIN_SLICE) return r;
    const size_t want = (grid + n_groups - 1) / n_groups;   // slices that would fill the grid
    size_t len = (k + want - 1) / want;
    if (len < INT_MIN_SLICE) len = INT_MIN_SLICE;
    r.len = len;
    r.slices = (k + len - 1) / len;
    return r;
}

// The unit that holds frame f of the call.
inline size_t integrate_unit_of(size_t f, size_t k, IntSplit sp) {
    const size_t g = f / k;
    return g * sp.slices + (f - g * k) / sp.len;
}

}  // namespace sdrk

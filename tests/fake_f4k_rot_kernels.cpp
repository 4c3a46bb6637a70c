// tests/fake_f4k_rot_kernels.cpp — stand-in for the "rot H" launcher of csrc/fft4096.hip (kernels.h), for the host-only
// sanitizer build of csrc/sdrk_plan.hip (with the stand-in runtime of tests/fake_hip).  The rows are fake_kernels.cpp's
// checkable "transform" (through its launch_fft4096); what this file adds is the kernel's side of the contract of
// csrc/f4k_rot.h: the "kernel" finds every head and the exit counter at zero — else an earlier launch has not cleaned up, or
// the host handed it something else, and it aborts — moves them as a launch does and leaves them zero.  It touches them on
// the stream's thread and without atomics, so two such launches of a plan that the host let overlap are a data race
// ThreadSanitizer reports.
#include "../sdr-iq-visualizer_amd/csrc/kernels.h"

#include <cstdio>
#include <cstdlib>

namespace sdrk {

hipError_t launch_fft4096_rot(const LaunchArgs& a, unsigned* d_heads, unsigned n_heads, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_rot_heads_ok(n_heads) ||
        a.n_frames > sdrk_host::F4K_TICKET_MAX_FRAMES)
        return hipErrorInvalidValue;
    const size_t n = a.n_frames;
    fakehip::of(a.stream).push([=] {
        unsigned& exits = d_heads[sdrk_host::F4K_ROT_EXIT_WORD];
        if (exits != 0) {
            fprintf(stderr, "fake rot launch: the exit counter stands at %u, not 0\n", exits);
            abort();
        }
        for (unsigned x = 0; x < n_heads; ++x) {
            unsigned& head = d_heads[x * sdrk_host::F4K_TICKET_HEAD_WORDS];
            if (head != 0) {
                fprintf(stderr, "fake rot launch: head %u stands at %u, not 0\n", x, head);
                abort();
            }
            head = (unsigned)((n + n_heads - 1 - x) / n_heads) + grid;   // its tickets below the end, one past it per workgroup
        }
        exits = grid;
        for (unsigned x = 0; x < n_heads; ++x) d_heads[x * sdrk_host::F4K_TICKET_HEAD_WORDS] = 0;
        exits = 0;
    });
    return launch_fft4096(a);
}

// The dealt probes (csrc/aux_kernels.hip): the heads of the probe call as a launch in its chosen order finds and leaves them
// — zero for the rot forms, the host's bases for the others — then the plain stand-in.
static void fake_dealt(sdrk_host::F4kProbeDeal& pd, size_t max_blocks, size_t n_units, hipStream_t s) {
    using namespace sdrk_host;
    if (!pd.d_heads || !f4k_ticket_takes(pd.choice.order, max_blocks, n_units, F4K_TICKET_DEFAULT)) return;
    const unsigned grid = f4k_ticket_grid(max_blocks, n_units);
    unsigned* const d_heads = pd.d_heads;
    const F4kTicketForm form = pd.choice.form;
    const unsigned n_heads = pd.choice.rot_heads ? pd.choice.rot_heads : form.heads;
    const bool rot = pd.choice.rot_heads != 0;
    const F4kTicketBases b = pd.bases;
    fakehip::of(s).push([=] {
        for (unsigned x = 0; x < n_heads; ++x) {
            unsigned& head = d_heads[x * F4K_TICKET_HEAD_WORDS];
            const unsigned want = rot ? 0u : b.base[x];
            if (head != want) {
                fprintf(stderr, "fake dealt probe: head %u stands at %u, not %u\n", x, head, want);
                abort();
            }
            if (!rot) head = f4k_ticket_advance(form, b.base[x], n_units, grid, x);
        }
        if (rot && d_heads[F4K_ROT_EXIT_WORD] != 0) {
            fprintf(stderr, "fake dealt probe: the exit counter stands at %u, not 0\n", d_heads[F4K_ROT_EXIT_WORD]);
            abort();
        }
    });
    if (!rot) f4k_ticket_advance(form, pd.bases, n_units, grid);
}

hipError_t launch_stream_mix_dealt(const void* d_in, void* d_out, size_t n_frames4096, int num_cus, hipStream_t stream,
                                   sdrk_host::F4kProbeDeal& pd) {
    if (n_frames4096 == 0) return hipSuccess;
    fake_dealt(pd, (size_t)num_cus * 3, n_frames4096, stream);
    return launch_stream_mix(d_in, d_out, n_frames4096, num_cus, stream);
}

hipError_t launch_copy_1to1_dealt(const void* d_in, void* d_out, size_t bytes, int num_cus, int blocks_per_cu, hipStream_t stream,
                                  sdrk_host::F4kProbeDeal& pd) {
    if (bytes / 16 == 0) return hipSuccess;
    fake_dealt(pd, (size_t)num_cus * blocks_per_cu, (bytes / 16 + 1023) / 1024, stream);
    return launch_copy_1to1(d_in, d_out, bytes, num_cus, blocks_per_cu, stream);
}

}  // namespace sdrk

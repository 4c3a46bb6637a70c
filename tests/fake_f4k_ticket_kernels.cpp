// tests/fake_f4k_ticket_kernels.cpp — stand-in for the ticketed launcher of csrc/fft4096.hip (kernels.h), for the host-only
// sanitizer build of csrc/sdrk_plan.hip (with the stand-in runtime of tests/fake_hip).  The rows are fake_kernels.cpp's
// checkable "transform" (through its launch_fft4096); what this file adds is the kernel's side of the head contract of
// csrc/f4k_ticket.h: the "kernel" finds every head where the host said it stands — else the host's bases and the device
// disagree, and it aborts — and leaves it where f4k_ticket_advance predicts.  It touches the heads on the stream's thread and
// without atomics, so two ticketed launches of a plan that the host let overlap are a data race ThreadSanitizer reports.
#include "../sdr-iq-visualizer_amd/csrc/kernels.h"

#include <cstdio>
#include <cstdlib>

namespace sdrk {

unsigned f4k_max_blocks(int num_cus) { return (unsigned)num_cus * 3u; }

hipError_t launch_fft4096_ticket(const LaunchArgs& a, unsigned* d_heads, const sdrk_host::F4kTicketBases& bases,
                                 sdrk_host::F4kTicketForm form, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_ticket_form_ok(form)) return hipErrorInvalidValue;
    const sdrk_host::F4kTicketBases b = bases;
    const size_t n = a.n_frames;
    fakehip::of(a.stream).push([=] {
        for (unsigned x = 0; x < form.heads; ++x) {
            unsigned& head = d_heads[x * sdrk_host::F4K_TICKET_HEAD_WORDS];
            if (head != b.base[x]) {
                fprintf(stderr, "fake ticketed launch: head %u stands at %u, the host said %u\n", x, head, b.base[x]);
                abort();
            }
            head = sdrk_host::f4k_ticket_advance(form, b.base[x], n, grid, x);
        }
    });
    return launch_fft4096(a);
}

}  // namespace sdrk

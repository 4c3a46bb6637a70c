// f4k_ticket.h — the ticket order of fft4096_ticket_kernel (fft4096.hip): which frames a ticket is, what a launch leaves in
// the heads, when plan_launch (sdrk_plan.hip) takes this order and into how many launches it cuts a call.  Pure arithmetic,
// no HIP; the kernel and the host share it.
//
// A workgroup of the ticketed kernel does not walk the frames grid-stride: it takes its next frames from a counter in device
// memory when it is ready for them, so that the frames in flight stay close to each other however long the launch is.  A
// form (F4kTicketForm) has `heads` counters, each on a 128-byte line of its own, and `frames` consecutive frames per ticket:
// workgroup b draws from head b % heads, and ticket t of head x is the frames (t * heads + x) * frames ... + frames - 1.
//
// A workgroup draws f4k_ticket_depth tickets with its first atomic and one more in every iteration whose prefetch reaches
// the last frame of a ticket (every iteration when a ticket is one frame), always that many tickets ahead of the frame it
// transforms, and it leaves the loop at the first frame of its own at or past the end.  Tickets of a head only grow, so every
// ticket with a frame below the end has been drawn by then, by a workgroup that transforms its frames.  The iterations that
// draw are those that transform frame f with f % frames == frames - 2 (every f for one frame per ticket), whoever owns f: a
// launch advances head x by
//     (such frames below the end whose ticket is of head x) + depth * (workgroups drawing from x),
// which the host knows beforehand.  The heads are never reset: each launch is told where they stand (its "base"), and the
// host advances its copy.  Heads are 32-bit and wrap; every difference is taken modulo 2^32, and one launch draws fewer than
// 2^32 tickets (F4K_TICKET_MAX_FRAMES).  Launches that share heads must not overlap on the device.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdrk_host {

constexpr unsigned F4K_TICKET_MAX_HEADS = 8;
constexpr unsigned F4K_TICKET_HEAD_WORDS = 32;     // 32-bit words between two heads: one 128-byte line each
constexpr size_t F4K_TICKET_MAX_FRAMES = (size_t)1 << 31;   // a longer launch keeps the grid-stride loop

struct F4kTicketForm {
    unsigned heads;    // 1, 2, 4 or 8
    unsigned frames;   // per ticket: 1, 2, 4 or 8
};
constexpr bool f4k_ticket_form_ok(F4kTicketForm f) {
    return f.heads >= 1 && f.heads <= F4K_TICKET_MAX_HEADS && !(f.heads & (f.heads - 1)) && f.frames >= 1 && f.frames <= 8 &&
           !(f.frames & (f.frames - 1));
}
// The product's form (profiles/f4k_ticket/SUMMARY.md); SDRK_F4K_TICKET_FORM=<heads>x<frames> names another for A/B work.
constexpr F4kTicketForm F4K_TICKET_FORM = {1, 2};

enum F4kOrder { F4K_ORDER_AUTO = 0, F4K_ORDER_STRIDE = 1, F4K_ORDER_TICKET = 2 };

struct F4kTicketBases {
    uint32_t base[F4K_TICKET_MAX_HEADS];
};

// tickets a workgroup holds beyond the one whose frames it transforms
constexpr unsigned f4k_ticket_depth(F4kTicketForm f) { return f.frames == 1 ? 4 : 3; }
constexpr size_t f4k_ticket_first_frame(F4kTicketForm f, uint32_t ticket, unsigned head) {
    return ((size_t)ticket * f.heads + head) * f.frames;
}
// iterations of a launch that draw, all workgroups together, and those of them that draw from head x
constexpr size_t f4k_ticket_draws(F4kTicketForm f, size_t n_frames) { return f.frames == 1 ? n_frames : (n_frames + 1) / f.frames; }
constexpr size_t f4k_ticket_class(F4kTicketForm f, size_t n_frames, unsigned head) {
    return (f4k_ticket_draws(f, n_frames) + f.heads - 1 - head) / f.heads;
}
constexpr unsigned f4k_ticket_pullers(F4kTicketForm f, unsigned grid, unsigned head) { return (grid + f.heads - 1 - head) / f.heads; }

// The grid of a ticketed launch: a multiple of 8 (every head has its workgroups, and the same number of them), no larger than
// max_blocks and no larger than the frames rounded up to 8.  0: no ticketed launch at this size (fewer than 8 resident
// workgroups, no frames, too many frames).
constexpr unsigned f4k_ticket_grid(size_t max_blocks, size_t n_frames) {
    if (max_blocks < F4K_TICKET_MAX_HEADS || n_frames == 0 || n_frames > F4K_TICKET_MAX_FRAMES) return 0;
    const size_t full = max_blocks - max_blocks % F4K_TICKET_MAX_HEADS;
    const size_t need = (n_frames + F4K_TICKET_MAX_HEADS - 1) / F4K_TICKET_MAX_HEADS * F4K_TICKET_MAX_HEADS;
    return (unsigned)(need < full ? need : full);
}

// Where head x stands after a launch of n_frames frames on `grid` workgroups that found it at `base`.
constexpr uint32_t f4k_ticket_advance(F4kTicketForm f, uint32_t base, size_t n_frames, unsigned grid, unsigned head) {
    return base + (uint32_t)f4k_ticket_class(f, n_frames, head) + f4k_ticket_depth(f) * f4k_ticket_pullers(f, grid, head);
}
inline void f4k_ticket_advance(F4kTicketForm f, F4kTicketBases& b, size_t n_frames, unsigned grid) {
    for (unsigned x = 0; x < f.heads; ++x) b.base[x] = f4k_ticket_advance(f, b.base[x], n_frames, grid, x);
}

// Does a launch of n_frames frames take the ticketed loop?  Forced either way by the plan's order (SDRK_F4K_ORDER) wherever
// a ticketed grid exists; left alone, only a full grid that is a multiple of 8 does: a shorter call has nothing to drift.
constexpr bool f4k_ticket_takes(int order, size_t max_blocks, size_t n_frames, bool by_default) {
    if (order == F4K_ORDER_STRIDE || f4k_ticket_grid(max_blocks, n_frames) == 0) return false;
    if (order == F4K_ORDER_TICKET) return true;
    return by_default && n_frames >= max_blocks && max_blocks % F4K_TICKET_MAX_HEADS == 0;
}

// Whether the ticket order is what a plan takes when SDRK_F4K_ORDER does not say (profiles/f4k_ticket/SUMMARY.md).
constexpr bool F4K_TICKET_DEFAULT = true;

// Into how many launches a ticketed call is cut (the grid-stride form: f4k_split_parts): one.  The window of frames in flight
// does not grow with the launch, and every boundary costs its drain and ramp: 2^20 frames as 1 / 2 / 4 / 8 / 16 launches of the
// product's form take 8.30 / 8.32 / 8.39 / 8.48 / 8.66 ms (profiles/f4k_ticket/SUMMARY.md).
constexpr size_t f4k_ticket_parts(size_t) { return 1; }

}  // namespace sdrk_host

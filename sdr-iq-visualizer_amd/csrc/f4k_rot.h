// f4k_rot.h — the "rot H" ticket order of fft4096_rot2_kernel and fft4096_rot_kernel (fft4096.hip): one frame per ticket,
// H = 2, 4 or 8 heads, and every workgroup draws from the heads in turn.  Pure arithmetic, no HIP; the kernels, the host and
// tests/f4k_rot_test.cpp, tests/f4k_rot2_test.cpp share it.
//
// Ticket t of head x is frame t * H + x, and the heads start every launch at zero.  Workgroup b's k-th draw goes to head
// (b + k) mod H: every workgroup feeds every head, so the heads advance in step whatever the pace of a CU or an XCD (two heads
// never differ by more than the grid), and a word sees 1/H of the draws — the one word of the 1x1 form saturates at 81 draws
// per microsecond where one frame per ticket needs 126 (profiles/f4k_ticket/SUMMARY.md).
//
// Look-ahead three (F4kRotDeal, fft4096_rot_kernel; the product's form until look-ahead two, now the selectable control):
// a workgroup holds F4K_ROT_AHEAD tickets beyond the frame it transforms: a ticket is drawn at the top of iteration i, ahead
// of that iteration's prefetch loads; it is in the drawing lane's register at the top of i + 1 (the wait for those loads has
// covered it), goes into an LDS slot there as a frame number, is read by every wave behind the barriers of i + 1, names the
// prefetch of i + 2 and is transformed in i + 3.  The first three tickets are drawn in the prologue.
//
// Look-ahead two (F4kRotDeal2; fft4096_rot2_kernel, profiles/f4k_ahead/SUMMARY.md, and fft4096_flow2_kernel, the product's form,
// F4K_ROT_DEFAULT_AHEAD below, which sends the draw out AHEAD of the row stores and does not wait for them at the loop top):
// the prologue draws two tickets, and the ticket that is in the register at the top of iteration i goes into the slot there, is
// read by every wave behind a barrier the frame body has anyway (the transform's entry barrier, which stands at the top of the
// iteration in that kernel) and names the prefetch of that same iteration i; it is transformed in i + 1.  The next draw goes out
// behind the iteration's row stores: the wait for the prefetched loads at the top of i + 1 covers it, so a ticket is drawn one
// atomic round trip, not one iteration, before it names a prefetch.  A workgroup thus holds two tickets beyond the frame it
// transforms: the frame it prefetches and one draw in flight.
//
// The end of a launch: a held frame at or past the end is skipped.  Once head x has shown a workgroup such a ticket the
// workgroup's rotation leaves x out (f4k_rot_next_head); with no head left it draws nothing, and F4K_ROT_NONE follows the last
// ticket through the slots.  The workgroup leaves when F4K_ROT_NONE is the frame to transform: everything it drew has then
// come back and has been transformed or skipped, so every frame below the end is drawn exactly once, by a workgroup that
// transforms it.  Leaving, the drawing lane adds one to the exit counter (a line of its own behind the heads); the workgroup
// that finds grid - 1 there is the last to have drawn and stores zero to the heads and the counter.  The host keeps no bases.
// Launches that share heads must not overlap on the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "f4k_ticket.h"

namespace sdrk_host {

constexpr unsigned F4K_ROT_AHEAD = 3;
constexpr unsigned F4K_ROT_EXIT_WORD = F4K_TICKET_MAX_HEADS * F4K_TICKET_HEAD_WORDS;      // the exit counter's line
constexpr unsigned F4K_ROT_WORDS = (F4K_TICKET_MAX_HEADS + 1) * F4K_TICKET_HEAD_WORDS;   // 32-bit words of a set of heads
constexpr uint32_t F4K_ROT_NONE = 0xFFFFFFFFu;                                           // "no ticket": behind a workgroup's last

constexpr bool f4k_rot_heads_ok(unsigned heads) { return heads == 2 || heads == 4 || heads == 8; }

// The frame of a ticket, as the 32-bit number the slots carry.  A workgroup draws at most twice from a head that is past the
// end (the prologue's first and third draw at H = 2), so no ticket exceeds frames / H + 1 + 2 * grid, and with at most
// F4K_TICKET_MAX_FRAMES = 2^31 frames and a grid below 2^16 the product stays below F4K_ROT_NONE.
// Look-ahead two: the prologue's two draws go to two different heads (H >= 2), and in the loop a draw goes out only after the
// one before it has been taken, so a workgroup never has two draws out at one head and draws at most ONCE from a head that is
// past the end: no ticket exceeds frames / H + 1 + grid, and the bound above covers it.
constexpr uint32_t f4k_rot_frame(unsigned heads, uint32_t ticket, unsigned head) { return ticket * heads + head; }

// The head of a workgroup's next draw: the first after `last` in the rotation among those still in (`live`, one bit a head,
// not zero).
constexpr unsigned f4k_rot_next_head(unsigned heads, unsigned live, unsigned last) {
    const unsigned twice = live | (live << heads);   // bit last + 1 + j: the head j places behind `last`
    return (last + 1 + (unsigned)__builtin_ctz(twice >> (last + 1))) & (heads - 1);
}

// The drawing lane's state, and what it does at the top of an iteration with the ticket that has come back: the frame for
// the slot, the heads still in, and whether (and where) it draws again.  The kernel and the CPU model run this same code.
struct F4kRotDrawer {
    unsigned heads;
    unsigned live;      // heads that have not yet shown this workgroup a ticket past the end
    unsigned head;      // of the last draw
    bool pending;       // a draw is out (or has just come back)
};
constexpr F4kRotDrawer f4k_rot_drawer(unsigned heads, unsigned workgroup) {
    return F4kRotDrawer{heads, (1u << heads) - 1u, workgroup & (heads - 1), false};
}
// a ticket of d.head has come back: its frame; at or past the end, the head leaves the rotation
constexpr uint32_t f4k_rot_take(F4kRotDrawer& d, uint32_t ticket, size_t n_frames) {
    const uint32_t fr = f4k_rot_frame(d.heads, ticket, d.head);
    if (fr >= n_frames) d.live &= ~(1u << d.head);
    return fr;
}
// moves to the head of the next draw; false: no head is left and nothing is drawn
constexpr bool f4k_rot_advance(F4kRotDrawer& d) {
    d.pending = d.live != 0;
    if (d.pending) d.head = f4k_rot_next_head(d.heads, d.live, d.head);
    return d.pending;
}

// SDRK_F4K_TICKET_FORM=rot2|rot4|rot8 -> 2, 4, 8; anything else -> 0
inline unsigned f4k_rot_parse(const char* s) {
    if (!s || s[0] != 'r' || s[1] != 'o' || s[2] != 't' || s[3] == 0 || s[4] != 0) return 0;
    const unsigned h = (unsigned)(s[3] - '0');
    return f4k_rot_heads_ok(h) ? h : 0;
}

// The heads a plan's ticketed launches take when SDRK_F4K_TICKET_FORM does not say (0 would be the form F4K_TICKET_FORM of
// f4k_ticket.h).  2^20 frames, launches alternating with a 1x2 plan on the same pair: rot2 / rot4 / rot8 gain 0.36 / 0.39 /
// 0.37 ms on 8.31, where a second 1x2 plan differs by 0.005 at the most (profiles/f4k_window/SUMMARY.md).
constexpr unsigned F4K_ROT_DEFAULT_HEADS = 4;

// The look-ahead of the rot form: three tickets beyond the frame transformed (F4kRotDeal, fft4096_rot_kernel) or two
// (F4kRotDeal2, fft4096_rot2_kernel: "2top", after the place of the transform's entry barrier).  2^20 frames, launches
// alternating with a rot4 plan at look-ahead three on the same pair: two ahead with the draw at the top gains 0.08 ms on 8.03
// (on every pair, 0.05 at the least), the draw behind the row stores another 0.16 (0.15 at the least), where a second plan of the
// control differs by 0.005 and 0.024 (profiles/f4k_ahead/SUMMARY.md).
// "2flow" (fft4096_flow2_kernel) is 2top's dealer and order with the draw ahead of the row stores and a loop that does not wait
// for those stores at its top (fft4096.hip); the enumerator's value is a name, not a count.  Launches alternating with a rot4 plan
// at 2top on the same pair: 2flow gains 0.18 ms on 7.90-8.01 (on every pair of nine, 0.11 at the least), where a second plan of
// the control differs by 0.014 at the most (profiles/f4k_flow/SUMMARY.md).
enum { F4K_AHEAD_3 = 3, F4K_AHEAD_2TOP = 2, F4K_AHEAD_2FLOW = 4 };
constexpr int F4K_ROT_DEFAULT_AHEAD = F4K_AHEAD_2FLOW;
// the dealer of a look-ahead is F4kRotDeal2 (f4k_deal.h), not F4kRotDeal
constexpr bool f4k_ahead_is_two(int ahead) { return ahead == F4K_AHEAD_2TOP || ahead == F4K_AHEAD_2FLOW; }

// What the environment asks of the N = 4096 order (plans at creation, the no-arithmetic probes per call):
// SDRK_F4K_ORDER = "stride" / "ticket" forces either loop wherever a ticketed grid exists (f4k_ticket_takes);
// SDRK_F4K_TICKET_FORM = "<heads>x<frames per ticket>" (f4k_ticket.h) or "rot<heads>" names a form for A/B work.
// SDRK_F4K_ROT_AHEAD = "3" | "2top" | "2flow" names the rot form's look-ahead (above); anything else leaves the default.
struct F4kChoice {
    int order = F4K_ORDER_AUTO;
    F4kTicketForm form = F4K_TICKET_FORM;
    unsigned rot_heads = F4K_ROT_DEFAULT_HEADS;   // 2, 4, 8: the rot form; 0: `form`
    int rot_ahead = F4K_ROT_DEFAULT_AHEAD;        // F4K_AHEAD_*; only the rot form has a choice
};
inline int f4k_rot_ahead_parse(const char* s) {
    if (!s) return -1;
    if (s[0] == '3' && s[1] == 0) return F4K_AHEAD_3;
    if (s[0] == '2' && s[1] == 't' && s[2] == 'o' && s[3] == 'p' && s[4] == 0) return F4K_AHEAD_2TOP;
    if (s[0] == '2' && s[1] == 'f' && s[2] == 'l' && s[3] == 'o' && s[4] == 'w' && s[5] == 0) return F4K_AHEAD_2FLOW;
    return -1;
}
inline F4kChoice f4k_choice(const char* order_env, const char* form_env, const char* ahead_env = nullptr) {
    F4kChoice c;
    if (const int ahead = f4k_rot_ahead_parse(ahead_env); ahead >= 0) c.rot_ahead = ahead;
    if (order_env) c.order = order_env[0] == 't' ? F4K_ORDER_TICKET : (order_env[0] == 's' ? F4K_ORDER_STRIDE : F4K_ORDER_AUTO);
    if (form_env) {
        F4kTicketForm f = {0, 0};
        if (const unsigned rot = f4k_rot_parse(form_env)) c.rot_heads = rot;
        else if (sscanf(form_env, "%ux%u", &f.heads, &f.frames) == 2 && f4k_ticket_form_ok(f)) { c.form = f; c.rot_heads = 0; }
    }
    return c;
}

// A launch's dealer and what it draws from (f4k_deal.h): `heads` = F4K_ROT_WORDS words; the forms of f4k_ticket.h find them at
// `bases`, the rot form at zero.
struct F4kDealArgs {
    unsigned* heads;
    F4kTicketBases bases;
    F4kTicketForm form;
    unsigned rot_heads;
};

// The heads of one probe call (sdrk_probes.hip) and where the host believes them: its launches, one after the other on one
// stream at a time, take their units of work by `choice` wherever f4k_ticket_takes says so.
struct F4kProbeDeal {
    F4kChoice choice;
    unsigned* d_heads = nullptr;
    F4kTicketBases bases = {};
};

}  // namespace sdrk_host

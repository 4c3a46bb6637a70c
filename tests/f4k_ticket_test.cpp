// f4k_ticket_test.cpp — csrc/f4k_ticket.h on the CPU: the workgroups of fft4096_ticket_kernel as state machines that draw
// from the 32-bit heads exactly as the kernel does (f4k_ticket_depth tickets with the first atomic, one more in every iteration
// whose prefetch reaches the end of a ticket, out at the first own frame at or past the end), stepped in seeded interleavings,
// for the product's form and the other forms the kernel takes (heads x frames per ticket).  Every frame must be transformed exactly once,
// nothing at or past the end, every head must end where f4k_ticket_advance says, and a second call on the same heads must
// start from that base — also across the 32-bit wrap.  Built with -fsanitize=address,undefined and run directly
// (tests/test_f4k_ticket.py).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../sdr-iq-visualizer_amd/csrc/f4k_ticket.h"

using namespace sdrk_host;

namespace {

int bad = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++bad <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                        \
    } while (0)

// One workgroup of the kernel.  step() is one of: the first atomic (prologue), or one iteration of the loop (a draw at its
// top, the transform of `cur`); returns false once the workgroup has left.
struct Puller {
    F4kTicketForm form = F4K_TICKET_FORM;
    unsigned hx = 0;
    uint32_t base = 0;
    int state = 0;        // 0: before the prologue; 1: in the loop; 2: gone
    uint32_t drawn = 0;   // lane 0's register: the head's value at the youngest ticket held
    uint32_t slot = 0;    // the LDS slot of this iteration
    size_t cur = 0, nx = 0, tn = 0;

    size_t first_of(uint32_t head_value) const { return f4k_ticket_first_frame(form, head_value - base, hx); }

    bool step(std::vector<uint32_t>& heads, size_t n_frames, std::vector<uint8_t>& done) {
        uint32_t& head = heads[hx * F4K_TICKET_HEAD_WORDS];
        const unsigned depth = f4k_ticket_depth(form);
        const size_t in_ticket = form.frames - 1;
        if (state == 0) {
            const uint32_t h = head;
            head += depth;
            drawn = h + depth - 1;
            cur = first_of(h);
            nx = in_ticket ? cur + 1 : first_of(h + 1);
            tn = first_of(h + depth - 2);
            state = 1;
            return true;
        }
        if (state == 2) return false;
        if (!(cur < n_frames)) {
            state = 2;
            return false;
        }
        const bool last_of_ticket = ((nx + 1) & in_ticket) == 0;
        if (last_of_ticket) {
            slot = drawn;
            drawn = head;
            head += 1;
        }
        CHECK(cur < done.size(), "frame %zu past the end is transformed", cur);
        if (cur < done.size()) {
            CHECK(done[cur] == 0, "frame %zu transformed twice", cur);
            done[cur] = 1;
        }
        size_t after = nx + 1;
        if (last_of_ticket) {
            after = tn;
            tn = first_of(slot);
        }
        cur = nx;
        nx = after;
        return true;
    }
};

enum Schedule { ROUND_ROBIN, RANDOM, ONE_FIRST, LAST_FIRST, BURSTS, SCHEDULES };

// One launch: `grid` pullers on `heads`, told `bases`; returns through `heads`.
void launch(F4kTicketForm form, std::vector<uint32_t>& heads, const F4kTicketBases& bases, size_t n_frames, unsigned grid, int schedule,
            unsigned seed) {
    std::vector<Puller> w(grid);
    for (unsigned b = 0; b < grid; ++b) {
        w[b].form = form;
        w[b].hx = b % form.heads;
        w[b].base = bases.base[w[b].hx];
    }
    std::vector<uint8_t> done(n_frames, 0);
    std::mt19937 rng(seed);
    std::vector<unsigned> alive(grid);
    for (unsigned b = 0; b < grid; ++b) alive[b] = b;
    auto run_out = [&](unsigned b) { while (w[b].step(heads, n_frames, done)) {} };
    if (schedule == ONE_FIRST) run_out(rng() % grid);          // one puller takes everything first
    if (schedule == LAST_FIRST) run_out(grid - 1);
    while (!alive.empty()) {
        size_t i = 0;
        unsigned steps = 1;
        if (schedule == RANDOM || schedule == ONE_FIRST) i = rng() % alive.size();
        if (schedule == BURSTS) { i = rng() % alive.size(); steps = 1 + rng() % 40; }
        if (schedule == ROUND_ROBIN || schedule == LAST_FIRST) {
            // everybody one step, in order
            for (size_t k = 0; k < alive.size();) {
                if (w[alive[k]].step(heads, n_frames, done)) ++k;
                else { alive[k] = alive.back(); alive.pop_back(); }
            }
            continue;
        }
        bool live = true;
        for (unsigned s = 0; s < steps && live; ++s) live = w[alive[i]].step(heads, n_frames, done);
        if (!live) { alive[i] = alive.back(); alive.pop_back(); }
    }
    size_t missing = 0;
    for (size_t f = 0; f < n_frames; ++f) missing += done[f] ? 0 : 1;
    CHECK(missing == 0, "%zu of %zu frames never transformed (grid %u, schedule %d)", missing, n_frames, grid, schedule);
}

void one_case(F4kTicketForm form, size_t n_frames, size_t max_blocks, uint32_t start, int schedule, unsigned seed) {
    const unsigned grid = f4k_ticket_grid(max_blocks, n_frames);
    CHECK(grid >= F4K_TICKET_MAX_HEADS && grid % F4K_TICKET_MAX_HEADS == 0 && grid <= max_blocks, "grid %u for %zu frames, %zu blocks", grid, n_frames, max_blocks);
    CHECK(grid < n_frames + F4K_TICKET_MAX_HEADS, "grid %u larger than %zu frames need", grid, n_frames);
    if (grid == 0) return;
    std::vector<uint32_t> heads(F4K_TICKET_MAX_HEADS * F4K_TICKET_HEAD_WORDS, 0xDEADBEEFu);
    F4kTicketBases bases = {};
    for (unsigned x = 0; x < form.heads; ++x) heads[x * F4K_TICKET_HEAD_WORDS] = bases.base[x] = start + 1000u * x;
    // three calls on the same heads: this size, a short one, this size again
    const size_t calls[3] = {n_frames, 5, n_frames};
    for (int c = 0; c < 3; ++c) {
        const unsigned g = f4k_ticket_grid(max_blocks, calls[c]);
        launch(form, heads, bases, calls[c], g, schedule, seed + 17 * c);
        size_t classes = 0;
        for (unsigned x = 0; x < form.heads; ++x) {
            const uint32_t want = f4k_ticket_advance(form, bases.base[x], calls[c], g, x);
            CHECK(heads[x * F4K_TICKET_HEAD_WORDS] == want, "head %u ends at %u, predicted %u (%zu frames, grid %u, call %d)", x,
                  heads[x * F4K_TICKET_HEAD_WORDS], want, calls[c], g, c);
            classes += f4k_ticket_class(form, calls[c], x);
        }
        CHECK(classes == f4k_ticket_draws(form, calls[c]), "classes sum to %zu of %zu", classes, f4k_ticket_draws(form, calls[c]));
        f4k_ticket_advance(form, bases, calls[c], g);
    }
    for (size_t i = 0; i < heads.size(); ++i)
        if (i % F4K_TICKET_HEAD_WORDS || i / F4K_TICKET_HEAD_WORDS >= form.heads)
            CHECK(heads[i] == 0xDEADBEEFu, "word %zu beside the heads was written", i);
}

}  // namespace

int main() {
    const size_t frames[] = {1, 7, 8, 9, 767, 768, 769, 2309, 98304, ((size_t)1 << 20) + 3};
    const size_t grids[] = {8, 760, 768};
    // bases: zero, far from the wrap, and within one call of it (every call above draws more than 4 tickets from head 0)
    const uint32_t starts[] = {0u, 123456789u, 0xFFFFFFFFu - 3u, 0xFFFFFE00u};
    const F4kTicketForm forms[] = {F4K_TICKET_FORM, {8, 1}, {1, 1}, {1, 2}, {1, 4}, {8, 2}, {2, 8}};
    int cases = 0;
    for (size_t fi = 0; fi < sizeof forms / sizeof forms[0]; ++fi) {
        const F4kTicketForm form = forms[fi];
        CHECK(f4k_ticket_form_ok(form), "form %ux%u", form.heads, form.frames);
        if (fi && form.heads == F4K_TICKET_FORM.heads && form.frames == F4K_TICKET_FORM.frames) continue;
        for (size_t n : frames)
            for (size_t g : grids)
                for (int s = 0; s < SCHEDULES; ++s) {
                    if (n > 100000 && s != ROUND_ROBIN && s != ONE_FIRST && s != BURSTS) continue;   // (the long one: three schedules)
                    if (fi && n > 100000 && s != BURSTS) continue;                                   // (... and one for the other forms)
                    for (unsigned k = 0; k < (n > 100000 ? 1u : 2u); ++k) {
                        one_case(form, n, g, starts[(cases + k) % 4], s, 1000u * (unsigned)cases + k);
                        ++cases;
                    }
                }
        // the wrap inside every size at least once
        for (size_t n : frames)
            if (n <= 100000) { one_case(form, n, 768, 0xFFFFFFFFu - 3u, RANDOM, (unsigned)n); ++cases; }
    }

    // the rules around the launches
    CHECK(f4k_ticket_grid(7, 100) == 0 && f4k_ticket_grid(768, 0) == 0, "no ticketed grid below 8 blocks or for no frames");
    CHECK(f4k_ticket_grid(770, 1 << 20) == 768 && f4k_ticket_grid(768, 9) == 16 && f4k_ticket_grid(768, 1) == 8, "grids");
    CHECK(!f4k_ticket_takes(F4K_ORDER_STRIDE, 768, 1 << 20, true) && f4k_ticket_takes(F4K_ORDER_TICKET, 768, 1, false), "forced orders");
    CHECK(f4k_ticket_takes(F4K_ORDER_AUTO, 768, 768, true) && !f4k_ticket_takes(F4K_ORDER_AUTO, 768, 767, true), "auto: full grids only");
    CHECK(!f4k_ticket_takes(F4K_ORDER_AUTO, 770, 1 << 20, true) && !f4k_ticket_takes(F4K_ORDER_AUTO, 768, 1 << 20, false), "auto: multiples of 8, default");
    CHECK(!f4k_ticket_takes(F4K_ORDER_TICKET, 6, 100, true), "forced ticket needs 8 blocks");
    CHECK(!f4k_ticket_form_ok({3, 1}) && !f4k_ticket_form_ok({16, 1}) && !f4k_ticket_form_ok({8, 0}) && !f4k_ticket_form_ok({1, 16}), "forms");
    for (size_t n : frames) {
        const size_t parts = f4k_ticket_parts(n);
        CHECK(parts >= 1 && parts <= n, "parts %zu for %zu frames", parts, n);
    }
    printf("f4k_ticket cases=%d bad=%d\n", cases, bad);
    return bad ? 1 : 0;
}

// f4k_rot2_test.cpp — csrc/f4k_rot.h at look-ahead two on the CPU: the workgroups of fft4096_rot2_kernel (F4kRotDeal2 of
// csrc/f4k_deal.h) as state machines that draw from the heads exactly as the kernel does — two draws in the prologue, to two
// different heads; at the top of every iteration the ticket that has come back goes into the slot as a frame (through
// F4kRotDrawer), is prefetched in that same iteration and transformed in the next; the next draw goes out behind the iteration's
// stores ("late", what the kernel does: a step of its own here, so that other workgroups get between) or at the top ("early",
// measured and not kept; modelled because nothing in the order may depend on which); out at
// F4K_ROT_NONE, one more on the exit counter, the last one out zeroes everything — stepped in the seeded interleavings of
// f4k_ticket_test.cpp, for H = 2, 4, 8 and both places of the draw.  Every frame must be transformed exactly once, nothing at
// or past the end, a workgroup never holds more than two tickets beyond the frame it transforms nor has two draws out at one
// head, the heads are never more than the grid apart, heads and exit counter are zero after every call — three calls in a row
// on the same heads — and no word beside them is written.  Built with -fsanitize=address,undefined and run directly
// (tests/test_f4k_rot2.py).
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../sdr-iq-visualizer_amd/csrc/f4k_rot.h"

using namespace sdrk_host;

namespace {

int bad = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++bad <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                        \
    } while (0)

constexpr uint32_t GUARD_WORD = 0xDEADBEEFu;

uint32_t largest_frame = 0;   // the largest frame number a slot ever carried, over all cases

// One workgroup of the kernel.  step() is one of: one of the prologue's two draws, the prologue's end (the first ticket into
// the slot), the top and body of one iteration (with the early draw), the late draw, the exit; false once the workgroup has left.
struct Puller {
    F4kRotDrawer dr = {};
    unsigned grid = 0;
    bool late = false;
    int state = 0;              // 0, 1: the prologue's draws; 2: its end; 3: in the loop; 4: the late draw; 5: gone
    uint32_t d0 = 0;            // the prologue's first ticket
    unsigned h0 = 0;            // ... and its head
    uint32_t drawn = 0;         // lane 0's register: the ticket of the last draw
    uint32_t cur = 0, nx = F4K_ROT_NONE;
    unsigned held = 0;          // tickets drawn and not yet through the loop as `cur`
    unsigned out_at = 0;        // one bit a head: a draw of this workgroup is out there and not yet taken

    uint32_t draw(std::vector<uint32_t>& heads, unsigned head) {
        CHECK(!(out_at & (1u << head)), "two draws out at head %u", head);
        out_at |= 1u << head;
        ++held;
        return heads[head * F4K_TICKET_HEAD_WORDS]++;
    }
    uint32_t take(uint32_t ticket, size_t n_frames) {
        out_at &= ~(1u << dr.head);
        const uint32_t fr = f4k_rot_take(dr, ticket, n_frames);
        CHECK(fr != F4K_ROT_NONE, "a frame number reaches F4K_ROT_NONE");
        if (fr > largest_frame) largest_frame = fr;
        return fr;
    }
    void next_draw(std::vector<uint32_t>& heads) {
        if (f4k_rot_advance(dr)) drawn = draw(heads, dr.head);
    }

    bool step(std::vector<uint32_t>& heads, size_t n_frames, std::vector<uint8_t>& done) {
        const unsigned H = dr.heads;
        switch (state) {
        case 0:
            h0 = dr.head;
            d0 = draw(heads, h0);
            state = 1;
            return true;
        case 1:
            dr.head = (h0 + 1) & (H - 1);
            drawn = draw(heads, dr.head);
            dr.pending = true;
            state = 2;
            return true;
        case 2: {
            const unsigned h1 = dr.head;
            dr.head = h0;
            cur = take(d0, n_frames);
            dr.head = h1;
            state = 3;
            return true;
        }
        case 3: {
            if (cur == F4K_ROT_NONE) {
                CHECK(!dr.pending && dr.live == 0 && out_at == 0 && held == 0, "a workgroup leaves with a draw out, a head in or a ticket held");
                uint32_t& exits = heads[F4K_ROT_EXIT_WORD];
                if (exits++ == grid - 1) {
                    for (unsigned x = 0; x < H; ++x) heads[x * F4K_TICKET_HEAD_WORDS] = 0;
                    exits = 0;
                }
                state = 5;
                return false;
            }
            // top(): the ticket that has come back is this iteration's prefetch
            nx = dr.pending ? take(drawn, n_frames) : F4K_ROT_NONE;
            if (!late) next_draw(heads);
            CHECK(held >= 1 && held - 1 <= 2, "%u tickets held beyond the frame transformed", held - 1);
            if (cur < n_frames) {
                CHECK(done[cur] == 0, "frame %u transformed twice", cur);
                done[cur] = 1;
            }
            if (late) { state = 4; return true; }
            --held;
            cur = nx;
            return true;
        }
        case 4:
            next_draw(heads);
            CHECK(held - 1 <= 2, "%u tickets held beyond the frame transformed", held - 1);
            --held;
            cur = nx;
            state = 3;
            return true;
        default:
            return false;
        }
    }
};

enum Schedule { ROUND_ROBIN, RANDOM, ONE_FIRST, LAST_FIRST, BURSTS, SCHEDULES };

unsigned widest = 0;   // the furthest two heads were ever apart, over all cases, in tickets

void check_apart(const std::vector<uint32_t>& heads, unsigned H, unsigned grid, bool cleared) {
    if (cleared) return;
    uint32_t lo = heads[0], hi = heads[0];
    for (unsigned x = 1; x < H; ++x) {
        const uint32_t v = heads[x * F4K_TICKET_HEAD_WORDS];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    CHECK(hi - lo <= grid, "heads %u apart on a grid of %u", hi - lo, grid);
    if (hi - lo > widest) widest = hi - lo;
}

// One launch: `grid` pullers of `H` heads on `heads`.
void launch(unsigned H, bool late, std::vector<uint32_t>& heads, size_t n_frames, unsigned grid, int schedule, unsigned seed) {
    std::vector<Puller> w(grid);
    for (unsigned b = 0; b < grid; ++b) {
        w[b].dr = f4k_rot_drawer(H, b);
        w[b].grid = grid;
        w[b].late = late;
    }
    std::vector<uint8_t> done(n_frames, 0);
    std::mt19937 rng(seed);
    std::vector<unsigned> alive(grid);
    for (unsigned b = 0; b < grid; ++b) alive[b] = b;
    unsigned left = grid;
    auto step = [&](unsigned b) {
        const bool live = w[b].step(heads, n_frames, done);
        if (!live) --left;
        check_apart(heads, H, grid, left == 0);
        return live;
    };
    auto run_out = [&](unsigned b) { while (step(b)) {} };
    if (schedule == ONE_FIRST) { const unsigned b = rng() % grid; run_out(b); alive[b] = alive.back(); alive.pop_back(); }
    if (schedule == LAST_FIRST) { run_out(grid - 1); alive.pop_back(); }
    while (!alive.empty()) {
        size_t i = 0;
        unsigned steps = 1;
        if (schedule == RANDOM || schedule == ONE_FIRST) i = rng() % alive.size();
        if (schedule == BURSTS) { i = rng() % alive.size(); steps = 1 + rng() % 40; }
        if (schedule == ROUND_ROBIN || schedule == LAST_FIRST) {
            // everybody one step, in order
            for (size_t k = 0; k < alive.size();) {
                if (step(alive[k])) ++k;
                else { alive[k] = alive.back(); alive.pop_back(); }
            }
            continue;
        }
        bool live = true;
        for (unsigned s = 0; s < steps && live; ++s) live = step(alive[i]);
        if (!live) { alive[i] = alive.back(); alive.pop_back(); }
    }
    size_t missing = 0;
    for (size_t f = 0; f < n_frames; ++f) missing += done[f] ? 0 : 1;
    CHECK(missing == 0, "%zu of %zu frames never transformed (H %u, late %d, grid %u, schedule %d)", missing, n_frames, H, (int)late, grid,
          schedule);
    // one draw past the end per workgroup and head at the most (the bound above f4k_rot_frame)
    CHECK((uint64_t)largest_frame < ((uint64_t)n_frames / H + 1 + grid) * H + H, "frame %u from %zu frames on a grid of %u", largest_frame,
          n_frames, grid);
}

void one_case(unsigned H, bool late, size_t n_frames, size_t max_blocks, int schedule, unsigned seed) {
    const unsigned grid = f4k_ticket_grid(max_blocks, n_frames);
    CHECK(grid >= F4K_TICKET_MAX_HEADS && grid % F4K_TICKET_MAX_HEADS == 0 && grid <= max_blocks, "grid %u for %zu frames, %zu blocks", grid, n_frames, max_blocks);
    if (grid == 0) return;
    std::vector<uint32_t> heads(F4K_ROT_WORDS + F4K_TICKET_HEAD_WORDS, GUARD_WORD);
    for (unsigned x = 0; x < H; ++x) heads[x * F4K_TICKET_HEAD_WORDS] = 0;
    heads[F4K_ROT_EXIT_WORD] = 0;
    // three calls on the same heads: this size, a short one, this size again
    const size_t calls[3] = {n_frames, 5, n_frames};
    for (int c = 0; c < 3; ++c) {
        const unsigned g = f4k_ticket_grid(max_blocks, calls[c]);
        largest_frame = 0;
        launch(H, late, heads, calls[c], g, schedule, seed + 17 * c);
        for (unsigned x = 0; x < H; ++x)
            CHECK(heads[x * F4K_TICKET_HEAD_WORDS] == 0, "head %u stands at %u after call %d (%zu frames, grid %u)", x,
                  heads[x * F4K_TICKET_HEAD_WORDS], c, calls[c], g);
        CHECK(heads[F4K_ROT_EXIT_WORD] == 0, "the exit counter stands at %u after call %d", heads[F4K_ROT_EXIT_WORD], c);
    }
    for (size_t i = 0; i < heads.size(); ++i) {
        const bool is_head = i % F4K_TICKET_HEAD_WORDS == 0 && i / F4K_TICKET_HEAD_WORDS < H;
        if (!is_head && i != F4K_ROT_EXIT_WORD) CHECK(heads[i] == GUARD_WORD, "word %zu beside the heads was written", i);
    }
}

}  // namespace

int main() {
    const size_t frames[] = {1, 7, 8, 9, 767, 768, 769, 2309, 98304};
    const size_t grids[] = {8, 760, 768};
    int cases = 0;
    for (unsigned H : {2u, 4u, 8u})
        for (bool late : {false, true})
            for (size_t n : frames)
                for (size_t g : grids)
                    for (int s = 0; s < SCHEDULES; ++s) {
                        if (n > 50000 && s != ROUND_ROBIN && s != BURSTS) continue;   // (the long one: two schedules)
                        for (unsigned k = 0; k < (n > 50000 ? 1u : 2u); ++k) {
                            one_case(H, late, n, g, s, 1000u * (unsigned)cases + k);
                            ++cases;
                        }
                    }

    // the choice by name
    CHECK(f4k_rot_ahead_parse("3") == F4K_AHEAD_3 && f4k_rot_ahead_parse("2top") == F4K_AHEAD_2TOP, "look-aheads by name");
    CHECK(f4k_rot_ahead_parse("2") < 0 && f4k_rot_ahead_parse("") < 0 && f4k_rot_ahead_parse(nullptr) < 0 && f4k_rot_ahead_parse("2topp") < 0 &&
          f4k_rot_ahead_parse("33") < 0 && f4k_rot_ahead_parse("2late") < 0, "other names");
    {
        const F4kChoice d = f4k_choice(nullptr, nullptr);
        CHECK(d.rot_ahead == F4K_ROT_DEFAULT_AHEAD && d.rot_heads == F4K_ROT_DEFAULT_HEADS, "defaults");
        const F4kChoice a = f4k_choice("ticket", "rot8", "2top");
        CHECK(a.order == F4K_ORDER_TICKET && a.rot_heads == 8 && a.rot_ahead == F4K_AHEAD_2TOP, "rot8, 2top");
        const F4kChoice b = f4k_choice(nullptr, nullptr, "3");
        CHECK(b.rot_ahead == F4K_AHEAD_3 && b.rot_heads == F4K_ROT_DEFAULT_HEADS, "3");
        const F4kChoice c = f4k_choice(nullptr, nullptr, "4");
        CHECK(c.rot_ahead == F4K_ROT_DEFAULT_AHEAD, "unknown names leave the default");
    }
    // the largest frame number a slot can carry at look-ahead two stays below F4K_ROT_NONE
    CHECK((uint64_t)(F4K_TICKET_MAX_FRAMES / 2 + 1 + 65535) * 2 + 1 < F4K_ROT_NONE &&
          (uint64_t)(F4K_TICKET_MAX_FRAMES / 8 + 1 + 65535) * 8 + 7 < F4K_ROT_NONE, "frame numbers fit 32 bits");
    printf("f4k_rot2 cases=%d bad=%d widest=%u\n", cases, bad, widest);
    return bad ? 1 : 0;
}

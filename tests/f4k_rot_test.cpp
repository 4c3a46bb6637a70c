// f4k_rot_test.cpp — csrc/f4k_rot.h on the CPU: the workgroups of fft4096_rot_kernel as state machines that draw from the
// heads exactly as the kernel does (three draws in the prologue, one more at the top of every iteration, through
// F4kRotDrawer; the frame of a ticket into the slot one iteration after its draw, prefetched one later, transformed one
// later still; out at F4K_ROT_NONE, one more on the exit counter, the last one out zeroes everything), stepped in the seeded
// interleavings of f4k_ticket_test.cpp, for H = 2, 4, 8.  Every frame must be transformed exactly once, nothing at or past
// the end, the heads never more than the grid apart, heads and exit counter zero after every call — three calls in a row on
// the same heads — and no word beside them written.  Built with -fsanitize=address,undefined and run directly
// (tests/test_f4k_rot.py).
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

// One workgroup of the kernel.  step() is one of: one of the prologue's three draws, the prologue's end (the first two
// tickets into the slots), one iteration of the loop, the exit; returns false once the workgroup has left.
struct Puller {
    F4kRotDrawer dr = {};
    unsigned grid = 0;
    int state = 0;              // 0..2: the prologue's draws; 3: its end; 4: in the loop; 5: gone
    uint32_t d[2] = {0, 0};     // the prologue's first two tickets
    unsigned h[2] = {0, 0};     // ... and their heads
    uint32_t drawn = 0;         // lane 0's register: the ticket of the last draw
    uint32_t cur = 0, nx = 0;

    static uint32_t draw(std::vector<uint32_t>& heads, unsigned head) { return heads[head * F4K_TICKET_HEAD_WORDS]++; }

    bool step(std::vector<uint32_t>& heads, size_t n_frames, std::vector<uint8_t>& done) {
        const unsigned H = dr.heads;
        switch (state) {
        case 0:
            h[0] = dr.head;
            d[0] = draw(heads, h[0]);
            state = 1;
            return true;
        case 1:
            h[1] = (h[0] + 1) & (H - 1);
            d[1] = draw(heads, h[1]);
            state = 2;
            return true;
        case 2:
            dr.head = (h[1] + 1) & (H - 1);
            drawn = draw(heads, dr.head);
            dr.pending = true;
            state = 3;
            return true;
        case 3: {
            const unsigned h2 = dr.head;
            dr.head = h[0];
            cur = f4k_rot_take(dr, d[0], n_frames);
            dr.head = h[1];
            nx = f4k_rot_take(dr, d[1], n_frames);
            dr.head = h2;
            state = 4;
            return true;
        }
        case 4: {
            if (cur == F4K_ROT_NONE) {
                CHECK(!dr.pending && dr.live == 0, "a workgroup leaves with a draw out or a head in");
                uint32_t& exits = heads[F4K_ROT_EXIT_WORD];
                if (exits++ == grid - 1) {
                    for (unsigned x = 0; x < H; ++x) heads[x * F4K_TICKET_HEAD_WORDS] = 0;
                    exits = 0;
                }
                state = 5;
                return false;
            }
            const uint32_t slot = dr.pending ? f4k_rot_take(dr, drawn, n_frames) : F4K_ROT_NONE;
            if (f4k_rot_advance(dr)) drawn = draw(heads, dr.head);
            if (cur < n_frames) {
                CHECK(done[cur] == 0, "frame %u transformed twice", cur);
                done[cur] = 1;
            }
            cur = nx;
            nx = slot;
            return true;
        }
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
void launch(unsigned H, std::vector<uint32_t>& heads, size_t n_frames, unsigned grid, int schedule, unsigned seed) {
    std::vector<Puller> w(grid);
    for (unsigned b = 0; b < grid; ++b) {
        w[b].dr = f4k_rot_drawer(H, b);
        w[b].grid = grid;
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
    CHECK(missing == 0, "%zu of %zu frames never transformed (H %u, grid %u, schedule %d)", missing, n_frames, H, grid, schedule);
}

void one_case(unsigned H, size_t n_frames, size_t max_blocks, int schedule, unsigned seed) {
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
        launch(H, heads, calls[c], g, schedule, seed + 17 * c);
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
    for (unsigned H : {2u, 4u, 8u}) {
        CHECK(f4k_rot_heads_ok(H), "heads %u", H);
        for (size_t n : frames)
            for (size_t g : grids)
                for (int s = 0; s < SCHEDULES; ++s) {
                    if (n > 50000 && s != ROUND_ROBIN && s != BURSTS) continue;   // (the long one: two schedules)
                    for (unsigned k = 0; k < (n > 50000 ? 1u : 2u); ++k) {
                        one_case(H, n, g, s, 1000u * (unsigned)cases + k);
                        ++cases;
                    }
                }
    }

    // the rules around the launches
    CHECK(!f4k_rot_heads_ok(0) && !f4k_rot_heads_ok(1) && !f4k_rot_heads_ok(3) && !f4k_rot_heads_ok(16), "heads");
    CHECK(f4k_rot_parse("rot2") == 2 && f4k_rot_parse("rot4") == 4 && f4k_rot_parse("rot8") == 8, "forms by name");
    CHECK(f4k_rot_parse("rot") == 0 && f4k_rot_parse("rot3") == 0 && f4k_rot_parse("rot16") == 0 && f4k_rot_parse("1x2") == 0 &&
          f4k_rot_parse("") == 0 && f4k_rot_parse(nullptr) == 0, "other names");
    CHECK(f4k_rot_next_head(8, 0xFFu, 7) == 0 && f4k_rot_next_head(8, 0x81u, 0) == 7 && f4k_rot_next_head(8, 0x01u, 0) == 0 &&
          f4k_rot_next_head(2, 0x2u, 1) == 1 && f4k_rot_next_head(4, 0x5u, 2) == 0, "rotation over the heads still in");
    CHECK(f4k_rot_frame(8, 5, 3) == 43 && f4k_rot_frame(2, 0, 1) == 1, "frames of tickets");
    // the largest frame number a slot can carry stays below F4K_ROT_NONE
    CHECK((uint64_t)(F4K_TICKET_MAX_FRAMES / 2 + 1 + 2 * 65535) * 2 + 1 < F4K_ROT_NONE &&
          (uint64_t)(F4K_TICKET_MAX_FRAMES / 8 + 1 + 2 * 65535) * 8 + 7 < F4K_ROT_NONE, "frame numbers fit 32 bits");
    printf("f4k_rot cases=%d bad=%d widest=%u\n", cases, bad, widest);
    return bad ? 1 : 0;
}

// Stand-alone driver for csrc/f4k_split.h (tests/test_f4k_split.py builds it with -fsanitize=address,undefined and runs it):
// the number of launches of an N = 4096 call, and that the parts plan_launch cuts with it cover every frame exactly once.
#include <cstdio>
#include <vector>

#include "../sdr-iq-visualizer_amd/csrc/f4k_split.h"

using sdrk_host::F4K_SPLIT_FRAMES;
using sdrk_host::f4k_split_parts;

static int bad = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } \
    } while (0)

// what plan_launch does with the count: parts of ceil(n / parts) frames, the last one what is left
static void cover(size_t n) {
    const size_t parts = f4k_split_parts(n);
    CHECK(parts >= 1);
    const size_t per = (n + parts - 1) / parts;
    size_t launches = 0, covered = 0, smallest = (size_t)-1, largest = 0;
    for (size_t f0 = 0; f0 < n; f0 += per) {
        const size_t nf = n - f0 < per ? n - f0 : per;
        CHECK(f0 == covered);                       // contiguous, in order, no overlap
        covered += nf;
        ++launches;
        if (nf < smallest) smallest = nf;
        if (nf > largest) largest = nf;
        if (launches > parts) break;
    }
    CHECK(covered == n);
    CHECK(n == 0 ? launches == 0 : launches == parts);
    if (parts > 1) {                                // no stub, no long launch
        CHECK(3 * smallest >= 2 * F4K_SPLIT_FRAMES - 3 * parts);
        CHECK(2 * largest <= 3 * F4K_SPLIT_FRAMES);
    }
}

int main() {
    const size_t S = F4K_SPLIT_FRAMES;
    static_assert(f4k_split_parts(0) == 1 && f4k_split_parts(1) == 1, "short calls are one launch");
    CHECK(S == 65536);
    CHECK(f4k_split_parts(S) == 1);
    CHECK(f4k_split_parts(S + S / 2 - 1) == 1);    // up to 1.5 S: one launch
    CHECK(f4k_split_parts(S + S / 2) == 2);
    CHECK(f4k_split_parts(2 * S + S / 2 - 1) == 2);
    CHECK(f4k_split_parts(2 * S + S / 2) == 3);
    CHECK(f4k_split_parts((size_t)1 << 20) == 16);  // the headline: 16 launches of 65536 frames
    CHECK(f4k_split_parts(((size_t)1 << 20) + 1000) == 16);
    CHECK(f4k_split_parts((size_t)1 << 40) == ((size_t)1 << 24));
    std::vector<size_t> sizes = {0, 1, 2, 767, 768, S - 1, S, S + 1, S + S / 2 - 1, S + S / 2, S + S / 2 + 1, 2 * S - 1, 2 * S,
                                 2 * S + 1001, 163917, 3 * S + 7, (size_t)1 << 20, ((size_t)1 << 20) + 1000, ((size_t)1 << 20) - 1,
                                 ((size_t)1 << 27) + 12345};
    for (size_t n : sizes) cover(n);
    for (size_t n = S; n < 6 * S; n += 4099) cover(n);
    printf("f4k_split bad=%d\n", bad);
    return bad ? 1 : 0;
}

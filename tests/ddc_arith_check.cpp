// tests/ddc_arith_check.cpp — the exhaustive checks of the digital down-converter's shared arithmetic (csrc/kernels_ddc.h: what
// the kernels of csrc/ddc4096.hip and the stand-in tests/fake_ddc_kernels.cpp both call), run on the CPU by tests/test_ddc_host.py.
// A stand-alone program built by g++ against tests/fake_hip; prints one line per check.
//   div     ddc_div(n, ddc_recip(D)) == n / D for every D in 1 .. 256 and every n < 8704
//   nco     ddc_factor((1, 0), r) against exp(-2 pi i r / 2^32) in float64 over all 2^20 values of r: the worst error of each part
//   keep    the block-to-block bookkeeping of a persistent workgroup (ddc_keep_first / _next / _base and the per-element test)
//           against the definition "(index0 + i) % D == 0, stored in ascending i", for every D, several L, grids and index0
//   bits    r == 0 returns the table entry itself
#include "../sdr-iq-visualizer_amd/csrc/kernels_ddc.h"

#include <cmath>
#include <cstdio>
#include <initializer_list>

using namespace sdrk;

int main() {
    long bad_div = 0;
    for (unsigned d = 1; d <= 256; ++d) {
        const unsigned recip = ddc_recip(d);
        for (unsigned n = 0; n < 8704; ++n) bad_div += ddc_div(n, recip) != n / d;
    }
    printf("div bad=%ld\n", bad_div);

    double worst_c = 0, worst_s = 0;
    for (uint32_t r = 0; r < (1u << 20); ++r) {
        const OlsC f = ddc_factor(OlsC{1.0f, 0.0f}, r);
        const double a = 2.0 * 3.14159265358979323846 * (double)r / 4294967296.0;
        worst_c = fmax(worst_c, fabs((double)f.x - cos(a)));
        worst_s = fmax(worst_s, fabs((double)f.y + sin(a)));
    }
    printf("nco worst_cos=%.6e worst_sin=%.6e\n", worst_c, worst_s);

    long bad_keep = 0, kept_total = 0;
    for (unsigned L : {2048u, 3072u, 3840u, 4096u})
        for (unsigned grid : {1u, 3u, 512u, 768u})
            for (unsigned d = 1; d <= 256; ++d)
                for (uint64_t index0 : {(uint64_t)0, (uint64_t)1, (uint64_t)(d - 1), (uint64_t)12345, ((uint64_t)1 << 40) + 3}) {
                    const unsigned r0 = (unsigned)(index0 % d), recip = ddc_recip(d), stride = grid * L;
                    for (unsigned first : {0u, grid - 1}) {   // the workgroups at both ends of the grid, four blocks each
                        DdcKeep k = ddc_keep_first(r0, first, L, d);
                        for (unsigned it = 0; it < 4; ++it) {
                            const uint64_t b = first + (uint64_t)it * grid, i0 = b * L;
                            uint64_t before = 0;   // kept outputs i < b L
                            {
                                const uint64_t i_first = (d - index0 % d) % d;
                                before = i_first >= i0 ? 0 : (i0 - 1 - i_first) / d + 1;
                            }
                            bad_keep += k.rem != (index0 + i0) % d;
                            bad_keep += ddc_keep_base(k, r0) != before;
                            const unsigned qmin = k.rem != 0;
                            uint64_t slot = before;
                            for (unsigned rel = 0; rel < L; ++rel) {
                                const unsigned n = k.rem + rel, q = ddc_div(n, recip);
                                const bool kept = n == q * d;
                                bad_keep += kept != ((index0 + i0 + rel) % d == 0);
                                if (kept) {
                                    bad_keep += before + (q - qmin) != slot;
                                    ++slot, ++kept_total;
                                }
                            }
                            ddc_keep_next(k, stride / d, stride % d, d);
                        }
                    }
                }
    printf("keep bad=%ld kept=%ld\n", bad_keep, kept_total);

    const OlsC w{-0.0f, 0.70710678f}, f = ddc_factor(w, 0x12300000u);
    printf("bits same=%d\n", __builtin_memcmp(&w, &f, sizeof w) == 0);
    return 0;
}

"""What the compiler made of the 8-bit kernels, read from the ELF notes of the gfx950 code objects inside the built libsdrk.so
(no GPU needed; the extraction of tests/code_objects.py): fft4096_ci8_kernel (window x epilogue: 4 — the direct load form is
the only one kept), fft4096_kgroup_ci8_kernel (window x detector: 6; the format is a run-time argument and adds none) and
unpack_ci8_kernel exist under those names, keep the budgets of their int16 forms, and leave every count the existing
code-object tests assert as it was.  No disassembly is searched."""
import re

from tests.code_objects import kernels, no_scratch_memory as _no_scratch  # noqa: F401  (the fixture)

LDS_RECT, LDS_WINDOW = 36992, 53376        # exchange buffer + tables, and with the window's 16 KiB
COUNTED = ("ci16", "fft4096_kernelILb", "integrate", "pfb", "ols", "sk4096", "sk_rows", "xspec", "chanbank", "ddc")


def _lds_of(name, k):
    return k["group_segment_fixed_size"] == (LDS_WINDOW if "kernelILb1E" in name else LDS_RECT)


def test_the_four_per_frame_kernels_keep_four_waves_per_simd(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "fft4096_ci8_kernel" in n}
    assert sorted(re.search(r"kernelILb(\d)ELi(\d)EE", n).groups() for n in hits) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 128, (n, k)
        assert _lds_of(n, k), (n, k)
        assert _no_scratch(k), (n, k)


def test_the_six_kgroup_kernels_keep_three_workgroups_per_cu_and_the_int16_budget(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "fft4096_kgroup_ci8_kernel" in n}
    assert sorted(re.search(r"kernelILb(\d)ELi(\d)EE", n).groups() for n in hits) == [(w, d) for w in "01" for d in "012"], sorted(hits)
    i16 = max(k["vgpr_count"] for n, k in kernels.items() if "fft4096_kgroup_ci16_kernelILb" in n)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168 and k["vgpr_count"] <= i16, (n, k, i16)
        assert _lds_of(n, k), (n, k)
        assert _no_scratch(k), (n, k)


def test_the_unpack_kernel_has_no_scratch(kernels):  # noqa: F811
    hits = [k for n, k in kernels.items() if "unpack_ci8_kernel" in n]
    assert len(hits) == 1, sorted(n for n in kernels if "ci8" in n)
    assert _no_scratch(hits[0]) and hits[0]["group_segment_fixed_size"] == 0, hits[0]


def test_every_count_of_the_existing_code_object_tests_still_holds(kernels):  # noqa: F811
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    new = [n for n in kernels if "ci8" in n]
    assert len(new) == 11, new
    for n in new:
        for fragment in COUNTED:
            assert fragment not in n, (n, fragment)
    assert count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("fft4096_integrate_kernelILb") == 6 and count("fft4096_kgroup_ci16_kernelILb") == 6
    assert count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("unpack_ci16_kernel") == 1 and count("synth_fill_ci16_kernel") == 1
    assert count("pfb4096_kernelILi") == 2 and count("pfb4096_groups_kernel") == 3 and count("pfb_fold_kernel") == 1
    assert count("sk4096_kernel") == 4 and count("sk_rows_kernel") == 1 and count("sk_finalize_kernel") == 1
    assert count("xspec") == 8 and count("ols4096_kernel") == 4 and count("chanbank_kernel") == 2

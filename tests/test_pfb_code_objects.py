"""What the compiler made of the polyphase-filter-bank kernels, read from the ELF notes of the gfx950 code objects inside the
built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py): pfb4096_kernel keeps the budgets of three
workgroups per CU and the LDS of the window-less N = 4096 kernels, and neither kernel uses scratch."""
import re

from tests.code_objects import kernels  # noqa: F401  (the fixture)


def test_pfb4096_kernels_keep_three_workgroups_per_cu(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "pfb4096_kernelILi" in n}
    assert sorted(re.search(r"pfb4096_kernelILi(\d)EE", n).group(1) for n in hits) == ["0", "1"], sorted(hits)   # both epilogues
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)                       # 512 / 3 waves per SIMD
        assert k["group_segment_fixed_size"] == 36992, (n, k)       # exchange buffer + the two tables, no window
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)


def test_pfb_fold_kernel_has_no_scratch(kernels):  # noqa: F811
    hits = [k for n, k in kernels.items() if "pfb_fold_kernel" in n]
    assert len(hits) == 1, sorted(n for n in kernels if "pfb" in n)
    assert hits[0]["private_segment_fixed_size"] == 0 and hits[0]["vgpr_spill_count"] == 0, hits[0]


def test_new_kernel_names_stay_out_of_the_existing_counts(kernels):  # noqa: F811
    for n in kernels:
        if "pfb" in n:
            for fragment in ("fft4096_kernelILb", "integrate", "ci16", "kgroup", "fft_lds"):
                assert fragment not in n, (n, fragment)

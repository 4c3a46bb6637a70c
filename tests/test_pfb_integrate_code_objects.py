"""What the compiler made of the integrated polyphase-filter-bank kernel, read from the ELF notes of the gfx950 code objects
inside the built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py): pfb4096_groups_kernel in its
three detectors keeps the budgets of three workgroups per CU — at most 168 VGPRs, a third of the LDS, no scratch.  The mean
keeps its 16 compensation terms per thread in LDS (the 16 KiB the windowed kernels keep the window in), so its LDS figure is
theirs and the hold detectors' is the window-less one.  No disassembly is searched."""
import re

from tests.code_objects import kernels  # noqa: F401  (the fixture)


def test_the_three_detectors_keep_three_workgroups_per_cu(kernels):  # noqa: F811
    hits = {re.search(r"pfb4096_groups_kernelILi(\d)EE", n).group(1): k for n, k in kernels.items() if "pfb4096_groups_kernel" in n}
    assert sorted(hits) == ["0", "1", "2"], sorted(n for n in kernels if "pfb" in n)      # mean / max / min, nothing else
    assert len([n for n in kernels if "pfb4096_groups_kernel" in n]) == 3
    for det, k in hits.items():
        assert k["vgpr_count"] <= 168, (det, k)                       # 512 / 3 waves per SIMD
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (det, k)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // 3, (det, k)
    # the mean's compensation lives in LDS: exchange buffer + the two tables + 16 KiB; max and min hold theirs in registers
    assert hits["0"]["group_segment_fixed_size"] == 36992 + 16384 == 53376, hits["0"]
    assert hits["1"]["group_segment_fixed_size"] == hits["2"]["group_segment_fixed_size"] == 36992, (hits["1"], hits["2"])
    assert max(hits["1"]["vgpr_count"], hits["2"]["vgpr_count"]) <= hits["0"]["vgpr_count"], hits


def test_the_name_stays_out_of_the_existing_counts(kernels):  # noqa: F811
    new = [n for n in kernels if "pfb4096_groups_kernel" in n]
    assert new
    for n in new:
        for fragment in ("integrate", "ci16", "kgroup", "fft_lds", "fft4096_kernelILb", "pfb4096_kernelILi", "pfb_fold_kernel"):
            assert fragment not in n, (n, fragment)
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "integrate_rows_kernel" in n]) == 3
    assert len([n for n in kernels if "integrate_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "pfb4096_kernelILi" in n]) == 2 and len([n for n in kernels if "pfb_fold_kernel" in n]) == 1

"""What the compiler made of the int16 polyphase-filter-bank kernels, read from the ELF notes of the gfx950 code objects inside
the built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py): pfb4096_i16_kernel (both epilogues),
pfb4096_i16_groups_kernel (three detectors) and pfb_fold_i16_kernel exist under those names, keep the budgets of their
complex64 forms — at most 168 VGPRs, no scratch, no spills, the same LDS — and leave every count the existing code-object
tests assert as it was.  No disassembly is searched."""
import re

from tests.code_objects import kernels, no_scratch_memory as _no_scratch  # noqa: F401  (the fixture)


def test_the_per_frame_kernels_keep_three_workgroups_per_cu(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "pfb4096_i16_kernelILi" in n}
    assert sorted(re.search(r"pfb4096_i16_kernelILi(\d)EE", n).group(1) for n in hits) == ["0", "1"], sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)
        assert k["group_segment_fixed_size"] == 36992, (n, k)
        assert _no_scratch(k), (n, k)
    # 16 dwords in flight instead of 16 qwords: not more registers than the complex64 form
    c64 = max(k["vgpr_count"] for n, k in kernels.items() if "pfb4096_kernelILi" in n)
    assert max(k["vgpr_count"] for k in hits.values()) <= c64, (hits, c64)


def test_the_three_detectors_keep_three_workgroups_per_cu(kernels):  # noqa: F811
    names = [n for n in kernels if "pfb4096_i16_groups_kernel" in n]
    hits = {re.search(r"pfb4096_i16_groups_kernelILi(\d)EE", n).group(1): kernels[n] for n in names}
    assert sorted(hits) == ["0", "1", "2"] and len(names) == 3, sorted(n for n in kernels if "pfb" in n)
    for det, k in hits.items():
        assert k["vgpr_count"] <= 168, (det, k)
        assert _no_scratch(k), (det, k)
    assert hits["0"]["group_segment_fixed_size"] == 36992 + 16384 == 53376, hits["0"]       # the mean's compensation in LDS
    assert hits["1"]["group_segment_fixed_size"] == hits["2"]["group_segment_fixed_size"] == 36992, hits


def test_the_fold_kernel_has_no_scratch(kernels):  # noqa: F811
    hits = [k for n, k in kernels.items() if "pfb_fold_i16_kernel" in n]
    assert len(hits) == 1, sorted(n for n in kernels if "pfb" in n)
    assert _no_scratch(hits[0]) and hits[0]["group_segment_fixed_size"] == 0, hits[0]


def test_every_count_of_the_existing_code_object_tests_still_holds(kernels):  # noqa: F811
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    assert count("pfb4096_kernelILi") == 2 and count("pfb4096_groups_kernel") == 3 and count("pfb_fold_kernel") == 1
    assert count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("fft4096_integrate_kernelILb") == 6 and count("fft4096_kgroup_ci16_kernelILb") == 6
    assert count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("unpack_ci16_kernel") == 1 and count("synth_fill_ci16_kernel") == 1
    for n in kernels:
        if "pfb" in n:
            for fragment in ("fft4096_kernelILb", "integrate", "ci16", "kgroup", "fft_lds"):
                assert fragment not in n, (n, fragment)

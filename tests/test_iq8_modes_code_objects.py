"""What the compiler made of the 8-bit filter-bank and spectral-kurtosis kernels (csrc/pfb4096_iq8.hip, pfb4096_iq8_groups.hip,
sk4096_iq8.hip, pfb_fold_iq8.hip), read from the ELF notes of the gfx950 code objects inside the built libsdrk.so (no GPU needed;
the extraction of tests/code_objects.py; no disassembly is searched): 5 + 2 + 1 kernels — the format being a run-time argument —
under their names, within the budgets of their int16 counterparts (three workgroups per CU: at most 168 VGPRs, 36,992 B of
LDS and 53,376 B where the mean's compensation or the window lives there, no scratch, no spilled VGPR), their names clear of
every fragment the other code-object tests count by, and those counts what they were."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

LDS, LDS_MORE = 36992, 53376               # exchange buffer + the two tables; ... + 16 KiB (compensation rows / the window)
FRAGMENTS = ("ci8", "ci16", "integrate", "kgroup", "fft_lds", "pfb4096_kernelILi", "pfb4096_groups_kernel", "pfb_fold_kernel",
             "pfb4096_i16", "pfb_fold_i16", "sk4096_kernel", "sk_rows_kernel", "sk_finalize_kernel", "xspec", "chanbank")


def new_kernels(kernels):  # noqa: F811
    return {n: k for n, k in kernels.items() if "_iq8_" in n and "downconv" not in n}


def test_eight_kernels_exist_and_meet_the_budgets(kernels):  # noqa: F811
    frames = {n: k for n, k in kernels.items() if "pfb4096_iq8_kernelILi" in n}
    groups = {n: k for n, k in kernels.items() if "pfb4096_iq8_groups_kernelILi" in n}
    sk = {n: k for n, k in kernels.items() if "sk4096_iq8_kernelILb" in n}
    fold = {n: k for n, k in kernels.items() if "pfb_fold_iq8_kernel" in n}
    assert (len(frames), len(groups), len(sk), len(fold)) == (2, 3, 2, 1), (sorted(frames), sorted(groups), sorted(sk), sorted(fold))
    assert len(new_kernels(kernels)) == 8                                                    # a format adds no instantiation
    assert sorted(n.split("kernelILi")[1][0] for n in frames) == ["0", "1"]                  # the two epilogues
    assert sorted(n.split("kernelILi")[1][0] for n in groups) == ["0", "1", "2"]             # mean, max, min
    for hits in (frames, groups, sk):
        for n, k in hits.items():
            print(n, k["vgpr_count"], k["group_segment_fixed_size"], k.get("sgpr_spill_count", 0))
            assert k["vgpr_count"] <= 168 <= 512 // 3, (n, k)                              # three workgroups per CU
            assert k["max_flat_workgroup_size"] == 256, (n, k)
            assert no_scratch_memory(k), (n, k)
    for n, k in frames.items():
        assert k["group_segment_fixed_size"] == LDS, (n, k)
    for n, k in groups.items():                                                              # the mean keeps its compensation in LDS
        assert k["group_segment_fixed_size"] == (LDS_MORE if "ILi0EE" in n else LDS), (n, k)
    for n, k in sk.items():                                                                  # the windowed one its window
        assert k["group_segment_fixed_size"] == (LDS_MORE if "ILb1EE" in n else LDS), (n, k)
    assert 3 * LDS_MORE <= 160 * 1024
    for n, k in fold.items():
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256 and no_scratch_memory(k), (n, k)


def test_no_new_name_contains_a_counted_fragment(kernels):  # noqa: F811
    new = new_kernels(kernels)
    assert len(new) == 8, sorted(new)
    for n in new:
        low = n.lower()
        assert "ddc" not in low and "downconv" not in low and not ("ols" in low and "4096" in n), n   # (the parameter struct types included)
        for fragment in FRAGMENTS:
            assert fragment not in n, (n, fragment)


def test_every_count_of_the_existing_code_object_tests_still_holds(kernels):  # noqa: F811
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    assert count("ci8") == 11 and len([n for n in kernels if "ddc" in n.lower()]) == 6
    assert len([n for n in kernels if "downconv" in n.lower()]) == 3
    assert count("ddc_kernel") == 4 and count("ddcbank_kernel") == 2
    assert count("ols4096_kernel") == 4 and len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    assert count("chanbank_kernel") == 2 and count("xspec") == 8
    assert count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("fft4096_integrate_kernelILb") == 6 and count("fft4096_kgroup_ci16_kernelILb") == 6
    assert count("fft4096_ci8_kernel") == 4 and count("fft4096_kgroup_ci8_kernel") == 6 and count("unpack_ci8_kernel") == 1
    assert count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("unpack_ci16_kernel") == 1 and count("synth_fill_ci16_kernel") == 1
    assert count("pfb4096_kernelILi") == 2 and count("pfb4096_groups_kernel") == 3 and count("pfb_fold_kernel") == 1
    assert count("pfb4096_i16_kernelILi") == 2 and count("pfb4096_i16_groups_kernel") == 3 and count("pfb_fold_i16_kernel") == 1
    assert count("sk4096_kernel") == 4 and count("sk_rows_kernel") == 1 and count("sk_finalize_kernel") == 1
    # the existing filter-bank and kurtosis kernels keep their budgets beside the new ones
    for n, k in kernels.items():
        if "pfb4096_" in n or "sk4096_kernel" in n:
            assert k["vgpr_count"] <= 168 and no_scratch_memory(k), (n, k)
            assert k["group_segment_fixed_size"] in (LDS, LDS_MORE), (n, k)

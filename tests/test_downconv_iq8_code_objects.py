"""What the compiler made of the 8-bit down-converter's kernels (csrc/downconv_iq8.hip), read from the ELF notes of the gfx950
code objects inside the built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): the
single call with the mixer on and off and the bank — three kernels, the format being a run-time argument — under their names,
within the budgets of their int16 counterparts (three and two workgroups per CU, 36,992 B of LDS, no scratch, no spilled VGPR),
their names clear of every fragment the other code-object tests count by, and those counts what they were."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

LDS = 36992                                # exchange buffer + the two tables, as the FIR and DDC kernels
FRAGMENTS = ("ci8", "ci16", "integrate", "pfb", "kgroup", "fft_lds", "fft4096_kernel", "sk4096", "sk_rows", "chanbank", "xspec", "4096")


def test_three_kernels_exist_and_meet_the_budgets_of_their_int16_counterparts(kernels):  # noqa: F811
    single = {n: k for n, k in kernels.items() if "downconv_iq8_kernel" in n}
    bank = {n: k for n, k in kernels.items() if "downconvbank_iq8_kernel" in n}
    assert len(single) == 2 and len(bank) == 1, (sorted(single), sorted(bank))
    assert sorted("ILb1EE" in n for n in single) == [False, True], sorted(single)          # the mixer off and on
    assert len([n for n in kernels if "downconv" in n.lower()]) == 3                       # a format adds no instantiation
    for hits, wg_per_cu, vgprs in ((single, 3, 168), (bank, 2, 256)):
        for n, k in hits.items():
            print(n, k["vgpr_count"], k["group_segment_fixed_size"])
            assert k["vgpr_count"] <= vgprs <= 512 // wg_per_cu, (n, k)                    # the SIMD's 512 registers per lane
            assert k["group_segment_fixed_size"] == LDS and LDS <= 160 * 1024 // wg_per_cu, (n, k)
            assert k["max_flat_workgroup_size"] == 256, (n, k)
            assert no_scratch_memory(k), (n, k)
    for n, k in bank.items():
        assert k["vgpr_count"] > 512 // 3, (n, k)                                          # (the bank does not declare fewer than it could)


def test_no_new_name_contains_a_counted_fragment(kernels):  # noqa: F811
    new = [n for n in kernels if "downconv" in n.lower()]
    assert len(new) == 3, sorted(new)
    for n in new:
        assert "ddc" not in n.lower() and not ("ols" in n.lower() and "4096" in n), n      # (the parameter struct types included)
        for fragment in FRAGMENTS:
            assert fragment not in n, (n, fragment)


def test_every_count_of_the_existing_code_object_tests_still_holds(kernels):  # noqa: F811
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    assert count("ci8") == 11 and len([n for n in kernels if "ddc" in n.lower()]) == 6
    assert count("ddc_kernel") == 4 and count("ddcbank_kernel") == 2
    assert count("ols4096_kernel") == 4 and len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    assert count("chanbank_kernel") == 2 and count("xspec") == 8
    assert count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("fft4096_integrate_kernelILb") == 6 and count("fft4096_kgroup_ci16_kernelILb") == 6
    assert count("fft4096_ci8_kernel") == 4 and count("fft4096_kgroup_ci8_kernel") == 6 and count("unpack_ci8_kernel") == 1
    assert count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("unpack_ci16_kernel") == 1 and count("synth_fill_ci16_kernel") == 1
    assert count("pfb4096_kernelILi") == 2 and count("pfb4096_groups_kernel") == 3 and count("pfb_fold_kernel") == 1
    assert count("sk4096_kernel") == 4 and count("sk_rows_kernel") == 1 and count("sk_finalize_kernel") == 1
    # the FIR, bank and DDC kernels' own figures, as test_ddc_code_objects.py holds them
    assert sorted(k["vgpr_count"] for n, k in kernels.items() if "ols4096_kernel" in n) == [132, 148, 158, 174]
    for n, k in kernels.items():
        if "ddc_kernel" in n or "ddcbank_kernel" in n or "chanbank_kernel" in n:
            assert k["group_segment_fixed_size"] == LDS and no_scratch_memory(k), (n, k)

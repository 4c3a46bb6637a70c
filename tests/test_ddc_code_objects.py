"""What the compiler made of the digital down-converter's kernels (csrc/ddc4096.hip), read from the ELF notes of the gfx950 code
objects inside the built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): the single
call in four instantiations (complex64 / int16 input x mixer on / off) and the bank in two, each within the registers and the LDS
of the workgroups per CU its __launch_bounds__ declares and not declaring fewer than fit, no scratch memory, no spilled VGPR — and
the FIR and channel-bank kernels next to them are what they were."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("integrate", "ci16", "kgroup", "pfb", "fft_lds", "fft4096_kernel", "fft4096_features_kernel", "sk4096", "sk_rows",
         "sk_finalize", "xspec", "row_pass", "col_pass", "4096", "chanbank", "ols4096")


def wg_per_cu(name):
    """ddc_wg_per_cu() / ddcbank_wg_per_cu() of ddc4096.hip: two for the bank and for complex64 input with the mixer, else three."""
    return 2 if "ddcbank_kernel" in name or ("OlsInC64" in name and "ELb1EE" in name) else 3


def test_every_instantiation_fits_the_workgroups_per_cu_it_declares(kernels):  # noqa: F811
    single = {n: k for n, k in kernels.items() if "ddc_kernel" in n}
    bank = {n: k for n, k in kernels.items() if "ddcbank_kernel" in n}
    assert len(single) == 4 and len(bank) == 2, (sorted(single), sorted(bank))
    for hits in (single, bank):
        assert len([n for n in hits if "OlsInI16" in n]) == len([n for n in hits if "OlsInC64" in n]) == len(hits) // 2, sorted(hits)
    assert len([n for n in single if "ELb1EE" in n]) == 2, sorted(single)
    for n, k in {**single, **bank}.items():
        w = wg_per_cu(n)
        print(n, k["vgpr_count"], w)
        assert k["vgpr_count"] <= 512 // w, (n, k)                            # the SIMD's 512 registers per lane, one wave per workgroup
        assert k["group_segment_fixed_size"] == 36992, (n, k)                 # exchange buffer + the two tables, as the FIR kernels
        assert k["group_segment_fixed_size"] <= 160 * 1024 // w, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        assert no_scratch_memory(k), (n, k)
    # the figures DESIGN.md 4.23 records: the general keep-predicate and the NCO cost 4 VGPRs on complex64 with the mixer (174 -> 178),
    # and every instantiation keeps the workgroups per CU of its FIR / bank counterpart
    vg = {(("I16" if "OlsInI16" in n else "C64"), "ELb1EE" in n): k["vgpr_count"] for n, k in single.items()}
    assert vg[("C64", True)] > 168 and vg[("C64", False)] <= 168 and vg[("I16", True)] <= 168 and vg[("I16", False)] <= 168, vg
    for n, k in bank.items():
        assert k["vgpr_count"] > 512 // 3, (n, k)                             # ... and the bank does not declare fewer than it could have


def test_the_new_names_keep_clear_of_the_counted_fragments_and_the_old_kernels_are_what_they_were(kernels):  # noqa: F811
    new = [n for n in kernels if "ddc" in n.lower()]
    assert len(new) == 6, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n, (n, fragment)
    # the FIR and channel-bank instantiations: their count and the figures test_fir_code_objects / test_fir_bank_code_objects hold
    fir = {n: k for n, k in kernels.items() if "ols4096_kernel" in n}
    assert len(fir) == 4 and len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    for n, k in fir.items():
        w = 2 if "OlsInC64" in n and "ELb1EE" in n else 3
        assert k["vgpr_count"] <= 512 // w and k["group_segment_fixed_size"] == 36992 and no_scratch_memory(k), (n, k)
    assert sorted(k["vgpr_count"] for k in fir.values()) == [132, 148, 158, 174], fir   # ols4096.hip's own comment
    old_bank = {n: k for n, k in kernels.items() if "chanbank_kernel" in n}
    assert len(old_bank) == 2
    for n, k in old_bank.items():
        assert 512 // 3 < k["vgpr_count"] <= 256 and k["group_segment_fixed_size"] == 36992 and no_scratch_memory(k), (n, k)
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4 and len([n for n in kernels if "xspec" in n]) == 8

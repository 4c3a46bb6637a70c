"""What the compiler made of the channel-bank kernel, read from the ELF notes of the gfx950 code objects inside the built
libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): two instantiations (complex64 /
int16 input), each within the registers and the LDS of the workgroups per CU its __launch_bounds__ declares, no scratch memory —
and the new names keep clear of the fragments by which the other code-object tests count theirs."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("integrate", "ci16", "kgroup", "pfb", "fft_lds", "fft4096_kernel", "fft4096_features_kernel", "sk4096", "sk_rows",
         "sk_finalize", "xspec", "row_pass", "col_pass", "4096")
WG_PER_CU = 2    # chanbank_wg_per_cu() of ols_bank.hip, both formats


def test_both_instantiations_fit_the_workgroups_per_cu_they_declare(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "chanbank_kernel" in n}
    assert len(hits) == 2, sorted(hits)                                       # complex64 / int16
    assert len([n for n in hits if "OlsInI16" in n]) == 1 and len([n for n in hits if "OlsInC64" in n]) == 1, sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 512 // WG_PER_CU, (n, k)                    # the SIMD's 512 registers per lane, one wave per workgroup
        assert k["vgpr_count"] > 512 // (WG_PER_CU + 1), (n, k)               # ... and it does not declare fewer than it could have
        assert k["group_segment_fixed_size"] == 36992, (n, k)                 # exchange buffer + the two tables; H comes from global memory
        assert k["group_segment_fixed_size"] <= 160 * 1024 // WG_PER_CU, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        assert no_scratch_memory(k), (n, k)


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "chanbank" in n]
    assert len(new) == 2, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n, (n, fragment)
    # and what the other tests count is what it was
    assert len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    assert len([n for n in kernels if "ols4096_kernel" in n]) == 4
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "integrate_rows_kernel" in n]) == 3
    assert len([n for n in kernels if "integrate_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "fft4096_kgroup_ci16_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4
    assert len([n for n in kernels if "sk4096_kernel" in n]) == 4
    assert len([n for n in kernels if "sk_rows_kernel" in n]) == 1 and len([n for n in kernels if "sk_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "xspec" in n]) == 8

"""What the compiler made of the overlap-save FIR kernel, read from the ELF notes of the gfx950 code objects inside the built
libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): four instantiations (complex64 /
int16 input x mixer on / off), each within the registers and the LDS of the workgroups per CU its __launch_bounds__ declares, no
scratch memory — and the new names keep clear of the fragments by which the other code-object tests count theirs."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("integrate", "ci16", "kgroup", "pfb", "fft_lds", "fft4096_kernel", "fft4096_features_kernel", "sk4096", "sk_rows",
         "sk_finalize", "xspec", "row_pass", "col_pass")


def wg_per_cu(name):
    """ols_wg_per_cu() of ols4096.hip: two for complex64 input with the mixer, three for the rest."""
    return 2 if "OlsInC64" in name and "ELb1EE" in name else 3


def test_every_instantiation_fits_the_workgroups_per_cu_it_declares(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "ols4096_kernel" in n}
    assert len(hits) == 4, sorted(hits)                                       # complex64 / int16 x mixer on / off
    assert len([n for n in hits if "OlsInI16" in n]) == 2 and len([n for n in hits if "OlsInC64" in n]) == 2, sorted(hits)
    assert len([n for n in hits if "ELb1EE" in n]) == 2, sorted(hits)
    for n, k in hits.items():
        w = wg_per_cu(n)
        assert k["vgpr_count"] <= 512 // w, (n, k)                            # the SIMD's 512 registers per lane, one wave per workgroup
        assert k["group_segment_fixed_size"] == 36992, (n, k)                 # exchange buffer + the two tables; H stays in registers
        assert k["group_segment_fixed_size"] <= 160 * 1024 // w, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        assert no_scratch_memory(k), (n, k)
    assert sum(wg_per_cu(n) == 2 for n in hits) == 1


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "ols" in n.lower() and "4096" in n]
    assert len(new) == 4, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n, (n, fragment)
    # and what the other tests count is what it was
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "integrate_rows_kernel" in n]) == 3
    assert len([n for n in kernels if "integrate_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "fft4096_kgroup_ci16_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4
    assert len([n for n in kernels if "sk4096_kernel" in n]) == 4
    assert len([n for n in kernels if "sk_rows_kernel" in n]) == 1 and len([n for n in kernels if "sk_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "xspec" in n]) == 8

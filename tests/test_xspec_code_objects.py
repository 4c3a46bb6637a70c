"""What the compiler made of the two-channel cross-spectrum kernels, read from the ELF notes of the gfx950 code objects inside
the built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): the N = 4096 kernel
with its 64 sums per thread is built for two workgroups per CU — at most 256 VGPRs, half of the LDS, no scratch — and the new
kernels' names keep clear of the fragments by which the other code-object tests count theirs."""
from tests.code_objects import kernels, no_scratch, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("integrate", "ci16", "kgroup", "pfb", "fft_lds", "fft4096_kernelILb", "sk4096_kernel", "sk_rows_kernel", "sk_finalize_kernel")
WG_PER_CU = 2          # __launch_bounds__(256, 2) in xspec4096.hip


def test_the_fused_kernel_fits_the_two_workgroups_per_cu_it_declares(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "xspec4096_kernel" in n}
    assert len(hits) == 4, sorted(hits)                                       # complex64 / int16 x window on / off
    assert len([n for n in hits if "I16" in n]) == 2 and len([n for n in hits if "ELb1EE" in n]) == 2, sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 512 // WG_PER_CU, (n, k)                    # the SIMD's 512 registers per lane, one wave per workgroup
        assert k["group_segment_fixed_size"] == (53376 if "ELb1EE" in n else 36992), (n, k)   # exchange + tables (+ window)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // WG_PER_CU, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        # no scratch memory and no vector register spilled (the unit bookkeeping overflows the scalar file, as in the
        # integrating kernels; the compiler parks those values in the lanes of a vector register: no memory behind that)
        assert no_scratch_memory(k), (n, k)


def test_the_split_the_column_kernel_and_the_finalize_do_not_spill(kernels):  # noqa: F811
    split = [k for n, k in kernels.items() if "xspec_split_kernel" in n]
    rows = [k for n, k in kernels.items() if "xspec_rows_kernel" in n]
    fin = [k for n, k in kernels.items() if "xspec_finalize_kernel" in n]
    assert len(split) == 2 and len(rows) == 1 and len(fin) == 1               # (the split: complex64 and int16 elements)
    assert all(no_scratch(k) for k in split + rows + fin)


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "xspec" in n]
    assert len(new) == 8, sorted(new)
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

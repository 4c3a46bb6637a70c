"""What the compiler made of the spectral-kurtosis kernels, read from the ELF notes of the gfx950 code objects inside the built
libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): the N = 4096 kernel with its 32
sums per thread fits three workgroups per CU — at most 168 VGPRs, a third of the LDS, no scratch — and the new kernels' names
keep clear of the fragments by which the other code-object tests count theirs."""
from tests.code_objects import kernels, no_scratch, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("integrate", "ci16", "kgroup", "pfb", "fft_lds", "fft4096_kernelILb")


def test_the_fused_kernel_fits_three_workgroups_per_cu(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "sk4096_kernel" in n}
    assert len(hits) == 4, sorted(hits)                                       # complex64 / int16 x window on / off
    assert len([n for n in hits if "I16" in n]) == 2 and len([n for n in hits if "ELb1EE" in n]) == 2, sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)
        assert k["group_segment_fixed_size"] == (53376 if "ELb1EE" in n else 36992), (n, k)   # exchange + tables (+ window)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // 3, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        # no scratch memory and no vector register spilled (the unit bookkeeping overflows the scalar file, as in the
        # integrating kernels; the compiler parks those values in the lanes of a vector register: no memory behind that)
        assert no_scratch_memory(k), (n, k)


def test_the_column_kernel_and_the_finalize_do_not_spill(kernels):  # noqa: F811
    rows = [k for n, k in kernels.items() if "sk_rows_kernel" in n]
    fin = [k for n, k in kernels.items() if "sk_finalize_kernel" in n]
    assert len(rows) == 1 and len(fin) == 1
    assert all(no_scratch(k) for k in rows + fin)


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "sk4096_kernel" in n or "sk_rows_kernel" in n or "sk_finalize_kernel" in n]
    assert len(new) == 6, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n, (n, fragment)
    # and what the other tests count is what it was
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "integrate_rows_kernel" in n]) == 3
    assert len([n for n in kernels if "integrate_finalize_kernel" in n]) == 1
    assert len([n for n in kernels if "fft4096_kgroup_ci16_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4

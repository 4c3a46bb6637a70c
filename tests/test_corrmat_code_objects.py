"""What the compiler made of the correlation-matrix kernels, read from the ELF notes of the gfx950 code objects inside the built
libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): the instantiation counts, the
budget the N = 4096 spectra kernel declares — three workgroups per CU: at most 168 VGPRs, a third of the LDS, no scratch — the
column kernel without scratch at every channel count, and the new kernels' names clear of the fragments by which the other
code-object tests count theirs, whose counts are what they were."""
from tests.code_objects import kernels, no_scratch, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("xspec", "integrate", "kgroup", "ci16", "ci8", "_iq8_", "pfb", "fft_lds", "ols", "ddc", "downconv", "chanbank", "sk4096",
         "sk_rows", "sk_finalize", "fft4096_kernelILb", "fft4096_ticket_kernel", "fft4096_rot_kernel")
WG_PER_CU = 3          # __launch_bounds__(256, 3) in corrmat4096.hip


def test_the_spectra_kernel_fits_the_three_workgroups_per_cu_it_declares(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "corrmat4096_spectra_kernel" in n}
    assert len(hits) == 6, sorted(hits)                                       # complex64 / int16 / 8-bit x window on / off
    for policy in ("CmInC64", "CmInS16", "CmInB8"):
        assert len([n for n in hits if policy in n]) == 2, (policy, sorted(hits))
    assert len([n for n in hits if "ELb1EE" in n]) == 3, sorted(hits)
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168 and k["vgpr_count"] <= 512 // WG_PER_CU, (n, k)   # 512 registers per lane of a SIMD
        assert k["group_segment_fixed_size"] == (53376 if "ELb1EE" in n else 36992), (n, k)   # exchange + tables (+ window)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // WG_PER_CU, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)
        assert no_scratch(k), (n, k)


def test_the_column_kernel_has_no_scratch_at_any_channel_count(kernels):  # noqa: F811
    rows = {n: k for n, k in kernels.items() if "corrmat_rows_kernel" in n}
    assert len(rows) == 7, sorted(rows)                                       # C = 2 .. 8
    for c in range(2, 9):
        hit = [k for n, k in rows.items() if f"kernelILi{c}E" in n]
        assert len(hit) == 1, (c, sorted(rows))
        # (at C >= 5 the plane offsets overflow the scalar file; the compiler parks those in the lanes of a vector register:
        # no memory behind that)
        assert no_scratch_memory(hit[0]) and hit[0]["vgpr_count"] <= 128, (c, hit[0])


def test_the_split_and_the_finalize_do_not_spill(kernels):  # noqa: F811
    split = [k for n, k in kernels.items() if "corrmat_split_kernel" in n]
    fin = [k for n, k in kernels.items() if "corrmat_finalize_kernel" in n]
    assert len(split) == 3 and len(fin) == 1                                  # (the split: complex64, int16 and 8-bit; the sign at run time)
    assert all(no_scratch(k) for k in split + fin)


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "corrmat" in n]
    assert len(new) == 6 + 7 + 3 + 1, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n, (n, fragment)
        assert "ols" not in n.lower() and "ddc" not in n.lower() and "downconv" not in n.lower(), n
    # and what the other tests count is what it was
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    assert count("fft4096_integrate_kernelILb") == 6 and count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("fft4096_kgroup_ci16_kernelILb") == 6 and count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("sk4096_kernel") == 4 and count("sk_rows_kernel") == 1 and count("sk_finalize_kernel") == 1
    assert count("xspec") == 8 and count("xspec4096_kernel") == 4
    assert count("ci8") == 11 and count("ols4096_kernel") == 4 and count("pfb4096_groups_kernel") == 3
    assert count("pfb4096_kernelILi") == 2 and count("pfb_fold_kernel") == 1
    assert len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    assert len([n for n in kernels if "ddc" in n.lower()]) == 6 and len([n for n in kernels if "downconv" in n.lower()]) == 3

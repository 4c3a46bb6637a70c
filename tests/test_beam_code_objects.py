"""What the compiler made of the filter-and-sum beamformer's kernel, read from the ELF notes of the gfx950 code objects inside the
built libsdrk.so (no GPU needed; the extraction of tests/code_objects.py; no disassembly is searched): six instantiations (three
input formats x mixer on / off), each within the registers and the LDS of the two workgroups per CU its __launch_bounds__
declares, no scratch memory, no spilled VGPR — and the new names keep clear of the fragments by which the other code-object tests
count theirs, whose counts are what they were.

Measured at this commit (VGPRs, mixer on / off): complex64 187 / 187, int16 189 / 188, 8-bit 193 / 193; 36,992 B of LDS each."""
from tests.code_objects import kernels, no_scratch_memory  # noqa: F401  (the fixture)

TAKEN = ("ddc", "downconv", "chanbank", "corrmat", "xspec", "ci8", "ci16", "pfb", "sk4096", "integrate", "kgroup", "fft_lds",
         "fft4096", "ols", "4096", "row_pass", "col_pass")
WG_PER_CU = 2    # BEAM_WG_PER_CU of beamsum.hip, every instantiation
VGPRS = {("BeamInC64", "Lb1"): 187, ("BeamInC64", "Lb0"): 187, ("BeamInS16", "Lb1"): 189, ("BeamInS16", "Lb0"): 188,
         ("BeamInB8", "Lb1"): 193, ("BeamInB8", "Lb0"): 193}
SLACK = 8        # a compiler update may move a figure by a few registers; the budget below is the hard limit


def _beam(kernels):  # noqa: F811
    return {n: k for n, k in kernels.items() if "beamsum_kernel" in n}


def test_six_instantiations_fit_the_two_workgroups_per_cu_they_declare(kernels):  # noqa: F811
    hits = _beam(kernels)
    assert len(hits) == 6, sorted(hits)
    for (policy, mix), measured in VGPRS.items():
        mine = [k for n, k in hits.items() if policy in n and mix + "EE" in n]
        assert len(mine) == 1, (policy, mix, sorted(hits))
        k = mine[0]
        assert k["vgpr_count"] <= 512 // WG_PER_CU, k                          # the SIMD's 512 registers per lane, one wave per workgroup
        assert k["vgpr_count"] > 512 // (WG_PER_CU + 1), k                     # ... and three workgroups per CU would not have fitted
        assert abs(k["vgpr_count"] - measured) <= SLACK, (k, measured)
        assert k["group_segment_fixed_size"] == 36992, k                       # exchange buffer + the two tables; H comes from global memory
        assert k["group_segment_fixed_size"] <= 160 * 1024 // WG_PER_CU, k
        assert k["max_flat_workgroup_size"] == 256, k
        assert no_scratch_memory(k), k


def test_the_new_names_keep_clear_of_the_counted_fragments(kernels):  # noqa: F811
    new = [n for n in kernels if "beam" in n.lower()]
    assert len(new) == 6, sorted(new)
    for n in new:
        for fragment in TAKEN:
            assert fragment not in n.lower(), (n, fragment)
    # and what the other tests count is what it was
    assert len([n for n in kernels if "ols" in n.lower() and "4096" in n]) == 4
    assert len([n for n in kernels if "ols4096_kernel" in n]) == 4
    assert len([n for n in kernels if "chanbank_kernel" in n]) == 2
    assert len([n for n in kernels if "ddc_kernel" in n]) == 4 and len([n for n in kernels if "ddcbank_kernel" in n]) == 2
    assert len([n for n in kernels if "downconv" in n]) == 3
    assert len([n for n in kernels if "corrmat4096_spectra_kernel" in n]) == 6
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4
    assert len([n for n in kernels if "sk4096_kernel" in n]) == 4
    assert len([n for n in kernels if "xspec" in n]) == 8

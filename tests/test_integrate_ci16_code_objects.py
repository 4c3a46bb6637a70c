"""What the compiler made of the int16 integrate kernel (csrc/fft4096_kgroup_ci16.hip), read from the ELF notes of the gfx950
code objects inside the built libsdrk.so (no GPU needed; notes only, nothing is disassembled): six instantiations, each within
the budget of three workgroups per CU — at most 168 VGPRs, a third of the LDS, no scratch, no spilled VGPR — and, with a
prefetch of 16 words where the complex64 kernel holds 32, fewer registers than that kernel."""
import re

from tests.code_objects import kernels  # noqa: F401  (the fixture)


def test_the_six_kernels_fit_three_workgroups_per_cu(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "fft4096_kgroup_ci16_kernelILb" in n}
    assert len(hits) == 6, sorted(hits)                                    # window on / off x mean / max / min
    assert sorted(re.search(r"ILb([01])ELi([012])EE", n).groups() for n in hits) == [(w, d) for w in "01" for d in "012"]
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)
        assert k["group_segment_fixed_size"] == (53376 if "ILb1E" in n else 36992), (n, k)   # exchange + tables (+ window)
        assert k["group_segment_fixed_size"] <= 160 * 1024 // 3, (n, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert k.get("sgpr_spill_count", 0) <= 16, (n, k)               # scalar values parked in VGPR lanes: no memory behind
    # the compensation is what the mean pays over max / min, as in the complex64 kernel
    mean = max(k["vgpr_count"] for n, k in hits.items() if "ELi0EE" in n)
    hold = max(k["vgpr_count"] for n, k in hits.items() if "ELi0EE" not in n)
    assert hold < mean, (hold, mean)


def test_fewer_registers_than_the_complex64_kernel(kernels):  # noqa: F811
    new = [k["vgpr_count"] for n, k in kernels.items() if "fft4096_kgroup_ci16_kernelILb" in n]
    c64 = [k["vgpr_count"] for n, k in kernels.items() if "fft4096_integrate_kernelILb" in n]
    assert len(new) == 6 and len(c64) == 6
    print(f"VGPRs: int16 {sorted(new)}, complex64 {sorted(c64)}")
    assert max(new) < max(c64), (new, c64)


def test_the_names_stay_out_of_the_other_kernels_counts(kernels):  # noqa: F811
    """The suite counts kernels by substrings of their mangled names; the new ones must fall under none of them."""
    for n in kernels:
        if "kgroup_ci16" in n:
            for taken in ("integrate", "fft4096_ci16_kernelILb", "fft4096_kernelILb", "unpack_ci16_kernel", "synth_fill_ci16_kernel"):
                assert taken not in n, (n, taken)
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_ci16_kernelILb" in n]) == 8
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4

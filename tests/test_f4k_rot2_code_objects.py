"""The look-ahead-two instantiations of the flagship kernel (fft4096_rot2_kernel, csrc/fft4096.hip) keep the budgets of the
grid-stride form: three workgroups per CU need at most 128 VGPRs and a third of the 160 KiB of LDS, and nothing spills."""
from tests.code_objects import code_objects, kernels, no_scratch  # noqa: F401  (fixtures)


def test_rot2_kernels_fit_three_workgroups_per_cu(kernels):  # noqa: F811
    ks = [k for n, k in kernels.items() if "fft4096_rot2_kernelILb" in n]
    assert len(ks) == 4, [k["name"] for k in ks]           # window yes/no x log-PSD/complex
    for k in ks:
        assert k["vgpr_count"] <= 128, k
        assert no_scratch(k), k
        assert k["group_segment_fixed_size"] * 3 <= 160 * 1024, k
        assert k["max_flat_workgroup_size"] == 256, k

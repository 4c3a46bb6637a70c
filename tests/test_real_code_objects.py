"""What the compiler made of the real-input kernels, read from the ELF notes of the gfx950 code objects inside the built
libsdrk.so (no GPU needed; the extraction of tests/code_objects.py): rspec4096_kernel (pair format x window x epilogue: 12 —
the 8-bit format is a run-time argument and adds none), real_pairs_kernel (pair format: 3) and real_split_kernel (epilogue: 2)
exist under those names, carry the recorded figures with no scratch, and leave every count the existing code-object tests
assert as it was.  No disassembly is searched."""
import re

from tests.code_objects import kernels, no_scratch  # noqa: F401  (the fixture)

LDS_RSPEC = 36992          # exchange buffer + the two tables; the window is read from global memory
# vgpr_count as recorded, by (pair format, window, epilogue): float32 / int16 / bytes, no window / window, dB / complex64
VGPRS = {("0", "0", "0"): 148, ("0", "0", "1"): 148, ("0", "1", "0"): 162, ("0", "1", "1"): 164,
         ("1", "0", "0"): 124, ("1", "0", "1"): 126, ("1", "1", "0"): 148, ("1", "1", "1"): 164,
         ("2", "0", "0"): 124, ("2", "0", "1"): 126, ("2", "1", "0"): 148, ("2", "1", "1"): 150}
COUNTED = ("ci16", "ci8", "iq8", "fft4096_kernelILb", "integrate", "pfb", "ols", "sk4096", "sk_rows", "xspec", "chanbank", "ddc",
           "beam", "corrmat", "f4k_", "unpack", "fft4096_")


def test_the_twelve_fused_kernels_keep_three_workgroups_per_cu_without_scratch(kernels):  # noqa: F811
    hits = {n: k for n, k in kernels.items() if "rspec4096_kernel" in n}
    keys = {re.search(r"kernelILi(\d)ELb(\d)ELi(\d)EE", n).groups(): n for n in hits}
    assert sorted(keys) == sorted(VGPRS), sorted(hits)
    for key, n in keys.items():
        k = hits[n]
        assert k["vgpr_count"] == VGPRS[key] and k["vgpr_count"] <= 168, (n, k)      # 168: three workgroups of 256 per CU
        assert k["group_segment_fixed_size"] == LDS_RSPEC and 3 * LDS_RSPEC <= 160 * 1024, (n, k)
        assert no_scratch(k), (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_the_staged_kernels_exist_once_per_choice_without_scratch_or_lds(kernels):  # noqa: F811
    pairs = {n: k for n, k in kernels.items() if "real_pairs_kernel" in n}
    split = {n: k for n, k in kernels.items() if "real_split_kernel" in n}
    assert sorted(re.search(r"kernelILi(\d)EE", n).group(1) for n in pairs) == ["0", "1", "2"], sorted(pairs)
    assert sorted(re.search(r"kernelILi(\d)EE", n).group(1) for n in split) == ["0", "1"], sorted(split)
    for n, k in {**pairs, **split}.items():
        assert no_scratch(k) and k["group_segment_fixed_size"] == 0 and k["vgpr_count"] <= 32, (n, k)


def test_every_count_of_the_existing_code_object_tests_still_holds(kernels):  # noqa: F811
    def count(fragment):
        return len([n for n in kernels if fragment in n])

    new = [n for n in kernels if "rspec4096" in n or "real_pairs" in n or "real_split" in n]
    assert len(new) == 17, new
    for n in new:
        for fragment in COUNTED:
            assert fragment not in n, (n, fragment)
    assert len(kernels) == 353 + 17
    assert count("fft4096_ci16_kernelILb") == 8 and count("fft4096_kernelILb") == 4
    assert count("fft4096_ci8_kernel") == 4 and count("fft4096_kgroup_ci8_kernel") == 6 and count("unpack_ci8_kernel") == 1
    assert count("fft4096_integrate_kernelILb") == 6 and count("fft4096_kgroup_ci16_kernelILb") == 6
    assert count("integrate_rows_kernel") == 3 and count("integrate_finalize_kernel") == 1
    assert count("unpack_ci16_kernel") == 1 and count("synth_fill_ci16_kernel") == 1
    assert count("pfb4096_kernelILi") == 2 and count("pfb4096_groups_kernel") == 3 and count("pfb_fold_kernel") == 1
    assert count("sk4096_kernel") == 4 and count("sk_rows_kernel") == 1 and count("sk_finalize_kernel") == 1
    assert count("xspec") == 8 and count("ols4096_kernel") == 4 and count("chanbank_kernel") == 2

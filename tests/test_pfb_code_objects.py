"""What the compiler made of the polyphase-filter-bank kernels, read from the ELF notes of the gfx950 code objects inside the
built libsdrk.so (no GPU needed; the extraction of tests/test_code_objects.py): pfb4096_kernel keeps the budgets of three
workgroups per CU and the LDS of the window-less N = 4096 kernels, and neither kernel uses scratch."""
import os
import re
import shutil
import subprocess

import pytest

from sdr_iq_visualizer_amd import _ffi

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    lib = _ffi.library_path()
    tools = [os.path.join(LLVM, t) for t in ("llvm-objdump", "llvm-readelf")]
    if not (os.path.exists(lib) and all(os.path.exists(t) for t in tools)):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    work = tmp_path_factory.mktemp("co_pfb")
    shutil.copy(lib, work / "libsdrk.so")
    subprocess.run([tools[0], "--offloading", "libsdrk.so"], cwd=work, check=True, capture_output=True)
    # a kernel's keys come sorted: .group_segment_fixed_size stands BEFORE its .name, the other figures after it
    rows, cur, lds = [], None, None
    for co in sorted(work.glob("libsdrk.so.*gfx950*")):
        notes = subprocess.run([tools[1], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            m = re.match(r"\s*\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s*(\S+)", ln)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                if not m.group(2).startswith("_Z"):
                    continue
                cur = {"name": m.group(2), "group_segment_fixed_size": lds}
                lds = None
                rows.append(cur)
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
    return {r["name"]: r for r in rows if "vgpr_count" in r}


def test_pfb4096_kernels_keep_three_workgroups_per_cu(kernels):
    hits = {n: k for n, k in kernels.items() if "pfb4096_kernelILi" in n}
    assert sorted(re.search(r"pfb4096_kernelILi(\d)EE", n).group(1) for n in hits) == ["0", "1"], sorted(hits)   # both epilogues
    for n, k in hits.items():
        assert k["vgpr_count"] <= 168, (n, k)                       # 512 / 3 waves per SIMD
        assert k["group_segment_fixed_size"] == 36992, (n, k)       # exchange buffer + the two tables, no window
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)


def test_pfb_fold_kernel_has_no_scratch(kernels):
    hits = [k for n, k in kernels.items() if "pfb_fold_kernel" in n]
    assert len(hits) == 1, sorted(n for n in kernels if "pfb" in n)
    assert hits[0]["private_segment_fixed_size"] == 0 and hits[0]["vgpr_spill_count"] == 0, hits[0]


def test_new_kernel_names_stay_out_of_the_existing_counts(kernels):
    for n in kernels:
        if "pfb" in n:
            for fragment in ("fft4096_kernelILb", "integrate", "ci16", "kgroup", "fft_lds"):
                assert fragment not in n, (n, fragment)

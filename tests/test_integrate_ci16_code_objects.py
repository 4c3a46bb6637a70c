"""What the compiler made of the int16 integrate kernel (csrc/fft4096_kgroup_ci16.hip), read from the ELF notes of the gfx950
code objects inside the built libsdrk.so (no GPU needed; notes only, nothing is disassembled): six instantiations, each within
the budget of three workgroups per CU — at most 168 VGPRs, a third of the LDS, no scratch, no spilled VGPR — and, with a
prefetch of 16 words where the complex64 kernel holds 32, fewer registers than that kernel."""
import os
import re
import shutil
import subprocess

import pytest

from sdr_iq_visualizer_amd import _ffi

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = "name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: its note fields} of every kernel in the library."""
    lib = _ffi.library_path()
    tools = [os.path.join(LLVM, t) for t in ("llvm-objdump", "llvm-readelf")]
    if not (os.path.exists(lib) and all(os.path.exists(t) for t in tools)):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    work = tmp_path_factory.mktemp("co_integrate_ci16")
    shutil.copy(lib, work / "libsdrk.so")
    subprocess.run([tools[0], "--offloading", "libsdrk.so"], cwd=work, check=True, capture_output=True)
    rows, cur, lds = [], None, None      # (the notes list a kernel's fields alphabetically: the LDS size comes before its name)
    for co in sorted(work.glob("libsdrk.so.*gfx950*")):
        notes = subprocess.run([tools[1], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            m = re.match(rf"\s*\.({FIELDS}):\s*(\S+)", ln)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                if not m.group(2).startswith("_Z"):
                    continue
                cur = {"name": m.group(2), "group_segment_fixed_size": lds}
                rows.append(cur)
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
    return {r["name"]: r for r in rows if "vgpr_count" in r}


def test_the_six_kernels_fit_three_workgroups_per_cu(kernels):
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


def test_fewer_registers_than_the_complex64_kernel(kernels):
    new = [k["vgpr_count"] for n, k in kernels.items() if "fft4096_kgroup_ci16_kernelILb" in n]
    c64 = [k["vgpr_count"] for n, k in kernels.items() if "fft4096_integrate_kernelILb" in n]
    assert len(new) == 6 and len(c64) == 6
    print(f"VGPRs: int16 {sorted(new)}, complex64 {sorted(c64)}")
    assert max(new) < max(c64), (new, c64)


def test_the_names_stay_out_of_the_other_kernels_counts(kernels):
    """The suite counts kernels by substrings of their mangled names; the new ones must fall under none of them."""
    for n in kernels:
        if "kgroup_ci16" in n:
            for taken in ("integrate", "fft4096_ci16_kernelILb", "fft4096_kernelILb", "unpack_ci16_kernel", "synth_fill_ci16_kernel"):
                assert taken not in n, (n, taken)
    assert len([n for n in kernels if "fft4096_integrate_kernelILb" in n]) == 6
    assert len([n for n in kernels if "fft4096_ci16_kernelILb" in n]) == 8
    assert len([n for n in kernels if "fft4096_kernelILb" in n]) == 4

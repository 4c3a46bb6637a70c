"""What the compiler made of the integrated real-input kernel (csrc/rspec4096_groups.hip), read from the ELF notes of the
gfx950 code objects inside the built companion library libsdrk_ext.so (no GPU needed; notes only, nothing is disassembled):
18 instantiations — pair format x window x detector; the 8-bit signedness is a run-time argument — each within the budget of
three workgroups per CU (at most 168 VGPRs, at most 54,613 B of LDS, no scratch, no spilled VGPR), with the VGPR counts as
compiled; and libsdrk.so keeps the 370 kernels its own code-object tests count."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from sdr_iq_visualizer_amd import _ffi
from tests.code_objects import FIELDS, OBJDUMP, READELF, kernels  # noqa: F401  (the fixture, of libsdrk.so)

EXT = os.path.join(os.path.dirname(_ffi.library_path()), "libsdrk_ext.so")
LDS = 36992 + 16384 + 8    # exchange buffer and tables, the state plane, bin 4096's state
# vgpr_count as compiled, by (pair format, window, detector): float32 / int16 / bytes, no window / window, mean / max / min
VGPRS = {("0", "0", "0"): 135, ("0", "0", "1"): 121, ("0", "0", "2"): 121, ("0", "1", "0"): 135, ("0", "1", "1"): 123, ("0", "1", "2"): 123,
         ("1", "0", "0"): 121, ("1", "0", "1"): 107, ("1", "0", "2"): 107, ("1", "1", "0"): 123, ("1", "1", "1"): 107, ("1", "1", "2"): 107,
         ("2", "0", "0"): 122, ("2", "0", "1"): 108, ("2", "0", "2"): 108, ("2", "1", "0"): 127, ("2", "1", "1"): 108, ("2", "1", "2"): 108}


@functools.lru_cache(maxsize=None)
def _ext_kernels():
    """{mangled name: its note fields} of every kernel in libsdrk_ext.so."""
    rows, cur, early = [], None, {}
    with tempfile.TemporaryDirectory(prefix="sdrk_ext_co_") as work:
        shutil.copy(EXT, os.path.join(work, "libsdrk_ext.so"))
        subprocess.run([OBJDUMP, "--offloading", "libsdrk_ext.so"], cwd=work, check=True, capture_output=True)
        for co in sorted(f for f in os.listdir(work) if f.startswith("libsdrk_ext.so.") and "gfx950" in f):
            notes = subprocess.run([READELF, "--notes", os.path.join(work, co)], check=True, capture_output=True, text=True).stdout
            for ln in notes.splitlines():   # a kernel's keys come sorted: two of the figures stand before its name, the rest after it
                m = re.match(rf"\s*\.({FIELDS}):\s*(\S+)", ln)
                if not m:
                    continue
                if m.group(1) in ("group_segment_fixed_size", "max_flat_workgroup_size"):
                    early[m.group(1)] = int(m.group(2))
                elif m.group(1) == "name":
                    if m.group(2).startswith("_Z"):
                        cur = {"name": m.group(2), **early}
                        early = {}
                        rows.append(cur)
                elif cur is not None:
                    cur[m.group(1)] = int(m.group(2))
    return {r["name"]: r for r in rows if "vgpr_count" in r}


@pytest.fixture(scope="module")
def ext_kernels():
    if not all(os.path.exists(p) for p in (EXT, OBJDUMP, READELF)):
        pytest.skip("needs the built companion library and the ROCm LLVM tools")
    return _ext_kernels()


def test_the_eighteen_kernels_keep_three_workgroups_per_cu_without_scratch(ext_kernels):
    hits = {n: k for n, k in ext_kernels.items() if "rspec4096_groups_kernel" in n}
    keys = {re.search(r"kernelILi(\d)ELb(\d)ELi(\d)EE", n).groups(): n for n in hits}
    assert sorted(keys) == sorted(VGPRS) and len(hits) == 18, sorted(hits)
    print({key: hits[n]["vgpr_count"] for key, n in sorted(keys.items())})
    for key, n in keys.items():
        k = hits[n]
        assert k["vgpr_count"] == VGPRS[key] and k["vgpr_count"] <= 168, (n, k)      # 168: three workgroups of 256 per CU
        assert k["group_segment_fixed_size"] == LDS and LDS <= 54613, (n, k)         # 54,613 = 160 KiB / 3
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert k.get("sgpr_spill_count", 0) <= 18, (n, k)       # scalar values parked in VGPR lanes: no memory behind them
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_the_companion_library_holds_nothing_else_and_libsdrk_keeps_its_count(ext_kernels, kernels):  # noqa: F811
    assert len(ext_kernels) == 18, sorted(ext_kernels)
    assert len(kernels) == 353 + 17
    assert not [n for n in kernels if "rspec4096_groups" in n]

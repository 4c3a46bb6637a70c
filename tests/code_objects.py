"""The gfx950 code objects inside the built libsdrk.so and what their ELF notes say of every kernel, for the code-object tests
(test_*code_objects.py): extracted and read once per pytest process, whichever tests ask, and handed out as the fixtures
`code_objects` and `kernels`, which those tests import by name.  No GPU needed."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from sdr_iq_visualizer_amd import _ffi

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP, READELF = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
FIELDS = "name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|max_flat_workgroup_size"


@functools.lru_cache(maxsize=None)
def _extracted():
    """(directory, paths of the gfx950 code objects); the directory lives as long as the cache entry."""
    work = tempfile.TemporaryDirectory(prefix="sdrk_co_")
    shutil.copy(_ffi.library_path(), os.path.join(work.name, "libsdrk.so"))
    subprocess.run([OBJDUMP, "--offloading", "libsdrk.so"], cwd=work.name, check=True, capture_output=True)
    return work, tuple(sorted(os.path.join(work.name, f) for f in os.listdir(work.name) if f.startswith("libsdrk.so.") and "gfx950" in f))


@functools.lru_cache(maxsize=None)
def _notes():
    # a kernel's keys come sorted: .group_segment_fixed_size stands BEFORE its .name, the other figures after it
    rows, cur, lds = [], None, None
    for co in _extracted()[1]:
        notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
        for ln in notes.splitlines():
            m = re.match(rf"\s*\.({FIELDS}):\s*(\S+)", ln)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                if not m.group(2).startswith("_Z"):      # argument names share the key
                    continue
                cur = {"name": m.group(2), "group_segment_fixed_size": lds}
                lds = None
                rows.append(cur)
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
    return {r["name"]: r for r in rows if "vgpr_count" in r}


def _need_library_and_tools():
    if not all(os.path.exists(p) for p in (_ffi.library_path(), OBJDUMP, READELF)):
        pytest.skip("needs the built library and the ROCm LLVM tools")


@pytest.fixture(scope="module")
def code_objects():
    """The paths of the extracted code objects (for the tests that disassemble them)."""
    _need_library_and_tools()
    return list(_extracted()[1])


@pytest.fixture(scope="module")
def kernels():
    """{mangled name: its note fields} of every kernel in the library."""
    _need_library_and_tools()
    return _notes()


def no_scratch(k):
    """No scratch memory, no spilled VGPR, no spilled SGPR."""
    return k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k.get("sgpr_spill_count", 0) == 0


def no_scratch_memory(k):
    """No scratch memory and no spilled VGPR (SGPRs parked in the lanes of a VGPR have no memory behind them)."""
    return k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0

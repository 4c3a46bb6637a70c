"""The double-precision path without a GPU: what the compiler made of csrc/fft_f64.hip (read from the gfx950 code objects in the
built libsdrk.so), and the host-side rules of precision= (validation, the "auto" dtype rule, non-power-of-two lengths refused before
any device call)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd import spectrum as sp

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def f64_code(tmp_path_factory):
    """name -> (notes dict, disassembly text) of every fft_f64 kernel in the library."""
    lib = _ffi.library_path()
    if not (os.path.exists(lib) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    work = tmp_path_factory.mktemp("co64")
    shutil.copy(lib, work / "libsdrk.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "libsdrk.so"], cwd=work, check=True, capture_output=True)
    notes, dis = {}, {}
    for co in sorted(work.glob("libsdrk.so.*gfx950*")):
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                             text=True).stdout
        cur = None
        for ln in txt.splitlines():
            m = re.match(r"\s*\.(name|private_segment_fixed_size|vgpr_spill_count|group_segment_fixed_size):\s*(\S+)", ln)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "fft_f64_kernel" in m.group(2) else None
                if cur:
                    notes[cur] = {}
            elif cur:
                notes[cur][m.group(1)] = int(m.group(2))
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(co)], check=True, capture_output=True, text=True).stdout
        cur = None
        for ln in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
            if m:
                cur = m.group(1) if "fft_f64_kernel" in m.group(1) else None
                if cur:
                    dis[cur] = []
            elif cur:
                dis[cur].append(ln)
    return notes, {k: "\n".join(v) for k, v in dis.items()}


def _inst(notes, ln, mode, epi):
    frag = f"fft_f64_kernelILi{ln}ELi{mode}ELi{epi}E"
    hits = [n for n in notes if frag in n]
    assert hits, frag
    return hits[0]


def test_f64_kernels_cover_every_size_class_without_scratch(f64_code):
    notes, dis = f64_code
    # one pass: every length 2 ... 4096, both epilogues; two passes: column lengths 2^6 ... 2^11, row lengths 2^7 ... 2^11
    want = [(ln, 0, epi) for ln in range(1, 13) for epi in (0, 1)] + [(ln, 1, 1) for ln in range(6, 12)] + \
           [(ln, 2, epi) for ln in range(7, 12) for epi in (0, 1)]
    for ln, mode, epi in want:
        name = _inst(notes, ln, mode, epi)
        k = notes[name]
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (name, k)
        assert k.get("group_segment_fixed_size", 0) <= 64 * 1024, (name, k)       # two workgroups per CU
        assert "v_fma_f64" in dis[name] or "v_mul_f64" in dis[name], name
    for name in (_inst(notes, 12, 0, 0), _inst(notes, 11, 1, 1), _inst(notes, 11, 2, 0)):
        assert "v_fma_f64" in dis[name], name                                     # double arithmetic, fused where written so
        assert "scratch_" not in dis[name], name


def test_precision_argument_and_auto_rule():
    r = sp.resolve_precision
    assert r("single") == "single" and r("double") == "double"
    for dt in (np.complex64, np.float32, np.float16):
        assert r("auto", np.zeros(4, dt)) == "single", dt
    for dt in (np.complex128, np.float64, np.int16, np.int32, np.int64, np.uint8):
        assert r("auto", np.zeros(4, dt)) == "double", dt
    assert r("auto", [1 + 2j, 3j]) == "double"                  # what numpy makes of a Python list
    with pytest.raises(ValueError):
        r("half")
    with pytest.raises(ValueError):
        sp.SpectrumPlan(4096, precision="quad")


@pytest.mark.parametrize("n", [3, 1000, 4097, 100000, 1 << 23])
def test_double_rejects_non_power_of_two_before_any_device_call(n, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_ffi, "require_device", no_device)
    monkeypatch.setattr(_ffi, "lib", no_device)
    x = np.zeros(n, np.complex128) if n < (1 << 23) else np.zeros(4, np.complex128)
    with pytest.raises(ValueError, match="powers of two 2..2\\^22"):
        sp.SpectrumPlan(n, precision="double")
    if n < (1 << 23):
        with pytest.raises(ValueError, match="powers of two"):
            pkg.spectrum_db(x, precision="double")
        with pytest.raises(ValueError, match="powers of two"):
            pkg.spectrum_db(x, precision="auto")
        with pytest.raises(ValueError, match="powers of two"):
            pkg.stft_db(np.zeros(2 * n, np.complex128), n, precision="double")
        with pytest.raises(ValueError, match="powers of two"):
            pkg.fft_c128(x)


def test_double_refuses_float32_only_options_and_sharding(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_ffi, "require_device", no_device)
    monkeypatch.setattr(_ffi, "lib", no_device)
    for kw in ({"fused64k": True}, {"fused64k": False}, {"overlap_passes": True}, {"tune_staging": True}):
        with pytest.raises(ValueError, match="float32 plans only"):
            sp.SpectrumPlan(65536, precision="double", **kw)
    x = np.zeros((2, 4096), np.complex128)
    with pytest.raises(ValueError, match="devices"):
        pkg.spectrum_db(x, devices=[0, 1], precision="double")
    with pytest.raises(ValueError, match="devices"):
        pkg.spectrum_db(x, devices=[0, 1], precision="auto")
    with pytest.raises(ValueError, match="devices"):
        pkg.stft_db(x.reshape(-1), 4096, devices=[0, 1], precision="double")


def test_public_names():
    assert "fft_c128" in pkg.__all__ and callable(pkg.fft_c128)
    names = {s[0] for s in _ffi.SYMBOLS}
    for s in ("sdrk_plan_create_f64", "sdrk_plan_precision", "sdrk_exec_host_f64", "sdrk_exec_fft_host_f64",
              "sdrk_exec_device_f64", "sdrk_exec_device_f64_timed_each"):
        assert s in names

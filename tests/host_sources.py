"""How the host side of the C ABI is built for the sanitizer legs (test_host_sanitizers.py, test_host_sanitizers_f64.py,
test_host_sanitizers_modes.py): which files it is made of, one g++ build of them per sanitizer and pytest process, and each
driver (a stand-alone program on tests/host_stress.h) linked against it once per sanitizer, whichever tests ask for it."""
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdr-iq-visualizer_amd", "csrc")

# The host translation units among the Makefile's SRCS: the files without a kernel (test_host_sources.py holds the list to that).
HOST_SOURCES = ("sdrk_api.hip", "sdrk_plan.hip", "sdrk_host_pipeline.hip", "sdrk_features.hip", "sdrk_waterfall.hip",
                "sdrk_probes.hip", "sdrk_f64.hip", "ci16_api.hip", "integrate_api.hip", "pfb_api.hip", "fir_api.hip")

SANITIZERS = {"tsan": ("-fsanitize=thread",),
              "asan_ubsan": ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")}


def makefile_sources():
    """The SRCS of csrc/Makefile, in its order."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        return re.search(r"^SRCS\s*:=\s*(.+)$", f.read(), re.M).group(1).split()


def kernel_stand_ins():
    """The stand-in kernels every build links: the launchers of the real kernel files, as host functions."""
    return [os.path.join(HERE, "fake_hip", "fake_kernels.cpp"), *sorted(glob.glob(os.path.join(HERE, "fake_*_kernels.cpp")))]


def _gxx(san):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    return [gxx, "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(HERE, "fake_hip"), *SANITIZERS[san]]


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@functools.lru_cache(maxsize=None)
def _common_objects(san):
    """(directory, objects): every host source and every stand-in compiled under `san`, once per process."""
    out = tempfile.TemporaryDirectory(prefix=f"sdrk_{san}_")     # lives as long as the cache entry
    objs = []
    for i, src in enumerate([*(os.path.join(CSRC, s) for s in HOST_SOURCES), *kernel_stand_ins()]):
        objs.append(os.path.join(out.name, f"{i}.o"))
        _run(_gxx(san) + (["-x", "c++"] if src.endswith(".hip") else []) + ["-c", src, "-o", objs[-1]])
    return out, tuple(objs)


@functools.lru_cache(maxsize=None)
def build_driver(san, driver):
    """tests/<driver> (a stand-alone program) compiled under sanitizer `san` ("tsan" / "asan_ubsan") and linked with the host
    side against the stand-in runtime of tests/fake_hip -> the path of the program."""
    out, objs = _common_objects(san)
    stem = os.path.join(out.name, os.path.splitext(driver)[0])
    _run(_gxx(san) + ["-c", os.path.join(HERE, driver), "-o", stem + ".o"])
    _run(_gxx(san) + [*objs, stem + ".o", "-ldl", "-o", stem])
    return stem


def build_drivers(driver):
    """{sanitizer: program} for both sanitizers."""
    return {san: build_driver(san, driver) for san in SANITIZERS}

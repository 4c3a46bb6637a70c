"""Sanitizer legs for the host side of the polyphase-filter-bank entry points (CPU).

csrc/pfb_api.hip with the host files csrc/sdrk_*.hip, compiled with g++ against the stand-in runtime of tests/fake_hip and the
stand-in kernels of tests/fake_pfb_kernels.cpp beside fake_kernels.cpp and fake_f64_kernels.cpp (the driver also hands an f64
plan to the entry points), driven by tests/host_api_pfb_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan
with leak checking: the device and host entries at N = 4096 and at staged lengths, the overlap every chunk of the numpy boundary
carries, pageable and pinned arrays, staging growing under work in flight, two streams on one plan, a chirp-z length, set_pfb
between calls, and the refusals — three threads on their own plans, every output element checked."""
import os
import shutil
import subprocess

import pytest

from tests.host_sources import CSRC, host_sources

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pfb_binaries(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san_pfb")
    srcs = [*(("-x c++", src) for src in host_sources(f64=True)), ("-x c++", os.path.join(CSRC, "pfb_api.hip")),
            ("", os.path.join(HERE, "fake_hip", "fake_kernels.cpp")), ("", os.path.join(HERE, "fake_f64_kernels.cpp")),
            ("", os.path.join(HERE, "fake_pfb_kernels.cpp")), ("", os.path.join(HERE, "host_api_pfb_stress.cpp"))]
    built = {}
    for name, flags in (("tsan", ["-fsanitize=thread"]),
                        ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        common = [gxx, "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(HERE, "fake_hip"), *flags]
        objs = []
        for i, (lang, src) in enumerate(srcs):
            obj = str(out / f"{name}_{i}.o")
            r = subprocess.run(common + lang.split() + ["-c", src, "-o", obj], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            objs.append(obj)
        exe = str(out / f"host_api_pfb_{name}")
        r = subprocess.run(common + objs + ["-ldl", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        built[name] = exe
    return built


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_pfb_host_entry_points_under_sanitizers(pfb_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([pfb_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 pfb threads=3" in r.stdout

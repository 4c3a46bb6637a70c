"""Sanitizer legs for the host side of the double-precision entry points (CPU).

csrc/sdrk_f64.hip and the other host files csrc/sdrk_*.hip (whose numpy-boundary pipeline the f64 calls share, with 16-byte
samples) compiled with
g++ against the stand-in runtime of tests/fake_hip and the stand-in f64 launcher of tests/fake_f64_kernels.cpp, driven by
tests/host_api_f64_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking: the small call,
chunked calls from pageable and from pinned arrays, two threads on their own plans, and the refusals across precisions."""
import os
import shutil
import subprocess

import pytest

from tests.host_sources import host_sources

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def f64_binaries(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san_f64")
    srcs = [*(("-x c++", src) for src in host_sources(f64=True)),
            ("", os.path.join(HERE, "fake_hip", "fake_kernels.cpp")), ("", os.path.join(HERE, "fake_f64_kernels.cpp")),
            ("", os.path.join(HERE, "host_api_f64_stress.cpp"))]
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
        exe = str(out / f"host_api_f64_{name}")
        r = subprocess.run(common + objs + ["-ldl", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        built[name] = exe
    return built


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_f64_host_entry_points_under_sanitizers(f64_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([f64_binaries[san], "2", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 f64 threads=2" in r.stdout

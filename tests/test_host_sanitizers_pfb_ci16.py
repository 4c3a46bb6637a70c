"""Sanitizer legs for the host side of the int16 polyphase-filter-bank entry points (CPU).

csrc/pfb_ci16_api.hip with csrc/pfb_api.hip, csrc/pfb_groups_api.hip, csrc/integrate_api.hip, the int16 host files and
csrc/sdrk_*.hip, compiled with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels of
tests/fake_pfb_ci16_kernels.cpp beside the existing ones, driven by the stand-alone program tests/host_api_pfb_ci16_stress.cpp
under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking (nothing is loaded into Python, nothing preloaded):
per-frame and integrated entries, device and host, at N = 4096, a staged length and a chirp-z length, K that does not divide a
chunk's frames, pageable and pinned arrays, two streams on one plan, set_pfb between calls, the refusals — three threads on
their own plans, every output element checked."""
import os
import shutil
import subprocess

import pytest

from tests.host_sources import CSRC, host_sources

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pfb_ci16_binaries(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("san_pfb_ci16")
    srcs = [*(("-x c++", src) for src in host_sources(f64=True)),
            *(("-x c++", os.path.join(CSRC, f)) for f in ("pfb_ci16_api.hip", "pfb_groups_api.hip", "pfb_api.hip", "integrate_api.hip", "kgroup_ci16_api.hip", "ci16_api.hip")),
            ("", os.path.join(HERE, "fake_hip", "fake_kernels.cpp")), ("", os.path.join(HERE, "fake_f64_kernels.cpp")),
            ("", os.path.join(HERE, "fake_pfb_kernels.cpp")), ("", os.path.join(HERE, "fake_integrate_kernels.cpp")),
            ("", os.path.join(HERE, "fake_pfb_groups_kernels.cpp")), ("", os.path.join(HERE, "fake_pfb_ci16_kernels.cpp")),
            ("", os.path.join(HERE, "fake_ci16_kernels.cpp")), ("", os.path.join(HERE, "fake_kgroup_ci16_kernels.cpp")),
            ("", os.path.join(HERE, "host_api_pfb_ci16_stress.cpp"))]
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
        exe = str(out / f"host_api_pfb_ci16_{name}")
        r = subprocess.run(common + objs + ["-ldl", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        built[name] = exe
    return built


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_pfb_ci16_host_entry_points_under_sanitizers(pfb_ci16_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([pfb_ci16_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 pfb_ci16 threads=3" in r.stdout

"""Sanitizer legs for the host side of the int16 integrated-spectrum entry points (CPU).

csrc/integrate_api.hip (the int16 entries beside the complex64 ones on the same csrc/integrate_call.h), csrc/ci16_api.hip
(launch_ci16: the transform of the staged lengths) and the other host files of csrc/ (tests/host_sources.py), compiled with g++ against the stand-in
runtime of tests/fake_hip and the stand-in kernels of tests/fake_kgroup_ci16_kernels.cpp beside the existing
fake_integrate_kernels.cpp, fake_ci16_kernels.cpp and fake_f64_kernels.cpp (the driver also hands an f64 plan to the entry
points), driven by tests/host_api_integrate_ci16_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak
checking: the device and host entries at the fused length and at staged ones, groups and slices carried across chunk and
staging boundaries, pageable and pinned arrays, state and staging growing under work in flight, two streams on one plan, the
complex64 entry between int16 calls on one plan, and the refusals — three threads on their own plans, every output element
checked."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def integrate_ci16_binaries():
    return build_drivers("host_api_integrate_ci16_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_integrate_ci16_host_entry_points_under_sanitizers(integrate_ci16_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([integrate_ci16_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 integrate_ci16 threads=3" in r.stdout

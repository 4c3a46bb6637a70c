"""Sanitizer legs for the host side of the integrated-spectrum entry points (CPU).

csrc/integrate_api.hip and the other host files of csrc/ (tests/host_sources.py; whose staging slots and copy streams the host entry shares) compiled
with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels of tests/fake_integrate_kernels.cpp (and
fake_f64_kernels.cpp: the driver also hands an f64 plan to the entry points), driven by tests/host_api_integrate_stress.cpp
under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking: the device and host entries at the fused and the
staged lengths, groups and slices carried across chunk and staging boundaries, pageable and pinned arrays, state and staging
growing under work in flight, two streams on one plan, and the refusals — three threads on their own plans, every output
element checked."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def integrate_binaries():
    return build_drivers("host_api_integrate_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_integrate_host_entry_points_under_sanitizers(integrate_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([integrate_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 integrate threads=3" in r.stdout

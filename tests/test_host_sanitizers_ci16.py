"""Sanitizer legs for the host side of the int16 entry points (CPU).

csrc/ci16_api.hip and the other host files of csrc/ (tests/host_sources.py; whose numpy-boundary pipeline the ci16 calls share, with 4-byte samples)
compiled with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels of tests/fake_ci16_kernels.cpp (and
fake_f64_kernels.cpp: the driver also hands an f64 plan to the int16 entry points), driven
by tests/host_api_ci16_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking: the small call,
zero-copy chunks, the pipeline from pageable and pinned arrays with ragged tails, the widening staging in several chunks with
halo, its growth under work in flight, and the refusals — three threads on their own plans, every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def ci16_binaries():
    return build_drivers("host_api_ci16_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_ci16_host_entry_points_under_sanitizers(ci16_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([ci16_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 ci16 threads=3" in r.stdout

"""Sanitizer legs for the host side of the double-precision entry points (CPU).

csrc/sdrk_f64.hip and the other host files of csrc/ (tests/host_sources.py; whose numpy-boundary pipeline the f64 calls share, with 16-byte
samples) compiled with
g++ against the stand-in runtime of tests/fake_hip and the stand-in f64 launcher of tests/fake_f64_kernels.cpp, driven by
tests/host_api_f64_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking: the small call,
chunked calls from pageable and from pinned arrays, two threads on their own plans, and the refusals across precisions."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def f64_binaries():
    return build_drivers("host_api_f64_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_f64_host_entry_points_under_sanitizers(f64_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([f64_binaries[san], "2", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 f64 threads=2" in r.stdout

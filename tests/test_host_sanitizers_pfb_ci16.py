"""Sanitizer legs for the host side of the int16 polyphase-filter-bank entry points (CPU).

csrc/pfb_api.hip and csrc/integrate_api.hip (the int16 entries) with the other host files of csrc/
(tests/host_sources.py), compiled with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels of
tests/fake_pfb_ci16_kernels.cpp beside the existing ones, driven by the stand-alone program tests/host_api_pfb_ci16_stress.cpp
under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking (nothing is loaded into Python, nothing preloaded):
per-frame and integrated entries, device and host, at N = 4096, a staged length and a chirp-z length, K that does not divide a
chunk's frames, pageable and pinned arrays, two streams on one plan, set_pfb between calls, the refusals — three threads on
their own plans, every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def pfb_ci16_binaries():
    return build_drivers("host_api_pfb_ci16_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_pfb_ci16_host_entry_points_under_sanitizers(pfb_ci16_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([pfb_ci16_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 pfb_ci16 threads=3" in r.stdout

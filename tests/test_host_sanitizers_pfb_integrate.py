"""Sanitizer legs for the host side of the integrated polyphase-filter-bank entry points (CPU).

csrc/integrate_api.hip (the PFB entries) with csrc/pfb_api.hip and the other host files of csrc/ (tests/host_sources.py), compiled with g++
against the stand-in runtime of tests/fake_hip and the stand-in kernels of tests/fake_pfb_groups_kernels.cpp beside
fake_pfb_kernels.cpp, fake_integrate_kernels.cpp, fake_kernels.cpp and fake_f64_kernels.cpp (the driver also hands an f64 plan
to the entry points), driven by tests/host_api_pfb_integrate_stress.cpp under ThreadSanitizer and under AddressSanitizer +
UBSan with leak checking: the device and host entries at N = 4096, at a staged length and at a chirp-z length, K that does not
divide a chunk's frames (units carried across chunks together with the T - 1 blocks of overlap), split calls with few groups,
pageable and pinned arrays, two streams on one plan, set_pfb between calls, and the refusals — three threads on their own
plans, every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import build_drivers


@pytest.fixture(scope="module")
def pfb_integrate_binaries():
    return build_drivers("host_api_pfb_integrate_stress.cpp")


@pytest.mark.parametrize("san", ["tsan", "asan_ubsan"])
def test_pfb_integrate_host_entry_points_under_sanitizers(pfb_integrate_binaries, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([pfb_integrate_binaries[san], "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 pfb_integrate threads=3" in r.stdout

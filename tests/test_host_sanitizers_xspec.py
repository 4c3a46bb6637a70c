"""Sanitizer legs for the host side of the two-channel cross-spectrum entry points (CPU).

csrc/integrate_api.hip (on csrc/integrate_call.h, which now also carries the width of a unit's state and the column kernel over
two staged spectra) and the other host files of csrc/ (tests/host_sources.py), compiled with g++ against the stand-in runtime of
tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_xspec_kernels.cpp among them), driven by the stand-alone
program tests/host_api_xspec_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking.  Nothing is
loaded into Python, nothing is preloaded.  Three threads on their own plans; both formats; device, timed and host entries at
N = 4096 and at a staged length; groups and slices carried across chunk and staging boundaries; four planes per group, every
output element checked; the refusals; an existing integrated call between cross-spectrum calls on one plan."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_xspec_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_xspec_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 xspec threads=3" in r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 50_000_000, r.stdout                     # (all four planes of every case, from every thread)

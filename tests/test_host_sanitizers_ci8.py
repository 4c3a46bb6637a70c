"""Sanitizer legs for the host side of the 8-bit entry points (CPU).

csrc/ci16_api.hip (launch_ci8, its unpack route through the staging the int16 route uses, the four per-frame entries) and
csrc/integrate_api.hip (the three integrated entries) with the other host files of csrc/ (tests/host_sources.py), compiled with
g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_ci8_kernels.cpp among
them), driven by the stand-alone program tests/host_api_ci8_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan
with leak checking.  Nothing is loaded into Python, nothing is preloaded.  Three threads on their own plans; both formats;
per-frame and integrated host calls across several chunks, pageable and pinned; the unpack route with two staging chunks; the
refusals; an int16 call between 8-bit calls on one plan; every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_ci8_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_ci8_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 ci8 threads=3" in r.stdout
    assert int(r.stdout.split("refused=")[1].split()[0]) >= 70, r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 250_000_000, r.stdout                    # (every case of both formats, from every thread: 270,584,576)

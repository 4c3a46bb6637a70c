"""Sanitizer legs for the host side of the correlation-matrix entry points (CPU).

csrc/integrate_api.hip (on csrc/integrate_call.h, which now also carries the channel count of an element: channels^2 floats of
unit state and as many planes, channels staged spectra per frame) and the other host files of csrc/ (tests/host_sources.py),
compiled with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp
(fake_corrmat_kernels.cpp among them), driven by the stand-alone program tests/host_api_corrmat_stress.cpp under ThreadSanitizer
and under AddressSanitizer + UBSan with leak checking.  Nothing is loaded into Python, nothing is preloaded.  Three threads on
their own plans; complex64, int16 and both 8-bit formats; C = 2, 3 and 8; device, timed and host entries at N = 4096 and at a
staged length; streams that start a sample, not an element, into their buffer; groups and slices carried across chunk and staging
boundaries; every output element of all planes checked; the refusals; existing integrated and two-channel calls between
correlation-matrix calls on one plan."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_corrmat_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_corrmat_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 corrmat threads=3" in r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 100_000_000, r.stdout                    # (all planes of every case, from every thread)
    assert int(r.stdout.split("refused=")[1].split()[0]) >= 4 * 13 * 3 + 9, r.stdout

"""Sanitizer legs for the host side of the real-input entry points (CPU).

csrc/ci16_api.hip (sdrk_plan_set_real_window, launch_real and its staged route, the four exec entries) on the numpy boundary of
csrc/sdrk_host_pipeline.hip (rows of nfft + 1 bins) with the other host files of csrc/ (tests/host_sources.py), compiled with
g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_real_kernels.cpp among
them), driven by the stand-alone program tests/host_api_real_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan
with leak checking.  Nothing is loaded into Python, nothing is preloaded.  Three threads on their own plans; the four formats;
device, timed and host entries in both output forms, pageable and pinned, across several host chunks and two staging chunks;
every refusal; a plain complex64 call between real calls on one plan; every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_real_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_real_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 real threads=3" in r.stdout
    assert int(r.stdout.split("refused=")[1].split()[0]) == 59, r.stdout    # (11 bad argument lists x 4 entries + 15 more)
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 400_000_000, r.stdout                    # (every case of the four formats, from every thread: 441,238,626)

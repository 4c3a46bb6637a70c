"""Sanitizer legs for the host side of the integrated real-input entry points (CPU).

csrc/ci16_api.hip (sdrk_exec_*_real_integrated) on the call machinery of csrc/integrate_call.h with rows, carry rows and partial
rows of nfft + 1 bins, with the other host files of csrc/ (tests/host_sources.py), compiled with g++ against the stand-in runtime
of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_real_groups_kernels.cpp among them), driven by the
stand-alone program tests/host_api_real_groups_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak
checking.  Nothing is loaded into Python, nothing is preloaded.  Three threads on their own plans; the four formats, the three
detectors, both output forms, K in {1, 2, 3, 7}; device, timed and host entries, pageable and pinned; a host call of more than
two 16 MiB chunks whose boundaries cut groups; two staging chunks; split groups; every refusal; a per-frame real call and a
complex integrated call between real-integrated calls on one plan; every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver

COMPARED = 29_290_519   # output elements of the driver's table: the refusals' two cases and three workers' cases


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_real_integrated_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_real_groups_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 real_groups threads=3" in r.stdout
    assert int(r.stdout.split("refused=")[1].split()[0]) == 61, r.stdout    # (17 bad argument lists x 3 entries + 10 more)
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared == COMPARED, r.stdout

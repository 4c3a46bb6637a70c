"""Sanitizer legs for the host side of the filter-and-sum beamformer's entry points (CPU).

csrc/fir_api.hip (sdrk_plan_set_beam, sdrk_exec_device_beam*, sdrk_exec_host_beam* on the down-converter's chunk loop and the
pinned staging slots) and the other host files of csrc/ (tests/host_sources.py), compiled with g++ against the stand-in runtime of
tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_beam_kernels.cpp among them: the real block geometry, one
forward transform per block and channel, the shared arithmetic of csrc/kernels_beam.h), driven by the stand-alone program
tests/host_api_beam_stress.cpp under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking.  Nothing is loaded into
Python, nothing is preloaded.  Three threads on their own plans; complex64, int16, ci8 and cu8; device, timed and host entries;
chunks of three blocks with D = 7; sample0 near 2^40; C = 1, 3 and 8; every output compared with the device entry, the integer
formats with complex64 on the widened elements, C = 1 with the down-converter; every refusal; a DDC call between beam calls."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_beam_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3", SDRK_FIR_CHUNK_BLOCKS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_beam_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 beam threads=3" in r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 2_000_000, r.stdout                                   # (the cases are fixed; every thread runs all of them)
    assert int(r.stdout.split("refused=")[1].split()[0]) == 26              # (every refusal of refusals())

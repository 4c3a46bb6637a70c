"""Sanitizer legs for the host side of the 8-bit filter-bank and spectral-kurtosis entry points (CPU).

csrc/pfb_api.hip (launch_pfb_iq8_fn, the four per-frame entries) and csrc/integrate_api.hip (pfb_iq8_io, sk_iq8_io,
sk_pfb_iq8_io and the nine entries behind them) with the other host files of csrc/ (tests/host_sources.py), compiled with g++
against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_iq8_modes_kernels.cpp
among them), driven by the stand-alone program tests/host_api_iq8_modes_stress.cpp under ThreadSanitizer and under
AddressSanitizer + UBSan with leak checking.  Nothing is loaded into Python, nothing is preloaded.  Two threads on their own
plans (and the library's three helper threads); both formats; per-frame, integrated and kurtosis host calls across several
chunks with the overlap and the carry each takes along, pageable and pinned; the staged lengths with two staging chunks; calls in flight together on one plan; the
refusals; every output element compared with the complex64 entry of the same plan on the widened samples."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_iq8_modes_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_iq8_modes_stress.cpp"), "2", "1"], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 iq8_modes threads=2" in r.stdout
    assert int(r.stdout.split("refused=")[1].split()[0]) >= 125, r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 105_000_000, r.stdout                    # (every case of both formats, from every thread: 109,885,585)

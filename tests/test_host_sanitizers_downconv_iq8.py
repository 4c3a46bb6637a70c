"""Sanitizer legs for the host side of the 8-bit down-converter's entry points (CPU).

csrc/fir_api.hip (sdrk_exec_*_downconv_iq8, sdrk_exec_*_downconvbank_iq8: the format value of ddc_launch and of the chunk loop on the
pinned staging slots, the NULL prefix of bytes 0 / 0x80) and the other host files of csrc/ (tests/host_sources.py), compiled with g++
against the stand-in runtime of tests/fake_hip and the stand-in kernels tests/fake_*_kernels.cpp (fake_downconv_iq8_kernels.cpp
among them), driven by the stand-alone program tests/host_api_downconv_iq8_stress.cpp under ThreadSanitizer and under
AddressSanitizer + UBSan with leak checking.  Nothing is loaded into Python, nothing is preloaded.  Three threads on their own
plans; both formats; device, timed and host entries; chunks of three blocks with D = 7; sample0 near 2^40; C = 1, 3 and 64; a NULL
and a given prefix; a final block shorter than 4096; every output compared with the complex64 stand-in call on the widened samples;
the refusals."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver


@pytest.mark.parametrize("san", list(SANITIZERS))
def test_downconv_iq8_host_entry_points_under_sanitizers(san):
    env = dict(os.environ, SDRK_HOST_THREADS="3", SDRK_FIR_CHUNK_BLOCKS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_downconv_iq8_stress.cpp"), "3", "1"], capture_output=True, text=True, env=env,
                       timeout=900)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and "sdrk 500 downconv_iq8 threads=3" in r.stdout
    compared = int(r.stdout.split("compared=")[1].split()[0])
    assert compared > 1_400_000, r.stdout                                   # (the cases are fixed; every thread runs all of them)
    assert int(r.stdout.split("refused=")[1].split()[0]) == 76             # (every refusal of refusals() in the driver)


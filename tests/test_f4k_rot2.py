"""csrc/f4k_rot.h at look-ahead two (CPU): the dealer of fft4096_rot2_kernel, draw early and late — every frame claimed exactly
once under any interleaving of the workgroups, nothing past the end, at most two tickets held beyond the frame transformed,
the heads in step, heads and exit counter zero after every call, call after call — tests/f4k_rot2_test.cpp, a stand-alone
program, built with AddressSanitizer + UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_rot2_order_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "f4k_rot2_test")
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(HERE, "f4k_rot2_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "bad=0" in r.stdout and "f4k_rot2 cases=" in r.stdout

"""Sanitizer legs for the host side of the int16, polyphase-filter-bank (PFB) and integrated entry points (CPU).

csrc/ci16_api.hip, csrc/pfb_api.hip, csrc/integrate_api.hip (on csrc/integrate_call.h) and the other host files of csrc/
(tests/host_sources.py), compiled with g++ against the stand-in runtime of tests/fake_hip and the stand-in kernels
tests/fake_*_kernels.cpp (fake_f64_kernels.cpp among them: every leg also hands an f64 plan to its entry points), driven by
the stand-alone program tests/host_api_modes_stress.cpp — one mode table, one set of case bodies, one table of cases per
leg — under ThreadSanitizer and under AddressSanitizer + UBSan with leak checking.  Nothing is loaded into Python, nothing is
preloaded.  Every leg: three threads on their own plans, the refusals, every output element checked."""
import os
import subprocess

import pytest

from tests.host_sources import SANITIZERS, build_driver

# leg -> what it covers
LEGS = {
    "ci16": """int16 per frame (csrc/ci16_api.hip, whose numpy-boundary pipeline the calls share with 4-byte samples; stand-ins
        fake_ci16_kernels.cpp): the small call, zero-copy chunks, the pipeline from pageable and pinned arrays with ragged tails,
        the widening staging in several chunks with halo, its growth under work in flight.""",
    "integrate": """complex64 integrated (csrc/integrate_api.hip, whose host entry shares the staging slots and copy streams;
        stand-ins fake_integrate_kernels.cpp): the device and host entries at the fused and the staged lengths, groups and slices
        carried across chunk and staging boundaries, pageable and pinned arrays, state and staging growing under work in flight,
        two streams on one plan.""",
    "integrate_ci16": """int16 integrated (the int16 entries beside the complex64 ones on the same csrc/integrate_call.h, and
        csrc/ci16_api.hip's launch_ci16 for the staged lengths; stand-ins fake_kgroup_ci16_kernels.cpp beside
        fake_integrate_kernels.cpp and fake_ci16_kernels.cpp): the device and host entries at the fused length and at staged
        ones, groups and slices carried across chunk and staging boundaries, pageable and pinned arrays, state and staging
        growing under work in flight, two streams on one plan, the complex64 entry between int16 calls on one plan.""",
    "pfb": """complex64 PFB per frame (csrc/pfb_api.hip; stand-ins fake_pfb_kernels.cpp beside fake_kernels.cpp): the device and
        host entries at N = 4096 and at staged lengths, the overlap every chunk of the numpy boundary carries, pageable and
        pinned arrays, staging growing under work in flight, two streams on one plan, a chirp-z length, set_pfb between calls.""",
    "pfb_integrate": """complex64 PFB integrated (the PFB entries of csrc/integrate_api.hip with csrc/pfb_api.hip; stand-ins
        fake_pfb_groups_kernels.cpp beside fake_pfb_kernels.cpp and fake_integrate_kernels.cpp): the device and host entries at
        N = 4096, at a staged length and at a chirp-z length, K that does not divide a chunk's frames (units carried across
        chunks together with the T - 1 blocks of overlap), split calls with few groups, pageable and pinned arrays, two streams
        on one plan, set_pfb between calls.""",
    "pfb_ci16": """int16 PFB, per frame and integrated (the int16 entries of csrc/pfb_api.hip and csrc/integrate_api.hip;
        stand-ins fake_pfb_ci16_kernels.cpp beside the others): device and host, at N = 4096, a staged length and a chirp-z
        length, K that does not divide a chunk's frames, pageable and pinned arrays, two streams on one plan, set_pfb between
        calls.""",
}


@pytest.mark.parametrize("san", list(SANITIZERS))
@pytest.mark.parametrize("leg", list(LEGS))
def test_mode_host_entry_points_under_sanitizers(leg, san):
    env = dict(os.environ, SDRK_HOST_THREADS="3",
               TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([build_driver(san, "host_api_modes_stress.cpp"), leg, "3", "1"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    assert "bad=0" in r.stdout and f"sdrk 500 {leg} threads=3" in r.stdout

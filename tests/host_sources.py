"""Which files make up the host side of the C ABI, for the g++ builds of the sanitizer tests (test_host_sanitizers*.py)."""
import glob
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr-iq-visualizer_amd", "csrc")


def host_sources(f64):
    """Every csrc/sdrk_*.hip: the host translation units (the kernels are in the other .hip files).  Without `f64`,
    sdrk_f64.hip is left out: it needs the stand-in f64 launcher (fake_f64_kernels.cpp), which only the f64 driver links."""
    srcs = sorted(glob.glob(os.path.join(CSRC, "sdrk_*.hip")))
    assert os.path.join(CSRC, "sdrk_f64.hip") in srcs and len(srcs) >= 7, srcs
    return [s for s in srcs if f64 or os.path.basename(s) != "sdrk_f64.hip"]

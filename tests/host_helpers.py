"""What the host-side (no GPU) tests of the PFB corners share (test_pfb_host, test_pfb_integrate_host, test_pfb_ci16_host)."""
import ctypes

from sdr_iq_visualizer_amd.spectrum import SpectrumPlan


def bare_plan(nfft, taps=0, wkey="rect", double=False):
    """A SpectrumPlan object without a device behind it: what the argument checks look at."""
    p = object.__new__(SpectrumPlan)
    p.nfft, p.pfb_taps, p._wkey, p._double = nfft, taps, wkey, double
    p._handle = ctypes.c_void_p()
    return p

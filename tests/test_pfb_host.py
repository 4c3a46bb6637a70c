"""CPU: the Python side of the polyphase filter bank — the default prototype against its formula, the frame arithmetic, the
argument errors raised before any device call, and the ABI table (tests/test_abi.py checks header = table = exports)."""
import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, spectrum
from sdr_iq_visualizer_amd.spectrum import pfb_prototype
from tests.host_helpers import bare_plan


@pytest.mark.parametrize("nfft,taps", [(64, 1), (64, 16), (1000, 3), (4096, 4), (4096, 32)])
def test_prototype_is_the_windowed_sinc_rounded_once(nfft, taps):
    h = pfb_prototype(nfft, taps)
    n = taps * nfft
    m = np.arange(n, dtype=np.float64)
    arg = (m - (n - 1) / 2.0) / nfft
    want = np.where(arg == 0, 1.0, np.sin(np.pi * arg) / np.where(arg == 0, 1.0, np.pi * arg)) * (0.5 - 0.5 * np.cos(2 * np.pi * m / (n - 1)))
    assert h.dtype == np.float32 and h.shape == (n,)
    assert np.abs(h.astype(np.float64) - want).max() <= 2.0 ** -24          # half an ulp of values up to 1, plus numpy's sinc
    assert np.array_equal(h, h[::-1])                                         # linear phase
    assert h[0] == 0.0 and abs(float(h[n // 2]) - 1.0) < 1e-3
    assert np.array_equal(pfb_prototype(nfft, taps, "hann"), h)


def test_prototype_windows_and_errors():
    assert np.array_equal(pfb_prototype(8, 2, None), np.sinc((np.arange(16) - 7.5) / 8).astype(np.float32))
    assert np.array_equal(pfb_prototype(8, 2, np.full(16, 2.0)), (2 * np.sinc((np.arange(16) - 7.5) / 8)).astype(np.float32))
    assert pfb_prototype(8, 2, "blackman").shape == (16,)
    for bad in (dict(nfft=8, taps=0), dict(nfft=8, taps=33), dict(nfft=1, taps=2), dict(nfft=8, taps=2, window="kaiser"),
                dict(nfft=8, taps=2, window=np.ones(8))):
        with pytest.raises(ValueError):
            pfb_prototype(**bad)


def test_frame_arithmetic():
    p = bare_plan(1024, taps=4)
    assert p.pfb_frames(4095) == 0 and p.pfb_frames(4096) == 1 and p.pfb_frames(4096 + 1023) == 1 and p.pfb_frames(5120) == 2
    assert p.pfb_frames(4096 + 10, hop=1) == 11 and p.pfb_frames(10 * 1024, hop=1500) == 1 + (10240 - 4096) // 1500
    with pytest.raises(ValueError):
        p.pfb_frames(8192, hop=0)
    with pytest.raises(ValueError, match="set_pfb"):
        bare_plan(1024).pfb_frames(8192)


def test_argument_errors_come_before_any_device_call():
    with pytest.raises(ValueError, match="rectangular"):
        bare_plan(64, wkey="hann").set_pfb(np.ones(128, np.float32))
    with pytest.raises(ValueError, match="double"):
        bare_plan(64, double=True).set_pfb(np.ones(128, np.float32))
    for h in (np.ones(100, np.float32), np.ones((2, 64), np.float32), np.ones(0, np.float32), np.ones(33 * 64, np.float32)):
        with pytest.raises(ValueError):
            bare_plan(64).set_pfb(h)
    for call in (lambda p: p.pfb_db(np.zeros(256, np.complex64)), lambda p: p.pfb_fft(np.zeros(256, np.complex64)),
                 lambda p: p.exec_device_pfb(0, 1, 0), lambda p: p.exec_device_pfb_timed_each(0, 1, 0)):
        with pytest.raises(ValueError, match="set_pfb"):
            call(bare_plan(64))
    with pytest.raises(ValueError):
        spectrum.pfb_db(np.zeros(1024, np.complex64), 64, 4, prototype=np.ones(64, np.float32))
    with pytest.raises(ValueError):
        spectrum.pfb_db(np.zeros(1024, np.complex64), 64, 0)


def test_abi_table_and_exports():
    lib = _ffi.lib()
    table = {name: (res, args) for name, res, args in _ffi.SYMBOLS}
    for name, nargs in (("sdrk_plan_set_pfb", 3), ("sdrk_plan_pfb_taps", 1), ("sdrk_exec_device_pfb", 6),
                        ("sdrk_exec_device_pfb_timed_each", 7), ("sdrk_exec_host_pfb", 5), ("sdrk_exec_fft_host_pfb", 5)):
        assert name in table and len(table[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert lib.sdrk_version() == 500
    assert lib.sdrk_plan_pfb_taps(None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
    assert lib.sdrk_plan_set_pfb(None, 2, None) == _ffi.SDRK_ERR_INVALID
    assert pkg.pfb_db is spectrum.pfb_db and pkg.pfb_prototype is pfb_prototype

"""CPU: the Python side of the integrated polyphase filter bank — the frame and group arithmetic, the argument errors raised
before any device call, and the ABI table (tests/test_abi.py checks header = table = exports)."""
import ctypes

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, spectrum
from tests.host_helpers import bare_plan


def test_frame_and_group_arithmetic():
    p = bare_plan(1024, taps=4)
    # frame f covers [f*hop, f*hop + 4096): 10240 samples hold 7 frames at hop 1024
    assert p.pfb_frames(10240) == 7
    assert p.pfb_integrated_groups(10240, 1) == 7 and p.pfb_integrated_groups(10240, 3) == 2 and p.pfb_integrated_groups(10240, 7) == 1
    assert p.pfb_integrated_groups(10240, 8) == 0 and p.pfb_integrated_groups(4095, 1) == 0
    assert p.pfb_integrated_groups(4096 + 10, 4, hop=1) == 2 and p.pfb_integrated_groups(10 * 1024, 2, hop=1500) == (1 + 6144 // 1500) // 2
    # a group of k frames needs (k - 1) * hop + taps * nfft samples, not one less
    for k, hop in ((5, 1024), (3, 700), (16, 1)):
        need = (k - 1) * hop + 4096
        assert p.pfb_integrated_groups(need, k, hop) == 1 and p.pfb_integrated_groups(need - 1, k, hop) == 0
    assert bare_plan(64, taps=1).pfb_integrated_groups(640, 5) == 2       # T = 1: integrated_groups
    for bad in (dict(k=0), dict(k=-1), dict(k=2, hop=0), dict(k=2, hop=-3)):
        with pytest.raises(ValueError):
            p.pfb_integrated_groups(8192, **bad)
    with pytest.raises(ValueError, match="set_pfb"):
        bare_plan(1024).pfb_integrated_groups(8192, 2)


def test_argument_errors_come_before_any_device_call():
    x = np.zeros(1024, np.complex64)
    calls = (lambda p, **kw: p.pfb_integrate(x, kw.pop("k", 2), **kw),
             lambda p, **kw: p.exec_device_pfb_integrated(0, 1, kw.pop("k", 2), 0, **kw),
             lambda p, **kw: p.exec_device_pfb_integrated_timed_each(0, 1, kw.pop("k", 2), 0, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="set_pfb"):
            call(bare_plan(64))
        with pytest.raises(ValueError, match="double"):
            call(bare_plan(64, taps=2, double=True))
        with pytest.raises(ValueError, match="rectangular"):
            call(bare_plan(64, taps=2, wkey="hann"))
        with pytest.raises(ValueError, match="detector"):
            call(bare_plan(64, taps=2), detector="median")
        with pytest.raises(ValueError, match="out"):
            call(bare_plan(64, taps=2), out="volts")
        with pytest.raises(ValueError):
            call(bare_plan(64, taps=2), k=0)
    with pytest.raises(ValueError):
        bare_plan(64, taps=2).pfb_integrate(x, 2, hop=0)
    for kw in (dict(frame_stride=0), ):
        with pytest.raises(ValueError):
            bare_plan(64, taps=2).exec_device_pfb_integrated(0, 1, 2, 0, **kw)
        with pytest.raises(ValueError):
            bare_plan(64, taps=2).exec_device_pfb_integrated_timed_each(0, 1, 2, 0, **kw)
    with pytest.raises(ValueError):
        bare_plan(64, taps=2).exec_device_pfb_integrated(0, 0, 2, 0)
    # the module function: prototype shape, taps, k, hop and detector before a plan is made
    with pytest.raises(ValueError):
        spectrum.pfb_integrated_db(x, 64, 4, 2, prototype=np.ones(64, np.float32))
    with pytest.raises(ValueError):
        spectrum.pfb_integrated_db(x, 64, 0, 2)
    with pytest.raises(ValueError):
        spectrum.pfb_integrated_db(x, 64, 4, 0)
    with pytest.raises(ValueError):
        spectrum.pfb_integrated_db(x, 64, 4, 2, hop=0)
    with pytest.raises(ValueError, match="detector"):
        spectrum.pfb_integrated_db(x, 64, 4, 2, detector="median")


def test_abi_table_and_exports():
    lib = _ffi.lib()
    table = {name: (res, args) for name, res, args in _ffi.SYMBOLS}
    for name, nargs in (("sdrk_exec_device_pfb_integrated", 10), ("sdrk_exec_device_pfb_integrated_timed_each", 11),
                        ("sdrk_exec_host_pfb_integrated", 9)):
        assert name in table and len(table[name][1]) == nargs, name
        assert table[name][1] == table[name.replace("_pfb", "")][1], name      # the signatures of the integrated entry points
        assert hasattr(lib, name), name
    assert lib.sdrk_version() == 500
    assert lib.sdrk_exec_host_pfb_integrated(None, None, 1, 1, 1, 0, 0, ctypes.c_float(1.0), None) == _ffi.SDRK_ERR_INVALID
    assert b"NULL" in lib.sdrk_last_error()
    assert pkg.pfb_integrated_db is spectrum.pfb_integrated_db

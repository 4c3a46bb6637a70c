"""CPU: the Python side of the int16 polyphase filter bank — frame and group counts, the array shapes and dtypes accepted and
refused before any device call, the package exports, and the header and the ctypes table in step."""
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.host_helpers import bare_plan

NEW = ("sdrk_exec_device_pfb_ci16", "sdrk_exec_device_pfb_ci16_timed_each", "sdrk_exec_host_pfb_ci16",
       "sdrk_exec_fft_host_pfb_ci16", "sdrk_exec_device_pfb_integrated_ci16", "sdrk_exec_device_pfb_integrated_ci16_timed_each",
       "sdrk_exec_host_pfb_integrated_ci16")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrk.h")


def test_header_and_table_declare_the_seven_with_their_counterparts_argument_lists():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    table = {name: (res, args) for name, res, args in _ffi.SYMBOLS}
    for name in NEW:
        twin = name.replace("_ci16", "")
        assert name in table and twin in table, name
        assert table[name][0] is table[twin][0] and list(table[name][1]) == list(table[twin][1]), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        decl_twin = re.search(r"\bint\s+" + twin + r"\s*\(([^;]*)\)\s*;", text)
        assert decl and decl_twin, name
        types = lambda d: [re.sub(r"\s*\w+$", "", a.strip()) for a in d.group(1).split(",")]   # noqa: E731
        assert types(decl) == types(decl_twin), name
        assert len(types(decl)) == len(table[name][1]), name


def test_the_names_are_exported_beside_the_existing_ones():
    for name in ("pfb_db_ci16", "pfb_integrated_db_ci16"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)
    for name in ("pfb_db_ci16", "pfb_fft_ci16", "exec_device_pfb_ci16", "exec_device_pfb_ci16_timed_each", "pfb_integrate_ci16",
                 "exec_device_pfb_integrated_ci16", "exec_device_pfb_integrated_ci16_timed_each"):
        assert callable(getattr(SpectrumPlan, name)), name


def test_frame_and_group_counts_follow_the_sample_count_not_the_bytes():
    p = bare_plan(1024, taps=4)
    x = np.zeros((4096 + 1023, 2), np.int16)
    assert p.pfb_frames(x.shape[0]) == 1 and p.pfb_frames(5120) == 2 and p.pfb_frames(4096 + 10, hop=1) == 11
    assert p.pfb_integrated_groups(4096 + 6 * 1024, 3) == 2 and p.pfb_integrated_groups(4096 + 6 * 1024, 8) == 0
    # a stream shorter than one span: empty results, no device call (the bare plan has none to make)
    out = p.pfb_db_ci16(np.zeros((4095, 2), np.int16))
    assert out.shape == (0, 1024) and out.dtype == np.float32
    assert p.pfb_fft_ci16(np.zeros((4095, 2), np.int16)).shape == (0, 1024)
    res = p.pfb_integrate_ci16(np.zeros((4096 + 1024, 2), np.int16), 3)
    assert res.shape == (0, 1024) and res.dtype == np.float32


@pytest.mark.parametrize("bad", [
    np.zeros(4096, np.complex64),                       # not int16
    np.zeros((4096, 2), np.int32),
    np.zeros((4096, 2), np.float32),
    np.zeros(8192, np.int16),                           # no (I, Q) axis
    np.zeros((4096, 3), np.int16),
    np.zeros((2, 2048, 2), np.int16),                   # frames, not a stream
    np.zeros((8192, 2), np.int16)[::2],                 # not contiguous
    [[1, 2], [3, 4]],                                   # not an array
])
def test_refused_arrays_raise_before_any_device_call(bad):
    p = bare_plan(64, taps=2)
    for call in (lambda: p.pfb_db_ci16(bad), lambda: p.pfb_fft_ci16(bad), lambda: p.pfb_integrate_ci16(bad, 2),
                 lambda: spectrum.pfb_db_ci16(bad, 64, 2), lambda: spectrum.pfb_integrated_db_ci16(bad, 64, 2, 2)):
        with pytest.raises(ValueError):
            call()


def test_plan_and_argument_errors_come_before_any_device_call():
    x = np.zeros((512, 2), np.int16)
    with pytest.raises(ValueError, match="set_pfb"):
        bare_plan(64).pfb_db_ci16(x)
    with pytest.raises(ValueError, match="double"):
        bare_plan(64, taps=2, double=True).pfb_db_ci16(x)
    with pytest.raises(ValueError, match="double"):
        bare_plan(64, taps=2, double=True).exec_device_pfb_ci16(1, 1, 1)
    with pytest.raises(ValueError, match="rectangular"):
        bare_plan(64, taps=2, wkey="hann").pfb_integrate_ci16(x, 2)
    p = bare_plan(64, taps=2)
    with pytest.raises(ValueError):
        p.pfb_db_ci16(x, hop=0)
    for kw in (dict(k=0), dict(k=2, detector="median"), dict(k=2, out="volts"), dict(k=2, hop=0)):
        with pytest.raises(ValueError):
            p.pfb_integrate_ci16(x, **kw)
    for args, kw in (((1, 0, 2, 1), {}), ((1, 1, 0, 1), {}), ((1, 1, 2, 1), dict(frame_stride=0)), ((1, 1, 2, 1), dict(detector="x"))):
        with pytest.raises(ValueError):
            p.exec_device_pfb_integrated_ci16(*args, **kw)
        with pytest.raises(ValueError):
            p.exec_device_pfb_integrated_ci16_timed_each(*args, **kw)
    for kw in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median")):
        with pytest.raises(ValueError):
            spectrum.pfb_integrated_db_ci16(x, 64, 2, **kw)

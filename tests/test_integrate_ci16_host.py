"""The int16 integrated-spectrum entry points without a GPU: exports and ctypes signatures, argument refusals through ctypes,
the frame / group arithmetic of SpectrumPlan.integrate_ci16 with the library stubbed, and the input checks that come before
any call into it."""
import ctypes
import os
import threading

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, processing, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sdrk_exec_device_integrated_ci16", "sdrk_exec_device_integrated_ci16_timed_each", "sdrk_exec_host_integrated_ci16")


def test_symbols_signatures_and_exports():
    table = {s[0]: s for s in _ffi.SYMBOLS}
    for ci16 in NAMES:
        c64 = ci16.replace("_ci16", "")
        assert ci16 in table and table[ci16][1:] == table[c64][1:], ci16       # the complex64 entry's signature
        assert getattr(_ffi.lib(), ci16).argtypes == table[ci16][2]
    header = open(os.path.join(REPO, "include", "sdrk.h")).read()
    for ci16 in NAMES:
        assert f"int {ci16}(sdrk_plan* plan, const void* " in header
    assert "#define SDRK_VERSION 500" in header and _ffi.lib().sdrk_version() == 500    # additions do not bump it
    for name in ("integrated_db_ci16", "welch_psd_streamed_ci16"):
        assert getattr(pkg, name) is getattr(spectrum, name) is getattr(processing, name) and name in pkg.__all__
    for name in ("integrate_ci16", "exec_device_integrated_ci16", "exec_device_integrated_ci16_timed_each",
                 "welch_psd_streamed_ci16"):
        assert callable(getattr(SpectrumPlan, name))


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_int16 * 32)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()

    def dev(plan, g, k, stride, det, form):
        return lib.sdrk_exec_device_integrated_ci16(plan, p, g, k, stride, det, form, 1.0, p, None)

    def host(plan, g, k, stride, det, form):
        return lib.sdrk_exec_host_integrated_ci16(plan, p, g, k, stride, det, form, 1.0, p)

    def timed(plan, g, k, stride, det, form):
        return lib.sdrk_exec_device_integrated_ci16_timed_each(plan, p, g, k, stride, det, form, 1.0, p, 2, each)

    for call in (dev, host, timed):
        assert call(None, 1, 1, 64, 3, 0) == _ffi.SDRK_ERR_INVALID and b"detector 3" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, -1, 0) == _ffi.SDRK_ERR_INVALID and b"detector -1" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, 0, 2) == _ffi.SDRK_ERR_INVALID and b"out_form 2" in lib.sdrk_last_error()
        assert call(None, 0, 1, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
        assert call(None, 1, 0, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
        assert call(None, 1 << 40, 1 << 40, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"out of range" in lib.sdrk_last_error()
        assert call(None, 1, 1, 0, 0, 0) == _ffi.SDRK_ERR_INVALID and b"frame_stride" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    for launches, ms in ((0, each), (4097, each), (2, None)):
        assert lib.sdrk_exec_device_integrated_ci16_timed_each(None, p, 1, 1, 64, 0, 0, 1.0, p, launches, ms) == _ffi.SDRK_ERR_INVALID
        assert b"launches" in lib.sdrk_last_error()
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.integrated_db_ci16(np.zeros((4096, 2), np.int16), 4096, 1)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


class _Lib:
    """Stands where _ffi.lib() stands: records the host call and fills the rows with the group number."""

    def __init__(self):
        self.calls = []

    def sdrk_exec_host_integrated_ci16(self, handle, iq, groups, k, hop, det, form, scale, out):
        self.calls.append((groups.value, k.value, hop.value, det, form, scale.value))
        rows = (ctypes.c_float * (groups.value * 64)).from_address(out.value)
        for g in range(groups.value):
            rows[g * 64:(g + 1) * 64] = [float(g)] * 64
        return 0

    def __getattr__(self, name):
        raise AssertionError(f"unexpected library call {name}")


class _Plan(SpectrumPlan):
    """The arithmetic of SpectrumPlan.integrate_ci16 without a device behind it."""

    def __init__(self, nfft):     # (SpectrumPlan.__init__ needs a device)
        self.nfft, self._double, self._handle, self._lock, self._wkey = nfft, False, ctypes.c_void_p(1), threading.Lock(), "hann"

    def close(self):
        pass


@pytest.fixture
def stub(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(spectrum, "lib", lambda: fake)
    return fake


def test_integrate_ci16_shapes_and_dropped_trailing_frames(stub):
    p = _Plan(64)
    z = lambda samples: np.zeros((samples, 2), np.int16)
    out = p.integrate_ci16(z(64 * 10), 3)                         # 10 frames: 3 groups, 1 frame dropped
    assert out.shape == (3, 64) and out.dtype == np.float32 and [float(r[0]) for r in out] == [0.0, 1.0, 2.0]
    assert stub.calls[-1] == (3, 3, 64, 0, 0, 1.0)
    assert p.integrate_ci16(z(64 * 10 + 63), 5, detector="max", out="power", scale=0.25).shape == (2, 64)
    assert stub.calls[-1] == (2, 5, 64, 1, 1, 0.25)
    assert p.integrate_ci16(z(64 + 32 * 7), 4, hop=32, detector="min").shape == (2, 64)      # 8 overlapped frames
    assert stub.calls[-1] == (2, 4, 32, 2, 0, 1.0)
    assert p.integrate_ci16(z(64 + 100 * 8 - 1), 3, hop=100).shape == (2, 64)                 # 8 gapped frames, the 9th short
    n_calls = len(stub.calls)
    for samples, k in ((64 * 2, 3), (63, 1), (0, 1)):                # no full group: nothing to run, an empty result
        out = p.integrate_ci16(z(samples), k)
        assert out.shape == (0, 64) and out.dtype == np.float32
    assert len(stub.calls) == n_calls
    w = p.welch_psd_streamed_ci16(z(64 * 5 + 3), 1e6)               # one group of all 5 full segments, mean, power
    assert w.shape == (64,) and stub.calls[-1][:5] == (1, 5, 64, 0, 1)
    assert stub.calls[-1][5] == pytest.approx(1.0 / (1e6 * float(np.sum(np.hanning(64) ** 2))), rel=1e-6)
    with pytest.raises(ValueError, match="shorter"):
        p.welch_psd_streamed_ci16(z(10), 1e6)


def test_wrong_dtype_shape_or_arguments_are_refused_before_any_call(stub):
    p = _Plan(64)
    good = np.zeros((256, 2), np.int16)
    bad_inputs = (np.zeros(256, np.complex64), good.astype(np.int32), good.astype(np.float32), np.zeros(256, np.int16),
                  np.zeros((2, 128, 2), np.int16), np.zeros((256, 3), np.int16), np.zeros((256, 4), np.int16)[:, ::2],
                  good.tolist())
    for bad in bad_inputs:
        with pytest.raises(ValueError, match="ci16"):
            p.integrate_ci16(bad, 2)
        with pytest.raises(ValueError, match="ci16"):
            p.welch_psd_streamed_ci16(bad, 1e6)
        with pytest.raises(ValueError, match="ci16"):
            spectrum.integrated_db_ci16(bad, 64, 2)                  # (refused before a plan, and so a device, is asked for)
        with pytest.raises(ValueError, match="ci16"):
            spectrum.welch_psd_streamed_ci16(bad, 64, 1e6)
    for kw in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median"), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            p.integrate_ci16(good, **kw)
    p._double = True
    with pytest.raises(ValueError, match="double"):
        p.integrate_ci16(good, 2)
    with pytest.raises(ValueError, match="double"):
        p.welch_psd_streamed_ci16(good, 1e6)
    with pytest.raises(ValueError, match="double"):
        p.exec_device_integrated_ci16(1, 1, 1, 1)
    with pytest.raises(ValueError, match="double"):
        p.exec_device_integrated_ci16_timed_each(1, 1, 1, 1)
    assert stub.calls == []

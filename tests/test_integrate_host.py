"""The integrated-spectrum entry points without a GPU: argument refusals through ctypes, the frame / group arithmetic of
SpectrumPlan.integrate, and the rule that cuts groups into slices (csrc/integrate_split.h, compiled here with g++)."""
import ctypes
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi, cli, spectrum
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sdr-iq-visualizer_amd", "csrc")


def test_symbols_and_codes():
    names = [s[0] for s in _ffi.SYMBOLS]
    for n in ("sdrk_exec_device_integrated", "sdrk_exec_device_integrated_timed_each", "sdrk_exec_host_integrated"):
        assert n in names
    assert _ffi.DETECTORS == {"mean": 0, "max": 1, "min": 2} and _ffi.INT_OUT_FORMS == {"db": 0, "power": 1}
    header = open(os.path.join(REPO, "include", "sdrk.h")).read()
    assert "SDRK_DET_MEAN = 0, SDRK_DET_MAX = 1, SDRK_DET_MIN = 2" in header
    assert "SDRK_INT_OUT_DB = 0, SDRK_INT_OUT_POWER = 1" in header
    assert "#define SDRK_VERSION 500" in header


def test_argument_refusals_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()

    def dev(plan, g, k, stride, det, form):
        return lib.sdrk_exec_device_integrated(plan, p, g, k, stride, det, form, 1.0, p, None)

    def host(plan, g, k, stride, det, form):
        return lib.sdrk_exec_host_integrated(plan, p, g, k, stride, det, form, 1.0, p)

    def timed(plan, g, k, stride, det, form):
        return lib.sdrk_exec_device_integrated_timed_each(plan, p, g, k, stride, det, form, 1.0, p, 2, each)

    for call in (dev, host, timed):
        assert call(None, 1, 1, 64, 3, 0) == _ffi.SDRK_ERR_INVALID and b"detector 3" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, -1, 0) == _ffi.SDRK_ERR_INVALID and b"detector -1" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, 0, 2) == _ffi.SDRK_ERR_INVALID and b"out_form 2" in lib.sdrk_last_error()
        assert call(None, 0, 1, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
        assert call(None, 1, 0, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"must be >= 1" in lib.sdrk_last_error()
        assert call(None, 1 << 40, 1 << 40, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and b"out of range" in lib.sdrk_last_error()
        assert call(None, 1, 1, 0, 0, 0) == _ffi.SDRK_ERR_INVALID and b"frame_stride" in lib.sdrk_last_error()
        assert call(None, 1, 1, 64, 0, 0) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_exec_device_integrated_timed_each(None, p, 1, 1, 64, 0, 0, 1.0, p, 0, each) == _ffi.SDRK_ERR_INVALID
    assert b"launches" in lib.sdrk_last_error()
    if _ffi.device_count() <= 0:
        with pytest.raises(_ffi.SdrkError) as e:
            spectrum.integrated_db(np.zeros(4096, np.complex64), 4096, 1)
        assert e.value.status == _ffi.SDRK_ERR_NO_DEVICE


class _Plan(SpectrumPlan):
    """The arithmetic of SpectrumPlan.integrate without a library handle behind it."""

    def __init__(self, nfft):     # (SpectrumPlan.__init__ needs a device)
        self.nfft, self._double, self._handle, self._lock, self._wkey = nfft, False, None, threading.Lock(), "hann"


def test_integrate_shapes_and_dropped_trailing_frames():
    p = _Plan(64)
    assert p.integrated_groups(64 * 10, 3) == 3                 # 10 frames: 3 groups, 1 frame dropped
    assert p.integrated_groups(64 * 10 + 63, 5) == 2
    assert p.integrated_groups(63, 1) == 0
    assert p.integrated_groups(64, 1) == 1
    assert p.integrated_groups(64 + 32 * 7, 4, hop=32) == 2     # 8 overlapped frames
    assert p.integrated_groups(64 + 100 * 8 - 1, 3, hop=100) == 2   # 8 gapped frames (the 9th is one sample short)
    out = p.integrate(np.zeros(64 * 2, np.complex64), 3)        # no full group: nothing to run, an empty result
    assert out.shape == (0, 64) and out.dtype == np.float32
    for bad in (dict(k=0), dict(k=2, hop=0), dict(k=2, detector="median"), dict(k=2, out="linear")):
        with pytest.raises(ValueError):
            p.integrate(np.zeros(64 * 4, np.complex64), **bad)
    p._double = True
    with pytest.raises(ValueError, match="double"):
        p.integrate(np.zeros(64 * 4, np.complex64), 2)
    with pytest.raises(ValueError, match="double"):
        p.welch_psd_streamed(np.zeros(64 * 4, np.complex64), 1e6)
    p._double = False
    with pytest.raises(ValueError, match="shorter"):
        p.welch_psd_streamed(np.zeros(10, np.complex64), 1e6)
    assert p.window_power() == pytest.approx(float(np.sum(np.hanning(64) ** 2)))


def test_cli_refuses_a_k_below_one(capsys):
    """(--integrate itself is unknown to the parser without the feature; here: its range check and what it says)"""
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit):
            cli.main(["psd", "x.sigmf-meta", "--integrate", bad])
        assert "must be >= 1" in capsys.readouterr().err


SPLIT_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "integrate_split.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        const size_t g = strtoull(argv[i], 0, 10), k = strtoull(argv[i + 1], 0, 10);
        const int cus = atoi(argv[i + 2]);
        const sdrk::IntSplit s = sdrk::integrate_split(g, k, cus);
        // walk every frame of the last group: the unit it falls in must belong to the group, and units follow each other
        size_t covered = 0, bad = 0, last_u = (size_t)-1, units = 0;
        for (size_t f = (g - 1) * k; f < g * k; ++f) {
            const size_t u = sdrk::integrate_unit_of(f, k, s);
            if (u / s.slices != g - 1) ++bad;
            if (u != last_u) {
                if (last_u != (size_t)-1 && u != last_u + 1) ++bad;
                ++units;
                last_u = u;
            }
            ++covered;
        }
        printf("%zu %zu %d %zu %zu %zu %zu %zu\n", g, k, cus, s.slices, s.len, covered, units, bad);
    }
    return 0;
}
"""


def test_split_rule(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    (tmp_path / "split.cpp").write_text(SPLIT_DRIVER)
    exe = str(tmp_path / "split")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(tmp_path / "split.cpp"), "-o", exe], check=True)
    cases = [(1, 1 << 20, 256), (1, 4096, 256), (1, 7, 256), (1, 8, 256), (3, 100, 256), (767, 16, 256), (768, 16, 256),
             (100000, 16, 256), (1, 1, 256), (5, 1, 8), (23, 64, 8), (24, 64, 8), (1, 64, 8), (2, 1000003, 256), (1, 9, 1)]
    args = [str(v) for c in cases for v in c]
    a = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    b = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    assert a == b                                                   # deterministic: a function of (n_groups, k, num_cus)
    rows = [tuple(int(v) for v in ln.split()) for ln in a.splitlines()]
    assert len(rows) == len(cases)
    for (g, k, cus), r in zip(cases, rows):
        slices, length, covered, units, bad = r[3:]
        grid = 3 * cus
        assert bad == 0 and covered == k, r
        assert (slices - 1) * length < k <= slices * length, r      # every slice has frames, together exactly k
        assert units == slices, r                                   # every frame of the group once, in slice order
        if g >= grid or k < 8:
            assert slices == 1 and length == k, r                   # enough groups (or too few frames): no split
        else:
            assert slices > 1 and length >= 4, r
            assert g * slices < 2 * grid + g, r                     # about one unit per resident workgroup, not many more
    by = dict(zip(cases, rows))
    assert by[(1, 1 << 20, 256)][3:5] == (768, 1366)
    assert by[(1, 64, 8)][3:5] == (16, 4)

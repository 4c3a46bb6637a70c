"""GPU: integrated one-sided spectra of real-sampled streams (sdrk_exec_*_real_integrated; SpectrumPlan.rintegrate /
exec_device_real_integrated; rintegrated_db / rwelch_psd) — one row of nfft + 1 bins per K frames — against the per-frame real
calls of the same build (bit for bit), against a float32 replay of the reduction, and against numpy's float64 rfft, at
N = 4096 (the kernel that reduces behind the split, real frames of 8192) and on the staged route of the other lengths.
The amplitude bar is test_integrate_gpu.py's: |sqrt(R_got) - sqrt(R_ref)| <= 1e-5 of the group's peak magnitude."""
import ctypes

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import DETECTORS, FORMS, DevBuf, check_amplitude, run_child, same_bits
from tests.real_groups_helpers import K4096_HOP, bound_stream, frames_of, k4096_stream, ref_power
from tests.test_real_gpu import FMT, L, N, device_rows, planted, widen_real

pytestmark = pytest.mark.gpu


class Resident:
    """A flat real-sampled stream resident on the device, and the integrated device entry of a plan on it."""

    def __init__(self, x, max_rows, bins):
        self.x, self.bins = x, bins
        self.dx, self.do = DevBuf(x.nbytes), DevBuf(max_rows * bins * 4)
        self.dx.put(x)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dx.__exit__()
        self.do.__exit__()

    def rows(self, plan, groups, k, det="mean", out="db", scale=1.0, hop=None):
        self.do.put(np.full((groups, self.bins), np.nan, np.float32))
        plan.exec_device_real_integrated(self.dx.p.value, groups, k, self.do.p.value, fmt=FMT[self.x.dtype], frame_stride=hop,
                                         detector=det, out=out, scale=scale)
        plan.sync()
        return self.do.get((groups, self.bins), np.float32)


def device_groups(plan, x, groups, k, **kw):
    with Resident(x, groups, plan.nfft + 1) as r:
        return r.rows(plan, groups, k, **kw)


@pytest.fixture(scope="module")
def plan4k():
    with SpectrumPlan(N, window="hann", shift=True) as p:   # (a windowed, shifting plan: neither may leak into this mode)
        yield p


# ---- 1. K = 1 at 4096 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [None, "hann"])
def test_k_1_in_db_is_the_per_frame_db_row_bit_for_bit(plan4k, window):
    x = bound_stream(N, 9, seed=1).reshape(-1)
    plan4k.set_real_window(window)
    try:
        per_frame = device_rows(plan4k, x, 9, out="db")
        for det in DETECTORS:
            assert same_bits(device_groups(plan4k, x, 9, 1, det=det), per_frame), (window, det)
    finally:
        plan4k.set_real_window(None)


# ---- 2. exact reduction at 4096 -------------------------------------------------------------------------------------------
CHILD_EXACT = r"""
import numpy as np
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import same_bits
from tests.real_groups_helpers import kahan_mean32
from tests.test_real_groups_gpu import Resident
from tests.test_real_gpu import L, N
GROUPS = 15                          # SDRK_NUM_CUS=2: a grid of 6 — unsplit, and the persistent loop turns more than twice
rng = np.random.default_rng(31)
with SpectrumPlan(N) as plan:
    plan.set_real_window((0.5 + rng.random(L)).astype(np.float32))
    for stride in (L, L // 2, L + 6):
        frames = GROUPS * 16
        s16 = rng.integers(-2000, 2000, size=(frames - 1) * stride + L).astype(np.int16)
        for x in (s16, s16.astype(np.float32)):
            with Resident(x, frames, N + 1) as r:
                P = r.rows(plan, frames, 1, det="mean", out="power", hop=stride)
                assert np.all(np.isfinite(P)) and P[:, 0].min() >= 0 and P[:, N].min() >= 0
                for k in (2, 3, 16):
                    g = P[:GROUPS * k].reshape(GROUPS, k, -1)
                    assert same_bits(r.rows(plan, GROUPS, k, det="max", out="power", hop=stride), g.max(axis=1)), (stride, k, "max")
                    assert same_bits(r.rows(plan, GROUPS, k, det="min", out="power", hop=stride), g.min(axis=1)), (stride, k, "min")
                    got = r.rows(plan, GROUPS, k, det="mean", out="power", hop=stride)
                    want = kahan_mean32(P[:GROUPS * k], GROUPS, k)
                    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                    assert bad.size == 0, (stride, k, str(x.dtype), bad[:8], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])
print("exact ok")
"""


def test_rows_are_the_exact_reduction_of_the_per_frame_powers():
    """P = the K = 1 POWER rows (scale 1).  MAX / MIN POWER rows for K in {2, 3, 16} are P's maxima / minima and the MEAN
    row the float32 replay of Kahan over P, then (acc - cmp) * float32(1 / K) — bit for bit, bins 0 and 4096 included;
    strides 8192, 4096 and 8198; float32 and int16; 15 unsplit groups on a grid of 6 workgroups."""
    run_child(CHILD_EXACT, "exact ok", SDRK_NUM_CUS="2")


def test_max_and_min_of_split_groups_are_exact_too(plan4k):
    x = bound_stream(N, 48, seed=2).reshape(-1)
    plan4k.set_real_window("hann")
    try:
        with Resident(x, 48, N + 1) as r:
            P = r.rows(plan4k, 48, 1, out="power")
            g = P.reshape(3, 16, -1)
            assert same_bits(r.rows(plan4k, 3, 16, det="max", out="power"), g.max(axis=1))
            assert same_bits(r.rows(plan4k, 3, 16, det="min", out="power"), g.min(axis=1))
    finally:
        plan4k.set_real_window(None)


# ---- 3. integer formats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 1024])
@pytest.mark.parametrize("dtype", [np.int16, np.int8, np.uint8])
@pytest.mark.parametrize("windowed", [False, True])
def test_integer_formats_have_the_float32_bits(n, dtype, windowed):
    x = planted(dtype, 6, 2 * n).reshape(-1)
    with SpectrumPlan(n) as plan:
        plan.set_real_window(np.hanning(2 * n).astype(np.float32) + np.float32(0.125) if windowed else None)
        with Resident(x, 2, n + 1) as a, Resident(widen_real(x), 2, n + 1) as b:
            for det in DETECTORS:
                for form in FORMS:
                    assert same_bits(a.rows(plan, 2, 3, det=det, out=form), b.rows(plan, 2, 3, det=det, out=form)), (det, form)


# ---- 4. split groups ------------------------------------------------------------------------------------------------------
CHILD_SPLIT = r"""
import numpy as np
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import check_amplitude, same_bits
from tests.real_groups_helpers import bound_stream, ref_power
from tests.test_real_groups_gpu import device_groups
from tests.test_real_gpu import L, N
K, TILES = 64, 24                    # SDRK_NUM_CUS=8: a grid of 24 — one group is cut into slices, 24 groups are not
x = np.rint(bound_stream(N, K, seed=4) * 200).astype(np.int16)
p = ref_power(x, "hann")
tiled = np.tile(x.reshape(-1), TILES)
with SpectrumPlan(N) as plan:
    plan.set_real_window("hann")
    for det in ("max", "min", "mean"):
        one = device_groups(plan, x.reshape(-1), 1, K, det=det, out="power")
        many = device_groups(plan, tiled, TILES, K, det=det, out="power")
        for g in range(1, TILES):
            assert same_bits(many[g], many[0]), (det, g)
        if det != "mean":
            assert same_bits(one[0], many[0]), det
        check_amplitude(one, "power", p, 1, K, det, f"split {det}")
        check_amplitude(many[:1], "power", p, 1, K, det, f"unsplit {det}")
print("split ok")
"""


def test_split_groups_against_unsplit_groups():
    """One group of 64 frames (cut into slices) and the same frames tiled to 24 groups (unsplit) on the grids of an 8-CU
    device: equal bits for MAX and MIN, MEAN within the amplitude bound either way."""
    run_child(CHILD_SPLIT, "split ok", SDRK_NUM_CUS="8")


# ---- 5. amplitude bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 256, 4096, 8192, 65536])
def test_amplitude_bound(n):
    """K in {1, 3, 100} (3, 2 and 1 groups of the same 100 frames), Hann and rectangular, dB and power, all detectors."""
    x = bound_stream(n, 100, seed=n)
    with SpectrumPlan(n) as plan, Resident(x.reshape(-1), 3, n + 1) as r:
        for window in (None, "hann"):
            plan.set_real_window(window)
            p = ref_power(x, window)
            for k, groups in ((1, 3), (3, 2), (100, 1)):
                for det in DETECTORS:
                    for form in FORMS:
                        got = r.rows(plan, groups, k, det=det, out=form)
                        check_amplitude(got, form, p, groups, k, det, f"N={n} K={k} {window} {det} {form}")


def test_k_4096_of_a_tone_in_weak_noise_holds_the_bound(plan4k):
    """A mean of 4096 nearly equal powers per bin: plain float32 summation drifts past the bound, the compensated sum does
    not.  One group, which the library splits."""
    x = k4096_stream()
    plan4k.set_real_window("hann")
    try:
        p = ref_power(frames_of(x, L, 4096, K4096_HOP), "hann")
        with Resident(x, 1, N + 1) as r:
            for form in FORMS:
                check_amplitude(r.rows(plan4k, 1, 4096, det="mean", out=form, hop=K4096_HOP), form, p, 1, 4096, "mean", f"K=4096 {form}")
    finally:
        plan4k.set_real_window(None)


# ---- 6. host entry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,groups", [(4096, 600), (1024, 600), (1024, 2400)])
def test_host_entry_has_the_device_bits_across_chunks(n, groups):
    """ru8, groups of 7: at 4096 (and with 2400 groups at 1024) more than two 16 MiB chunks, whose boundaries cut groups
    (a chunk holds 2048 frames of 8192 bytes, no multiple of 7); pageable and pinned."""
    k, length = 7, 2 * n
    x = np.random.default_rng(n + groups).integers(0, 256, size=groups * k * length).astype(np.uint8)
    with SpectrumPlan(n) as plan:
        plan.set_real_window("hann")
        for det, form in (("mean", "db"), ("max", "power")):
            dev = device_groups(plan, x, groups, k, det=det, out=form)
            assert np.all(np.isfinite(dev))
            assert same_bits(plan.rintegrate(x, k, detector=det, out=form), dev), (det, form, "pageable")
            pinned = pkg.pinned_empty(x.shape, x.dtype)
            pinned[...] = x
            assert same_bits(plan.rintegrate(pinned, k, detector=det, out=form), dev), (det, form, "pinned")


def test_staged_device_call_larger_than_the_staging():
    """N = 1024, K = 100, 100 groups of ru8: 10,000 staged spectra of 1025 bins are 82 MB, more than the 64 MiB staging."""
    n, k, groups = 1024, 100, 100
    x = np.random.default_rng(7).integers(0, 256, size=(groups * k, 2 * n)).astype(np.uint8)
    p = ref_power(widen_real(x), None)
    with SpectrumPlan(n) as plan:
        for det in DETECTORS:
            dev = device_groups(plan, x.reshape(-1), groups, k, det=det, out="power")
            assert same_bits(plan.rintegrate(x.reshape(-1), k, detector=det, out="power"), dev), det
            check_amplitude(dev, "power", p, groups, k, det, f"staged {det}")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_status_and_text():
    lib = _ffi.lib()
    vp, sz, cf = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
    with DevBuf(4 * L * 4) as dx, DevBuf(4 * 4200 * 4) as do, SpectrumPlan(N) as plan:
        h, x, o = plan.handle, dx.p.value, do.p.value
        dx.put(np.ones(4 * L, np.float32))
        do.put(np.full(4 * 4200, -3.0, np.float32))

        def call(handle=h, xp=x, fmt=_ffi.REAL_F32, groups=2, k=2, stride=L, det=0, form=0, op=o):
            st = lib.sdrk_exec_device_real_integrated(handle, vp(xp), fmt, sz(groups), sz(k), sz(stride), det, form, cf(1.0), vp(op), None)
            return st, lib.sdrk_last_error().decode()

        for (st, text), word in ((call(stride=L + 1), "odd"), (call(xp=x + 4), "aligned"),
                                 (call(fmt=_ffi.REAL_S16, xp=x + 2), "aligned"), (call(fmt=_ffi.REAL_S8, xp=x + 1), "aligned"),
                                 (call(fmt=7), "real_format"), (call(det=3), "detector"), (call(form=2), "out_form"),
                                 (call(k=0), "k_frames"), (call(groups=0), "n_groups"), (call(xp=None), "NULL"),
                                 (call(op=None), "NULL"), (call(stride=0), "frame_stride")):
            assert st == _ffi.SDRK_ERR_INVALID and word in text, (st, text, word)
        ms = (ctypes.c_float * 1)()
        st = lib.sdrk_exec_device_real_integrated_timed_each(h, vp(x), 0, sz(2), sz(2), sz(L + 1), 0, 0, cf(1.0), vp(o), 1, ms)
        assert st == _ffi.SDRK_ERR_INVALID and "odd" in lib.sdrk_last_error().decode()
        host = np.zeros(4 * L + 1, np.float32)
        out = np.full((2, N + 1), -3.0, np.float32)
        st = lib.sdrk_exec_host_real_integrated(h, host.ctypes.data_as(vp), 0, sz(2), sz(2), sz(L + 1), 0, 0, cf(1.0), out.ctypes.data_as(vp))
        assert st == _ffi.SDRK_ERR_INVALID and "odd" in lib.sdrk_last_error().decode()
        st = lib.sdrk_exec_host_real_integrated(h, host.ctypes.data_as(vp), 0, sz(2), sz(0), sz(L), 0, 0, cf(1.0), out.ctypes.data_as(vp))
        assert st == _ffi.SDRK_ERR_INVALID and np.all(out == -3.0)
        plan.sync()
        assert np.all(do.get((4 * 4200,), np.float32) == -3.0)                # nothing was launched
        with SpectrumPlan(N, precision="double") as p64:
            st, text = call(handle=p64.handle)
            assert st == _ffi.SDRK_ERR_INVALID and "float64" in text, (st, text)
        with SpectrumPlan(1000) as pz:
            st, text = call(handle=pz.handle, stride=2000)
            assert st == _ffi.SDRK_ERR_UNSUPPORTED and "chirp-z" in text, (st, text)
        with SpectrumPlan(1 << 21, max_batch=1) as pbig:
            st, text = call(handle=pbig.handle, groups=1, k=1)
            assert st == _ffi.SDRK_ERR_UNSUPPORTED and "2^20" in text, (st, text)
        # a plan that has refused still works
        assert call()[0] == _ffi.SDRK_OK
        plan.sync()
        rows = do.get((2, N + 1), np.float32)
        assert np.all(np.isfinite(rows)) and abs(float(rows[0, 0]) - 20 * np.log10(L)) < 1e-3   # bin 0 of a frame of ones


# ---- 8. module level ------------------------------------------------------------------------------------------------------
def test_rintegrated_db_and_rwelch_psd_end_to_end():
    n, fs = 512, 48000.0
    x = bound_stream(n // 2, 21, seed=8).reshape(-1)
    w = np.hanning(n)
    p = ref_power(x.reshape(21, n), "hann")
    for det in DETECTORS:
        got = pkg.rintegrated_db(x, n, 5, detector=det, window="hann")
        assert got.shape == (4, n // 2 + 1) and got.dtype == np.float32
        check_amplitude(got, "db", p, 4, 5, det, f"rintegrated_db {det}")
    hop = n // 2
    frames = 1 + (x.shape[0] - n) // hop
    pw = ref_power(frames_of(x, n, frames, hop), "hann").mean(axis=0) / (fs * np.sum(w ** 2))
    pw[1:n // 2] *= 2.0
    got = pkg.rwelch_psd(x, n, fs, hop=hop)
    assert got.shape == (n // 2 + 1,) and got.dtype == np.float32
    assert np.abs(np.sqrt(got.astype(np.float64)) - np.sqrt(pw)).max() <= 1e-5 * np.sqrt(pw.max())

"""GPU: one-sided spectra of real-sampled frames (sdrk_exec_*_real; SpectrumPlan.rspectrum_db / rfft / rstft_db /
exec_device_real) against numpy's float64 rfft and against each other, at N = 4096 (the fused kernel, real frames of 8192)
and on the staged route of the other lengths.  The bar is the suite's: 1e-5 of the frame's peak magnitude."""
import ctypes

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.gpu_helpers import DevBuf, run_child, same_bits
from tests.parity import REL_TOL, assert_complex_parity

pytestmark = pytest.mark.gpu

N, L = 4096, 8192
EPS = 1e-12
FMT = {np.dtype(np.float32): "f32", np.dtype(np.int16): "s16", np.dtype(np.int8): "s8", np.dtype(np.uint8): "u8"}


def widen_real(x):
    """The float32 samples an integer array stands for (uint8: v - 127.5), exactly."""
    f = x.astype(np.float32)
    return f - np.float32(127.5) if x.dtype == np.uint8 else f


def device_rows(plan, x, n_frames, out="complex", frame_stride=None, out_stride=None, fill=None):
    """exec_device_real on a flat host array: the (n_frames, out_stride or nfft + 1) block the call wrote into."""
    bins = plan.nfft + 1
    width = out_stride or bins
    dtype = np.complex64 if out == "complex" else np.float32
    with DevBuf(x.nbytes) as dx, DevBuf(n_frames * width * np.dtype(dtype).itemsize) as do:
        dx.put(x)
        if fill is not None:
            do.put(np.full((n_frames, width), fill, dtype))
        plan.exec_device_real(dx.p.value, n_frames, do.p.value, fmt=FMT[x.dtype], out=out, frame_stride=frame_stride,
                              out_stride=out_stride)
        plan.sync()
        return do.get((n_frames, width), dtype)


def ref_rfft(frames, window=None):
    x = frames.astype(np.float64)
    return np.fft.rfft(x if window is None else x * window.astype(np.float64), axis=-1)


def check_complex(got, ref, what):
    for i in range(ref.shape[0]):
        peak = np.abs(ref[i]).max() or 1.0
        err = np.abs(got[i].astype(np.complex128) - ref[i]).max() / peak
        print(f"{what} frame {i}: err/tol {err / REL_TOL:.3f}")
    assert_complex_parity(got, ref, rel=REL_TOL, what=what)
    assert np.all(got[:, 0].imag == 0) and not np.any(np.signbit(got[:, 0].imag)), what
    assert np.all(got[:, -1].imag == 0) and not np.any(np.signbit(got[:, -1].imag)), what


def check_db(got, ref, what):
    """Every bin within 40 dB of its frame's peak within 0.01 dB: 1e-5 of the peak on a bin at >= 1e-2 of it is <= 1e-3
    relative, 0.0087 dB."""
    r = 20 * np.log10(np.abs(ref) + EPS)
    sel = r >= r.max(axis=-1, keepdims=True) - 40.0
    d = np.abs(got.astype(np.float64) - r)[sel]
    print(f"{what}: worst |delta dB| {d.max():.2e} on {int(sel.sum())} bins")
    assert d.max() <= 0.01, (what, float(d.max()))


def basis_frames():
    rng = np.random.default_rng(11)
    n = np.arange(L)
    rows = []
    for at in (0, 1, 2, 8190, 8191):
        e = np.zeros(L)
        e[at] = 1.0
        rows.append(e)
    rows.append(np.full(L, 0.75))
    for k0 in (0, 1, 255, 256, 257, 2048, 4095, 4096):
        rows.append(np.cos(2 * np.pi * k0 * n / L))
    rows.append(30.0 * np.cos(2 * np.pi * 611.3 * n / L + 0.3) + rng.standard_normal(L))
    rows.append(rng.standard_normal(L))
    return np.ascontiguousarray(np.array(rows, dtype=np.float32))


@pytest.fixture(scope="module")
def plan4k():
    with SpectrumPlan(N, window="hann", shift=True) as p:   # (a windowed, shifting plan: neither may leak into this mode)
        yield p


@pytest.fixture(scope="module")
def basis():
    x = basis_frames()
    return x, ref_rfft(x)


def test_basis_at_4096_complex_and_db(plan4k, basis):
    x, ref = basis
    plan4k.set_real_window(None)
    got = device_rows(plan4k, x.reshape(-1), x.shape[0])
    check_complex(got, ref, "basis")
    check_db(device_rows(plan4k, x.reshape(-1), x.shape[0], out="db"), ref, "basis dB")


def test_all_zero_frame_gives_the_eps_floor_on_every_bin(plan4k):
    plan4k.set_real_window(None)
    rows = device_rows(plan4k, np.zeros(L, np.float32), 1, out="db")
    assert rows.shape == (1, N + 1) and np.all(rows == rows[0, 0])
    assert abs(float(rows[0, 0]) - 20 * np.log10(EPS)) <= 1e-3
    z = device_rows(plan4k, np.zeros(L, np.float32), 1)
    assert same_bits(z, np.zeros((1, N + 1), np.complex64))


@pytest.mark.parametrize("kind", ["hann", "random", "even_only"])
def test_window_at_4096(plan4k, basis, kind):
    x, _ = basis
    if kind == "hann":
        w = np.hanning(L).astype(np.float32)
    elif kind == "random":
        w = (0.25 + np.random.default_rng(5).random(L)).astype(np.float32)
    else:
        w = np.zeros(L, np.float32)    # 1 on even samples, 0 on odd ones: swapped pair halves would show
        w[0::2] = 1.0
    plan4k.set_real_window("hann" if kind == "hann" else w)
    try:
        ref = ref_rfft(x, w)
        check_complex(device_rows(plan4k, x.reshape(-1), x.shape[0]), ref, f"window {kind}")
        check_db(device_rows(plan4k, x.reshape(-1), x.shape[0], out="db"), ref, f"window {kind} dB")
    finally:
        plan4k.set_real_window(None)


def planted(dtype, frames, length, seed=3):
    info = np.iinfo(dtype)
    rng = np.random.default_rng(seed)
    x = rng.integers(info.min, info.max + 1, size=(frames, length), dtype=np.int64).astype(dtype)
    edge = np.array([info.min, info.max, 0, info.max, info.min, 0], dtype=dtype)
    x[0, :6] = edge
    x[-1, -6:] = edge
    x[frames // 2, 1::997] = info.min
    x[frames // 2, 2::997] = info.max
    return x


@pytest.mark.parametrize("dtype", [np.int16, np.int8, np.uint8])
@pytest.mark.parametrize("windowed", [False, True])
def test_integer_formats_have_the_float32_bits_at_4096(plan4k, dtype, windowed):
    x = planted(dtype, 5, L)
    plan4k.set_real_window(np.hanning(L).astype(np.float32) + np.float32(0.125) if windowed else None)
    try:
        for out in ("complex", "db"):
            a = device_rows(plan4k, x.reshape(-1), 5, out=out)
            b = device_rows(plan4k, widen_real(x).reshape(-1), 5, out=out)
            assert same_bits(a, b), (dtype, windowed, out)
        assert_complex_parity(device_rows(plan4k, x.reshape(-1), 5), ref_rfft(widen_real(x), None if not windowed else
                              np.hanning(L).astype(np.float32) + np.float32(0.125)), rel=REL_TOL, what=str(dtype))
    finally:
        plan4k.set_real_window(None)


CHILD_PLACEMENT = r"""
import numpy as np
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan
from tests.test_real_gpu import L, N, device_rows, same_bits
CUS = 2
GRID = 3 * CUS                      # three workgroups per CU
rng = np.random.default_rng(21)
with SpectrumPlan(N) as plan:
    plan.set_real_window((0.5 + rng.random(L)).astype(np.float32))
    for frames in (1, 5, 2 * GRID + 3):         # the last: the persistent loop turns more than twice
        for stride in (L, L // 2, L + 6):
            s16 = rng.integers(-2000, 2000, size=(frames - 1) * stride + L).astype(np.int16)
            for x in (s16, s16.astype(np.float32)):
                for out, fill in (("complex", np.complex64(complex(-7.5, 3.25))), ("db", np.float32(-1234.5))):
                    for out_stride in (None, 4100):
                        rows = device_rows(plan, x, frames, out=out, frame_stride=stride, out_stride=out_stride, fill=fill)
                        if out_stride:
                            assert np.all(rows[:, N + 1:] == fill), (frames, stride, out)
                        for i in sorted({0, frames // 2, frames - 1}):
                            one = device_rows(plan, np.ascontiguousarray(x[i * stride:i * stride + L]), 1, out=out)
                            assert same_bits(rows[i, :N + 1], one[0]), (frames, stride, out, out_stride, i, str(x.dtype))
print("placement ok")
"""


def test_rows_do_not_depend_on_their_place_in_a_call():
    """SDRK_NUM_CUS=2 (read when a plan is made: a child process): calls of 1, 5 and 2 * grid + 3 frames, strides L, L/2
    and L + 6, out_stride packed and 4100 — every checked row carries the bits of the one-frame call on its samples, and
    what lies between rows keeps its planted pattern."""
    run_child(CHILD_PLACEMENT, "placement ok", SDRK_NUM_CUS="2")


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint8])
def test_host_calls_have_the_device_bits_at_4096(dtype):
    frames = 72 if dtype == np.float32 else 150 if dtype == np.int16 else 300      # > 2 MiB of input: several chunks
    rng = np.random.default_rng(8)
    x = (rng.integers(0, 256, size=(frames, L)).astype(dtype) if dtype != np.float32
         else rng.standard_normal((frames, L)).astype(np.float32))
    with SpectrumPlan(N) as plan:
        plan.set_real_window("hann")
        dev_c, dev_db = device_rows(plan, x.reshape(-1), frames), device_rows(plan, x.reshape(-1), frames, out="db")
        assert same_bits(plan.rfft(x), dev_c) and same_bits(plan.rspectrum_db(x), dev_db)
        pinned = pkg.pinned_empty(x.shape, x.dtype)
        pinned[...] = x
        out = pkg.pinned_empty((frames, N + 1), np.float32)
        assert same_bits(plan.rspectrum_db(pinned, out=out), dev_db) and same_bits(plan.rfft(pinned), dev_c)
        hop = L // 2
        rows = plan.rstft_db(x.reshape(-1)[:5 * L], hop=hop)
        assert rows.shape == (9, N + 1)
        assert same_bits(rows, device_rows(plan, x.reshape(-1)[:5 * L], 9, out="db", frame_stride=hop))
        assert same_bits(plan.rspectrum_db(x[3]), dev_db[3])            # one frame, flat: one row


@pytest.mark.parametrize("n,frames", [(16, 3), (256, 3), (8192, 3), (65536, 3), (1 << 20, 1)])
def test_staged_route(n, frames):
    length = 2 * n
    rng = np.random.default_rng(n)
    t = np.arange(length)
    f32 = (rng.standard_normal((frames, length)) + 20 * np.cos(2 * np.pi * (0.1234 * length + 0.3) * t / length)).astype(np.float32)
    i16 = planted(np.int16, frames, length, seed=n)
    w = (0.25 + rng.random(length)).astype(np.float32)
    with SpectrumPlan(n, window="hann", max_batch=8) as plan:
        for window in (None, w):
            plan.set_real_window(window)
            got = device_rows(plan, f32.reshape(-1), frames)
            check_complex(got, ref_rfft(f32, window), f"N={n} float32 window={window is not None}")
            check_db(device_rows(plan, f32.reshape(-1), frames, out="db"), ref_rfft(f32, window), f"N={n} dB")
            assert same_bits(plan.rfft(f32), got)
            g16 = device_rows(plan, i16.reshape(-1), frames)
            check_complex(g16, ref_rfft(i16, window), f"N={n} int16 window={window is not None}")
            assert same_bits(g16, device_rows(plan, widen_real(i16).reshape(-1), frames))
            assert same_bits(plan.rfft(i16), g16)
            assert same_bits(plan.rspectrum_db(i16), device_rows(plan, i16.reshape(-1), frames, out="db"))


def test_staged_route_int8_and_overlap_at_1024():
    n, length, frames, hop = 1024, 2048, 7, 512
    x = planted(np.uint8, 1, (frames - 1) * hop + length).reshape(-1)
    with SpectrumPlan(n) as plan:
        rows = device_rows(plan, x, frames, frame_stride=hop, out_stride=n + 5, fill=np.complex64(complex(1.5, -2.5)))
        assert np.all(rows[:, n + 1:] == np.complex64(complex(1.5, -2.5)))
        idx = (np.arange(frames) * hop)[:, None] + np.arange(length)[None, :]
        check_complex(rows[:, :n + 1], ref_rfft(widen_real(x)[idx]), "N=1024 uint8 overlapped")
        assert same_bits(rows[:, :n + 1], device_rows(plan, widen_real(x), frames, frame_stride=hop))


def _status(fn, *args):
    st = fn(*args)
    return st, _ffi.lib().sdrk_last_error().decode()


def test_refusals_status_and_text():
    lib = _ffi.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    with DevBuf(4 * L * 4) as dx, DevBuf(4 * 4200 * 8) as do, SpectrumPlan(N) as plan:
        h, x, o = plan.handle, dx.p.value, do.p.value
        do.put(np.full(4 * 4200 * 2, -3.0, np.float32))

        def call(handle=h, xp=x, fmt=_ffi.REAL_F32, frames=2, stride=L, form=_ffi.REAL_OUT_DB, op=o, out_stride=0):
            return _status(lib.sdrk_exec_device_real, handle, vp(xp), fmt, sz(frames), sz(stride), form, vp(op), sz(out_stride), None)

        for (st, text), word in ((call(stride=L + 1), "odd"), (call(xp=x + 4), "aligned"),
                                 (call(fmt=_ffi.REAL_S16, xp=x + 2), "aligned"), (call(fmt=_ffi.REAL_S8, xp=x + 1), "aligned"),
                                 (call(fmt=7), "real_format"), (call(form=5), "out_form"), (call(out_stride=N), "out_stride"),
                                 (call(xp=None), "NULL")):
            assert st == _ffi.SDRK_ERR_INVALID and word in text, (st, text, word)
        w = np.ones(L + 2, np.float32)
        st, text = _status(lib.sdrk_plan_set_real_window, h, w.ctypes.data_as(vp), sz(L + 2))
        assert st == _ffi.SDRK_ERR_INVALID and "2*nfft" in text, (st, text)
        with pytest.raises(ValueError):
            plan.set_real_window(np.ones(L - 2, np.float32))
        ms = (ctypes.c_float * 1)()
        st = lib.sdrk_exec_device_real_timed_each(h, vp(x), 0, sz(2), sz(L + 1), 0, vp(o), sz(0), 1, ms)
        assert st == _ffi.SDRK_ERR_INVALID
        host = np.zeros(2 * L + 1, np.float32)
        out = np.zeros((2, N + 1), np.float32)
        st, text = _status(lib.sdrk_exec_host_real, h, host.ctypes.data_as(vp), 0, sz(2), sz(L + 1), out.ctypes.data_as(vp))
        assert st == _ffi.SDRK_ERR_INVALID and "odd" in text
        plan.sync()
        assert np.all(do.get((4 * 4200 * 2,), np.float32) == -3.0)                # nothing was launched
        with SpectrumPlan(N, precision="double") as p64:
            st, text = call(handle=p64.handle)
            assert st == _ffi.SDRK_ERR_INVALID and "float64" in text, (st, text)
        with SpectrumPlan(1000) as pz:
            st, text = call(handle=pz.handle, stride=2000)
            assert st == _ffi.SDRK_ERR_UNSUPPORTED and "chirp-z" in text, (st, text)
        with SpectrumPlan(1 << 21, max_batch=1) as pbig:
            st, text = call(handle=pbig.handle, frames=0)
            assert st == _ffi.SDRK_ERR_UNSUPPORTED and "2^20" in text, (st, text)
        # a plan that has refused still works
        assert call()[0] == _ffi.SDRK_OK
        plan.sync()


def test_module_level_calls_and_python_refusals():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 512)).astype(np.float32)
    w = np.hanning(512).astype(np.float32)
    assert_complex_parity(pkg.rfft(x, 512, "hann"), ref_rfft(x, w), rel=REL_TOL, what="rfft hann 512")
    check_db(pkg.rspectrum_db(x, 512), ref_rfft(x), "rspectrum_db 512")
    with pytest.raises(ValueError):
        pkg.rfft(x.astype(np.float64), 512)
    with pytest.raises(ValueError):
        pkg.rfft(x, 256)

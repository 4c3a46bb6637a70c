"""The channel bank on the GPU (sdrk_exec_device_chanbank* / sdrk_exec_host_chanbank*): C tuned channels from one pass over the
input.  The yardstick is the single-channel call the repository already trusts: plane c of a bank call carries THE BITS of
sdrk_exec_device_fir with (shift_bins[c], phase0[c]) on the same input (np.array_equal on the uint32 views), for every shape here;
one test holds the planes to the float64 numpy reference of tests/test_fir_gpu.py as well, under that file's bound
1e-5 * ||h||_1 * max|x|.

Inputs are a few blocks long with 12-bit integer samples: the smallest shapes at which the block geometry (one output, a ragged
last block, a last block exactly full), the channel loop (C = 1, 5 with a duplicate, 64) and the loads in flight across channels
and blocks (the 8-CU child at the end: several blocks per workgroup) can go wrong.

Measured on the device (profiles/fir_bank/SUMMARY.md): every plane equal in bits; worst err/tol against float64 numpy 5.5e-3 at (257, 16), 2.3e-3 at (2049, 64)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from sdr_iq_visualizer_amd import _ffi
from sdr_iq_visualizer_amd.spectrum import ChannelBankStream, ChannelStream, SpectrumPlan, channel_taps, fir_bank, pfb_prototype
from tests.gpu_helpers import DevBuf, same_bits, widen_flat
from tests.test_fir_gpu import GUARD, block_len, check, device_fir, random_taps, ref_fir, tol_of

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
SHIFTS = (0, 611, -2048, 2047, 611)      # one without a mixer, the two limits, a duplicate
PHASES = (0, 5, 4095, -7, 5)
SHAPES = [(1, 1), (2, 4), (257, 16), (1793, 256), (2049, 64)]   # (M, D)


def same_u32(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ints12(seed, n):
    """complex64 samples with 12-bit integer parts"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2048, 2048, n) + 1j * rng.integers(-2048, 2048, n)).astype(np.complex64)


def ints12_i16(seed, n):
    return np.random.default_rng(seed).integers(-2048, 2048, size=(n, 2)).astype(np.int16)


def device_bank(plan, x, d, shifts, phases=None, ci16=False, pad=0):
    """The device entry's planes (C, n_out); the pad between planes and the GUARD behind the last are checked to be untouched."""
    n_in, c = x.shape[0], len(shifts)
    n_out = plan.fir_outputs(n_in, d)
    stride = n_out + pad
    with DevBuf(x.nbytes) as d_in, DevBuf((c * stride + GUARD) * 8) as d_out:
        d_in.put(x)
        d_out.put(np.full(c * stride + GUARD, np.nan + 1j * np.nan, np.complex64))
        run = plan.exec_device_fir_bank_ci16 if ci16 else plan.exec_device_fir_bank
        run(d_in.p.value, n_in, d_out.p.value, shifts, decim=d, phase0=phases, out_stride=stride if pad else None)
        plan.sync()
        got = d_out.get(c * stride + GUARD, np.complex64)
    assert np.all(np.isnan(got[c * stride:].real)), "stored past the last plane"
    planes = got[: c * stride].reshape(c, stride)
    assert np.all(np.isnan(planes[:, n_out:].real)), "stored between the planes"
    return np.ascontiguousarray(planes[:, :n_out])


def assert_planes_are_the_single_calls(plan, x, d, shifts, phases, planes, what, ci16=False):
    assert planes.shape == (len(shifts), plan.fir_outputs(x.shape[0], d)) and planes.dtype == np.complex64, what
    for c, (s, ph) in enumerate(zip(shifts, phases)):
        assert same_u32(planes[c], device_fir(plan, x, d, s, ph, ci16=ci16)), (what, "channel", c, s, ph)


# ---- 1, 2: the bits of the single call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", SHAPES)
def test_each_plane_carries_the_bits_of_the_single_call(m, d):
    L = block_len(m)
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m, m))
        for n_in in (m, 3 * L + 1000, 2 * L + N):                 # one output; a ragged last block; the last block exactly full
            x = ints12(m + n_in, n_in)
            if (m, n_in) == (257, 3 * L + 1000):                  # the channel with s = 0 runs NO mixer: a product with (1, 0)
                x[5] = complex(-0.0, -0.0)                        # would not keep these bits
                x[3 * L + 700] = complex(np.inf, 1.0)             # (the last block only: the others stay finite)
            planes = device_bank(plan, x, d, SHIFTS, PHASES)
            assert_planes_are_the_single_calls(plan, x, d, SHIFTS, PHASES, planes, f"M={m} D={d} n_in={n_in}")
            assert same_u32(planes[1], planes[4])                 # the duplicate


def test_a_block_of_negative_zeros_keeps_its_sign_in_the_channel_without_a_mixer():
    """All samples -0.0 and taps (1, 0): the single call with s = 0 returns what its transform makes of them, bit for bit, and
    so does the bank's channel 0 beside a channel with a mixer."""
    x = np.full(N + 100, complex(-0.0, -0.0), np.complex64)
    with SpectrumPlan(N) as plan:
        plan.set_fir(np.ones(1, np.complex64))
        planes = device_bank(plan, x, 1, (0, 7), (0, 0))
        assert_planes_are_the_single_calls(plan, x, 1, (0, 7), (0, 0), planes, "negative zeros")


def test_one_channel_and_sixty_four():
    m, d = 257, 16
    n_in = 2 * block_len(m) + 300
    x = ints12(9, n_in)
    rng = np.random.default_rng(64)
    shifts = [int(v) for v in rng.integers(-2048, 2048, 64)]
    phases = [int(v) for v in rng.integers(-5000, 5000, 64)]
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(3, m))
        for s, ph in ((0, 0), (-1000, 77)):
            assert_planes_are_the_single_calls(plan, x, d, (s,), (ph,), device_bank(plan, x, d, (s,), (ph,)), f"C=1 s={s}")
        assert_planes_are_the_single_calls(plan, x, d, shifts, phases, device_bank(plan, x, d, shifts, phases), "C=64")
        zeros = device_bank(plan, x, d, shifts[:3])                # phase0 omitted: zeros
        assert_planes_are_the_single_calls(plan, x, d, shifts[:3], (0, 0, 0), zeros, "phase0 = None")


def test_more_blocks_than_workgroups():
    """600 blocks: more than the 512 workgroups of a whole device (and 37 per workgroup of the 8-CU child), so every workgroup's
    second block runs on loads issued during the channel loop of its first."""
    m, d = 257, 16
    n_in = 600 * block_len(m) + 100
    x = ints12(6, n_in)
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(6, m))
        assert_planes_are_the_single_calls(plan, x, d, SHIFTS, PHASES, device_bank(plan, x, d, SHIFTS, PHASES), "600 blocks")


# ---- 3: an independent yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(257, 16), (2049, 64)])
def test_every_channel_is_within_the_fir_bound_of_float64_numpy(m, d):
    n_in = 3 * block_len(m) + 1000
    x, h = ints12(m, n_in), channel_taps(d, m)
    shifts, phases = (0, 611, -2048), (0, 5, 4095)
    worst = 0.0
    with SpectrumPlan(N) as plan:
        plan.set_fir(h)
        planes = device_bank(plan, x, d, shifts, phases)
        for c, (s, ph) in enumerate(zip(shifts, phases)):
            worst = max(worst, check(planes[c], ref_fir(x, h, d, s, ph), tol_of(x, h), f"M={m} D={d} channel {c} (s={s})"))
    print(f"M={m} D={d}: worst err/tol {worst:.2e}")


# ---- 4: the stride between planes -----------------------------------------------------------------------------------------------
def test_padding_between_planes_is_left_alone_and_equal_strides_pack_the_planes():
    m, d = 129, 4
    x = ints12(4, 2 * block_len(m) + 77)
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(4, m))
        packed = device_bank(plan, x, d, SHIFTS, PHASES)                        # out_stride == n_out
        padded = device_bank(plan, x, d, SHIFTS, PHASES, pad=37)                # (device_bank checks the sentinels)
        assert same_u32(packed, padded)
        assert_planes_are_the_single_calls(plan, x, d, SHIFTS, PHASES, packed, "packed")


# ---- 5: int16, and the host entries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(257, 16), (2049, 64), (1, 1)])
def test_int16_equals_complex64_on_the_widened_samples(m, d):
    n_in = 3 * block_len(m) + 1000
    x16 = ints12_i16(m, n_in)
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m, m))
        a = device_bank(plan, x16, d, SHIFTS, PHASES, ci16=True)
        assert same_u32(a, device_bank(plan, widen_flat(x16), d, SHIFTS, PHASES)), m
        assert_planes_are_the_single_calls(plan, x16, d, SHIFTS, PHASES, a, f"int16 M={m}", ci16=True)


@pytest.mark.parametrize("m,d,sample0", [(257, 16, 0), (257, 16, 16 * 5 + 3), (2049, 64, 64 * 7), (2, 4, 2)])
def test_host_entry_equals_device_entry_across_chunks(m, d, sample0, monkeypatch):
    """Chunks of 3 blocks over 10 blocks: the host entry on (prefix, iq) returns the device entry's bits on prefix || iq from the
    first sample whose stream index is a multiple of D, with a non-zero prefix and with none, from both formats."""
    monkeypatch.setenv("SDRK_FIR_CHUNK_BLOCKS", "3")
    n = 9 * block_len(m) + 77                                                   # 10 blocks of the virtual stream
    x16, pre16 = ints12_i16(m + d, n), ints12_i16(m + d + 1, max(m - 1, 1))[: m - 1]
    x, pre = widen_flat(x16), widen_flat(pre16)
    j0 = (-sample0) % d
    with SpectrumPlan(N) as plan:
        plan.set_fir(random_taps(m + 1, m))
        for prefix, prefix16 in ((pre, pre16), (None, None)):
            virt = np.concatenate((pre if prefix is not None else np.zeros(m - 1, np.complex64), x))
            phases = [(s * (sample0 + j0)) % N for s in SHIFTS]
            dev = device_bank(plan, virt[j0:], d, SHIFTS, phases)
            host = plan.fir_bank(x, SHIFTS, decim=d, prefix=prefix, sample0=sample0)
            assert host.shape == dev.shape == (5, (n - j0 - 1) // d + 1) and same_u32(host, dev), (m, d, prefix is not None)
            assert same_u32(plan.fir_bank_ci16(x16, SHIFTS, decim=d, prefix=prefix16, sample0=sample0), host), (m, "int16")
            assert same_u32(host[1], plan.fir(x, decim=d, shift_bins=611, prefix=prefix, sample0=sample0))   # the single host call
        monkeypatch.delenv("SDRK_FIR_CHUNK_BLOCKS")                              # the shipped chunk size (one chunk here)
        assert same_u32(plan.fir_bank(x, SHIFTS, decim=d, prefix=None, sample0=sample0), host)
        assert same_u32(fir_bank(x, random_taps(m + 1, m), SHIFTS, d), plan.fir_bank(x, SHIFTS, decim=d)), "module function"


# ---- 6: streaming ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci16", [False, True])
def test_channel_bank_stream_in_pieces_equals_channel_streams(ci16):
    pieces, d, fs = (1, 4095, 4097, 10000), 16, 2.4e6
    n = sum(pieces)
    x = ints12_i16(21, n) if ci16 else ints12(21, n)
    h = channel_taps(d)
    offsets = [s * fs / N + 100.0 for s in (300, 0, -2048, 300)]
    with ChannelBankStream(None, h, d, offsets, fs) as bank:
        assert bank.shift_bins == [300, 0, -2048, 300] and bank.out_rate == fs / d
        assert bank.tuned_hz == [s * fs / N for s in bank.shift_bins]
        got, at = [], 0
        for p in pieces:
            got.append(bank.push(x[at:at + p]))
            at += p
        assert bank.sample_index == n
    for c, f in enumerate(offsets):
        with ChannelStream(None, h, d, f, fs) as ch:
            at = 0
            for i, p in enumerate(pieces):
                assert same_u32(got[i][c], ch.push(x[at:at + p])), (c, i)
                at += p
    assert np.concatenate(got, axis=1).shape == (4, (n + d - 1) // d)


# ---- 7: repeated calls, and the neighbours ----------------------------------------------------------------------------------------
def test_repeated_calls_give_identical_bits_and_the_neighbours_are_unchanged():
    m, d = 257, 16
    x = ints12(3, 8 * N)
    with SpectrumPlan(N) as plan:
        plan.set_pfb(pfb_prototype(N, 4))
        row, pfb_row = plan.spectrum_db(x[:N]), plan.pfb_db(x)
        plan.set_fir(random_taps(m, m))
        one = plan.fir(x, decim=d, shift_bins=611)
        a = device_bank(plan, x, d, SHIFTS, PHASES)
        assert same_u32(a, device_bank(plan, x, d, SHIFTS, PHASES))
        h = plan.fir_bank(x, SHIFTS, decim=d)
        assert same_u32(h, plan.fir_bank(x, SHIFTS, decim=d)) and same_u32(h[1], one)
        assert same_bits(plan.spectrum_db(x[:N]), row) and same_bits(plan.pfb_db(x), pfb_row)
        assert same_bits(plan.fir(x, decim=d, shift_bins=611), one)
        assert plan.pfb_taps == 4 and plan.fir_taps == m


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_device():
    lib = _ffi.lib()
    h = channel_taps(4)
    m = h.shape[0]
    n_out = ctypes.c_size_t()
    each = (ctypes.c_float * 2)()
    ok = (ctypes.c_int * 3)(0, 5, -5)
    many = (ctypes.c_int * 65)()
    x = ints12(1, N)
    full = N - m + 1
    device = (lib.sdrk_exec_device_chanbank, lib.sdrk_exec_device_chanbank_ci16)
    host = (lib.sdrk_exec_host_chanbank, lib.sdrk_exec_host_chanbank_ci16)
    with SpectrumPlan(1024) as p, DevBuf(1 << 16) as d:
        assert lib.sdrk_exec_device_chanbank(p.handle, d.p, 1024, 1, 3, ok, None, d.p, 1024, None) == _ffi.SDRK_ERR_UNSUPPORTED
        assert b"4096" in lib.sdrk_last_error()
        assert lib.sdrk_exec_host_chanbank(p.handle, None, d.p, 1024, 1, 3, ok, 0, d.p, 1024, ctypes.byref(n_out)) == _ffi.SDRK_ERR_UNSUPPORTED
        assert p.spectrum_db(x[:1024]).shape == (1024,)                           # a plan that has refused still works
    with SpectrumPlan(N, precision="double") as p64, DevBuf(1 << 16) as d:
        for fn in device:
            assert fn(p64.handle, d.p, N, 1, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"float64" in lib.sdrk_last_error()
        assert p64.spectrum_db(x.astype(np.complex128)).shape == (N,)
    with SpectrumPlan(N) as p, DevBuf(1 << 18) as d:
        for fn in device:
            assert fn(p.handle, d.p, N, 1, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"no FIR filter" in lib.sdrk_last_error()
        for fn in host:
            assert fn(p.handle, None, d.p, N, 1, 3, ok, 0, d.p, N, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        with pytest.raises(ValueError):
            p.fir_bank(x, [0, 1])
        p.set_fir(h)
        for fn in device:
            for c in (0, -1, 65):
                assert fn(p.handle, d.p, N, 1, c, many, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"n_chan" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 1, 3, None, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"shift_bins pointer" in lib.sdrk_last_error()
            for bad in ((0, -2049, 5), (0, 5, 2048)):
                assert fn(p.handle, d.p, N, 1, 3, (ctypes.c_int * 3)(*bad), None, d.p, N, None) == _ffi.SDRK_ERR_INVALID
                assert b"shift_bins[" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 1, 3, ok, None, d.p, full - 1, None) == _ffi.SDRK_ERR_INVALID and b"out_stride" in lib.sdrk_last_error()
            assert fn(p.handle, None, N, 1, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, N, 1, 3, ok, None, None, N, None) == _ffi.SDRK_ERR_INVALID and b"NULL" in lib.sdrk_last_error()
            assert fn(p.handle, d.p, m - 1, 1, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"n_in" in lib.sdrk_last_error()
            for decim in (0, 3, 512, -4):
                assert fn(p.handle, d.p, N, decim, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and b"decim" in lib.sdrk_last_error()
            assert fn(None, d.p, N, 1, 3, ok, None, d.p, N, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
        for fn in host:
            for c in (0, 65):
                assert fn(p.handle, None, d.p, N, 1, c, many, 0, d.p, N, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
                assert b"n_chan" in lib.sdrk_last_error()
            assert fn(p.handle, None, d.p, N, 1, 3, None, 0, d.p, N, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
            assert fn(p.handle, None, d.p, N, 1, 3, (ctypes.c_int * 3)(0, 5, 2048), 0, d.p, N, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
            assert fn(p.handle, None, d.p, N, 4, 3, ok, 0, d.p, N // 4 - 1, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
            assert b"out_stride" in lib.sdrk_last_error()
            assert fn(p.handle, None, d.p, N, 1, 3, ok, 0, d.p, N, None) == _ffi.SDRK_ERR_INVALID
            assert fn(p.handle, None, None, N, 1, 3, ok, 0, d.p, N, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_chanbank_timed_each(p.handle, d.p, N, 1, 3, ok, None, d.p, N, 0, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_chanbank_timed_each(p.handle, d.p, N, 1, 65, many, None, d.p, N, 2, each) == _ffi.SDRK_ERR_INVALID
        assert lib.sdrk_exec_device_chanbank_timed_each(p.handle, d.p, N, 1, 3, ok, None, d.p, full - 1, 2, each) == _ffi.SDRK_ERR_INVALID
        # after all the refusals the plan still works: 4096 samples in (32 KiB), three planes of outputs behind them
        ms = p.exec_device_fir_bank_timed_each(d.p.value, N, d.p.value + (1 << 15), [0, 5, -5], launches=3, decim=4)
        assert len(ms) == 3 and all(v > 0 for v in ms)
        planes = p.fir_bank(x, [0, 5, -5], decim=4)
        for c, s in enumerate((0, 5, -5)):
            check(planes[c], ref_fir(np.concatenate((np.zeros(m - 1), x)), h, 4, s), tol_of(x, h), f"after the refusals, channel {c}")


# ---- 9: once more with several blocks per workgroup -------------------------------------------------------------------------------
def test_everything_above_with_the_grids_of_an_8_cu_device():
    """SDRK_NUM_CUS=8: 16 workgroups, so several blocks per workgroup wherever there are more than 16 blocks, and the loads in
    flight across iterations and across the channel loop are covered — in a fresh child process, as the plans read the variable
    when they are made."""
    env = dict(os.environ, SDRK_NUM_CUS="8", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.abspath(__file__), "-k", "not 8_cu"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])

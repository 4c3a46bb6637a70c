"""The filter-and-sum beamformer without a GPU: header, ctypes table and exports agree on the twelve symbols (SDRK_VERSION stays
500, the section is the header's last); the refusals that need no device; beam_taps and mvdr_weights in plain numpy; BeamStream's
bookkeeping with the C call replaced by the float64 numpy definition; `extract` without --weights still refuses a multi-channel
recording with the message it had."""
import ctypes
import os
import re

import numpy as np
import pytest

import sdr_iq_visualizer_amd as pkg
from sdr_iq_visualizer_amd import _ffi, cli, sigmf_io, spectrum
from sdr_iq_visualizer_amd.spectrum import BeamStream, beam_taps, freq_word, mvdr_weights
from tests.host_helpers import bare_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
TWELVE = sorted(["sdrk_plan_set_beam", "sdrk_plan_beam_channels", "sdrk_plan_beam_taps", "sdrk_exec_device_beam",
                 "sdrk_exec_device_beam_ci16", "sdrk_exec_device_beam_iq8", "sdrk_exec_device_beam_timed_each",
                 "sdrk_exec_device_beam_ci16_timed_each", "sdrk_exec_device_beam_iq8_timed_each", "sdrk_exec_host_beam",
                 "sdrk_exec_host_beam_ci16", "sdrk_exec_host_beam_iq8"])


def test_header_table_and_exports_agree_on_the_twelve_symbols():
    text = open(os.path.join(REPO, "include", "sdrk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sdrk_[a-z0-9_]+)\s*\(", header)) if "beam" in n)
    table = {name: args for name, _, args in _ffi.SYMBOLS}
    assert declared == TWELVE == sorted(n for n in table if "beam" in n)
    for fragment in ("_fir", "ddc", "chanbank", "downconv", "_xspec", "_corrmat"):    # the sets the other header tests pin stay theirs
        assert not [n for n in TWELVE if fragment in n], fragment
    for n in TWELVE:
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", header).group(1).split(",")
        assert len(params) == len(table[n]), n
    assert "#define SDRK_VERSION 500" in text and _ffi.ABI_VERSION == 500
    titles = re.findall(r"^/\* ---- (.*?) -", text, flags=re.M)
    assert titles[-1].startswith("filter-and-sum beamformer"), titles[-3:]        # a new section at the END of the header
    section = text.split("filter-and-sum beamformer")[1]
    for word in ("h_c = conj(w_c) h", "C + 1 transforms", "plain float32 adds", "+0.0 + 0.0i in every channel, for cu8 too",
                 "byte 0x80 for SDRK_IQ8_UNSIGNED", "sdrk_plan_set_beam", "several beams per call"):
        assert word in section, word
    handle = ctypes.CDLL(_ffi.library_path())
    assert all(hasattr(handle, n) for n in TWELVE)
    for name in ("BeamStream", "beam_taps", "beamform", "mvdr_weights"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(spectrum, name)


def test_refusals_that_need_no_device():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    each = (ctypes.c_float * 2)()
    n_out = ctypes.c_size_t()
    assert lib.sdrk_plan_set_beam(None, 2, 3, p) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_plan_beam_channels(None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_plan_beam_taps(None) == _ffi.SDRK_ERR_INVALID
    for fn in (lib.sdrk_exec_device_beam, lib.sdrk_exec_device_beam_ci16):
        assert fn(None, p, 8, 5, 7, 0, p, None) == _ffi.SDRK_ERR_INVALID and lib.sdrk_last_error() == b"plan is NULL"
    assert lib.sdrk_exec_device_beam_iq8(None, p, 2, 8, 5, 7, 0, p, None) == _ffi.SDRK_ERR_INVALID
    assert b"iq8_format 2 is neither" in lib.sdrk_last_error()                    # the 8-bit spectra's message, before the plan
    assert lib.sdrk_exec_device_beam_iq8(None, p, 1, 8, 5, 7, 0, p, None) == _ffi.SDRK_ERR_INVALID
    assert lib.sdrk_exec_host_beam_iq8(None, None, p, 7, 8, 5, 7, 0, p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
    assert b"iq8_format 7" in lib.sdrk_last_error()
    for fn in (lib.sdrk_exec_device_beam_timed_each, lib.sdrk_exec_device_beam_ci16_timed_each):
        assert fn(None, p, 8, 5, 7, 0, p, 0, each) == _ffi.SDRK_ERR_INVALID and b"launches" in lib.sdrk_last_error()
    for fn in (lib.sdrk_exec_host_beam, lib.sdrk_exec_host_beam_ci16):
        assert fn(None, None, p, 8, 5, 7, 0, p, ctypes.byref(n_out)) == _ffi.SDRK_ERR_INVALID
    # the Python layer: before any device call
    plan = bare_plan(N)
    plan.beam_channels, plan.beam_taps = 0, 0
    x = np.zeros((100, 3), np.complex64)
    with pytest.raises(ValueError, match="set_beam"):
        plan.beam(x, 5)
    plan.beam_channels, plan.beam_taps = 3, 9
    for bad in (np.zeros((2, 0)), np.zeros((9, 4)), np.zeros((3, 2050)), np.zeros(5)):
        with pytest.raises(ValueError, match="beam taps"):
            plan.set_beam(bad)
    for kw in ({"decim": 0}, {"decim": 257}, {"sample0": -1}, {"prefix": np.zeros((7, 3), np.complex64)}):
        with pytest.raises(ValueError):
            plan.beam(x, 5, **kw)
    with pytest.raises(ValueError, match="channels"):
        plan.beam(np.zeros((100, 2), np.complex64), 5)
    with pytest.raises(ValueError, match="int16"):
        plan.beam_ci16(np.zeros((100, 3, 2), np.int8), 5)
    with pytest.raises(ValueError, match=r"\(n, C, 2\)"):
        plan.beam_ci8(np.zeros((100, 3), np.uint8), 5)
    with pytest.raises(ValueError, match="dtype of iq"):
        plan.beam_ci8(np.zeros((100, 3, 2), np.uint8), 5, prefix=np.zeros((8, 3, 2), np.int8))
    with pytest.raises(ValueError, match="at least the 9 taps"):
        plan.beam_outputs(8)


def test_beam_taps_is_conj_w_times_h():
    w, h = np.array([1.0, 1j, -0.5 + 0.25j]), np.array([0.25, 0.5, 0.25 - 1j, 3.0])
    t = beam_taps(w, h)
    assert t.shape == (3, 4) and t.dtype == np.complex64 and t.flags.c_contiguous
    assert np.array_equal(t, (np.conj(w)[:, None] * h[None, :]).astype(np.complex64))
    x = np.array([2.0 - 1j, 0.5j, 1.0])                                           # one element: y = w^H x, then the filter
    assert np.allclose((t * x[:, None]).sum(axis=0), np.vdot(w, x) * h, rtol=1e-6)
    for bad_w, bad_h in ((np.zeros(0), h), (np.zeros(9), h), (w, np.zeros(0)), (w, np.zeros(2050))):
        with pytest.raises(ValueError):
            beam_taps(bad_w, bad_h)


def test_mvdr_weights_are_distortionless_and_null_a_rank_one_interferer():
    c = 5
    a = np.exp(0.7j * np.arange(c))
    j = np.exp(-1.1j * np.arange(c))
    rng = np.random.default_rng(3)
    g = rng.standard_normal((c, c)) + 1j * rng.standard_normal((c, c))
    for R in (np.eye(c), g @ g.conj().T + np.eye(c)):
        w = mvdr_weights(R, a)
        assert w.shape == (c,) and w.dtype == np.complex128 and abs(np.vdot(w, a) - 1) < 1e-12
    loading, power = 1e-3, 1e6
    R = power * np.outer(j, j.conj())                                             # singular without the loading
    w = mvdr_weights(R, a, loading)
    assert abs(np.vdot(w, a) - 1) < 1e-12
    # the closed form (matrix inversion lemma): w ~ a - j (j^H a) P / (loading + P C); what is left of the interferer is
    # |w^H j| = loading |j^H a| / ((loading + P C) a^H R^-1 a loading) ~ loading / (P C) relative to its amplitude
    ria = (a - j * np.vdot(j, a) * power / (loading + power * c)) / loading
    want = ria / np.vdot(a, ria)
    assert np.abs(w - want).max() < 1e-6 * np.abs(want).max()
    assert abs(np.vdot(w, j)) < 1e-6                                              # nulled: 1e-9 / (1 - |j^H a|^2 / C^2) analytically
    assert abs(np.vdot(mvdr_weights(R + np.eye(c), a), j)) < 1e-5
    for bad in ((np.eye(3), a, 0.0), (np.eye(c), a, -1.0), (np.zeros((c, c + 1)), a, 0.0)):
        with pytest.raises(ValueError):
            mvdr_weights(*bad)


def ref_beam(x, h, word, d, index0):
    """float64, the header's definition on the virtual stream x (prefix included)."""
    c, m = h.shape
    s = ((word + 0x80000) >> 20) & 4095
    rot = np.exp(2j * np.pi * s * np.arange(m) / N)
    v = sum(np.convolve(x[:, k].astype(np.complex128), h[k].astype(np.complex128) * rot, "valid") for k in range(c))
    i = np.arange(v.shape[0], dtype=np.uint64)
    phase = (np.uint64(word) * ((np.uint64(index0) + i) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)
    y = v * np.exp(-2j * np.pi * (phase.astype(np.float64) / 2.0 ** 32))
    return y[((np.uint64(index0 % d) + i) % np.uint64(d)) == 0]


class NumpyBeamPlan:
    """Stands in for SpectrumPlan behind a BeamStream: the float64 definition, and a record of what it was handed."""

    def __init__(self):
        self.calls = []

    def set_beam(self, taps):
        self.h = np.asarray(taps, np.complex64)
        return self.h.shape[0]

    def _run(self, x, wide, word, decim, prefix, sample0):
        m = self.h.shape[1]
        assert (prefix is None) if (m == 1 or sample0 == 0) else (prefix.shape == (m - 1,) + x.shape[1:] and prefix.dtype == x.dtype)
        self.calls.append((x.dtype, x.shape[0], sample0))
        pad = np.zeros((m - 1, x.shape[1]), np.complex64) + ((0.5 + 0.5j) if x.dtype == np.uint8 else 0)
        virt = np.concatenate((pad if prefix is None else wide(prefix), wide(x)))
        return ref_beam(virt, self.h, word, decim, sample0).astype(np.complex64)

    def beam(self, x, word, *, decim, prefix, sample0):
        return self._run(x, lambda a: a, word, decim, prefix, sample0)

    def beam_ci16(self, x, word, *, decim, prefix, sample0):
        return self._run(x, lambda a: a[..., 0].astype(np.float32) + 1j * a[..., 1].astype(np.float32), word, decim, prefix, sample0)

    def beam_ci8(self, x, word, *, decim, prefix, sample0):
        return self._run(x, spectrum.iq8_to_c64, word, decim, prefix, sample0)


@pytest.mark.parametrize("dtype", [np.complex64, np.int16, np.int8, np.uint8])
def test_beam_stream_keeps_the_tail_the_index_and_the_exact_offset(dtype):
    c, m, d, fs = 3, 33, 7, 2.4e6
    rng = np.random.default_rng(5)
    h = ((rng.standard_normal((c, m)) + 1j * rng.standard_normal((c, m))) / m).astype(np.complex64)
    n = 5000
    if dtype == np.complex64:
        x = (rng.standard_normal((n, c)) + 1j * rng.standard_normal((n, c))).astype(np.complex64)
        wide = x
    else:
        info = np.iinfo(dtype)
        x = rng.integers(max(info.min, -2000), min(info.max, 2000) + 1, (n, c, 2)).astype(dtype)
        wide = spectrum.iq8_to_c64(x) if x.dtype.itemsize == 1 else (x[..., 0].astype(np.float32) + 1j * x[..., 1]).astype(np.complex64)
    plan = NumpyBeamPlan()
    bs = BeamStream(plan, h, d, 123456.0, fs)
    assert bs.freq_word == freq_word(123456.0, fs) and bs.channels == c and bs.ntaps == m and bs.out_rate == fs / d
    cuts = [0, 1, 2, 40, 40, 1000, 4999, n]
    out = [bs.push(x[a:b]) for a, b in zip(cuts, cuts[1:])]
    assert bs.sample_index == n and bs._tail.shape == (m - 1,) + x.shape[1:] and np.array_equal(bs._tail, x[-(m - 1):])
    assert [k[2] for k in plan.calls] == [a for a, b in zip(cuts, cuts[1:]) if b > a]       # an empty piece makes no call
    assert [v.shape[0] for v in out] == [len(range(-(-a // d) * d, b, d)) for a, b in zip(cuts, cuts[1:])]
    pad = np.zeros((m - 1, c), np.complex64) + ((0.5 + 0.5j) if dtype == np.uint8 else 0)
    want = ref_beam(np.concatenate((pad, wide)), h, bs.freq_word, d, 0)
    got = np.concatenate(out)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    with pytest.raises(ValueError, match="one kind throughout"):
        bs.push(np.zeros((4, c, 2), np.int16) if dtype != np.int16 else np.zeros((4, c), np.complex64))
    with pytest.raises(ValueError, match="shape"):
        bs.push(x[:4, :2])


def test_cli_extract_without_weights_still_refuses_a_multi_channel_recording(tmp_path, capsys):
    x = np.zeros((N, 3, 2), np.uint8)
    sigmf_io.write_sigmf(str(tmp_path / "rec"), x, 2.4e6, 100e6, datatype="cu8", num_channels=3)
    rc = cli.main(["extract", str(tmp_path / "rec"), "--offset-hz", "1e5", "--decim", "4", "--out", str(tmp_path / "out")])
    assert rc == 2
    assert "extract takes a single-channel recording; this one has core:num_channels = 3" in capsys.readouterr().err
    # with --weights the arguments are checked before any device call
    np.save(tmp_path / "w2.npy", np.ones(2))
    np.save(tmp_path / "w3.npy", np.ones(3))
    base = ["extract", str(tmp_path / "rec"), "--decim", "4", "--out", str(tmp_path / "out")]
    assert cli.main(base + ["--weights", str(tmp_path / "w2.npy"), "--offset-hz", "1e5"]) == 2
    assert "(3,) weights or (3, M) taps" in capsys.readouterr().err
    assert cli.main(base + ["--weights", str(tmp_path / "w3.npy"), "--offset-hz", "1e5", "2e5"]) == 2
    assert "one --offset-hz" in capsys.readouterr().err

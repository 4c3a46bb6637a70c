"""int16 I,Q input against complex64 input, leg by leg (profiles/ci16/SUMMARY.md is written from this tool's output).

    python tools/bench_ci16.py [--frames-log2 20] [--host-samples-log2 27] [--json out.json] [--only device|lengths|host|live]

Both legs of a comparison run in ONE process on the same sample values, alternating, after a warm-up by time (an idle MI355X
needs tens of milliseconds of load to reach its sustained clock); the figure of a leg is the MEDIAN of its per-launch times
(sdrk_exec_device*_timed_each: events between consecutive launches) or, at the numpy boundary, of its per-call wall times.
Requirements checked here (exit status 1 when one is missed): ci16 samples/s >= 1.06 x complex64 samples/s device-resident at
N = 4096 (Hann) and at the numpy boundary from pageable and from pinned arrays."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)
import numpy as np

import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd import _ffi, synth  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

HBM_PEAK = 8.0e12
REQUIRED = 1.06


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    _ffi.check(_ffi.lib().sdrk_dev_alloc(0, nbytes, ctypes.byref(p)))
    return p


def set_form(form):
    """The load form of the N = 4096 int16 kernel for the launches that follow (SDRK_CI16_FORM; None: the library's default)."""
    if form is None:
        os.environ.pop("SDRK_CI16_FORM", None)
    else:
        os.environ["SDRK_CI16_FORM"] = form


def device_leg(n, n_frames, window, rounds=6, per_round=5, warm_s=0.4, forms=()):
    """Median ms per launch of exec_device (complex64) and exec_device_ci16 on the same generated values, alternating;
    `forms`: also the named load forms of the N = 4096 int16 kernel, in the same alternation."""
    lib = _ffi.lib()
    d16, d64, out = dev_alloc(n_frames * n * 4), dev_alloc(n_frames * n * 8), dev_alloc(n_frames * n * 4)
    try:
        _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, n_frames, n, d16, None))
        _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, n, d64, None))
        with SpectrumPlan(n, window=window) as plan:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                plan.exec_device_timed_each(d64.value, n_frames, out.value, 2)
                plan.exec_device_ci16_timed_each(d16.value, n_frames, out.value, 2)
                for form in forms:
                    set_form(form)
                    plan.exec_device_ci16_timed_each(d16.value, n_frames, out.value, 2)
                set_form(None)
            c64, ci16, by_form = [], [], {form: [] for form in forms}
            for _ in range(rounds):
                c64 += plan.exec_device_timed_each(d64.value, n_frames, out.value, per_round)
                ci16 += plan.exec_device_ci16_timed_each(d16.value, n_frames, out.value, per_round)
                for form in forms:
                    set_form(form)
                    by_form[form] += plan.exec_device_ci16_timed_each(d16.value, n_frames, out.value, per_round)
                set_form(None)
    finally:
        for d in (d16, d64, out):
            lib.sdrk_dev_free(0, d)
    m64, m16 = statistics.median(c64), statistics.median(ci16)
    samples = n_frames * n
    extra = {}
    for form, ms in by_form.items():
        m = statistics.median(ms)
        extra[f"ci16_{form}_ms"] = round(m, 4)
        extra[f"ci16_{form}_ratio_samples_per_s"] = round(m64 / m, 4)
        extra[f"ci16_{form}_fraction_of_8TBs_at_8B"] = round(samples * 8 / (m * 1e-3) / HBM_PEAK, 4)
    return {**extra, "nfft": n, "frames": n_frames, "window": window or "rect", "launches_per_leg": len(c64),
            "c64_ms": round(m64, 4), "ci16_ms": round(m16, 4), "ratio_samples_per_s": round(m64 / m16, 4),
            "c64_gsamples_s": round(samples / m64 / 1e6, 2), "ci16_gsamples_s": round(samples / m16 / 1e6, 2),
            "c64_fraction_of_8TBs_at_12B": round(samples * 12 / (m64 * 1e-3) / HBM_PEAK, 4),
            "ci16_fraction_of_8TBs_at_8B": round(samples * 8 / (m16 * 1e-3) / HBM_PEAK, 4),
            "c64_ms_min_max": [round(min(c64), 4), round(max(c64), 4)], "ci16_ms_min_max": [round(min(ci16), 4), round(max(ci16), 4)]}


def host_leg(n, log2_samples, pinned, calls=15, warm_s=0.6):
    n_frames = (1 << log2_samples) // n
    x16 = synth.synth_iq_ci16(7, 0, 64, n)
    reps = n_frames // 64
    make = pkg.pinned_empty if pinned else (lambda shape, dtype: np.empty(shape, dtype))
    a16 = make((n_frames, n, 2), np.int16)
    a64 = make((n_frames, n), np.complex64)
    out = make((n_frames, n), np.float32)
    a16.reshape(reps, 64, n, 2)[...] = x16
    a64[...] = (a16[..., 0].astype(np.float32) + 1j * a16[..., 1].astype(np.float32))
    out[...] = 0
    t64, t16 = [], []
    with SpectrumPlan(n) as plan:
        t_warm = time.perf_counter()
        while time.perf_counter() - t_warm < warm_s:                 # warm-up by time, both legs
            plan.spectrum_db(a64, out=out); plan.spectrum_db_ci16(a16, out=out)
        for i in range(calls):
            t0 = time.perf_counter(); plan.spectrum_db(a64, out=out); t1 = time.perf_counter()
            plan.spectrum_db_ci16(a16, out=out); t2 = time.perf_counter()
            t64.append(t1 - t0); t16.append(t2 - t1)
        same = bool(np.array_equal(plan.spectrum_db_ci16(a16[:256]).view(np.uint32), plan.spectrum_db(a64[:256]).view(np.uint32)))
    m64, m16 = statistics.median(t64), statistics.median(t16)
    s = n_frames * n
    return {"nfft": n, "samples": s, "input": "pinned" if pinned else "pageable", "calls_per_leg": calls, "bit_identical": same,
            "c64_ms": round(m64 * 1e3, 2), "ci16_ms": round(m16 * 1e3, 2), "ratio_samples_per_s": round(m64 / m16, 4),
            "c64_input_GBs": round(s * 8 / m64 / 1e9, 2), "ci16_input_GBs": round(s * 4 / m16 / 1e9, 2),
            "c64_gsamples_s": round(s / m64 / 1e9, 3), "ci16_gsamples_s": round(s / m16 / 1e9, 3)}


def live_leg(n=4096, calls=3000):
    x16 = synth.synth_iq_ci16(1, 0, 1, n)[0]
    x64 = synth.synth_iq(1, 0, 1, n)[0]
    out = np.empty(n, np.float32)
    with SpectrumPlan(n) as plan:
        for _ in range(300):
            plan.spectrum_db(x64, out=out); plan.spectrum_db_ci16(x16, out=out)
        t64, t16 = [], []
        for _ in range(calls):
            t0 = time.perf_counter(); plan.spectrum_db(x64, out=out); t1 = time.perf_counter()
            plan.spectrum_db_ci16(x16, out=out); t2 = time.perf_counter()
            t64.append(t1 - t0); t16.append(t2 - t1)
    return {"nfft": n, "calls": calls, "c64_us": round(statistics.median(t64) * 1e6, 2), "ci16_us": round(statistics.median(t16) * 1e6, 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=20)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--only", default=None, choices=["device", "lengths", "host", "live"])
    ap.add_argument("--only-lengths", action="store_true", help="with --only device: also the N = 65536 leg (kernel traces)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    want = (lambda k: args.only in (None, k))
    if want("device"):
        r = device_leg(4096, 1 << args.frames_log2, "hann", forms=("direct", "wide"))
        r["required_ratio"], r["met"] = REQUIRED, r["ratio_samples_per_s"] >= REQUIRED
        ok &= r["met"]
        res["device_4096_hann"] = r
        print(json.dumps({"device_4096_hann": r}), flush=True)
    if args.only == "device" and args.only_lengths:
        print(json.dumps({"lengths": [device_leg(65536, 4096, "hann")]}), flush=True)
    if want("lengths"):
        res["lengths"] = [device_leg(1024, 1 << 18, "hann"), device_leg(16384, 1 << 14, "hann"), device_leg(65536, 4096, "hann")]
        print(json.dumps({"lengths": res["lengths"]}), flush=True)
    if want("host"):
        res["host"] = []
        for pinned in (False, True):
            r = host_leg(4096, args.host_samples_log2, pinned)
            r["required_ratio"], r["met"] = REQUIRED, r["ratio_samples_per_s"] >= REQUIRED
            ok &= r["met"]
            res["host"].append(r)
            print(json.dumps({"host": r}), flush=True)
    if want("live"):
        res["live_frame"] = live_leg()
        print(json.dumps({"live_frame": res["live_frame"]}), flush=True)
    res["requirements_met"] = bool(ok)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

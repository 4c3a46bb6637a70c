"""Integrated spectra from int16 I,Q against the two calls it combines, leg by leg (profiles/integrate_ci16/SUMMARY.md is
written from this tool's output).

    python tools/bench_integrate_ci16.py [--frames-log2 20] [--host-samples-log2 27] [--json out.json]
                                         [--only required|k|detectors|host]

Device legs: N = 4096, Hann, dB rows, the same synthetic values resident as complex64 and as int16 pairs; the legs alternate in
one process after a warm-up by time (an idle MI355X needs tens of milliseconds of load to reach its sustained clock) and a
leg's figure is the MEDIAN of its per-launch times (the *_timed_each entry points: events between consecutive launches).
Required (exit status 1 when missed): at K = 16, mean, samples/s of sdrk_exec_device_integrated_ci16 >= 1.06 x EACH of
sdrk_exec_device_integrated (complex64, same K) and sdrk_exec_device_ci16 (per-frame rows), measured in that same alternation.
The byte model allows (8 + 4/K) / (4 + 4/K) and 8 / (4 + 4/K).
Host leg: SpectrumPlan.integrate_ci16 on pageable int16 samples against SpectrumPlan.integrate on the same values as complex64,
median of 7 calls, alternating; required >= 1.5 x in samples/s (the model is 2: upload-bound, almost no output).  Pinned input
is reported without a bar."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.hostmem import pinned_empty  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

HBM_PEAK = 8.0e12
REQUIRED_DEVICE = 1.06
REQUIRED_HOST = 1.5


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    _ffi.check(_ffi.lib().sdrk_dev_alloc(0, nbytes, ctypes.byref(p)))
    return p


def device_legs(n, n_frames, window, legs, rounds=6, per_round=5, warm_s=0.4):
    """legs: [(name, k, detector)].  Per leg three calls on the same values, alternating: the int16 integrated call, the
    complex64 integrated call at the same k and detector, and (once per round) the int16 per-frame call."""
    lib = _ffi.lib()
    d_c64, d_i16 = dev_alloc(n_frames * n * 8), dev_alloc(n_frames * n * 4)
    d_rows, d_int = dev_alloc(n_frames * n * 4), dev_alloc(n_frames * n * 4)
    try:
        _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, n, d_c64, None))
        _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, n_frames, n, d_i16, None))
        with SpectrumPlan(n, window=window) as plan:
            def new(k, det, launches):
                return plan.exec_device_integrated_ci16_timed_each(d_i16.value, n_frames // k, k, d_int.value, launches, detector=det)

            def c64(k, det, launches):
                return plan.exec_device_integrated_timed_each(d_c64.value, n_frames // k, k, d_int.value, launches, detector=det)

            def rows(launches):
                return plan.exec_device_ci16_timed_each(d_i16.value, n_frames, d_rows.value, launches)

            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                rows(2)
                for _, k, det in legs:
                    new(k, det, 2)
                    c64(k, det, 2)
            t_rows, t_new, t_c64 = [], {name: [] for name, _, _ in legs}, {name: [] for name, _, _ in legs}
            for _ in range(rounds):
                t_rows += rows(per_round)
                for name, k, det in legs:
                    t_c64[name] += c64(k, det, per_round)
                    t_new[name] += new(k, det, per_round)
    finally:
        for d in (d_c64, d_i16, d_rows, d_int):
            lib.sdrk_dev_free(0, d)
    m_rows, samples = statistics.median(t_rows), n_frames * n
    out = {"nfft": n, "frames": n_frames, "window": window or "rect", "launches_per_leg": len(t_rows),
           "ci16_per_frame_ms": round(m_rows, 4), "ci16_per_frame_gsamples_s": round(samples / m_rows / 1e6, 2),
           "ci16_per_frame_fraction_of_8TBs_at_8B": round(samples * 8 / (m_rows * 1e-3) / HBM_PEAK, 4),
           "ci16_per_frame_ms_min_max": [round(min(t_rows), 4), round(max(t_rows), 4)], "legs": []}
    for name, k, det in legs:
        m, mc = statistics.median(t_new[name]), statistics.median(t_c64[name])
        byts = 4 + 4.0 / k
        out["legs"].append({"leg": name, "k": k, "groups": n_frames // k, "detector": det,
                            "ci16_integrated_ms": round(m, 4), "ci16_integrated_ms_min_max": [round(min(t_new[name]), 4), round(max(t_new[name]), 4)],
                            "c64_integrated_ms": round(mc, 4), "c64_integrated_ms_min_max": [round(min(t_c64[name]), 4), round(max(t_c64[name]), 4)],
                            "gsamples_s": round(samples / m / 1e6, 2), "c64_integrated_gsamples_s": round(samples / mc / 1e6, 2),
                            "ratio_vs_c64_integrated": round(mc / m, 4), "byte_model_vs_c64_integrated": round((8 + 4.0 / k) / byts, 4),
                            "ratio_vs_ci16_per_frame": round(m_rows / m, 4), "byte_model_vs_ci16_per_frame": round(8 / byts, 4),
                            "fraction_of_8TBs": round(samples * byts / (m * 1e-3) / HBM_PEAK, 4)})
    return out


def host_leg(n, k, log2_samples, calls=7, warm_s=0.5):
    """integrate_ci16 against integrate on the same values, pageable (required) and pinned (reported): wall time per call."""
    rng = np.random.default_rng(1)
    block = rng.integers(-2048, 2048, size=(1 << 20, 2), dtype=np.int64).astype(np.int16)
    x16 = np.tile(block, ((1 << log2_samples) // block.shape[0], 1))
    x64 = x16.astype(np.float32).view(np.complex64).reshape(-1)
    out = {"nfft": n, "k": k, "samples": int(x64.size), "calls": calls}
    with SpectrumPlan(n, window="hann") as plan:
        for kind in ("pageable", "pinned"):
            if kind == "pinned":
                p16, p64 = pinned_empty(x16.shape, np.int16), pinned_empty(x64.shape, np.complex64)
                p16[:] = x16
                p64[:] = x64
                x16, x64 = p16, p64
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                plan.integrate(x64, k); plan.integrate_ci16(x16, k)
            t_old, t_new = [], []
            for _ in range(calls):
                a = time.perf_counter(); old = plan.integrate(x64, k); b = time.perf_counter()
                new = plan.integrate_ci16(x16, k); c = time.perf_counter()
                t_old.append(b - a); t_new.append(c - b)
            mo, mn = statistics.median(t_old), statistics.median(t_new)
            out[kind] = {"integrate_c64_ms": round(mo * 1e3, 2), "integrate_ci16_ms": round(mn * 1e3, 2),
                         "ratio_samples_per_s": round(mo / mn, 4), "ci16_gsamples_s": round(x64.size / mn / 1e9, 3),
                         "ci16_input_GBs": round(x16.nbytes / mn / 1e9, 2), "c64_input_GBs": round(x64.nbytes / mo / 1e9, 2),
                         "same_bits": bool(np.array_equal(old.view(np.uint32), new.view(np.uint32)))}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=20)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--only", default=None, choices=["required", "k", "detectors", "host"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    want = (lambda k: args.only in (None, k))
    frames = 1 << args.frames_log2
    if want("required"):
        r = device_legs(4096, frames, "hann", [("k16", 16, "mean")])
        leg = r["legs"][0]
        leg["required_ratio"] = REQUIRED_DEVICE
        leg["met"] = leg["ratio_vs_c64_integrated"] >= REQUIRED_DEVICE and leg["ratio_vs_ci16_per_frame"] >= REQUIRED_DEVICE
        ok &= leg["met"]
        res["required_4096_hann_mean_db_k16"] = r
        print(json.dumps({"required_4096_hann_mean_db_k16": r}), flush=True)
    if want("k"):
        res["k_sweep"] = device_legs(4096, frames, "hann", [(f"k{k}", k, "mean") for k in (2, 4, 64, 1024)])
        print(json.dumps({"k_sweep": res["k_sweep"]}), flush=True)
    if want("detectors"):
        res["detectors"] = device_legs(4096, frames, "hann", [("max_k16", 16, "max"), ("min_k16", 16, "min")])
        print(json.dumps({"detectors": res["detectors"]}), flush=True)
    if want("host"):
        h = host_leg(4096, 16, args.host_samples_log2)
        h["required_ratio"], h["met"] = REQUIRED_HOST, h["pageable"]["ratio_samples_per_s"] >= REQUIRED_HOST
        ok &= h["met"]
        res["host_4096_k16"] = h
        print(json.dumps({"host_4096_k16": h}), flush=True)
    res["requirements_met"] = bool(ok)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

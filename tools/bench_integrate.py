"""Integrated spectra against the per-frame call, leg by leg (profiles/integrate/SUMMARY.md is written from this tool's output).

    python tools/bench_integrate.py [--frames-log2 20] [--host-samples-log2 27] [--json out.json] [--only required|k|detectors|generic|welch]

The baseline of every device leg is sdrk_exec_device (the per-frame kernels, which this feature does not touch) over the
same resident frames in the same process; legs alternate after a warm-up by time (an idle MI355X needs tens of milliseconds of
load to reach its sustained clock) and a leg's figure is the MEDIAN of its per-launch times (the *_timed_each entry points:
events between consecutive launches).  Required (exit status 1 when missed): N = 4096, Hann, mean, dB — samples/s >= 1.06 x the
per-frame call at K = 16 and with all frames as ONE group (the split path and its finalize).  The byte model allows
12 / (8 + 4/K)."""
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
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

HBM_PEAK = 8.0e12
REQUIRED = 1.06


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    _ffi.check(_ffi.lib().sdrk_dev_alloc(0, nbytes, ctypes.byref(p)))
    return p


def device_legs(n, n_frames, window, legs, rounds=6, per_round=5, warm_s=0.4):
    """legs: [(name, k, detector)] with k frames per group (n_frames // k groups).  Returns the per-frame baseline and one
    record per leg, all measured in the same alternation on the same buffers."""
    lib = _ffi.lib()
    d_in, d_rows, d_int = dev_alloc(n_frames * n * 8), dev_alloc(n_frames * n * 4), dev_alloc(n_frames * n * 4)
    try:
        _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, n, d_in, None))
        with SpectrumPlan(n, window=window) as plan:
            def run(k, det, launches):
                return plan.exec_device_integrated_timed_each(d_in.value, n_frames // k, k, d_int.value, launches, detector=det)
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                plan.exec_device_timed_each(d_in.value, n_frames, d_rows.value, 2)
                for _, k, det in legs:
                    run(k, det, 2)
            base, ms = [], {name: [] for name, _, _ in legs}
            for _ in range(rounds):
                base += plan.exec_device_timed_each(d_in.value, n_frames, d_rows.value, per_round)
                for name, k, det in legs:
                    ms[name] += run(k, det, per_round)
    finally:
        for d in (d_in, d_rows, d_int):
            lib.sdrk_dev_free(0, d)
    mb, samples = statistics.median(base), n_frames * n
    out = {"nfft": n, "frames": n_frames, "window": window or "rect", "launches_per_leg": len(base),
           "per_frame_ms": round(mb, 4), "per_frame_gsamples_s": round(samples / mb / 1e6, 2),
           "per_frame_fraction_of_8TBs_at_12B": round(samples * 12 / (mb * 1e-3) / HBM_PEAK, 4),
           "per_frame_ms_min_max": [round(min(base), 4), round(max(base), 4)], "legs": []}
    for name, k, det in legs:
        m = statistics.median(ms[name])
        byts = 8 + 4.0 / k
        out["legs"].append({"leg": name, "k": k, "groups": n_frames // k, "detector": det, "ms": round(m, 4),
                            "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                            "ratio_samples_per_s": round(mb / m, 4), "byte_model_ratio": round(12 / byts, 4),
                            "gsamples_s": round(samples / m / 1e6, 2),
                            "fraction_of_8TBs": round(samples * byts / (m * 1e-3) / HBM_PEAK, 4)})
    return out


def welch_leg(n, log2_samples, calls=7, warm_s=0.5):
    """welch_psd_streamed against welch_psd on the same pageable host samples: wall time per call."""
    rng = np.random.default_rng(1)
    block = (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)).astype(np.complex64)
    x = np.tile(block, (1 << log2_samples) // block.size)
    t_old, t_new = [], []
    with SpectrumPlan(n, window="hann") as plan:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_s:
            plan.welch_psd(x, 1e6); plan.welch_psd_streamed(x, 1e6)
        for _ in range(calls):
            a = time.perf_counter(); old = plan.welch_psd(x, 1e6); b = time.perf_counter()
            new = plan.welch_psd_streamed(x, 1e6); c = time.perf_counter()
            t_old.append(b - a); t_new.append(c - b)
    mo, mn = statistics.median(t_old), statistics.median(t_new)
    return {"nfft": n, "samples": int(x.size), "welch_psd_ms": round(mo * 1e3, 2), "welch_psd_streamed_ms": round(mn * 1e3, 2),
            "ratio_samples_per_s": round(mo / mn, 4), "streamed_input_GBs": round(x.nbytes / mn / 1e9, 2),
            "max_rel_difference": float(np.abs(new - old).max() / old.max())}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=20)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--only", default=None, choices=["required", "k", "detectors", "generic", "welch"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    want = (lambda k: args.only in (None, k))
    frames = 1 << args.frames_log2
    if want("required"):
        r = device_legs(4096, frames, "hann", [("k16", 16, "mean"), ("one_group", frames, "mean")])
        for leg in r["legs"]:
            leg["required_ratio"], leg["met"] = REQUIRED, leg["ratio_samples_per_s"] >= REQUIRED
            ok &= leg["met"]
        res["required_4096_hann_mean_db"] = r
        print(json.dumps({"required_4096_hann_mean_db": r}), flush=True)
    if want("k"):
        res["k_sweep"] = device_legs(4096, frames, "hann", [(f"k{k}", k, "mean") for k in (2, 4, 64, 1024)])
        print(json.dumps({"k_sweep": res["k_sweep"]}), flush=True)
    if want("detectors"):
        res["detectors"] = device_legs(4096, frames, "hann", [("max_k16", 16, "max"), ("min_k16", 16, "min")])
        print(json.dumps({"detectors": res["detectors"]}), flush=True)
    if want("generic"):
        res["generic"] = [device_legs(1024, 1 << 18, "hann", [("k16", 16, "mean")]),
                          device_legs(65536, 4096, "hann", [("k16", 16, "mean")])]
        print(json.dumps({"generic": res["generic"]}), flush=True)
    if want("welch"):
        res["welch"] = welch_leg(1024, args.host_samples_log2)
        print(json.dumps({"welch": res["welch"]}), flush=True)
    res["requirements_met"] = bool(ok)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

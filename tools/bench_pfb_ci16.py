"""Polyphase-filter-bank spectra from int16 I,Q against the complex64 forms, leg by leg (profiles/pfb_ci16/SUMMARY.md is
written from this tool's output).

    python tools/bench_pfb_ci16.py [--frames-log2 16] [--k 16 65536] [--host-samples-log2 26] [--json out.json]

One process on one device, warmed up by time, legs alternating, a leg's figure the MEDIAN of 30 per-launch times (the
*_timed_each entry points; torch.cuda events for the torch widening).  Device-resident: N = 4096, T = 4, hop N, default
prototype, 2^16 frames, per frame and one row per K frames:
  (a) sdrk_exec_device_pfb_ci16 / _pfb_integrated_ci16      the new call on the int16 stream (4 B/sample)
  (b) sdrk_exec_device_pfb / _pfb_integrated                on the widened samples (8 B/sample)
  (c) a torch widen of the int16 stream to float32 pairs, then (b) on the same stream, timed together by events around
      the pair: what a user does today on the device (the widen alone is timed too, as c_torch_widen_alone)
  (d) sdrk_exec_device_ci16 / _integrated_ci16              on as many packed int16 frames: the floor
Asked of the figures: (a) faster than (c) by more than the spread (b) shows between its own rounds of the alternation (exit
status 1 otherwise).  (a) against (b) has no bar: the ratio and (b)'s spread are recorded.
Numpy boundary: pfb_db_ci16 against pfb_db on the widened array, pfb_integrate_ci16 against pfb_integrate at K = 16, 2^26
samples, pageable and pinned; the legs warmed up in turn for a second (staging slots and pinned buffers are allocated by
then), then wall-clock medians of 7 calls, legs alternating.  Asked: the int16 call faster than the complex64 call beyond that
call's own spread (largest / smallest of its 7 calls); the ratios are recorded beside the link-byte model's
(8 + 4)/(4 + 4) = 1.5 per frame and (8 + 4/K)/(4 + 4/K) = 1.94 integrated.
The flagship line is bench.py's own (bench.py --gpus 1 --steps 20 --warmup 5), kept beside this tool's JSON."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd.hostmem import pinned_empty  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype  # noqa: E402


def timed_torch(fn, reps, stream):
    """fn() reps times on a torch stream of its own (not the null stream: its handle, 0, means "the plan's stream" to the
    library), an event between each."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with torch.cuda.stream(stream):
        ev[0].record()
        for i in range(reps):
            fn()
            ev[i + 1].record()
    stream.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def alternate(legs, rounds, per_round, warm_s):
    """Every leg at least once untimed, and on until warm_s has passed; then the timed rounds."""
    t0 = time.perf_counter()
    while True:
        for fn in legs.values():
            fn(1)
        if time.perf_counter() - t0 >= warm_s:
            break
    t = {name: [] for name in legs}
    round_med = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            v = fn(per_round)
            t[name] += v
            round_med[name].append(statistics.median(v))
    return t, round_med


def device_legs(n, taps, frames, k, rounds=6, per_round=5, warm_s=0.4):
    """k = 0: per frame; otherwise one row per k frames (mean)."""
    dev = torch.device("cuda:0")
    hop = n
    L = (frames - 1) * hop + taps * n
    x16 = torch.randint(-32768, 32768, (L, 2), device=dev, dtype=torch.int32).to(torch.int16)
    xw = x16.to(torch.float32)
    tmp = torch.empty_like(xw)
    rows_out = frames if k == 0 else frames // k
    out = torch.empty((rows_out, n), dtype=torch.float32, device=dev)
    plan = SpectrumPlan(n)
    plan.set_pfb(pfb_prototype(n, taps))
    o = out.data_ptr()
    side = torch.cuda.Stream()
    ts = side.cuda_stream
    torch.cuda.synchronize()

    def widen_then(b):
        def pair():
            tmp.copy_(x16)
            b()
        return lambda r: timed_torch(pair, r, side)

    if k == 0:
        legs = {
            "a_ci16": lambda r: plan.exec_device_pfb_ci16_timed_each(x16.data_ptr(), frames, o, r, frame_stride=hop),
            "b_c64": lambda r: plan.exec_device_pfb_timed_each(xw.data_ptr(), frames, o, r, frame_stride=hop),
            "c_widen_then_b": widen_then(lambda: plan.exec_device_pfb(tmp.data_ptr(), frames, o, frame_stride=hop, stream=ts)),
            "c_torch_widen_alone": lambda r: timed_torch(lambda: tmp.copy_(x16), r, side),
            "d_floor_packed_ci16": lambda r: plan.exec_device_ci16_timed_each(x16.data_ptr(), frames, o, r),
        }
    else:
        g = frames // k
        legs = {
            "a_ci16": lambda r: plan.exec_device_pfb_integrated_ci16_timed_each(x16.data_ptr(), g, k, o, r, frame_stride=hop),
            "b_c64": lambda r: plan.exec_device_pfb_integrated_timed_each(xw.data_ptr(), g, k, o, r, frame_stride=hop),
            "c_widen_then_b": widen_then(lambda: plan.exec_device_pfb_integrated(tmp.data_ptr(), g, k, o, frame_stride=hop,
                                                                                 stream=ts)),
            "c_torch_widen_alone": lambda r: timed_torch(lambda: tmp.copy_(x16), r, side),
            "d_floor_packed_ci16": lambda r: plan.exec_device_integrated_ci16_timed_each(x16.data_ptr(), g, k, o, r),
        }
    t, round_med = alternate(legs, rounds, per_round, warm_s)
    torch.cuda.synchronize()
    plan.close()
    med = {name: statistics.median(v) for name, v in t.items()}
    b_rounds = round_med["b_c64"]
    b_spread = max(b_rounds) / min(b_rounds)
    c_total = med["c_widen_then_b"]
    res = {"nfft": n, "taps": taps, "frames": frames, "k": k, "hop": hop, "launches_per_leg": rounds * per_round,
           "ms": {name: round(v, 4) for name, v in med.items()},
           "ms_min_max": {name: [round(min(v), 4), round(max(v), 4)] for name, v in t.items()},
           "b_round_medians_ms": [round(v, 4) for v in b_rounds], "b_spread": round(b_spread, 4),
           "c_sum_of_parts_ms": round(med["b_c64"] + med["c_torch_widen_alone"], 4),
           "a_over_b": round(med["a_ci16"] / med["b_c64"], 4),
           "c_over_a": round(c_total / med["a_ci16"], 4),
           "a_over_d": round(med["a_ci16"] / med["d_floor_packed_ci16"], 4),
           "a_gsamples_s": round(frames * n / med["a_ci16"] / 1e6, 2)}
    res["a_faster_than_c_beyond_b_spread"] = res["c_over_a"] > b_spread
    del x16, xw, tmp, out
    torch.cuda.empty_cache()
    return res


def host_legs(n, taps, samples, k, pinned, reps=7):
    rng = np.random.default_rng(1)
    src16 = rng.integers(-32768, 32768, size=(samples, 2), dtype=np.int64).astype(np.int16)
    if pinned:
        x16 = pinned_empty(src16.shape, np.int16)
        x16[...] = src16
        xw = pinned_empty((samples,), np.complex64)
    else:
        x16 = src16
        xw = np.empty((samples,), np.complex64)
    xw.view(np.float32).reshape(-1, 2)[...] = src16
    plan = SpectrumPlan(n)
    plan.set_pfb(pfb_prototype(n, taps))
    rows = plan.pfb_frames(samples)
    out = pinned_empty((rows, n), np.float32) if pinned else np.empty((rows, n), np.float32)

    def wall(fn):
        def run(r):
            v = []
            for _ in range(r):
                t0 = time.perf_counter()
                fn()
                v.append((time.perf_counter() - t0) * 1e3)
            return v
        return run

    legs = {
        "per_frame_ci16": wall(lambda: plan.pfb_db_ci16(x16, out=out)),
        "per_frame_c64": wall(lambda: plan.pfb_db(xw, out=out)),
        "integrated_ci16": wall(lambda: plan.pfb_integrate_ci16(x16, k)),
        "integrated_c64": wall(lambda: plan.pfb_integrate(xw, k)),
    }
    t, round_med = alternate(legs, reps, 1, 1.0)   # (warmed up by time: at least one untimed call of each leg)
    plan.close()
    med = {name: statistics.median(v) for name, v in t.items()}
    spread = {name: max(v) / min(v) for name, v in t.items()}
    res = {"nfft": n, "taps": taps, "samples": samples, "k": k, "pinned": pinned, "calls_per_leg": reps,
           "ms": {name: round(v, 3) for name, v in med.items()},
           "ms_min_max": {name: [round(min(v), 3), round(max(v), 3)] for name, v in t.items()},
           "c64_spread": {"per_frame": round(spread["per_frame_c64"], 4), "integrated": round(spread["integrated_c64"], 4)},
           "per_frame_c64_over_ci16": round(med["per_frame_c64"] / med["per_frame_ci16"], 4),
           "integrated_c64_over_ci16": round(med["integrated_c64"] / med["integrated_ci16"], 4),
           "model": {"per_frame": 1.5, "integrated": round((8 + 4 / k) / (4 + 4 / k), 4)}}
    res["faster_beyond_c64_spread"] = (res["per_frame_c64_over_ci16"] > spread["per_frame_c64"]
                                       and res["integrated_c64_over_ci16"] > spread["integrated_c64"])
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=16)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 1 << 16])
    ap.add_argument("--host-samples-log2", type=int, default=26)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    frames = 1 << args.frames_log2
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    for k in [0] + [min(k, frames) for k in args.k]:
        r = device_legs(4096, 4, frames, k)
        ok &= r["a_faster_than_c_beyond_b_spread"]
        key = "n4096_t4_hop_n_per_frame" if k == 0 else f"n4096_t4_hop_n_k{k}"
        res[key] = r
        print(json.dumps({key: r}), flush=True)
    if args.host_samples_log2 > 0:
        for pinned in (False, True):
            r = host_legs(4096, 4, 1 << args.host_samples_log2, 16, pinned)
            ok &= r["faster_beyond_c64_spread"]
            key = "host_pinned" if pinned else "host_pageable"
            res[key] = r
            print(json.dumps({key: r}), flush=True)
    res["requirements_met"] = bool(ok)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

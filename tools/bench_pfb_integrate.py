"""Integrated polyphase-filter-bank spectra against what a user could do before, leg by leg (profiles/pfb_integrate/SUMMARY.md
is written from this tool's output).

    python tools/bench_pfb_integrate.py [--frames-log2 16] [--k 16 65536] [--json out.json]

One process on one device, warmed up by time, legs alternating, a leg's figure the MEDIAN of 30 per-launch times (the
*_timed_each entry points; torch.cuda events for the torch reduction).  N = 4096, T = 4, hop N, default prototype, 2^16 frames
(2 GiB of input), one row per K frames:
  (a) sdrk_exec_device_pfb_integrated        the new call (mean; max recorded beside it)
  (b) sdrk_exec_device_pfb                   the per-frame PFB call on the same frames: the same loads, fold and transform,
                                             4 B/sample more written
  (c) (b) + a torch reduction of its dB rows to one row per K (undo the dB, mean over K, dB again): what a user does today
  (d) sdrk_exec_device_integrated            on as many packed frames: the floor
Asked of the figures: (a) not slower than (b) beyond the spread (b) shows between its own rounds of the alternation (exit
status 1 otherwise), (a) faster than (c); (a)/(d) is recorded without a bar."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype  # noqa: E402


def timed_torch(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def legs_for(n, taps, frames, k, rounds=6, per_round=5, warm_s=0.4):
    dev = torch.device("cuda:0")
    hop, groups = n, frames // k
    L = (frames - 1) * hop + taps * n
    x = torch.randint(-2048, 2048, (L, 2), device=dev, dtype=torch.int32).to(torch.float32)
    rows = torch.empty((frames, n), dtype=torch.float32, device=dev)
    out = torch.empty((groups, n), dtype=torch.float32, device=dev)
    red = torch.empty((groups, n), dtype=torch.float32, device=dev)
    plan = SpectrumPlan(n)
    plan.set_pfb(pfb_prototype(n, taps))

    def torch_reduce():   # dB rows -> power -> mean over K -> dB, at most 2^14 rows (256 MiB) of intermediate per pass
        blk = 1 << 14
        if k <= blk:      # whole groups per pass
            step = blk // k
            for g0 in range(0, groups, step):
                g1 = min(groups, g0 + step)
                p = torch.pow(10.0, rows[g0 * k:g1 * k].view(g1 - g0, k, n) * 0.1)
                red[g0:g1] = 10.0 * torch.log10(p.mean(dim=1))
        else:             # a group in passes over its rows, the power summed between them
            for g in range(groups):
                acc = torch.zeros(n, dtype=torch.float32, device=dev)
                for r0 in range(g * k, (g + 1) * k, blk):
                    acc += torch.pow(10.0, rows[r0:min(r0 + blk, (g + 1) * k)] * 0.1).sum(dim=0)
                red[g] = 10.0 * torch.log10(acc / k)

    a = (x.data_ptr(), groups, k, out.data_ptr())
    legs = {
        "a_pfb_integrated_mean": lambda r: plan.exec_device_pfb_integrated_timed_each(*a, r, frame_stride=hop),
        "a_pfb_integrated_max": lambda r: plan.exec_device_pfb_integrated_timed_each(*a, r, frame_stride=hop, detector="max"),
        "b_pfb_per_frame": lambda r: plan.exec_device_pfb_timed_each(x.data_ptr(), frames, rows.data_ptr(), r, frame_stride=hop),
        "c_torch_reduce": lambda r: timed_torch(torch_reduce, r),
        "d_integrated_packed": lambda r: plan.exec_device_integrated_timed_each(*a, r),
    }
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for fn in legs.values():
            fn(1)
    t = {name: [] for name in legs}
    round_med = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            v = fn(per_round)
            t[name] += v
            round_med[name].append(statistics.median(v))
    plan.close()
    med = {name: statistics.median(v) for name, v in t.items()}
    b_rounds = round_med["b_pfb_per_frame"]
    b_spread = max(b_rounds) / min(b_rounds)
    c_total = med["b_pfb_per_frame"] + med["c_torch_reduce"]
    res = {"nfft": n, "taps": taps, "frames": frames, "k": k, "groups": groups, "hop": hop, "launches_per_leg": rounds * per_round,
           "ms": {name: round(v, 4) for name, v in med.items()},
           "ms_min_max": {name: [round(min(v), 4), round(max(v), 4)] for name, v in t.items()},
           "b_round_medians_ms": [round(v, 4) for v in b_rounds], "b_spread": round(b_spread, 4),
           "c_total_ms": round(c_total, 4),
           "a_over_b": round(med["a_pfb_integrated_mean"] / med["b_pfb_per_frame"], 4),
           "a_max_over_b": round(med["a_pfb_integrated_max"] / med["b_pfb_per_frame"], 4),
           "c_over_a": round(c_total / med["a_pfb_integrated_mean"], 4),
           "a_over_d": round(med["a_pfb_integrated_mean"] / med["d_integrated_packed"], 4),
           "a_gsamples_s": round(frames * n / med["a_pfb_integrated_mean"] / 1e6, 2)}
    res["a_not_slower_than_b"] = res["a_over_b"] <= b_spread
    res["a_faster_than_c"] = res["c_over_a"] > 1.0
    del x, rows, out, red
    torch.cuda.empty_cache()
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=16)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 1 << 16])
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    frames = 1 << args.frames_log2
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    for k in args.k:
        k = min(k, frames)
        r = legs_for(4096, 4, frames, k)
        ok &= r["a_not_slower_than_b"] and r["a_faster_than_c"]
        res[f"n4096_t4_hop_n_k{k}"] = r
        print(json.dumps({f"n4096_t4_hop_n_k{k}": r}), flush=True)
    res["requirements_met"] = bool(ok)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

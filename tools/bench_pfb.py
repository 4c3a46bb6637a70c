"""Polyphase filter bank spectra against what a user could do before, leg by leg (profiles/pfb/SUMMARY.md is written from this
tool's output).

    python tools/bench_pfb.py [--frames-log2 18] [--host-samples-log2 27] [--only main|sweep|generic|host] [--json out.json]

Device legs, one process, warmed up by time, alternating, a leg's figure the MEDIAN of 30 per-launch times (the *_timed_each
entry points; torch.cuda events for the torch fold).  N = 4096, T = 4, hop N, default prototype:
  floor (recorded, no bar)   sdrk_exec_device on the same number of packed frames: the PFB call cannot beat it
  the bar                    a torch fold on the device that materialises the folded frames y (the faster of
                             as_strided-multiply-sum and a loop of T multiply-adds), then sdrk_exec_device on y.  HBM byte
                             model: >= 8 + 8 + 8 + 4 = 28 B/sample against 12 fused.  Required (exit status 1 when missed):
                             the fused call at least 1.06 x faster.
  frame assignment           the fused call with each of SDRK_PFB_ASSIGN = 0 (grid-stride), 1 (per-XCD ranges), 2 (runs per
                             workgroup), same buffers, same alternation
Also recorded: T = 2 and 8, hop N/2, the staged route at N = 1024 and 65536 against the per-frame call on as many packed
frames, and the numpy boundary (SpectrumPlan.pfb_db) from pageable and pinned arrays."""
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
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, pfb_prototype  # noqa: E402

REQUIRED = 1.06
ASSIGN = {"stride": "0", "xcd": "1", "runs": "2"}


def pfb_plan(n, taps, assign=None):
    """A rectangular plan with the default prototype; `assign` overrides the frame assignment (read when the prototype is set)."""
    old = os.environ.get("SDRK_PFB_ASSIGN")
    if assign is not None:
        os.environ["SDRK_PFB_ASSIGN"] = assign
    try:
        plan = SpectrumPlan(n)
        plan.set_pfb(pfb_prototype(n, taps))
    finally:
        if assign is not None:
            os.environ.pop("SDRK_PFB_ASSIGN")
            if old is not None:
                os.environ["SDRK_PFB_ASSIGN"] = old
    return plan


def torch_fold_legs(x, h, n, taps, frames, hop):
    """x: float32 (L, 2) on the device, h: float32 (taps*n,).  -> {name: callable that writes y (frames, n, 2)}."""
    y = torch.empty((frames, n, 2), dtype=torch.float32, device=x.device)
    hv = h.view(taps, n, 1)

    def seg(t):
        return torch.as_strided(x, (frames, n, 2), (2 * hop, 2, 1), storage_offset=2 * t * n)

    def strided_sum():
        v = torch.as_strided(x, (frames, taps, n, 2), (2 * hop, 2 * n, 2, 1))
        torch.sum(v * hv, dim=1, out=y)

    def loop():
        torch.mul(seg(0), hv[0], out=y)
        for t in range(1, taps):
            y.addcmul_(seg(t), hv[t])

    return y, {"as_strided_multiply_sum": strided_sum, "loop_of_multiply_adds": loop}


def timed_torch(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def main_legs(n, taps, frames, hop, with_torch=True, assigns=("stride", "xcd", "runs"), rounds=6, per_round=5, warm_s=0.4):
    dev = torch.device("cuda:0")
    L = (frames - 1) * hop + taps * n
    x = torch.randint(-2048, 2048, (L, 2), device=dev, dtype=torch.int32).to(torch.float32)
    rows = torch.empty((frames, n), dtype=torch.float32, device=dev)
    h = torch.from_numpy(pfb_prototype(n, taps)).to(dev)
    plans = {a: pfb_plan(n, taps, ASSIGN[a]) for a in assigns}
    plain = SpectrumPlan(n)
    y, folds = torch_fold_legs(x, h, n, taps, frames, hop) if with_torch else (None, {})
    if with_torch and frames * taps * n * 8 > 48 << 30:
        folds.pop("as_strided_multiply_sum")        # its intermediate would not fit beside the buffers
    torch.cuda.synchronize()
    legs = {f"pfb_{a}": (lambda k, p=plans[a]: p.exec_device_pfb_timed_each(x.data_ptr(), frames, rows.data_ptr(), k, frame_stride=hop))
            for a in assigns}
    legs["plain_packed"] = lambda k: plain.exec_device_timed_each(x.data_ptr(), frames, rows.data_ptr(), k)
    if with_torch:
        legs["plain_on_y"] = lambda k: plain.exec_device_timed_each(y.data_ptr(), frames, rows.data_ptr(), k)
        for name, fn in folds.items():
            legs[f"torch_{name}"] = lambda k, fn=fn: timed_torch(fn, k)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for fn in legs.values():
            fn(1)
    t = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            t[name] += fn(per_round)
    for p in list(plans.values()) + [plain]:
        p.close()
    med = {name: statistics.median(v) for name, v in t.items()}
    samples = frames * n
    out = {"nfft": n, "taps": taps, "frames": frames, "hop": hop, "launches_per_leg": rounds * per_round,
           "ms": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}}
    best = min(assigns, key=lambda a: med[f"pfb_{a}"])
    out["fastest_assignment"] = best
    out["pfb_over_plain"] = {a: round(med[f"pfb_{a}"] / med["plain_packed"], 4) for a in assigns}
    out["pfb_gsamples_s"] = {a: round(samples / med[f"pfb_{a}"] / 1e6, 2) for a in assigns}
    out["pfb_fraction_of_8TBs_at_12B"] = {a: round(samples * 12 / (med[f"pfb_{a}"] * 1e-3) / 8e12, 4) for a in assigns}
    if with_torch:
        fold = min((med[f"torch_{k}"], k) for k in folds)
        base = fold[0] + med["plain_on_y"]
        out["baseline"] = {"fold": fold[1], "fold_ms": round(fold[0], 4), "transform_ms": round(med["plain_on_y"], 4),
                           "total_ms": round(base, 4), "byte_model_ratio": round(28 / 12, 3)}
        out["speedup_vs_baseline"] = {a: round(base / med[f"pfb_{a}"], 4) for a in assigns}
    del x, rows, y
    torch.cuda.empty_cache()
    return out


def generic_leg(n, taps, frames, rounds=6, per_round=5, warm_s=0.3):
    """The staged route against the plan's per-frame call on as many packed frames."""
    dev = torch.device("cuda:0")
    x = torch.randint(-2048, 2048, ((frames - 1 + taps) * n, 2), device=dev, dtype=torch.int32).to(torch.float32)
    rows = torch.empty((frames, n), dtype=torch.float32, device=dev)
    with pfb_plan(n, taps) as plan:
        legs = {"pfb": lambda k: plan.exec_device_pfb_timed_each(x.data_ptr(), frames, rows.data_ptr(), k),
                "plain": lambda k: plan.exec_device_timed_each(x.data_ptr(), frames, rows.data_ptr(), k)}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_s:
            for fn in legs.values():
                fn(1)
        t = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                t[name] += fn(per_round)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"nfft": n, "taps": taps, "frames": frames, "pfb_ms": round(med["pfb"], 4), "plain_ms": round(med["plain"], 4),
            "pfb_over_plain": round(med["pfb"] / med["plain"], 4)}


def host_leg(n, taps, log2_samples, calls=5):
    rng = np.random.default_rng(1)
    block = (rng.integers(-2048, 2048, 1 << 20) + 1j * rng.integers(-2048, 2048, 1 << 20)).astype(np.complex64)
    x = np.tile(block, (1 << log2_samples) // block.size)
    out = {"nfft": n, "taps": taps, "samples": int(x.size), "calls": calls}
    with pfb_plan(n, taps) as plan:
        rows = np.empty((plan.pfb_frames(x.size), n), np.float32)
        for kind in ("pageable", "pinned"):
            if kind == "pinned":
                xp, rows = pinned_empty(x.shape, np.complex64), pinned_empty(rows.shape, np.float32)
                xp[:] = x
                x = xp
            plan.pfb_db(x, out=rows)
            plan.stft_db(x[: rows.shape[0] * n], out=rows)
            t_pfb, t_stft = [], []
            for _ in range(calls):
                a = time.perf_counter(); plan.pfb_db(x, out=rows); b = time.perf_counter()
                plan.stft_db(x[: rows.shape[0] * n], out=rows); c = time.perf_counter()
                t_pfb.append(b - a); t_stft.append(c - b)
            mp, ms = statistics.median(t_pfb), statistics.median(t_stft)
            out[kind] = {"pfb_db_ms": round(mp * 1e3, 2), "stft_db_ms": round(ms * 1e3, 2), "pfb_over_stft": round(mp / ms, 4),
                         "pfb_input_GBs": round(x.nbytes / mp / 1e9, 2)}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=18)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--only", default=None, choices=["main", "sweep", "generic", "host"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res, ok = {"device": pkg.device_info(0).split(", pci")[0]}, True
    want = (lambda k: args.only in (None, k))
    frames = 1 << args.frames_log2

    def emit(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)

    if want("main"):
        r = main_legs(4096, 4, frames, 4096)
        r["required_speedup"] = REQUIRED
        r["met"] = r["speedup_vs_baseline"][r["fastest_assignment"]] >= REQUIRED
        ok &= r["met"]
        emit("n4096_t4_hop_n", r)
    if want("sweep"):
        emit("n4096_t2_hop_n", main_legs(4096, 2, frames, 4096))
        emit("n4096_t8_hop_n", main_legs(4096, 8, frames, 4096))
        emit("n4096_t4_hop_half", main_legs(4096, 4, frames, 2048))
    if want("generic"):
        emit("n1024_t4", generic_leg(1024, 4, frames * 4))
        emit("n65536_t4", generic_leg(65536, 4, max(frames // 16, 8)))
    if want("host"):
        emit("host_n4096_t4", host_leg(4096, 4, args.host_samples_log2))
    res["requirements_met"] = bool(ok)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps({"requirements_met": bool(ok)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""The 8-bit filter-bank and spectral-kurtosis calls (SigMF ci8 / cu8) against their int16 twins of the same build, leg by leg.
Writes <out-dir>/bench_iq8_modes.json and <out-dir>/SUMMARY.md (every figure in profiles/iq8_modes/, the README and DESIGN.md
§4.26 comes from a run of this tool).

    python tools/bench_iq8_modes.py [--frames-log2 16] [--host-samples-log2 27] [--out-dir profiles/iq8_modes] [--bench-line FILE]
                                    [--bench-line-before FILE]

Method (tools/bench_ci8.py's).  One process; input made on the device with torch; N = 4096, T = 4 (the default prototype), hop
N, 2^16 frames.  Device legs run on torch's stream (the entry points take it), timed by device events between consecutive
launches; after a warm-up by time the legs alternate, three rounds of ten launches each.  A leg's figure is the median of its
30 per-launch times, its spread the largest over the smallest of its three per-round medians.  Legs:
    per-frame PFB; integrated PFB at K = 16 and as one group of all frames; spectral kurtosis at K = 16 with a Hann window
    each as ci8, cu8, int16 (the twin, on the same values) and complex64.
Host legs: wall time of the numpy-boundary calls on 2^27 pageable samples, alternating, three rounds of three calls: the 8-bit
call, the int16 call (link-byte model 2x), the complex64 call (4x) and what cli.py psd did before — iq8_to_c64 on the host and
then the complex64 call.
Nothing is a number fixed in advance.  Recorded for the summary: a device leg whose 8-bit time is worse than its int16 twin's
by more than twice that twin's own spread is marked "to be explained"."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch  # (first: one HIP runtime shared with libsdrk)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, iq8_to_c64, pfb_prototype  # noqa: E402

N, T, K = 4096, 4, 16
ROUNDS, PER_ROUND = 3, 10


def timed(fn, launches):
    """`launches` calls of fn() on torch's stream, device events between them -> the milliseconds of each."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
    ev[0].record()
    for i in range(launches):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(launches)]


def alternate(legs, warm_s=0.5):
    """legs: {name: fn}.  -> {name: {ms, spread, round_medians}}"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for fn in legs.values():
            timed(fn, 2)
    times = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            times[name].append(timed(fn, PER_ROUND))
    out = {}
    for name, rounds in times.items():
        meds = [statistics.median(r) for r in rounds]
        out[name] = {"ms": round(statistics.median([t for r in rounds for t in r]), 4), "spread": round(max(meds) / min(meds), 4),
                     "round_medians_ms": [round(m, 4) for m in meds]}
    return out


def device_legs(frames):
    # a stream of torch's own, not the null stream (whose handle 0 means "the plan's stream" to the entry points)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        return _device_legs(frames, side.cuda_stream)


def _device_legs(frames, stream):
    g = torch.Generator(device="cuda").manual_seed(7)
    samples = (frames + T - 1) * N                 # hop N: frame f covers blocks f .. f + T - 1
    s8 = torch.randint(-128, 128, (samples, 2), dtype=torch.int16, device="cuda", generator=g).to(torch.int8)
    u8 = (s8.to(torch.int16) + 128).to(torch.uint8)
    i16 = s8.to(torch.int16)
    c64 = torch.view_as_complex(s8.to(torch.float32))
    rows = torch.empty((frames, N), dtype=torch.float32, device="cuda")
    assert stream and torch.cuda.current_stream().cuda_stream == stream
    p8, pu, p16, p64, out = s8.data_ptr(), u8.data_ptr(), i16.data_ptr(), c64.data_ptr(), rows.data_ptr()
    res = {}
    with SpectrumPlan(N) as plan, SpectrumPlan(N, window="hann") as hann:
        plan.set_pfb(pfb_prototype(N, T))
        res["pfb_per_frame"] = alternate({
            "ci8": lambda: plan.exec_device_pfb_ci8(p8, frames, out, stream=stream),
            "cu8": lambda: plan.exec_device_pfb_ci8(pu, frames, out, unsigned=True, stream=stream),
            "int16": lambda: plan.exec_device_pfb_ci16(p16, frames, out, stream=stream),
            "complex64": lambda: plan.exec_device_pfb(p64, frames, out, stream=stream),
        })
        for name, k in (("pfb_integrated_k16", K), ("pfb_integrated_one_group", frames)):
            groups = frames // k
            res[name] = alternate({
                "ci8": lambda: plan.exec_device_pfb_integrated_ci8(p8, groups, k, out, stream=stream),
                "cu8": lambda: plan.exec_device_pfb_integrated_ci8(pu, groups, k, out, unsigned=True, stream=stream),
                "int16": lambda: plan.exec_device_pfb_integrated_ci16(p16, groups, k, out, stream=stream),
                "complex64": lambda: plan.exec_device_pfb_integrated(p64, groups, k, out, stream=stream),
            })
        groups = frames // K
        res["kurtosis_k16_hann"] = alternate({
            "ci8": lambda: hann.exec_device_sk_ci8(p8, groups, K, out, stream=stream),
            "cu8": lambda: hann.exec_device_sk_ci8(pu, groups, K, out, unsigned=True, stream=stream),
            "int16": lambda: hann.exec_device_sk_ci16(p16, groups, K, out, stream=stream),
            "complex64": lambda: hann.exec_device_sk(p64, groups, K, out, stream=stream),
        })
        torch.cuda.synchronize()
        # the bits: the 8-bit rows are the complex64 call's
        plan.exec_device_pfb_ci8(p8, 64, out, stream=stream)
        a = rows[:64].clone()
        plan.exec_device_pfb(p64, 64, out, stream=stream)
        torch.cuda.synchronize()
        res["same_bits_as_complex64"] = bool(torch.equal(a.view(torch.int32), rows[:64].view(torch.int32)))
    for name, legs in res.items():
        if isinstance(legs, dict):
            for leg in legs.values():
                leg["gsamples_s"] = round(frames * N / leg["ms"] / 1e6, 1)
            new, twin = legs["ci8"], legs["int16"]
            legs["ci8"]["of_int16"] = round(new["ms"] / twin["ms"], 3)
            legs["cu8"]["of_int16"] = round(legs["cu8"]["ms"] / twin["ms"], 3)
            legs["ci8"]["to_be_explained"] = new["ms"] > twin["ms"] * (1 + 2 * (twin["spread"] - 1))
    return res


def wall(calls):
    """calls: {name: fn}; three rounds of three calls each, alternating -> {name: {ms, spread}}"""
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            r = []
            for _ in range(3):
                t = time.perf_counter(); fn(); r.append((time.perf_counter() - t) * 1e3)
            times[name].append(r)
    out = {}
    for name, rounds in times.items():
        meds = [statistics.median(r) for r in rounds]
        out[name] = {"ms": round(statistics.median([t for r in rounds for t in r]), 3), "spread": round(max(meds) / min(meds), 4)}
    return out


def host_legs(log2_samples):
    rng = np.random.default_rng(1)
    block = rng.integers(-128, 128, size=(1 << 20, 2), dtype=np.int64).astype(np.int8)
    x8 = np.tile(block, ((1 << log2_samples) // block.shape[0], 1))
    x16 = x8.astype(np.int16)
    x64 = iq8_to_c64(x8)
    t = time.perf_counter()
    iq8_to_c64(x8)
    res = {"samples": int(x8.shape[0]), "iq8_to_c64_ms": round((time.perf_counter() - t) * 1e3, 1)}
    frames = x8.shape[0] // N
    with SpectrumPlan(N, max_batch=frames) as plan, SpectrumPlan(N, window="hann", max_batch=frames) as hann:
        plan.set_pfb(pfb_prototype(N, T))
        rows = np.empty((frames - T + 1, N), np.float32)
        res["pfb_per_frame"] = wall({
            "ci8": lambda: plan.pfb_db_ci8(x8, out=rows), "int16": lambda: plan.pfb_db_ci16(x16, out=rows),
            "complex64": lambda: plan.pfb_db(x64, out=rows), "iq8_to_c64 + complex64": lambda: plan.pfb_db(iq8_to_c64(x8), out=rows)})
        res["pfb_integrated_k16"] = wall({
            "ci8": lambda: plan.pfb_integrate_ci8(x8, K), "int16": lambda: plan.pfb_integrate_ci16(x16, K),
            "complex64": lambda: plan.pfb_integrate(x64, K), "iq8_to_c64 + complex64": lambda: plan.pfb_integrate(iq8_to_c64(x8), K)})
        res["kurtosis_k16_hann"] = wall({
            "ci8": lambda: hann.spectral_kurtosis_ci8(x8, K), "int16": lambda: hann.spectral_kurtosis_ci16(x16, K),
            "complex64": lambda: hann.spectral_kurtosis(x64, K), "iq8_to_c64 + complex64": lambda: hann.spectral_kurtosis(iq8_to_c64(x8), K)})
    for name, legs in res.items():
        if isinstance(legs, dict):
            for leg in legs.values():
                leg["gsamples_s"] = round(res["samples"] / leg["ms"] / 1e6, 2)
    return res


def ratio(a, b):
    return round(b["ms"] / a["ms"], 3)


DEVICE_TITLES = (("pfb_per_frame", "Per-frame PFB (2 + 4 B/sample through HBM; int16 4 + 4; complex64 8 + 4)"),
                 ("pfb_integrated_k16", "Integrated PFB, K = 16 (2.25 B/sample; int16 4.25; complex64 8.25)"),
                 ("pfb_integrated_one_group", "Integrated PFB, one group of all frames (slices + finalize)"),
                 ("kurtosis_k16_hann", "Spectral kurtosis, K = 16, Hann (2.5 B/sample; int16 4.5; complex64 8.5)"))
HOST_TITLES = (("pfb_per_frame", "per-frame PFB"), ("pfb_integrated_k16", "integrated PFB, K = 16"), ("kurtosis_k16_hann", "spectral kurtosis, K = 16, Hann"))


def summary(res):
    dev, host = res["device"], res["host"]
    L = ["# 8-bit I,Q (ci8 / cu8) into the filter bank and spectral kurtosis", "",
         f"Written by `tools/bench_iq8_modes.py` from one run on {res['device_name']}: one process, input made on the device with torch, "
         f"N = 4096, T = 4, hop N, {res['frames']} frames; legs alternating after a warm-up by time; ms = median of 30 per-launch times "
         "between device events; spread = largest / smallest of the leg's three per-round medians.  `bench_iq8_modes.json` holds the run.", "",
         "## Device resident: each 8-bit call against its int16 twin of the same build, in the same process", ""]
    for name, title in DEVICE_TITLES:
        legs = dev[name]
        L += [f"### {title}", "", "| leg | ms | spread | Gsamples/s | time / int16's |", "|---|---|---|---|---|"]
        for leg, v in legs.items():
            L.append(f"| {leg} | {v['ms']} | {v['spread']} | {v['gsamples_s']} | {round(v['ms'] / legs['int16']['ms'], 3)} |")
        twin = legs["int16"]
        L += ["", f"(ci8 at {legs['ci8']['of_int16']} of the int16 twin's time, whose own spread is {twin['spread']}: "
              + ("worse by more than twice that spread — to be explained" if legs["ci8"]["to_be_explained"] else "within twice that spread, or faster") + ")", ""]
    L += [f"## Host entries, {host['samples']} pageable samples (wall time per call, three rounds of three, alternating)", "",
          f"`iq8_to_c64` alone on these samples: {host['iq8_to_c64_ms']} ms.", "",
          "| call | leg | ms | spread | Gsamples/s | ci8 is x faster | link-byte model |", "|---|---|---|---|---|---|---|"]
    models = {"ci8": "1", "int16": "2", "complex64": "4", "iq8_to_c64 + complex64": "4, plus the widening"}
    for name, title in HOST_TITLES:
        for leg, v in host[name].items():
            L.append(f"| {title} | {leg} | {v['ms']} | {v['spread']} | {v['gsamples_s']} | {ratio(host[name]['ci8'], v)} | {models[leg]} |")
    L += ["", f"The 8-bit rows have the complex64 call's bits in this run: {dev['same_bits_as_complex64']}.", ""]
    if res.get("bench_line") or res.get("bench_line_before"):
        L += ["## Flagship", "", "`python bench.py --gpus 1 --steps 20 --warmup 5`, the parent commit's build and this one, one after the other:", "", "```"]
        for when, key in (("before", "bench_line_before"), ("after ", "bench_line")):
            d = json.loads(res[key]) if res.get(key) else {}
            L.append(f"{when}  " + json.dumps({k: d.get(k) for k in ("value", "unit", "ms_per_step", "hbm_peak_frac", "steps", "warmup")}))
        L += ["```", "", "(the whole lines are in `bench_iq8_modes.json`)", ""]
    return "\n".join(L)


def last_json_line(path):
    if not path or not os.path.exists(path):
        return None
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
    return lines[-1] if lines else None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=16)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "iq8_modes"))
    ap.add_argument("--bench-line", default=None, help="a file holding bench.py's JSON line of the same build, quoted in SUMMARY.md")
    ap.add_argument("--bench-line-before", default=None, help="... and of the parent commit's build")
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device_name": pkg.device_info(0).split(", pci")[0], "frames": 1 << args.frames_log2}
    res["device"] = device_legs(1 << args.frames_log2)
    print(json.dumps({"device": res["device"]}), flush=True)
    res["host"] = host_legs(args.host_samples_log2)
    print(json.dumps({"host": res["host"]}), flush=True)
    res["bench_line"], res["bench_line_before"] = last_json_line(args.bench_line), last_json_line(args.bench_line_before)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_iq8_modes.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out_dir, "SUMMARY.md"), "w") as fh:
        fh.write(summary(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

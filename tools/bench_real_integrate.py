"""Integrated real-sampled input (sdrk_exec_device_real_integrated) against the per-frame real call of the same build on the
same frames, and against that call followed by a torch reduction of its rows.  Writes profiles/real_integrate/
bench_real_integrate.json and profiles/real_integrate/SUMMARY.md (every figure in that file, the README row and DESIGN.md §4.30
comes from a run of this tool).

    python tools/bench_real_integrate.py [--frames-log2 17] [--out-dir profiles/real_integrate]

Method.  One process.  Per format (float32, int16, uint8): real frames of 8192 made on the device with torch, Hann; legs run on
a stream of torch's own, timed by device events between consecutive launches; after a warm-up by time the legs alternate, three
rounds of ten launches each.  A leg's figure is the median of its 30 per-launch times, its spread the largest over the smallest
of its three per-round medians.  Legs:
    p   per-frame dB               exec_device_real, dB rows of 4097 bins, one per frame
    i16 integrated, K = 16         exec_device_real_integrated, mean, dB: one row per 16 frames
    i1  integrated, one group      the same with all frames as one group (which the library cuts into slices and finalizes)
    p+t per-frame dB + torch mean  leg p, then 10 log10(mean over 16 rows of 10^(dB/10)) in torch
Expectation, stated and not a bar: i16 and i1 read the same bytes as p and write 1/K of its rows, so they should take no longer
than p; the margin they get is p's own spread in the same run.  The summary gives the ratios as they came out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, L, K = 4096, 8192, 16
ROUNDS, PER_ROUND = 3, 10
HBM_PEAK = 8.0e12            # bytes/s, MI355X
FORMATS = {"f32": 4, "s16": 2, "u8": 1}


def measure(fmt: str, frames: int) -> dict:
    import torch  # (first: one HIP runtime shared with libsdrk)
    from sdr_iq_visualizer_amd.spectrum import SpectrumPlan

    def timed(fn, launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
        ev[0].record()
        for i in range(launches):
            fn()
            ev[i + 1].record()
        ev[-1].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(launches)]

    def alternate(legs, warm_s=0.5):
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

    groups = frames // K
    side = torch.cuda.Stream()   # not the null stream (whose handle 0 means "the plan's stream" to the entry points)
    with torch.cuda.stream(side):
        stream = side.cuda_stream
        g = torch.Generator(device="cuda").manual_seed(7)
        if fmt == "f32":
            x = torch.randn((frames, L), dtype=torch.float32, device="cuda", generator=g)
        elif fmt == "s16":
            x = torch.randint(-2048, 2048, (frames, L), dtype=torch.int16, device="cuda", generator=g)
        else:
            x = torch.randint(0, 256, (frames, L), dtype=torch.int16, device="cuda", generator=g).to(torch.uint8)
        rows = torch.empty((frames, N + 1), dtype=torch.float32, device="cuda")
        rows_k = torch.empty((groups, N + 1), dtype=torch.float32, device="cuda")
        row_1 = torch.empty((1, N + 1), dtype=torch.float32, device="cuda")
        with SpectrumPlan(N) as plan:
            plan.set_real_window("hann")

            def per_frame():
                plan.exec_device_real(x.data_ptr(), frames, rows.data_ptr(), fmt=fmt, stream=stream)

            def torch_mean():
                per_frame()
                return 10 * torch.log10(torch.pow(10.0, rows / 10).view(groups, K, N + 1).mean(dim=1))

            legs = {
                "p per-frame dB": per_frame,
                "i16 integrated, K = 16": lambda: plan.exec_device_real_integrated(x.data_ptr(), groups, K, rows_k.data_ptr(), fmt=fmt,
                                                                                   stream=stream),
                "i1 integrated, one group": lambda: plan.exec_device_real_integrated(x.data_ptr(), 1, frames, row_1.data_ptr(), fmt=fmt,
                                                                                     stream=stream),
                "p+t per-frame dB + torch mean": torch_mean,
            }
            res = {"legs": alternate(legs)}
            torch.cuda.synchronize()
            # the two routes agree: the K = 16 rows against torch's reduction of the per-frame rows, in dB
            legs["i16 integrated, K = 16"]()
            ref = torch_mean()
            torch.cuda.synchronize()
            res["worst_db_difference_to_torch_mean"] = float((rows_k[:64].double() - ref[:64].double()).abs().max())
    in_b = FORMATS[fmt]
    for name, leg in res["legs"].items():
        leg["gsamples_s"] = round(frames * L / leg["ms"] / 1e6, 1)
    p = res["legs"]["p per-frame dB"]
    p["hbm_fraction"] = round(frames * L * (in_b + (N + 1) * 4 / L) / (p["ms"] * 1e-3) / HBM_PEAK, 4)
    for name, k in (("i16 integrated, K = 16", K), ("i1 integrated, one group", frames)):
        leg = res["legs"][name]
        leg["bytes_per_real_sample"] = round(in_b + 4 / k, 5)
        leg["hbm_fraction"] = round(frames * L * (in_b + 4 / k) / (leg["ms"] * 1e-3) / HBM_PEAK, 4)
        leg["p_over_this"] = round(p["ms"] / leg["ms"], 3)
        leg["no_longer_than_p_within_its_spread"] = bool(leg["ms"] <= p["ms"] * p["spread"])
    t = res["legs"]["p+t per-frame dB + torch mean"]
    t["over_i16"] = round(t["ms"] / res["legs"]["i16 integrated, K = 16"]["ms"], 3)
    return res


def summary(res):
    out = ["# Integrated one-sided spectra from real input: K-frame mean inside the transform", "",
           f"Written by `tools/bench_real_integrate.py` from one run on {res['device_name']}: {res['frames']} real frames of 8192 resident "
           "on the device, Hann, mean detector, dB rows; one process, legs alternating after a warm-up by time; ms = median of 30 "
           "per-launch times between device events; spread = largest / smallest of the leg's three per-round medians.  "
           "`bench_real_integrate.json` holds the run.  Byte model of the integrated call: 4 | 2 | 1 + 4/K B per real sample; "
           f"HBM peak taken as {HBM_PEAK / 1e12:g} TB/s.", ""]
    for fmt, r in res["formats"].items():
        legs = r["legs"]
        p = legs["p per-frame dB"]
        out += [f"## {fmt}: {FORMATS[fmt]} B in per real sample", "",
                "| leg | ms | spread | G real samples/s | fraction of HBM peak | p / this |", "|---|---|---|---|---|---|"]
        for name, v in legs.items():
            out.append(f"| {name} | {v['ms']} | {v['spread']} | {v['gsamples_s']} | {v.get('hbm_fraction', '')} | "
                       f"{v.get('p_over_this', round(p['ms'] / v['ms'], 3))} |")
        i16, i1, t = legs["i16 integrated, K = 16"], legs["i1 integrated, one group"], legs["p+t per-frame dB + torch mean"]
        out += ["", f"Against the per-frame call (spread {p['spread']}): K = 16 takes {round(i16['ms'] / p['ms'], 3)} of its time — the "
                f"expectation \"no longer than p within p's spread\" is {'met' if i16['no_longer_than_p_within_its_spread'] else 'NOT met'}; "
                f"all frames as one group takes {round(i1['ms'] / p['ms'], 3)} of it — "
                f"{'met' if i1['no_longer_than_p_within_its_spread'] else 'NOT met'}.  The per-frame call followed by torch's reduction of "
                f"its rows takes {t['over_i16']} times the K = 16 call.  Worst |dB| between the K = 16 rows and torch's reduction, 64 "
                f"groups: {r['worst_db_difference_to_torch_mean']:.2e}.", ""]
    return "\n".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=17)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "real_integrate"))
    args = ap.parse_args(argv)
    frames = 1 << args.frames_log2
    import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)
    import sdr_iq_visualizer_amd as pkg
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"frames": frames, "k": K, "device_name": pkg.device_info(0).split(", pci")[0], "formats": {}}
    for fmt in FORMATS:
        res["formats"][fmt] = measure(fmt, frames)
        print(json.dumps({fmt: res["formats"][fmt]["legs"]}), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_real_integrate.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out_dir, "SUMMARY.md"), "w") as fh:
        fh.write(summary(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

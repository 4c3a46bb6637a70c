"""8-bit I,Q input (SigMF ci8 / cu8) against what a user could do before it, leg by leg.  Writes profiles/ci8/bench_ci8.json and
profiles/ci8/SUMMARY.md (every figure in that file, the README and DESIGN.md §4.24 comes from a run of this tool).

    python tools/bench_ci8.py [--frames-log2 18] [--host-samples-log2 27] [--out-dir profiles/ci8] [--bench-line FILE]

Method.  One process; input made on the device with torch; N = 4096, Hann.  Device legs run on torch's stream (the entry
points take it), timed by device events between consecutive launches; after a warm-up by time the legs alternate, three rounds
of ten launches each.  A leg's figure is the median of its 30 per-launch times, its spread the largest over the smallest of
its three per-round medians.  Legs, per frame and integrated (K = 16, and one group of all frames):
    ci8, cu8                      the new calls
    int16                         the int16 call on the same values (widened once, outside the timing)
    complex64                     the complex64 call on the same values
    torch widen + int16           x8.to(torch.int16) and then the int16 call: what a user could do before
Host legs: wall time of the numpy-boundary calls on 2^27 samples, pageable and pinned, integrated (K = 16) and per frame, 8-bit
against int16, alternating, three rounds of three calls.
Conditions (exit status 1 when one is missed; none is a number fixed in advance):
    device, per frame and integrated K = 16: ci8 faster than "torch widen + int16" by more than that leg's spread;
    host integrated, pageable: ci8 faster than the int16 host integrated call by more than that call's spread.
Recorded only: 8-bit against the int16 call on the device, the ci8 call on the buffer the cu8 leg reads (one kernel serves both
formats: what differs between the two legs is the arguments and where the input lies), the per-frame host ratio, one live frame, cu8 against ci8, and the
mid-size host call with the kernel reading pinned host memory itself against the staged copy (SDRK_CI8_ZERO_COPY)."""
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
from sdr_iq_visualizer_amd.hostmem import pinned_empty  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

N = 4096
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
    s8 = torch.randint(-128, 128, (frames * N, 2), dtype=torch.int16, device="cuda", generator=g).to(torch.int8)
    u8 = (s8.to(torch.int16) + 128).to(torch.uint8)
    i16 = s8.to(torch.int16)
    c64 = torch.view_as_complex(s8.to(torch.float32))
    rows = torch.empty((frames, N), dtype=torch.float32, device="cuda")
    assert stream and torch.cuda.current_stream().cuda_stream == stream
    res = {}
    with SpectrumPlan(N, window="hann") as plan:
        def widen_then(call):
            def f():
                w = s8.to(torch.int16)
                call(w)
            return f

        per_frame = {
            "ci8": lambda: plan.exec_device_ci8(s8.data_ptr(), frames, rows.data_ptr(), stream=stream),
            "cu8": lambda: plan.exec_device_ci8(u8.data_ptr(), frames, rows.data_ptr(), unsigned=True, stream=stream),
            "ci8 call on the cu8 leg's buffer": lambda: plan.exec_device_ci8(u8.data_ptr(), frames, rows.data_ptr(), stream=stream),
            "int16": lambda: plan.exec_device_ci16(i16.data_ptr(), frames, rows.data_ptr(), stream=stream),
            "complex64": lambda: plan.exec_device(c64.data_ptr(), frames, rows.data_ptr(), stream=stream),
            "torch widen + int16": widen_then(lambda w: plan.exec_device_ci16(w.data_ptr(), frames, rows.data_ptr(), stream=stream)),
        }
        res["per_frame"] = alternate(per_frame)
        for name, k in (("integrated_k16", 16), ("integrated_one_group", frames)):
            groups = frames // k
            legs = {
                "ci8": lambda: plan.exec_device_integrated_ci8(s8.data_ptr(), groups, k, rows.data_ptr(), stream=stream),
                "cu8": lambda: plan.exec_device_integrated_ci8(u8.data_ptr(), groups, k, rows.data_ptr(), unsigned=True, stream=stream),
                "ci8 call on the cu8 leg's buffer": lambda: plan.exec_device_integrated_ci8(u8.data_ptr(), groups, k, rows.data_ptr(), stream=stream),
                "int16": lambda: plan.exec_device_integrated_ci16(i16.data_ptr(), groups, k, rows.data_ptr(), stream=stream),
                "complex64": lambda: plan.exec_device_integrated(c64.data_ptr(), groups, k, rows.data_ptr(), stream=stream),
                "torch widen + int16": widen_then(lambda w: plan.exec_device_integrated_ci16(w.data_ptr(), groups, k, rows.data_ptr(), stream=stream)),
            }
            res[name] = alternate(legs)
        torch.cuda.synchronize()
        # the bits: the 8-bit rows are the complex64 call's
        plan.exec_device_ci8(s8.data_ptr(), 64, rows.data_ptr(), stream=stream)
        a = rows[:64].clone()
        plan.exec_device(c64.data_ptr(), 64, rows.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        res["same_bits_as_complex64"] = bool(torch.equal(a.view(torch.int32), rows[:64].view(torch.int32)))
    for legs in (res["per_frame"], res["integrated_k16"], res["integrated_one_group"]):
        for leg in legs.values():
            leg["gsamples_s"] = round(frames * N / leg["ms"] / 1e6, 1)
    return res


def wall(calls):
    """calls: {name: fn}; three rounds of three calls each, alternating -> {name: {ms, spread}}"""
    for fn in calls.values():
        fn(); fn()
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
    frames = x8.shape[0] // N
    res = {"samples": int(x8.shape[0])}
    with SpectrumPlan(N, window="hann", max_batch=frames) as plan:
        rows = np.empty((frames, N), np.float32)
        for kind in ("pageable", "pinned"):
            if kind == "pinned":
                p8, p16, prow = pinned_empty(x8.shape, np.int8), pinned_empty(x16.shape, np.int16), pinned_empty(rows.shape, np.float32)
                p8[:], p16[:] = x8, x16
                x8, x16, rows = p8, p16, prow
            f8 = x8.reshape(frames, N, 2)
            f16 = x16.reshape(frames, N, 2)
            res[kind] = {
                "integrated_k16": wall({"ci8": lambda: plan.integrate_ci8(x8, 16), "int16": lambda: plan.integrate_ci16(x16, 16)}),
                "per_frame": wall({"ci8": lambda: plan.spectrum_db_ci8(f8, out=rows), "int16": lambda: plan.spectrum_db_ci16(f16, out=rows)}),
            }
        # one live frame, and a mid-size call (256 frames, pageable) with and without the kernel reading host memory itself
        one8, one16, one64 = np.ascontiguousarray(block[:N]), block[:N].astype(np.int16), block[:N].astype(np.float32).view(np.complex64).reshape(-1)
        res["one_frame_us"] = {k: round(v["ms"] * 1e3 / 200, 2) for k, v in wall({
            "ci8": lambda: [plan.spectrum_db_ci8(one8) for _ in range(200)], "int16": lambda: [plan.spectrum_db_ci16(one16) for _ in range(200)],
            "complex64": lambda: [plan.spectrum_db(one64) for _ in range(200)]}).items()}
        mid8 = np.ascontiguousarray(block[: 256 * N].reshape(256, N, 2))
        mid_rows = np.empty((256, N), np.float32)

        def mid(flag):
            def f():
                os.environ["SDRK_CI8_ZERO_COPY"] = flag
                for _ in range(20):
                    plan.spectrum_db_ci8(mid8, out=mid_rows)
            return f
        res["mid_size_256_frames_ms"] = {k: round(v["ms"] / 20, 4) for k, v in wall({"kernel reads host memory": mid("1"), "staged copy": mid("0")}).items()}
        os.environ.pop("SDRK_CI8_ZERO_COPY", None)
    return res


def ratio(a, b):
    return round(b["ms"] / a["ms"], 3)


def conditions(dev, host):
    c = []
    for name in ("per_frame", "integrated_k16"):
        new, old = dev[name]["ci8"], dev[name]["torch widen + int16"]
        c.append({"condition": f"device {name}: ci8 faster than torch widen + int16 by more than that leg's spread",
                  "ratio": ratio(new, old), "spread": old["spread"], "met": ratio(new, old) > old["spread"]})
    new, old = host["pageable"]["integrated_k16"]["ci8"], host["pageable"]["integrated_k16"]["int16"]
    c.append({"condition": "host integrated K = 16, pageable: ci8 faster than the int16 call by more than that call's spread",
              "ratio": ratio(new, old), "spread": old["spread"], "link_byte_model": 2.0, "met": ratio(new, old) > old["spread"]})
    return c


def summary(res):
    dev, host = res["device"], res["host"]
    frames = res["frames"]
    L = ["# 8-bit I,Q input (SigMF ci8 / cu8)", "",
         f"Written by `tools/bench_ci8.py` from one run on {res['device_name']}: one process, input made on the device with torch, "
         f"N = 4096, Hann, {frames} frames; legs alternating after a warm-up by time; ms = median of 30 per-launch times between "
         "device events; spread = largest / smallest of the leg's three per-round medians.  `bench_ci8.json` holds the run.", ""]
    for name, title, model in (("per_frame", "Per frame (2 + 4 B/sample; int16 4 + 4; complex64 8 + 4)", "byte model vs int16: 1.33"),
                               ("integrated_k16", "Integrated, K = 16 (2.25 B/sample; int16 4.25; complex64 8.25)", "byte model vs int16: 1.89"),
                               ("integrated_one_group", "Integrated, one group of all frames (slices + finalize)", "byte model vs int16: 2")):
        legs = dev[name]
        L += [f"## {title}", "", "| leg | ms | spread | Gsamples/s | ci8 is x faster |", "|---|---|---|---|---|"]
        for leg, v in legs.items():
            L.append(f"| {leg} | {v['ms']} | {v['spread']} | {v['gsamples_s']} | {ratio(legs['ci8'], v) if leg != 'ci8' else '1'} |")
        swapped = legs["ci8 call on the cu8 leg's buffer"]
        L += ["", f"({model}; cu8 against ci8: {ratio(legs['cu8'], legs['ci8'])}; cu8 against the ci8 call on the cu8 leg's own buffer — the same "
              f"kernel, the same addresses, the other format arguments: {ratio(legs['cu8'], swapped)})", ""]
    L += [f"## Host boundary, {host['samples']} samples (wall time per call, three rounds of three, alternating)", "",
          "| arrays | call | ci8 ms (spread) | int16 ms (spread) | ci8 is x faster | link-byte model |", "|---|---|---|---|---|---|"]
    for kind in ("pageable", "pinned"):
        for call, model in (("integrated_k16", "2"), ("per_frame", "1.33 (rows come back at 4 B/sample)")):
            a, b = host[kind][call]["ci8"], host[kind][call]["int16"]
            L.append(f"| {kind} | {call} | {a['ms']} ({a['spread']}) | {b['ms']} ({b['spread']}) | {ratio(a, b)} | {model} |")
    L += ["", f"One live frame (host call, median over calls of 200): {host['one_frame_us']} microseconds.", "",
          f"Mid-size host call, 256 pageable frames, ms per call: {host['mid_size_256_frames_ms']}.", "", "## Conditions", ""]
    for c in res["conditions"]:
        L.append(f"- {c['condition']}: ratio {c['ratio']}, spread {c['spread']}" + (f", model {c['link_byte_model']}" if "link_byte_model" in c else "")
                 + f" — {'met' if c['met'] else 'MISSED'}")
    L += ["", f"The 8-bit rows have the complex64 call's bits in this run: {dev['same_bits_as_complex64']}.", ""]
    if res.get("bench_line"):
        L += ["## Flagship", "", "`python bench.py --gpus 1 --steps 20 --warmup 5` on the same build:", "", "```", res["bench_line"], "```", ""]
    return "\n".join(L)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=18)
    ap.add_argument("--host-samples-log2", type=int, default=27)
    ap.add_argument("--out-dir", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ci8"))
    ap.add_argument("--bench-line", default=None, help="a file holding bench.py's JSON line of the same build, quoted in SUMMARY.md")
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device_name": pkg.device_info(0).split(", pci")[0], "frames": 1 << args.frames_log2}
    res["device"] = device_legs(1 << args.frames_log2)
    print(json.dumps({"device": res["device"]}), flush=True)
    res["host"] = host_legs(args.host_samples_log2)
    print(json.dumps({"host": res["host"]}), flush=True)
    res["conditions"] = conditions(res["device"], res["host"])
    res["conditions_met"] = all(c["met"] for c in res["conditions"])
    if args.bench_line and os.path.exists(args.bench_line):
        lines = [ln for ln in open(args.bench_line).read().splitlines() if ln.startswith("{")]
        res["bench_line"] = lines[-1] if lines else None
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_ci8.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out_dir, "SUMMARY.md"), "w") as fh:
        fh.write(summary(res))
    print(json.dumps({"conditions": res["conditions"], "conditions_met": res["conditions_met"]}))
    return 0 if res["conditions_met"] else 1


if __name__ == "__main__":
    sys.exit(main())

"""Real-sampled input (SigMF rf32_le / ri16_le / ri8 / ru8) against what a user could do before it, leg by leg.  Writes
profiles/real/bench_real.json and profiles/real/SUMMARY.md (every figure in that file, the README and DESIGN.md §4.29 comes
from a run of this tool).

    python tools/bench_real.py [--frames-log2 17] [--out-dir profiles/real] [--bench-line FILE] [--parent-bench-line FILE]

Method.  The parent process opens no GPU: each format (float32, int16, uint8) is one child process under its own time limit,
and the first one that fails ends the run.  In a child: real frames of 8192 made on the device with torch, Hann; legs run on a
stream of torch's own, timed by device events between consecutive launches; after a warm-up by time the legs alternate, three
rounds of ten launches each.  A leg's figure is the median of its 30 per-launch times, its spread the largest over the smallest
of its three per-round medians.  Legs:
    a  real                        the new call on an nfft = 4096 plan, dB rows of 4097 bins
    b  complex64 of 8192           this project's complex call on an nfft = 8192 plan, fed the samples widened to complex64
                                   with a zero imaginary part (widened once, outside the timing)
    b+ torch widen + complex64     the same with the torch widening inside the timing
    c  torch rfft                  20 * log10(abs(torch.fft.rfft(float32(x) * w)) + eps) on the same tensor
Expectation, stated and not a bar: (a) does half of (b)'s transform on under half of its bytes, so it should be faster than (b)
by more than (b)'s own spread; the summary says whether it was."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, L = 4096, 8192
ROUNDS, PER_ROUND = 3, 10
HBM_PEAK = 8.0e12            # bytes/s, MI355X
FORMATS = {"f32": 4, "s16": 2, "u8": 1}
CHILD_LIMIT_S = 240


def child(fmt: str, frames: int) -> dict:
    import torch  # (first: one HIP runtime shared with libsdrk)
    import sdr_iq_visualizer_amd as pkg
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

    assert pkg.device_count() >= 1, "needs a GPU"
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

        def as_f32():
            return x if fmt == "f32" else (x.to(torch.float32) - 127.5 if fmt == "u8" else x.to(torch.float32))

        def widen():
            return torch.complex(as_f32(), torch.zeros((), dtype=torch.float32, device="cuda").expand(frames, L))

        c64 = widen().contiguous()
        w = torch.hann_window(L, periodic=False, dtype=torch.float32, device="cuda")
        rows_r = torch.empty((frames, N + 1), dtype=torch.float32, device="cuda")
        rows_c = torch.empty((frames, L), dtype=torch.float32, device="cuda")
        with SpectrumPlan(N) as p4k, SpectrumPlan(L, window="hann", shift=False) as p8k:
            p4k.set_real_window("hann")

            def leg_b_widen():
                z = widen().contiguous()
                p8k.exec_device(z.data_ptr(), frames, rows_c.data_ptr(), stream=stream)

            legs = {
                "a real": lambda: p4k.exec_device_real(x.data_ptr(), frames, rows_r.data_ptr(), fmt=fmt, stream=stream),
                "b complex64 of 8192": lambda: p8k.exec_device(c64.data_ptr(), frames, rows_c.data_ptr(), stream=stream),
                "b+ torch widen + complex64": leg_b_widen,
                "c torch rfft": lambda: 20 * torch.log10(torch.fft.rfft(as_f32() * w).abs() + 1e-12),
            }
            res = {"legs": alternate(legs)}
            torch.cuda.synchronize()
            # the two routes agree: (a) against (b)'s first 4097 bins, in dB on the bins within 40 dB of the frame's peak
            legs["a real"]()
            legs["b complex64 of 8192"]()
            torch.cuda.synchronize()
            a, b = rows_r[:64].double(), rows_c[:64, : N + 1].double()
            sel = b >= b.max(dim=-1, keepdim=True).values - 40.0
            res["worst_db_difference_to_b"] = float((a - b).abs()[sel].max())
    in_b, out_b = FORMATS[fmt], (N + 1) * 4 / L
    for name, leg in res["legs"].items():
        leg["gsamples_s"] = round(frames * L / leg["ms"] / 1e6, 1)
    a = res["legs"]["a real"]
    res["bytes_per_real_sample"] = {"in": in_b, "out": round(out_b, 4)}
    res["hbm_fraction"] = round(frames * L * (in_b + out_b) / (a["ms"] * 1e-3) / HBM_PEAK, 4)
    bl = res["legs"]["b complex64 of 8192"]
    res["b_hbm_fraction"] = round(frames * L * (8 + 4) / (bl["ms"] * 1e-3) / HBM_PEAK, 4)
    res["device_name"] = pkg.device_info(0).split(", pci")[0]
    return res


def ratio(a, b):
    return round(b["ms"] / a["ms"], 3)


def summary(res):
    out = ["# Real-sampled input: one-sided spectra from rf32 / ri16 / ru8", "",
           f"Written by `tools/bench_real.py` from one run on {res['device_name']}: {res['frames']} real frames of 8192 resident on the "
           "device, Hann, dB rows; one child process per format, legs alternating after a warm-up by time; ms = median of 30 "
           "per-launch times between device events; spread = largest / smallest of the leg's three per-round medians.  "
           "`bench_real.json` holds the run.", ""]
    for fmt, r in res["formats"].items():
        legs = r["legs"]
        a = legs["a real"]
        out += [f"## {fmt}: {r['bytes_per_real_sample']['in']} B in + {r['bytes_per_real_sample']['out']} B out per real sample", "",
                "| leg | ms | spread | G real samples/s | (a) is x faster |", "|---|---|---|---|---|"]
        for name, v in legs.items():
            out.append(f"| {name} | {v['ms']} | {v['spread']} | {v['gsamples_s']} | {ratio(a, v) if name != 'a real' else '1'} |")
        b = legs["b complex64 of 8192"]
        met = ratio(a, b) > b["spread"]
        out += ["", f"(a) moves {r['hbm_fraction']:.1%} of the HBM peak of {HBM_PEAK / 1e12:g} TB/s ((b): {r['b_hbm_fraction']:.1%} at 8 + 4 B per "
                f"sample of 8192).  a/b = {ratio(a, b)} against (b)'s spread {b['spread']}: the expectation \"faster than (b) by more than "
                f"(b)'s spread\" is {'met' if met else 'NOT met'}.  a/c = {ratio(a, legs['c torch rfft'])}.  Worst |dB| between (a) and (b)'s "
                f"bins 0 ... 4096 within 40 dB of the peak, 64 frames: {r['worst_db_difference_to_b']:.2e}.", ""]
    for key, title in (("bench_line", "this build"), ("parent_bench_line", "the parent commit, same job")):
        if res.get(key):
            out += [f"## Flagship, {title}", "", "```", res[key], "```", ""]
    return "\n".join(out)


def last_json_line(path):
    if not path or not os.path.exists(path):
        return None
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
    return lines[-1] if lines else None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=17)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "real"))
    ap.add_argument("--bench-line", default=None, help="a file holding bench.py's JSON line of the same build, quoted in SUMMARY.md")
    ap.add_argument("--parent-bench-line", default=None, help="... and of the parent commit, measured in the same job")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    frames = 1 << args.frames_log2
    if args.child:
        print(json.dumps(child(args.child, frames)))
        return 0
    res = {"frames": frames, "formats": {}}
    for fmt in FORMATS:   # each GPU step in a process of its own, under its own limit; a failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", fmt,
                            "--frames-log2", str(args.frames_log2)], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{fmt}: child ended with status {r.returncode}\n{r.stderr[-3000:]}", file=sys.stderr)
            return 2
        res["formats"][fmt] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        print(json.dumps({fmt: res["formats"][fmt]["legs"]}), flush=True)
    res["device_name"] = next(iter(res["formats"].values()))["device_name"]
    res["bench_line"], res["parent_bench_line"] = last_json_line(args.bench_line), last_json_line(args.parent_bench_line)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_real.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(args.out_dir, "SUMMARY.md"), "w") as fh:
        fh.write(summary(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

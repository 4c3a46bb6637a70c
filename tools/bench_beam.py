"""Filter-and-sum beamformer against the same result composed from single-channel calls.

    python tools/bench_beam.py [--blocks 8192] [--out profiles/beam]

One GPU, one process, N = 4096, device resident.  Per point (M, D) x C x format, two legs that ALTERNATE launch by launch:
  beam    one exec_device_beam* call on the (n, C) element stream;
  compose a torch de-interleave into C contiguous streams (with the widen to complex64 for the integer formats), C
          exec_device_ddc calls on C plans holding set_fir(h_c), a torch sum of the C outputs
both on one torch side stream and timed with its events.  Warm-up by time (0.5 s), then three rounds of 30 launches per leg; a
leg's figure is the median of its round medians and its spread the largest over the smallest of them.  Also the single ddc call
on one channel's samples (the (C + 1) / 2 transform model's unit).  Writes SUMMARY.md and bench_beam.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, beam_taps, ddc_taps  # noqa: E402

N, WORD = 4096, 0x12345678
POINTS, CHANNELS, FORMATS = ((257, 50), (2049, 200)), (2, 4, 8), ("c64", "ci16", "cu8")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(legs, rounds=3, launches=30, warm_s=0.5):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for fn in legs.values():
            timed(fn)
    meds = {k: [] for k in legs}
    for _ in range(rounds):
        ms = {k: [] for k in legs}
        for _ in range(launches):
            for k, fn in legs.items():              # the legs alternate
                ms[k].append(timed(fn))
        for k in legs:
            meds[k].append(float(np.median(ms[k])))
    return {k: {"ms": float(np.median(v)), "spread": max(v) / min(v), "rounds": v} for k, v in meds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 13)
    ap.add_argument("--out", default="profiles/beam")
    args = ap.parse_args()
    side = torch.cuda.Stream()                      # (the default stream's handle is 0, which the library reads as "the plan's stream")
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream != 0
    rows = []
    for m, d in POINTS:
        L = (4097 - m) // 256 * 256
        n = args.blocks * L + m - 1
        h = ddc_taps(d, m)
        for c in CHANNELS:
            filt = beam_taps(np.exp(0.4j * np.arange(c)) / c, h)
            plan = SpectrumPlan(N)
            plan.set_beam(filt)
            singles = []
            for k in range(c):
                p = SpectrumPlan(N)
                p.set_fir(filt[k])
                singles.append(p)
            n_out = plan.beam_outputs(n, d, 0)
            rng = np.random.default_rng(c + m)
            raw8 = torch.from_numpy(rng.integers(0, 256, (n, c, 2), dtype=np.uint8)).cuda()
            for fmt in FORMATS:
                if fmt == "c64":
                    x = (raw8.to(torch.float32) - 127.5).contiguous()
                    x = torch.view_as_complex(x)
                    beam = lambda: plan.exec_device_beam(x.data_ptr(), n, out.data_ptr(), WORD, decim=d, stream=stream)  # noqa: E731
                    widen = lambda t: t  # noqa: E731
                elif fmt == "ci16":
                    x = ((raw8.to(torch.int16) - 128) * 200).contiguous()
                    beam = lambda: plan.exec_device_beam_ci16(x.data_ptr(), n, out.data_ptr(), WORD, decim=d, stream=stream)  # noqa: E731
                    widen = lambda t: torch.view_as_complex(t.to(torch.float32))  # noqa: E731
                else:
                    x = raw8
                    beam = lambda: plan.exec_device_beam_ci8(x.data_ptr(), n, out.data_ptr(), WORD, unsigned=True, decim=d, stream=stream)  # noqa: E731
                    widen = lambda t: torch.view_as_complex(t.to(torch.float32) - 127.5)  # noqa: E731
                out = torch.empty(n_out, dtype=torch.complex64, device="cuda")
                parts = torch.empty((c, n_out), dtype=torch.complex64, device="cuda")

                def compose():
                    streams = [widen(x[:, k]).contiguous() for k in range(c)]       # de-interleave (+ widen)
                    for k in range(c):
                        singles[k].exec_device_ddc(streams[k].data_ptr(), n, parts[k].data_ptr(), WORD, decim=d, stream=stream)
                    return parts.sum(dim=0)

                one = widen(x[:, 0]).contiguous()
                single = lambda: singles[0].exec_device_ddc(one.data_ptr(), n, parts[0].data_ptr(), WORD, decim=d, stream=stream)  # noqa: E731
                got = compose()
                beam()
                torch.cuda.synchronize()
                err = float((out - got).abs().max() / got.abs().max())
                r = measure({"beam": beam, "compose": compose, "single_ddc": single})
                row = {"taps": m, "decim": d, "channels": c, "format": fmt, "blocks": args.blocks, "elements": n, **r,
                       "speedup": r["compose"]["ms"] / r["beam"]["ms"], "beats_spread": r["compose"]["ms"] / r["beam"]["ms"] > r["compose"]["spread"],
                       "per_block_vs_single": r["beam"]["ms"] / r["single_ddc"]["ms"], "model": (c + 1) / 2,
                       "gsamples_per_s": n * c / r["beam"]["ms"] / 1e6, "rel_diff_to_composition": err}
                rows.append(row)
                print(json.dumps({k: v for k, v in row.items() if k not in ("beam", "compose", "single_ddc")}), flush=True)
                del x, out, parts, one
            for p in singles + [plan]:
                p.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_beam.json"), "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    with open(os.path.join(args.out, "SUMMARY.md"), "w") as f:
        f.write("# Filter-and-sum beamformer against C single-channel DDC calls\n\n"
                f"`tools/bench_beam.py --blocks {args.blocks}` on {torch.cuda.get_device_name(0)}: legs alternate, warm-up 0.5 s, median of "
                "3 round medians of 30 launches; spread = largest / smallest round median.\n\n"
                "| M | D | C | format | beam ms (spread) | composed ms (spread) | speed-up | beats spread | beam / single ddc | model (C+1)/2 | Gsample/s |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['taps']} | {r['decim']} | {r['channels']} | {r['format']} | {r['beam']['ms']:.3f} ({r['beam']['spread']:.3f}) | "
                    f"{r['compose']['ms']:.3f} ({r['compose']['spread']:.3f}) | {r['speedup']:.2f} | {'yes' if r['beats_spread'] else 'NO'} | "
                    f"{r['per_block_vs_single']:.2f} | {r['model']:.1f} | {r['gsamples_per_s']:.1f} |\n")


if __name__ == "__main__":
    main()

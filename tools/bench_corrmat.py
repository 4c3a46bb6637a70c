"""The correlation-matrix calls against the routes a user has without them, leg by leg (profiles/corrmat/SUMMARY.md and
bench_corrmat.json beside it are written by this tool; it is the only place a timing of these calls is taken).

    python tools/bench_corrmat.py [--frames-log2 13] [--out-dir profiles/corrmat] [--parity-log pytest_output.txt]

N = 4096, Hann, device resident, 2^13 frames of elements, K = 16 and all frames as ONE group (the split path and its
finalize), C = 2, 4, 5, 8 from complex64, int16 and 8-bit (cu8) elements.  Per leg, in the same process and the same
alternation after a warm-up by time (an idle MI355X needs tens of milliseconds of load to reach its sustained clock):
  direct   corrmat4096_spectra_kernel reads the element stream, corrmat_rows_kernel reduces (SDRK_CORRMAT_ROUTE=direct);
  split    the staged split route at N = 4096 (SDRK_CORRMAT_ROUTE=split: de-interleave, the plan's transform per channel);
           the library takes whichever of the two measured faster for the format and C (cm4k_reads_directly);
  pairs    C(C-1)/2 two-channel calls (complex64 and int16): ONE call on the re-interleaved pair (0, 1) is timed and multiplied;
  xspec    at C = 2, the fused two-channel call on the same buffer;
  torch    torch.fft.fft per channel plus an einsum over the frames of a group (complex64, wall time).
A leg's figure is the MEDIAN of its per-launch times (the *_timed_each entry points: events between consecutive launches) and
every leg's own spread (of its round medians, over its median) stands beside it.  No ratio is required.  Bytes per element are
the model's: the elements read once, the spectra written and read once (24 C from complex64, (16 + 2) C from 8-bit), the split
route 16 C more.  --parity-log: the output of `pytest -s tests/test_corrmat_gpu.py`; its err/tol lines go into the summary."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

N = 4096
HBM_PEAK = 8.0e12
CHANNELS = (2, 4, 5, 8)
SAMPLE_BYTES = {"c64": 8, "i16": 4, "u8": 2}


def torch_route(x, k, reps=3):
    """Wall time of: every channel's windowed FFT with torch.fft and the einsum of X_c conj(X_d) over the frames of a group
    (everything stays on the device).  x: (frames * N, C) complex64."""
    frames, C = x.shape[0] // N, x.shape[1]
    w = torch.hann_window(N, periodic=False, dtype=torch.float32, device=x.device)[None, :, None]
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = torch.fft.fft(x.view(frames, N, C) * w, dim=1).view(frames // k, k, N, C)
        r = torch.einsum("gknc,gknd->gncd", s, s.conj()) / k
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del s, r
    return statistics.median(times[1:]) * 1e3


def with_route(route, run):
    def go(n):
        if route:
            os.environ["SDRK_CORRMAT_ROUTE"] = route
        try:
            return run(n)
        finally:
            os.environ.pop("SDRK_CORRMAT_ROUTE", None)
    return go


def measure_channels(plan, C, n_frames, rounds, per_round, warm_s):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2024 + C)
    L = n_frames * N
    x = {"i16": torch.randint(-2048, 2048, (L, C, 2), dtype=torch.int16, device=dev, generator=g),
         "u8": torch.randint(0, 256, (L, C, 2), dtype=torch.uint8, device=dev, generator=g)}
    x["c64"] = torch.view_as_complex(x["i16"].to(torch.float32).contiguous())
    pair = {"c64": x["c64"][:, :2].contiguous(), "i16": x["i16"][:, :2].contiguous()}
    out = torch.empty((n_frames // 16 * C * C * N,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    d_out = out.data_ptr()
    entry = {"c64": plan.exec_device_corrmat_timed_each, "i16": plan.exec_device_corrmat_ci16_timed_each,
             "u8": lambda *a: plan.exec_device_corrmat_ci8_timed_each(*a, unsigned=True)}
    xspec = {"c64": plan.exec_device_xspec_timed_each, "i16": plan.exec_device_xspec_ci16_timed_each}
    legs = {}
    for kname, k in (("k16", 16), ("one_group", n_frames)):
        groups = n_frames // k
        for fmt, sb in SAMPLE_BYTES.items():
            p = x[fmt].data_ptr()
            call = lambda n, p=p, fmt=fmt, groups=groups, k=k: entry[fmt](p, C, groups, k, d_out, n)   # noqa: E731
            legs[f"direct_{fmt}_{kname}"] = (k, (sb + 16) * C, with_route("direct", call))
            legs[f"split_{fmt}_{kname}"] = (k, (sb + 32) * C, with_route("split", call))
            if fmt in xspec:
                pp = pair[fmt].data_ptr()
                legs[f"pair01_{fmt}_{kname}"] = (k, 2 * sb, lambda n, pp=pp, fmt=fmt, groups=groups, k=k: xspec[fmt](pp, groups, k, d_out, n))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for _, _, run in legs.values():
            run(2)
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (_, _, run) in legs.items():
            ms[name].append(run(per_round))
    res = {"channels": C, "legs": {}, "torch_route_ms": {kn: round(torch_route(x["c64"], k), 4) for kn, k in (("k16", 16), ("one_group", n_frames))}}
    for name, (k, byts, _) in legs.items():
        flat = [v for r in ms[name] for v in r]
        med, per_round_med = statistics.median(flat), [statistics.median(r) for r in ms[name]]
        res["legs"][name] = {"k": k, "ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                             "spread_of_round_medians": round((max(per_round_med) - min(per_round_med)) / med, 4),
                             "gelements_s": round(L / med / 1e6, 2), "model_bytes_per_element": byts,
                             "fraction_of_8TBs": round(L * byts / (med * 1e-3) / HBM_PEAK, 4)}
    n_pairs = C * (C - 1) // 2
    for kname in ("k16", "one_group"):
        for fmt in SAMPLE_BYTES:
            d, s = res["legs"][f"direct_{fmt}_{kname}"], res["legs"][f"split_{fmt}_{kname}"]
            d["split_route_over_this"] = round(s["ms"] / d["ms"], 3)
            d["torch_route_over_this"] = round(res["torch_route_ms"][kname] / d["ms"], 2)
            if f"pair01_{fmt}_{kname}" in res["legs"]:
                one = res["legs"][f"pair01_{fmt}_{kname}"]
                d["pair_calls"] = n_pairs
                d["pair_calls_over_this"] = round(n_pairs * one["ms"] / d["ms"], 3)
    return res


def measure(n_frames, rounds=5, per_round=4, warm_s=0.3):
    with SpectrumPlan(N, window="hann") as plan:
        per_c = [measure_channels(plan, C, n_frames, rounds, per_round, warm_s) for C in CHANNELS]
    return {"nfft": N, "element_frames": n_frames, "window": "hann", "launches_per_leg": rounds * per_round, "per_channels": per_c}


def compiler_figures():
    """The ELF-note figures of the new kernels (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"corrmat", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    return [ln.strip().lstrip(".") for ln in open(path) if "err/tol" in ln]   # (pytest's dots)


def write_summary(res, path):
    t = res["timing"]
    lines = ["# Correlation matrix of 2..8 channels (sdrk_exec_*_corrmat): measured on " + res["device"], "",
             f"Written by tools/bench_corrmat.py.  N = 4096, Hann, device resident, {t['element_frames']} frames of elements; median of "
             f"{t['launches_per_leg']} launches per leg, legs alternating in one process after a warm-up by time.  `direct`: the spectra "
             "kernel reads the element stream; `split`: the staged split route at N = 4096; `pair01`: ONE two-channel call on the pair "
             "(0, 1) (`pairs / this` multiplies it by C(C-1)/2).  B/element is the model's.", ""]
    for pc in t["per_channels"]:
        lines += [f"## C = {pc['channels']}", "",
                  "| leg | K | ms | own spread | Gelements/s | B/element (model) | of 8 TB/s | split / this | pairs / this | torch / this |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for name, leg in pc["legs"].items():
            lines.append(f"| {name} | {leg['k']} | {leg['ms']} | {leg['spread_of_round_medians']} | {leg['gelements_s']} | "
                         f"{leg['model_bytes_per_element']} | {leg['fraction_of_8TBs']} | {leg.get('split_route_over_this', '')} | "
                         f"{leg.get('pair_calls_over_this', '')} | {leg.get('torch_route_over_this', '')} |")
        lines += ["", "The torch route (torch.fft.fft per channel, einsum over the frames of a group; complex64, wall time): " +
                  ", ".join(f"{n} {v} ms" for n, v in pc["torch_route_ms"].items()) + ".", ""]
    lines += ["## Compiler figures of the new kernels (corrmat4096_spectra_kernel: built for 3 workgroups per CU)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        worst = [max(float(v) for v in re.findall(rf"{w} ([0-9.e+-]+)", "\n".join(res["parity"]))) for w in ("autos", "pairs")]
        lines += ["", "## err/tol of tests/test_corrmat_gpu.py on this device", "",
                  f"Worst over every check: autos {worst[0]:.2e}, pairs {worst[1]:.2e}.", ""] + [f"- {ln}" for ln in res["parity"]]
    reading = ""          # a hand-written "## Reading the figures" at the end of the last summary is kept
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Reading the figures" in old:
            reading = old[old.index("\n## Reading the figures"):]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n" + reading)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=13)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "corrmat"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.frames_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_corrmat.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps({pc["channels"]: {n: leg["ms"] for n, leg in pc["legs"].items()} for pc in res["timing"]["per_channels"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

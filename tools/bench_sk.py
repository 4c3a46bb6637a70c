"""Spectral kurtosis against the integrated MEAN call, leg by leg (profiles/sk/SUMMARY.md and bench_sk.json beside it are written
by this tool; it is the only place a timing of the SK calls is taken).

    python tools/bench_sk.py [--frames-log2 16] [--out-dir profiles/sk] [--parity-log pytest_output.txt]

N = 4096, Hann, device resident.  The SK call at K = 16 and with all frames as ONE group (the split path and its finalize),
from complex64 and from int16 I,Q; in the same process and the same alternation the unchanged sdrk_exec_device_integrated
(MEAN, dB) on the same frames, with that call's own run-to-run spread; and for context the numpy-style route — the per-frame
call followed by a torch reduction of its rows to S1, S2 and SK.  Legs alternate after a warm-up by time (an idle MI355X
needs tens of milliseconds of load to reach its sustained clock); a leg's figure is the MEDIAN of its per-launch times (the
*_timed_each entry points: events between consecutive launches).  No rate is required: the structural gate is the code-object
budget (tests/test_sk_code_objects.py), whose figures the summary quotes.  --parity-log: the output of
`pytest -s tests/test_sk_gpu.py`; its worst err/tol lines go into the summary."""
from __future__ import annotations

import argparse
import ctypes
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
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

N = 4096
HBM_PEAK = 8.0e12


def dev_alloc(nbytes):
    p = ctypes.c_void_p()
    _ffi.check(_ffi.lib().sdrk_dev_alloc(0, nbytes, ctypes.byref(p)))
    return p


def numpy_style_route(plan, d_in, n_frames, k, reps=5):
    """Wall time of: every per-frame dB row to device memory, then S1, S2 and SK from the rows with torch (what a user does
    today, minus the copy of the rows to the host)."""
    rows = torch.empty((n_frames, N), dtype=torch.float32, device="cuda:0")
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.exec_device(d_in, n_frames, rows.data_ptr())
        plan.sync()
        p = torch.pow(10.0, rows * 0.1).view(n_frames // k, k, N)
        s1, s2 = p.sum(dim=1), (p * p).sum(dim=1)
        sk = (k + 1.0) / (k - 1.0) * (k * s2 / (s1 * s1) - 1.0)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del p, s1, s2, sk
    return statistics.median(times[1:]) * 1e3


def measure(n_frames, rounds=6, per_round=5, warm_s=0.4):
    lib = _ffi.lib()
    d_in, d16 = dev_alloc(n_frames * N * 8), dev_alloc(n_frames * N * 4)
    d_out = dev_alloc(n_frames // 16 * 2 * N * 4)
    samples = n_frames * N
    try:
        _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, N, d_in, None))
        _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, n_frames, N, d16, None))
        with SpectrumPlan(N, window="hann") as plan:
            legs = {}
            for name, k in (("k16", 16), ("one_group", n_frames)):
                g = n_frames // k
                legs[f"mean_{name}"] = (k, 8 + 4.0 / k, lambda n, g=g, k=k: plan.exec_device_integrated_timed_each(d_in.value, g, k, d_out.value, n))
                legs[f"sk_{name}"] = (k, 8 + 8.0 / k, lambda n, g=g, k=k: plan.exec_device_sk_timed_each(d_in.value, g, k, d_out.value, n))
                legs[f"mean_i16_{name}"] = (k, 4 + 4.0 / k, lambda n, g=g, k=k: plan.exec_device_integrated_ci16_timed_each(d16.value, g, k, d_out.value, n))
                legs[f"sk_i16_{name}"] = (k, 4 + 8.0 / k, lambda n, g=g, k=k: plan.exec_device_sk_ci16_timed_each(d16.value, g, k, d_out.value, n))
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                for _, _, run in legs.values():
                    run(2)
            ms = {name: [] for name in legs}
            for _ in range(rounds):
                for name, (_, _, run) in legs.items():
                    ms[name].append(run(per_round))
            context = numpy_style_route(plan, d_in.value, n_frames, 16)
    finally:
        for d in (d_in, d16, d_out):
            lib.sdrk_dev_free(0, d)
    out = {"nfft": N, "frames": n_frames, "window": "hann", "launches_per_leg": rounds * per_round, "legs": {},
           "numpy_style_route_k16_ms": round(context, 4)}
    for name, (k, byts, _) in legs.items():
        flat = [v for r in ms[name] for v in r]
        med, per_round_med = statistics.median(flat), [statistics.median(r) for r in ms[name]]
        out["legs"][name] = {"k": k, "ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                             "spread_of_round_medians": round((max(per_round_med) - min(per_round_med)) / med, 4),
                             "gsamples_s": round(samples / med / 1e6, 2), "bytes_per_sample": round(byts, 4),
                             "fraction_of_8TBs": round(samples * byts / (med * 1e-3) / HBM_PEAK, 4)}
    for kind in ("", "_i16"):
        for name in ("k16", "one_group"):
            sk, mean = out["legs"][f"sk{kind}_{name}"], out["legs"][f"mean{kind}_{name}"]
            sk["time_over_mean_call"] = round(sk["ms"] / mean["ms"], 4)
            sk["allowed"] = round(1.05 + mean["spread_of_round_medians"], 4)      # that call's spread plus 5 %
            sk["within_allowed"] = sk["time_over_mean_call"] <= sk["allowed"]
    return out


def compiler_figures():
    """The ELF-note figures of the new kernels (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"sk4096_kernel|sk_rows_kernel|sk_finalize_kernel", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    return [ln.strip().lstrip(".") for ln in open(path) if "err/tol" in ln or "|SK|/tol" in ln or "bits agree" in ln]   # (pytest's dots)


def write_summary(res, path):
    lines = ["# Spectral kurtosis (sdrk_exec_*_sk): measured on " + res["device"], "",
             f"Written by tools/bench_sk.py.  N = 4096, Hann, device resident, {res['timing']['frames']} frames; median of "
             f"{res['timing']['launches_per_leg']} launches per leg, legs alternating in one process after a warm-up by time.", "",
             "| leg | K | ms | Gsamples/s | B/sample | of 8 TB/s | time / MEAN call | allowed (spread + 5 %) |", "|---|---|---|---|---|---|---|---|"]
    for name, leg in res["timing"]["legs"].items():
        lines.append(f"| {name} | {leg['k']} | {leg['ms']} | {leg['gsamples_s']} | {leg['bytes_per_sample']} | {leg['fraction_of_8TBs']} | "
                     f"{leg.get('time_over_mean_call', '')} | {leg.get('allowed', '')} |")
    lines += ["", "Run-to-run spread of the MEAN call (range of its round medians over its median): " +
              ", ".join(f"{n} {leg['spread_of_round_medians']}" for n, leg in res["timing"]["legs"].items() if n.startswith("mean")) + ".",
              f"The numpy-style route (per-frame rows, then S1, S2 and SK with torch, K = 16): {res['timing']['numpy_style_route_k16_ms']} ms wall.",
              "", "## Compiler figures of the new kernels", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        lines += ["", "## Worst err/tol of tests/test_sk_gpu.py on this device", ""] + [f"- {ln}" for ln in res["parity"]]
    reading = ""          # a hand-written "## Reading the figures" at the end of the last summary is kept
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Reading the figures" in old:
            reading = old[old.index("\n## Reading the figures"):]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n" + reading)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=16)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "sk"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.frames_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_sk.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps(res["timing"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Two-channel cross-spectra against the integrated MEAN call and against the route a user has without them, leg by leg
(profiles/xspec/SUMMARY.md and bench_xspec.json beside it are written by this tool; it is the only place a timing of the
cross-spectrum calls is taken).

    python tools/bench_xspec.py [--frames-log2 15] [--out-dir profiles/xspec] [--parity-log pytest_output.txt]

N = 4096, Hann, device resident, 2^15 frames of elements (2^16 transforms).  The cross-spectrum call at K = 16 and with all
frames as ONE group (the split path and its finalize), from complex64 and from int16 elements; in the same process and the same
alternation the unchanged sdrk_exec_device_integrated (MEAN, dB) on 2^16 packed frames — the same transforms and the same input
bytes — with that call's own run-to-run spread; and the route a user has today: torch.fft.fft of both channels, the products
and a reduction over the group.  Legs alternate after a warm-up by time (an idle MI355X needs tens of milliseconds of load to
reach its sustained clock); a leg's figure is the MEDIAN of its per-launch times (the *_timed_each entry points: events between
consecutive launches).  No ratio is required: the structural gate is the code-object budget
(tests/test_xspec_code_objects.py), whose figures the summary quotes.  --parity-log: the output of
`pytest -s tests/test_xspec_gpu.py`; its err/tol lines go into the summary."""
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
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

N = 4096
HBM_PEAK = 8.0e12


def torch_route(x, k, reps=4):
    """Wall time of: both channels' windowed FFTs with torch.fft, |A|^2, |B|^2 and A conj(B), and their means over groups of k
    frames (everything stays on the device).  x: (frames * N, 2) complex64."""
    frames = x.shape[0] // N
    w = torch.hann_window(N, periodic=False, dtype=torch.float32, device=x.device)
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = x.view(frames, N, 2)
        a, b = torch.fft.fft(f[:, :, 0] * w, dim=1), torch.fft.fft(f[:, :, 1] * w, dim=1)
        paa = (a.real * a.real + a.imag * a.imag).view(frames // k, k, N).mean(dim=1)
        pbb = (b.real * b.real + b.imag * b.imag).view(frames // k, k, N).mean(dim=1)
        c = (a * b.conj()).view(frames // k, k, N).mean(dim=1)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del f, a, b, paa, pbb, c
    return statistics.median(times[1:]) * 1e3


def measure(n_frames, rounds=6, per_round=5, warm_s=0.4):
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    x = torch.empty((n_frames * N, 2), dtype=torch.complex64, device=dev)         # elements; also 2 n_frames packed frames
    x16 = torch.empty((n_frames * N, 4), dtype=torch.int16, device=dev)
    out = torch.empty((n_frames // 16 * 4 * N,), dtype=torch.float32, device=dev)
    _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, 2 * n_frames, N, x.data_ptr(), None))
    _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, 2 * n_frames, N, x16.data_ptr(), None))
    torch.cuda.synchronize()
    d_in, d16, d_out = x.data_ptr(), x16.data_ptr(), out.data_ptr()
    elements = n_frames * N
    with SpectrumPlan(N, window="hann") as plan:
        legs = {}
        for name, k in (("k16", 16), ("one_group", n_frames)):
            g = n_frames // k
            # the yardstick: 2 n_frames packed frames in groups of 2 k — the same transforms, input bytes and output rows / 4
            legs[f"mean_{name}"] = (2 * k, 16 + 8.0 / k, lambda n, g=g, k=k: plan.exec_device_integrated_timed_each(d_in, g, 2 * k, d_out, n))
            legs[f"xspec_{name}"] = (k, 16 + 16.0 / k, lambda n, g=g, k=k: plan.exec_device_xspec_timed_each(d_in, g, k, d_out, n))
            legs[f"mean_i16_{name}"] = (2 * k, 8 + 8.0 / k, lambda n, g=g, k=k: plan.exec_device_integrated_ci16_timed_each(d16, g, 2 * k, d_out, n))
            legs[f"xspec_i16_{name}"] = (k, 8 + 16.0 / k, lambda n, g=g, k=k: plan.exec_device_xspec_ci16_timed_each(d16, g, k, d_out, n))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_s:
            for _, _, run in legs.values():
                run(2)
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, (_, _, run) in legs.items():
                ms[name].append(run(per_round))
        torch_ms = {name: torch_route(x, k) for name, k in (("k16", 16), ("one_group", n_frames))}
    res = {"nfft": N, "element_frames": n_frames, "transforms": 2 * n_frames, "window": "hann",
           "launches_per_leg": rounds * per_round, "legs": {}, "torch_route_ms": {k: round(v, 4) for k, v in torch_ms.items()}}
    for name, (k, byts, _) in legs.items():
        flat = [v for r in ms[name] for v in r]
        med, per_round_med = statistics.median(flat), [statistics.median(r) for r in ms[name]]
        res["legs"][name] = {"k": k, "ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                             "spread_of_round_medians": round((max(per_round_med) - min(per_round_med)) / med, 4),
                             "gelements_s": round(elements / med / 1e6, 2), "bytes_per_element": round(byts, 4),
                             "fraction_of_8TBs": round(elements * byts / (med * 1e-3) / HBM_PEAK, 4)}
    for kind in ("", "_i16"):
        for name in ("k16", "one_group"):
            xs, mean = res["legs"][f"xspec{kind}_{name}"], res["legs"][f"mean{kind}_{name}"]
            xs["time_over_mean_call"] = round(xs["ms"] / mean["ms"], 4)
            xs["mean_call_spread"] = mean["spread_of_round_medians"]
            xs["torch_route_over_this"] = round(torch_ms[name] / xs["ms"], 2)
    return res


def compiler_figures():
    """The ELF-note figures of the new kernels (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"xspec", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    keep = ("err/tol", "mean coherence", "bits agree")
    return [ln.strip().lstrip(".") for ln in open(path) if any(w in ln for w in keep)]   # (pytest's dots)


def write_summary(res, path):
    t = res["timing"]
    lines = ["# Two-channel cross-spectra (sdrk_exec_*_xspec): measured on " + res["device"], "",
             f"Written by tools/bench_xspec.py.  N = 4096, Hann, device resident, {t['element_frames']} frames of elements "
             f"({t['transforms']} transforms); median of {t['launches_per_leg']} launches per leg, legs alternating in one process after "
             "a warm-up by time.  The MEAN legs are sdrk_exec_device_integrated on the same bytes read as twice as many packed frames.", "",
             "| leg | K | ms | Gelements/s | B/element | of 8 TB/s | time / MEAN call | MEAN call's spread | torch route / this |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, leg in t["legs"].items():
        lines.append(f"| {name} | {leg['k']} | {leg['ms']} | {leg['gelements_s']} | {leg['bytes_per_element']} | {leg['fraction_of_8TBs']} | "
                     f"{leg.get('time_over_mean_call', '')} | {leg.get('mean_call_spread', '')} | {leg.get('torch_route_over_this', '')} |")
    lines += ["", "The torch route (torch.fft.fft of both channels, the products, the means over the group; complex64, wall time): " +
              ", ".join(f"{n} {v} ms" for n, v in t["torch_route_ms"].items()) + ".",
              "", "## Compiler figures of the new kernels (xspec4096_kernel: built for 2 workgroups per CU)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        lines += ["", "## err/tol of tests/test_xspec_gpu.py on this device", ""] + [f"- {ln}" for ln in res["parity"]]
    reading = ""          # a hand-written "## Reading the figures" at the end of the last summary is kept
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Reading the figures" in old:
            reading = old[old.index("\n## Reading the figures"):]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n" + reading)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-log2", type=int, default=15)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "xspec"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.frames_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_xspec.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps(res["timing"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

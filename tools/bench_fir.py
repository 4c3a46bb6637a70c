"""The overlap-save FIR call against the plan's own per-frame call and against a torch composition of the same overlap-save, leg
by leg (profiles/fir/SUMMARY.md and bench_fir.json beside it are written by this tool; it is the only place a timing of the FIR
calls is taken).

    python tools/bench_fir.py [--blocks-log2 14] [--out-dir profiles/fir] [--parity-log pytest_output.txt]

Device resident, 2^14 blocks of input at (M, D, s) = (257, 1, 0), (257, 16, 611), (2049, 64, 611), from complex64 and from int16,
with the blocks dealt grid-stride and in contiguous runs (SDRK_OLS_ASSIGN, read when the filter is set: two plans).  In the same
process and the same alternation: the plan's own per-frame call on as many packed frames of 4096 (sdrk_exec_device, dB rows: the
library has no device entry for complex spectra; one transform per frame, 8 B in and 4 B out per sample) with its own run-to-run
spread, and a torch composition of the same overlap-save on the same buffer (unfold into blocks -> torch.fft.fft -> multiply ->
torch.fft.ifft -> slice -> mix -> stride).  Legs alternate after a warm-up by time; a leg's figure is the MEDIAN of its
per-launch times.  The one condition: the fused call is not slower than the torch composition at (257, 1).
--parity-log: the output of `pytest -s tests/test_fir_gpu.py`; its err/tol lines go into the summary."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: one HIP runtime shared with libsdrk)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sdr_iq_visualizer_amd as pkg  # noqa: E402
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, channel_taps  # noqa: E402

N = 4096
HBM_PEAK = 8.0e12
SHAPES = [(257, 1, 0), (257, 16, 611), (2049, 64, 611)]


def block_len(m):
    return (N + 1 - m) // 256 * 256


def torch_route(x, h, m, d, s, n_blocks, reps=3, batch=2048):
    """Wall time of the same overlap-save with torch on the resident buffer, in batches of blocks (the spectra of all 2^14 blocks
    at once would take three more copies of the band)."""
    L = block_len(m)
    hs = torch.zeros(N, dtype=torch.complex64, device=x.device)
    hs[:m] = torch.as_tensor(h, device=x.device)
    H = torch.roll(torch.fft.fft(hs), s)
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = []
        for b0 in range(0, n_blocks, batch):
            nb = min(batch, n_blocks - b0)
            blocks = x[b0 * L:(b0 + nb - 1) * L + N].unfold(0, N, L)
            y = torch.fft.ifft(torch.fft.fft(blocks, dim=1) * H, dim=1)[:, m - 1:m - 1 + L].reshape(-1)
            if s:
                i = torch.arange(b0 * L, (b0 + nb) * L, device=x.device)
                y = y * torch.exp(-2j * np.pi * ((s * i) % N).to(torch.float32) / N)
            outs.append(y[::d].contiguous())
        out = torch.cat(outs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del outs, out, y, blocks
    return statistics.median(times[1:]) * 1e3


def timed_i16(plan, d16, n_in, d_out, d, s, launches):
    """Per-launch milliseconds of the int16 entry (it has no *_timed_each form): events around each launch on the plan's stream
    would need the stream; wall time over `launches` launches and one sync instead."""
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        plan.exec_device_fir_ci16(d16, n_in, d_out, decim=d, shift_bins=s)
    plan.sync()
    return [(time.perf_counter() - t0) * 1e3 / launches] * launches


def measure(n_blocks, rounds=6, per_round=5, warm_s=0.4):
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    n_frames = n_blocks + 1                                                        # every shape's input fits: L <= 4096
    x = torch.empty((n_frames * N,), dtype=torch.complex64, device=dev)
    x16 = torch.empty((n_frames * N, 2), dtype=torch.int16, device=dev)
    out = torch.empty((n_frames * N,), dtype=torch.complex64, device=dev)
    _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, N, x.data_ptr(), None))
    _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, n_frames, N, x16.data_ptr(), None))
    torch.cuda.synchronize()
    d_in, d16, d_out = x.data_ptr(), x16.data_ptr(), out.data_ptr()
    res = {"blocks": n_blocks, "launches_per_leg": rounds * per_round, "shapes": {}}
    for m, d, s in SHAPES:
        L = block_len(m)
        n_in = n_blocks * L + m - 1
        h = channel_taps(d, m)
        plans = {}
        for name, assign in (("stride", "0"), ("runs", "1")):
            os.environ["SDRK_OLS_ASSIGN"] = assign
            plans[name] = SpectrumPlan(N)
            plans[name].set_fir(h)
        os.environ.pop("SDRK_OLS_ASSIGN")
        ps, pr = plans["stride"], plans["runs"]
        legs = {
            "frames_db": lambda n: ps.exec_device_timed_each(d_in, n_blocks, d_out, n),
            "fir_c64_stride": lambda n: ps.exec_device_fir_timed_each(d_in, n_in, d_out, n, decim=d, shift_bins=s),
            "fir_c64_runs": lambda n: pr.exec_device_fir_timed_each(d_in, n_in, d_out, n, decim=d, shift_bins=s),
            "fir_i16_stride": lambda n: timed_i16(ps, d16, n_in, d_out, d, s, n),
            "fir_i16_runs": lambda n: timed_i16(pr, d16, n_in, d_out, d, s, n),
        }
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < warm_s:
            for run in legs.values():
                run(2)
        ms = {name: [] for name in legs}
        for _ in range(rounds):
            for name, run in legs.items():
                ms[name].append(run(per_round))
        torch_ms = torch_route(x, h, m, d, s, n_blocks)
        for p in plans.values():
            p.close()
        shape = {"taps": m, "decim": d, "shift_bins": s, "block_len": L, "n_in": n_in, "torch_route_ms": round(torch_ms, 4), "legs": {}}
        for name in legs:
            flat = [v for r in ms[name] for v in r]
            med, rmed = statistics.median(flat), [statistics.median(r) for r in ms[name]]
            elem = 4 if "i16" in name else 8
            byts = 12.0 if name == "frames_db" else elem * N / L + 8.0 / d
            samples = n_blocks * N if name == "frames_db" else n_in
            shape["legs"][name] = {"ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                                   "spread_of_round_medians": round((max(rmed) - min(rmed)) / med, 4),
                                   "gsamples_s": round(samples / med / 1e6, 2), "bytes_per_sample": round(byts, 4),
                                   "fraction_of_8TBs": round(samples * byts / (med * 1e-3) / HBM_PEAK, 4)}
        base = shape["legs"]["frames_db"]
        for name, leg in shape["legs"].items():
            if name != "frames_db":
                leg["time_per_sample_over_frames_call"] = round((leg["ms"] / n_in) / (base["ms"] / (n_blocks * N)), 4)
                leg["torch_route_over_this"] = round(torch_ms / leg["ms"], 2)
        res["shapes"][f"M{m}_D{d}"] = shape
    return res


def compiler_figures():
    """The ELF-note figures of the new kernel (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"ols4096", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    return [ln.strip().lstrip(".") for ln in open(path) if "worst err/tol" in ln or "100 blocks" in ln or "stopband tone" in ln
            or "ChannelStream" in ln or ln.lstrip(".").startswith("host M=")]


def write_summary(res, path):
    t = res["timing"]
    lines = ["# FIR filtering and channel extraction (sdrk_exec_*_fir): measured on " + res["device"], "",
             f"Written by tools/bench_fir.py.  Overlap-save in blocks of 4096, device resident, {t['blocks']} blocks; median of "
             f"{t['launches_per_leg']} launches per leg, legs alternating in one process after a warm-up by time.  frames_db is the "
             "plan's own per-frame call (dB rows, one transform per frame) on as many packed frames; stride / runs is how the blocks "
             "are dealt to the workgroups (SDRK_OLS_ASSIGN = 0 / 1).  Byte model: 8*4096/L + 8/D per input sample (4*4096/L + 8/D "
             "from int16).", ""]
    for key, shape in t["shapes"].items():
        lines += [f"## M = {shape['taps']}, D = {shape['decim']}, s = {shape['shift_bins']} (L = {shape['block_len']})", "",
                  "| leg | ms | Gsamples/s in | B/sample | of 8 TB/s | spread | time per sample / frames_db | torch route / this |",
                  "|---|---|---|---|---|---|---|---|"]
        for name, leg in shape["legs"].items():
            lines.append(f"| {name} | {leg['ms']} | {leg['gsamples_s']} | {leg['bytes_per_sample']} | {leg['fraction_of_8TBs']} | "
                         f"{leg['spread_of_round_medians']} | {leg.get('time_per_sample_over_frames_call', '')} | "
                         f"{leg.get('torch_route_over_this', '')} |")
        lines += ["", f"The torch composition of the same overlap-save: {shape['torch_route_ms']} ms.", ""]
    lines += ["## Compiler figures (ols4096_kernel: 3 workgroups per CU; complex64 with the mixer: 2)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        lines += ["", "## err/tol of tests/test_fir_gpu.py on this device", ""] + [f"- {ln}" for ln in res["parity"]]
    reading = ""          # a hand-written "## Reading the figures" at the end of the last summary is kept
    if os.path.exists(path):
        old = open(path).read()
        if "\n## Reading the figures" in old:
            reading = old[old.index("\n## Reading the figures"):]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n" + reading)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks-log2", type=int, default=14)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "fir"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.blocks_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_fir.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps(res["timing"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

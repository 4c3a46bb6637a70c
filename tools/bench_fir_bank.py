"""The channel bank against C single-channel calls of the same build, leg by leg (profiles/fir_bank/SUMMARY.md and
bench_fir_bank.json beside it are written by this tool; it is the only place a timing of the bank call is taken).

    python tools/bench_fir_bank.py [--blocks-log2 14] [--out-dir profiles/fir_bank] [--parity-log pytest_output.txt]

The method of tools/bench_fir.py: device resident, 2^14 blocks of complex64 input at (M, D) = (257, 16) and (2049, 64), for
C = 2, 8, 32 channels spread over the band.  Two legs alternate in one process after a warm-up by time:
    bank      one sdrk_exec_device_chanbank_timed_each launch: the input read once, 1 + C transforms per block;
    singles   C back-to-back sdrk_exec_device_fir_timed_each launches with the same shifts into the same planes, their times
              summed: the input read C times, 2 C transforms per block.  This is the yardstick: the existing kernel.
A leg's figure is the MEDIAN of its 30 per-launch times; its spread is that of the medians of the 6 rounds.  The one condition:
bank / singles < 1 by more than the singles leg's own spread, at every measured point.
--parity-log: the output of `pytest -s tests/test_fir_bank_gpu.py`; its err/tol lines go into the summary."""
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
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, channel_taps  # noqa: E402

N = 4096
HBM_PEAK = 8.0e12
SHAPES = [(257, 16), (2049, 64)]
CHANNELS = [2, 8, 32]


def block_len(m):
    return (N + 1 - m) // 256 * 256


def shifts_of(c):
    """C channel centres spread evenly over the band, none at 0 (every channel runs its mixer, in both legs)."""
    return [((k * N) // c + 100 + N // 2) % N - N // 2 for k in range(c)]


def measure(n_blocks, rounds=6, per_round=5, warm_s=0.4):
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    n_frames = n_blocks + 1                                                        # every shape's input fits: L <= 4096
    x = torch.empty((n_frames * N,), dtype=torch.complex64, device=dev)
    _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, N, x.data_ptr(), None))
    torch.cuda.synchronize()
    d_in = x.data_ptr()
    res = {"blocks": n_blocks, "launches_per_leg": rounds * per_round, "points": {}}
    for m, d in SHAPES:
        L = block_len(m)
        n_in = n_blocks * L + m - 1
        n_out = (n_in - m) // d + 1
        plan = SpectrumPlan(N)
        plan.set_fir(channel_taps(d, m))
        for c in CHANNELS:
            shifts = shifts_of(c)
            out = torch.empty((c * n_out,), dtype=torch.complex64, device=dev)
            d_out = out.data_ptr()

            def bank(n):
                return plan.exec_device_fir_bank_timed_each(d_in, n_in, d_out, shifts, n, decim=d)

            def singles(n):
                total = [0.0] * n
                for k, s in enumerate(shifts):
                    each = plan.exec_device_fir_timed_each(d_in, n_in, d_out + 8 * k * n_out, n, decim=d, shift_bins=s)
                    total = [a + b for a, b in zip(total, each)]
                return total

            legs = {"bank": bank, "singles": singles}
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < warm_s:
                for run in legs.values():
                    run(2)
            ms = {name: [] for name in legs}
            for _ in range(rounds):
                for name, run in legs.items():
                    ms[name].append(run(per_round))
            del out
            point = {"taps": m, "decim": d, "channels": c, "shift_bins": shifts, "block_len": L, "n_in": n_in, "legs": {}}
            for name in legs:
                flat = [v for r in ms[name] for v in r]
                med, rmed = statistics.median(flat), [statistics.median(r) for r in ms[name]]
                reads = 1 if name == "bank" else c
                byts = reads * 8.0 * N / L + c * 8.0 / d
                point["legs"][name] = {"ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                                       "spread_of_round_medians": round((max(rmed) - min(rmed)) / med, 4),
                                       "gsamples_s_in": round(n_in / med / 1e6, 2), "bytes_per_input_sample": round(byts, 4),
                                       "fraction_of_8TBs": round(n_in * byts / (med * 1e-3) / HBM_PEAK, 4),
                                       "transforms_per_block": 1 + c if name == "bank" else 2 * c}
            b, s = point["legs"]["bank"], point["legs"]["singles"]
            point["bank_over_singles"] = round(b["ms"] / s["ms"], 4)
            point["transform_model"] = round((1 + c) / (2 * c), 4)
            point["byte_model"] = round(b["bytes_per_input_sample"] / s["bytes_per_input_sample"], 4)
            point["faster_by_more_than_the_singles_spread"] = bool(b["ms"] < s["ms"] * (1 - s["spread_of_round_medians"]))
            res["points"][f"M{m}_D{d}_C{c}"] = point
        plan.close()
    return res


def compiler_figures():
    """The ELF-note figures of the new kernel (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"chanbank", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    return [ln.strip().lstrip(".") for ln in open(path) if "err/tol" in ln]


def write_summary(res, path):
    t = res["timing"]
    lines = ["# Channel bank (sdrk_exec_*_chanbank): measured on " + res["device"], "",
             f"Written by tools/bench_fir_bank.py.  Overlap-save in blocks of 4096, complex64, device resident, {t['blocks']} blocks; "
             f"median of {t['launches_per_leg']} launches per leg, legs alternating in one process after a warm-up by time.  `bank` is "
             "one bank call for C channels; `singles` is C back-to-back single-channel calls (sdrk_exec_device_fir) of the same build "
             "with the same shifts into the same planes, their times summed.  Transform model: (1 + C) / (2 C) transforms per block.  "
             "Byte model per input sample: bank 8*4096/L + C*8/D, singles C*(8*4096/L + 8/D).", "",
             "| M | D | C | bank ms | singles ms | bank / singles | transform model | byte model | singles spread | bank spread | "
             "bank Gsamples/s in | bank of 8 TB/s | singles of 8 TB/s | condition |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for p in t["points"].values():
        b, s = p["legs"]["bank"], p["legs"]["singles"]
        lines.append(f"| {p['taps']} | {p['decim']} | {p['channels']} | {b['ms']} | {s['ms']} | {p['bank_over_singles']} | "
                     f"{p['transform_model']} | {p['byte_model']} | {s['spread_of_round_medians']} | {b['spread_of_round_medians']} | "
                     f"{b['gsamples_s_in']} | {b['fraction_of_8TBs']} | {s['fraction_of_8TBs']} | "
                     f"{'holds' if p['faster_by_more_than_the_singles_spread'] else 'FAILS'} |")
    lines += ["", "## Compiler figures (chanbank_kernel: 2 workgroups per CU; H per channel from global memory, one channel ahead)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        lines += ["", "## err/tol of tests/test_fir_bank_gpu.py on this device (every plane also equals the single call in bits)", ""]
        lines += [f"- {ln}" for ln in res["parity"]]
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
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "fir_bank"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.blocks_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_fir_bank.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps(res["timing"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

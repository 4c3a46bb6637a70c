"""The down-converter from 8-bit I,Q against its int16 form and against today's extract route, leg by leg
(profiles/ddc_ci8/SUMMARY.md and bench_ddc_ci8.json beside it are written by this tool; it is the only place a timing of the 8-bit
down-converter calls is taken).

    python tools/bench_ddc_ci8.py [--blocks-log2 14] [--host-log2 27] [--out-dir profiles/ddc_ci8]

Points: (M, D) = (257, 50) and (2049, 200), the single call and the bank at C = 8.  The legs of a point alternate in one process after
a warm-up by time; a leg's figure is the MEDIAN of its launches (calls), its spread that of the medians of its rounds.
    (a) device  resident input of 2^14 blocks: the 8-bit call against the int16 DDC call (cu8; the format is a run-time argument of
                one kernel), each launch between two device events on one stream;
    (b) host    the host entry on 2^27 pageable samples: 8-bit (2 B/sample over the link) against int16 (4 B/sample), wall clock;
    (c) route   the same against what `cli.py extract` did with an 8-bit recording: numpy widens it to complex64
                (spectrum.iq8_to_c64), then the complex64 host call (8 B/sample) — the widening is timed on its own and added.
Nothing here is a gate: the figures are written down as measured."""
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
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, ddc_taps, iq8_to_c64  # noqa: E402

N = 4096
FINE = 0x12345678
SHAPES = ((257, 50), (2049, 200))
BANK_C = 8
ROUNDS, PER_ROUND, WARM_S = 6, 5, 0.4
HOST_ROUNDS, HOST_PER_ROUND = 4, 1


def block_len(m):
    return (N + 1 - m) // 256 * 256


def words_of(c):
    """C fine words spread over the band, none on a bin."""
    return [((k << 32) // c + FINE) & 0xFFFFFFFF for k in range(c)]


def timed(run, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    run()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def wall(run, _stream=None):
    t0 = time.perf_counter()
    run()
    return (time.perf_counter() - t0) * 1e3


def race(legs, clock, stream, rounds, per_round, warm_s):
    """{leg: {ms, spread, ...}}: the legs alternating after a warm-up by time (at least one call each)."""
    t0 = time.perf_counter()
    while True:
        for run in legs.values():
            clock(run, stream)
        if time.perf_counter() - t0 >= warm_s:
            break
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name, run in legs.items():
            ms[name].append([clock(run, stream) for _ in range(per_round)])
    out = {}
    for name, rs in ms.items():
        flat = [v for r in rs for v in r]
        med, rmed = statistics.median(flat), [statistics.median(r) for r in rs]
        out[name] = {"ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                     "spread_of_round_medians": round((max(rmed) - min(rmed)) / med, 4)}
    return out


def byte_model(m, d):
    """Bytes per input sample: in_elem 4096 / L in, 8 / D out."""
    L = block_len(m)
    return {fmt: round(elem * N / L + 8 / d, 4) for fmt, elem in (("ci8", 2), ("ci16", 4), ("c64", 8))}


def measure_device(n_blocks):
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    points = {}
    with torch.cuda.stream(stream):
        n_samples = (n_blocks + 1) * N
        gen = torch.Generator(device=dev).manual_seed(2024)
        x8 = torch.randint(0, 256, (n_samples, 2), dtype=torch.uint8, device=dev, generator=gen)
        x16 = (x8.to(torch.int16) - 128) * 16                                      # a 12-bit radio's range
        torch.cuda.synchronize()
        for m, d in SHAPES:
            n_in = n_blocks * block_len(m) + m - 1
            with SpectrumPlan(N) as plan:
                plan.set_fir(ddc_taps(d, m))
                n_out = plan.ddc_outputs(n_in, d)
                out = torch.empty((BANK_C * n_out,), dtype=torch.complex64, device=dev)
                words = words_of(BANK_C)
                for kind, legs in (
                        ("single", {"ci8": lambda: plan.exec_device_ddc_ci8(x8.data_ptr(), n_in, out.data_ptr(), FINE, unsigned=True, decim=d, stream=sp),
                                    "ci16": lambda: plan.exec_device_ddc_ci16(x16.data_ptr(), n_in, out.data_ptr(), FINE, decim=d, stream=sp)}),
                        ("bank", {"ci8": lambda: plan.exec_device_ddc_bank_ci8(x8.data_ptr(), n_in, out.data_ptr(), words, unsigned=True, decim=d, stream=sp),
                                  "ci16": lambda: plan.exec_device_ddc_bank_ci16(x16.data_ptr(), n_in, out.data_ptr(), words, decim=d, stream=sp)})):
                    r = race(legs, timed, stream, ROUNDS, PER_ROUND, WARM_S)
                    a, b = r["ci8"], r["ci16"]
                    points[f"device_{kind}_M{m}_D{d}"] = {
                        "leg": "a", "kind": kind, "taps": m, "decim": d, "channels": BANK_C if kind == "bank" else 1, "n_in": n_in, "legs": r,
                        "ci8_over_ci16": round(a["ms"] / b["ms"], 4), "gsamples_s_in_ci8": round(n_in / a["ms"] / 1e6, 2),
                        "slower_than_ci16_by_more_than_twice_its_spread": bool(a["ms"] > b["ms"] * (1 + 2 * b["spread_of_round_medians"]))}
                del out
    return points


def measure_host(n):
    rng = np.random.default_rng(2024)
    raw = rng.integers(0, 256, size=(n, 2), dtype=np.uint8)                        # pageable, as np.fromfile delivers a recording
    i16 = (raw.astype(np.int16) - 128) * 16
    t = [wall(lambda: iq8_to_c64(raw)) for _ in range(3)]
    wide = iq8_to_c64(raw)
    widen = {"ms": round(statistics.median(t), 2), "ms_min_max": [round(min(t), 2), round(max(t), 2)],
             "gsamples_s": round(n / statistics.median(t) / 1e6, 3)}
    points = {}
    for m, d in SHAPES:
        with SpectrumPlan(N) as plan:
            plan.set_fir(ddc_taps(d, m))
            words = words_of(BANK_C)
            for kind, legs in (
                    ("single", {"ci8": lambda: plan.ddc_ci8(raw, FINE, decim=d), "ci16": lambda: plan.ddc_ci16(i16, FINE, decim=d),
                                "c64": lambda: plan.ddc(wide, FINE, decim=d)}),
                    ("bank", {"ci8": lambda: plan.ddc_bank_ci8(raw, words, decim=d), "ci16": lambda: plan.ddc_bank_ci16(i16, words, decim=d),
                              "c64": lambda: plan.ddc_bank(wide, words, decim=d)})):
                r = race(legs, wall, None, HOST_ROUNDS, HOST_PER_ROUND, 0.0)
                a, b, c = r["ci8"], r["ci16"], r["c64"]
                route = c["ms"] + widen["ms"]
                points[f"host_{kind}_M{m}_D{d}"] = {
                    "leg": "b,c", "kind": kind, "taps": m, "decim": d, "channels": BANK_C if kind == "bank" else 1, "n": n, "legs": r,
                    "bytes_per_sample_model": byte_model(m, d), "ci16_over_ci8": round(b["ms"] / a["ms"], 3),
                    "beats_ci16_by_more_than_its_spread": bool(a["ms"] < b["ms"] * (1 - b["spread_of_round_medians"])),
                    "gsamples_s_ci8": round(n / a["ms"] / 1e6, 3), "gsamples_s_ci16": round(n / b["ms"] / 1e6, 3),
                    "link_gb_s_ci8": round(2 * n / a["ms"] / 1e6, 2), "link_gb_s_ci16": round(4 * n / b["ms"] / 1e6, 2),
                    "link_gb_s_c64": round(8 * n / c["ms"] / 1e6, 2),
                    "route_today_ms": round(route, 2), "route_today_over_ci8": round(route / a["ms"], 2)}
    return {"samples": n, "numpy_widen": widen, "points": points}


def compiler_figures():
    """The ELF-note figures of the new kernels and their int16 counterparts (tests/code_objects.py reads them from the library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"downconv", n) or (re.search(r"ddc", n) and "OlsInI16" in n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def write_summary(res, path):
    dv, h = res["device_legs"], res["host_legs"]
    lines = ["# Down-converter from 8-bit I,Q (sdrk_exec_*_downconv_iq8, sdrk_exec_*_downconvbank_iq8): measured on " + res["device"], "",
             "Written by tools/bench_ddc_ci8.py.  The legs of a point alternate in one process after a warm-up by time; a figure is the "
             "median of a leg's launches, a spread that of its round medians.  Nothing was tuned against these figures.", "",
             f"## (a) Device resident, {res['blocks']} blocks: the 8-bit call against the int16 DDC call "
             f"({ROUNDS * PER_ROUND} launches a leg, device events)", "",
             "| point | M | D | C | ci8 ms | ci16 ms | ci8 / ci16 | ci16 spread | ci8 spread | Gsamples/s in (ci8) | slower by > 2 x ci16 spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, p in dv.items():
        a, b = p["legs"]["ci8"], p["legs"]["ci16"]
        lines.append(f"| {name} | {p['taps']} | {p['decim']} | {p['channels']} | {a['ms']} | {b['ms']} | {p['ci8_over_ci16']} | "
                     f"{b['spread_of_round_medians']} | {a['spread_of_round_medians']} | {p['gsamples_s_in_ci8']} | "
                     f"{'YES' if p['slower_than_ci16_by_more_than_twice_its_spread'] else 'no'} |")
    w = h["numpy_widen"]
    lines += ["", f"## (b), (c) Host entry on 2^{res['host_log2']} pageable samples ({HOST_ROUNDS * HOST_PER_ROUND} calls a leg, wall clock)", "",
              f"numpy widening to complex64 (spectrum.iq8_to_c64, one core): {w['ms']} ms, {w['gsamples_s']} Gsamples/s "
              f"(min / max {w['ms_min_max']}).  `route today` = that + the complex64 host call: what `extract` did with an 8-bit recording.", "",
              "| point | M | D | C | ci8 ms | ci16 ms | c64 ms | ci16 / ci8 (link model 2) | ci16 spread | beats ci16 by > its spread | "
              "link GB/s ci8 / ci16 / c64 | route today ms | route today / ci8 |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, p in h["points"].items():
        a, b, c = p["legs"]["ci8"], p["legs"]["ci16"], p["legs"]["c64"]
        lines.append(f"| {name} | {p['taps']} | {p['decim']} | {p['channels']} | {a['ms']} | {b['ms']} | {c['ms']} | {p['ci16_over_ci8']} | "
                     f"{b['spread_of_round_medians']} | {'yes' if p['beats_ci16_by_more_than_its_spread'] else 'NO'} | "
                     f"{p['link_gb_s_ci8']} / {p['link_gb_s_ci16']} / {p['link_gb_s_c64']} | {p['route_today_ms']} | {p['route_today_over_ci8']} |")
    lines += ["", "## Compiler figures (the new kernels and the int16 DDC kernels they stand beside)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
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
    ap.add_argument("--host-log2", type=int, default=27)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "ddc_ci8"))
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "blocks": 1 << args.blocks_log2, "host_log2": args.host_log2,
           "device_legs": measure_device(1 << args.blocks_log2), "host_legs": measure_host(1 << args.host_log2),
           "compiler": compiler_figures()}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_ddc_ci8.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps({"device_legs": res["device_legs"], "host_legs": res["host_legs"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())

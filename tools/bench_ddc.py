"""The digital down-converter against the FIR call and against what a user composes today, leg by leg (profiles/ddc/SUMMARY.md and
bench_ddc.json beside it are written by this tool; it is the only place a timing of the DDC calls is taken).

    python tools/bench_ddc.py [--blocks-log2 14] [--out-dir profiles/ddc] [--parity-log pytest_output.txt]

Device resident, 2^14 blocks of input.  Every leg is enqueued on one torch stream between two device events (the compositions have
torch kernels in them, so all legs are timed the same way); the legs of a point alternate in one process after a warm-up by time.
A leg's figure is the MEDIAN of its 30 per-launch times; its spread is that of the medians of the 6 rounds.
    tune      ddc with a fine word against fir at the nearest bin, (M, D) = (257, 1), (257, 16), (2049, 64), complex64 and int16
    decim50   ddc at D = 50 against fir at D = 2 followed by a torch strided copy [::25]             } the two compositions a
    phasor    ddc at (257, 1) against fir followed by a torch multiply by the fine phasor             } user has today
    bank      the DDC bank at C = 8 and 32 against C single ddc calls, their times summed
Nothing here is a gate: the figures are written down as measured.
--parity-log: the output of `pytest -s tests/test_ddc_gpu.py`; its err/tol lines go into the summary."""
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
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, ddc_taps  # noqa: E402

N = 4096
FINE = 0x12345678            # bin 291.27: the FIR legs tune to bin 291
ROUNDS, PER_ROUND, WARM_S = 6, 5, 0.4


def block_len(m):
    return (N + 1 - m) // 256 * 256


def bin_of(word):
    return ((word + 0x80000) >> 20) & 4095


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


def race(legs, stream):
    """{leg: {ms, spread, ...}}: the legs alternating after a warm-up by time."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for run in legs.values():
            timed(run, stream)
    ms = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, run in legs.items():
            ms[name].append([timed(run, stream) for _ in range(PER_ROUND)])
    out = {}
    for name, rounds in ms.items():
        flat = [v for r in rounds for v in r]
        med, rmed = statistics.median(flat), [statistics.median(r) for r in rounds]
        out[name] = {"ms": round(med, 4), "ms_min_max": [round(min(flat), 4), round(max(flat), 4)],
                     "spread_of_round_medians": round((max(rmed) - min(rmed)) / med, 4)}
    return out


def compare(legs, new, old):
    a, b = legs[new], legs[old]
    return {"legs": legs, "ratio": round(a["ms"] / b["ms"], 4), "new": new, "old": old,
            "no_slower_than_old_by_more_than_its_spread": bool(a["ms"] <= b["ms"] * (1 + b["spread_of_round_medians"]))}


def measure(n_blocks):
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))    # a stream of the tool's own: the library's calls and torch's kernels
    with torch.cuda.stream(stream):
        return measure_on(stream, n_blocks)


def measure_on(stream, n_blocks):
    lib = _ffi.lib()
    dev = torch.device("cuda:0")
    sp = stream.cuda_stream
    n_frames = n_blocks + 1                                                        # every shape's input fits: L <= 4096
    x = torch.empty((n_frames * N,), dtype=torch.complex64, device=dev)
    x16 = torch.empty((n_frames * N, 2), dtype=torch.int16, device=dev)
    _ffi.check(lib.sdrk_synth_fill(0, 2024, 0, n_frames, N, x.data_ptr(), None))
    _ffi.check(lib.sdrk_synth_fill_ci16(0, 2024, 0, n_frames, N, x16.data_ptr(), None))
    torch.cuda.synchronize()
    res = {"blocks": n_blocks, "launches_per_leg": ROUNDS * PER_ROUND, "points": {}}
    s = bin_of(FINE)

    def shape(m):
        L = block_len(m)
        return L, n_blocks * L + m - 1

    # tune: a fine word against the nearest bin, both formats
    for m, d in ((257, 1), (257, 16), (2049, 64)):
        L, n_in = shape(m)
        with SpectrumPlan(N) as plan:
            plan.set_fir(ddc_taps(d, m))
            out = torch.empty((plan.ddc_outputs(n_in, d),), dtype=torch.complex64, device=dev)
            for fmt, src in (("c64", x), ("i16", x16)):
                ddc = plan.exec_device_ddc if fmt == "c64" else plan.exec_device_ddc_ci16
                fir = plan.exec_device_fir if fmt == "c64" else plan.exec_device_fir_ci16
                legs = race({"ddc": lambda: ddc(src.data_ptr(), n_in, out.data_ptr(), FINE, decim=d, stream=sp),
                             "fir": lambda: fir(src.data_ptr(), n_in, out.data_ptr(), decim=d, shift_bins=s, stream=sp)}, stream)
                p = compare(legs, "ddc", "fir")
                p.update(kind="tune", taps=m, decim=d, format=fmt, n_in=n_in, gsamples_s_in=round(n_in / legs["ddc"]["ms"] / 1e6, 2))
                res["points"][f"tune_M{m}_D{d}_{fmt}"] = p
            del out
    # decim50: one call against fir at D = 2 and a strided copy
    m, d = 801, 50
    L, n_in = shape(m)
    with SpectrumPlan(N) as plan:
        plan.set_fir(ddc_taps(d, m))
        out = torch.empty((plan.ddc_outputs(n_in, d),), dtype=torch.complex64, device=dev)
        half = torch.empty((plan.fir_outputs(n_in, 2),), dtype=torch.complex64, device=dev)
        picked = torch.empty((half[::25].shape[0],), dtype=torch.complex64, device=dev)

        def composed():
            plan.exec_device_fir(x.data_ptr(), n_in, half.data_ptr(), decim=2, shift_bins=s, stream=sp)
            picked.copy_(half[::25])

        legs = race({"ddc": lambda: plan.exec_device_ddc(x.data_ptr(), n_in, out.data_ptr(), FINE, decim=d, stream=sp),
                     "fir_then_copy": composed}, stream)
        p = compare(legs, "ddc", "fir_then_copy")
        p.update(kind="decim50", taps=m, decim=d, format="c64", n_in=n_in)
        res["points"]["decim50_M801"] = p
        del out, half, picked
    # phasor: one call against fir and an elementwise multiply by the fine phasor
    m, d = 257, 1
    L, n_in = shape(m)
    with SpectrumPlan(N) as plan:
        plan.set_fir(ddc_taps(d, m))
        n_out = plan.ddc_outputs(n_in, d)
        out = torch.empty((n_out,), dtype=torch.complex64, device=dev)
        y = torch.empty((n_out,), dtype=torch.complex64, device=dev)
        resid = (FINE - (s << 20)) / 2.0 ** 32
        ang = (torch.arange(n_out, device=dev, dtype=torch.float64) * (-2 * torch.pi * resid)).remainder(2 * torch.pi).to(torch.float32)
        ph = torch.polar(torch.ones(n_out, device=dev), ang)                        # the fine phasor, as a user would precompute it
        del ang

        def composed():
            plan.exec_device_fir(x.data_ptr(), n_in, y.data_ptr(), decim=d, shift_bins=s, stream=sp)
            torch.mul(y, ph, out=out)

        legs = race({"ddc": lambda: plan.exec_device_ddc(x.data_ptr(), n_in, out.data_ptr(), FINE, decim=d, stream=sp),
                     "fir_then_multiply": composed}, stream)
        p = compare(legs, "ddc", "fir_then_multiply")
        p.update(kind="phasor", taps=m, decim=d, format="c64", n_in=n_in)
        res["points"]["phasor_M257"] = p
        del out, y, ph
    # bank: C channels from one pass against C single calls
    m, d = 257, 16
    L, n_in = shape(m)
    with SpectrumPlan(N) as plan:
        plan.set_fir(ddc_taps(d, m))
        n_out = plan.ddc_outputs(n_in, d)
        for c in (8, 32):
            words = words_of(c)
            out = torch.empty((c * n_out,), dtype=torch.complex64, device=dev)

            def singles():
                for k, w in enumerate(words):
                    plan.exec_device_ddc(x.data_ptr(), n_in, out.data_ptr() + 8 * k * n_out, w, decim=d, stream=sp)

            legs = race({"bank": lambda: plan.exec_device_ddc_bank(x.data_ptr(), n_in, out.data_ptr(), words, decim=d, stream=sp),
                         "singles": singles}, stream)
            p = compare(legs, "bank", "singles")
            p.update(kind="bank", taps=m, decim=d, format="c64", n_in=n_in, channels=c, transform_model=round((1 + c) / (2 * c), 4))
            res["points"][f"bank_M{m}_D{d}_C{c}"] = p
            del out
    return res


def compiler_figures():
    """The ELF-note figures of the new kernels (tests/code_objects.py reads them from the built library)."""
    try:
        from tests.code_objects import _notes
        return {n: {f: k.get(f) for f in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size")}
                for n, k in _notes().items() if re.search(r"ddc", n)}
    except Exception as e:  # pragma: no cover - the ROCm LLVM tools are missing
        return {"unavailable": repr(e)}


def parity_lines(path):
    if not path or not os.path.exists(path):
        return []
    keep = ("worst err/tol", "600 blocks", "tone", "turns")
    return [ln.strip().lstrip(".") for ln in open(path) if any(k in ln for k in keep)]


def write_summary(res, path):
    t = res["timing"]
    lines = ["# Digital down-converter (sdrk_exec_*_ddc, sdrk_exec_*_ddcbank): measured on " + res["device"], "",
             f"Written by tools/bench_ddc.py.  Overlap-save in blocks of 4096, device resident, {t['blocks']} blocks; every leg enqueued on "
             f"one stream between two device events, median of {t['launches_per_leg']} launches per leg, the legs of a point alternating "
             "in one process after a warm-up by time.  `new / old` below 1: the DDC call is the faster one.  The condition column: the "
             "new leg is no slower than the old one by more than the old leg's own spread (of its round medians).  Nothing was tuned "
             "against these figures.", "",
             "| point | M | D | format | new | ms | old | ms | new / old | old spread | new spread | no slower |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, p in t["points"].items():
        a, b = p["legs"][p["new"]], p["legs"][p["old"]]
        lines.append(f"| {name} | {p['taps']} | {p['decim']} | {p['format']} | {p['new']} | {a['ms']} | {p['old']} | {b['ms']} | "
                     f"{p['ratio']} | {b['spread_of_round_medians']} | {a['spread_of_round_medians']} | "
                     f"{'yes' if p['no_slower_than_old_by_more_than_its_spread'] else 'NO'} |")
    lines += ["", "## Compiler figures (ddc_kernel: 3 workgroups per CU, 2 from complex64 with the mixer; ddcbank_kernel: 2)", ""]
    for n, f in res["compiler"].items():
        lines.append(f"- `{n}`: {f}")
    if res["parity"]:
        lines += ["", "## tests/test_ddc_gpu.py on this device (the bit identities hold as well)", ""]
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
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "ddc"))
    ap.add_argument("--parity-log", default=None)
    args = ap.parse_args(argv)
    assert pkg.device_count() >= 1, "needs a GPU"
    res = {"device": pkg.device_info(0).split(", pci")[0], "timing": measure(1 << args.blocks_log2),
           "compiler": compiler_figures(), "parity": parity_lines(args.parity_log)}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "bench_ddc.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    write_summary(res, os.path.join(args.out_dir, "SUMMARY.md"))
    print(json.dumps(res["timing"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Developer helper (GPU box): is the level a resident pair runs at local to PARTS of the pair?

One process: the 32 GiB input, then K 16 GiB row buffers one after the other (all kept), a warm-up by time, then for every
row buffer the N = 4096 Hann plan timed over the whole pair and over each of S equal slices (slice k: d_in + k * in/S,
d_out + k * out/S, frames/S frames); every figure the median of `--reps` launches.  One record per process is appended to
the JSON list in --out; run it in several processes and compare (profiles/placement_chunks/SUMMARY.md).

    python tools/placement_slots.py --out profiles/placement_chunks/slots_parent.json
    python tools/placement_slots.py --pair-call --out ...     # only: wall time of sdrk_dev_alloc_stream_pair at the bench's size
With SDRK_PLACEMENT_LOG set, --pair-call also copies the line the call appended there into its record.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402,F401  (first: one HIP runtime in the process, see _ffi.py)
from bench import warm_up_by_time  # noqa: E402
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan, placement_report  # noqa: E402

NFFT = 4096


def append_record(path, rec):
    recs = []
    if os.path.exists(path):
        recs = json.load(open(path))
    recs.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


def pair_call(lib, plan, dev, frames, candidates):
    d_in, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    probe, chosen = (ctypes.c_float * candidates)(), ctypes.c_int(0)
    log = os.environ.get("SDRK_PLACEMENT_LOG")
    before = os.path.getsize(log) if log and os.path.exists(log) else 0
    t0 = time.perf_counter()
    _ffi.check(lib.sdrk_dev_alloc_stream_pair(dev, frames * NFFT * 8, frames * NFFT * 4, candidates, plan.handle,
                                              ctypes.byref(d_in), ctypes.byref(d_out), probe, ctypes.byref(chosen)))
    wall = time.perf_counter() - t0
    rec = {"kind": "pair_call", "frames": frames, "candidates": candidates, "wall_s": round(wall, 3),
           "probe_ms": [round(float(v), 4) for v in probe], "chosen": int(chosen.value), **placement_report()}
    warm_up_by_time(lambda: plan.exec_device_timed(d_in.value, frames, d_out.value, 1))
    rec["whole_ms_after"] = round(statistics.median(plan.exec_device_timed_each(d_in.value, frames, d_out.value, 7)), 4)
    if log and os.path.exists(log):
        with open(log) as f:
            f.seek(before)
            lines = [ln for ln in f.read().splitlines() if ln.strip()]
        if lines:
            rec["log"] = json.loads(lines[-1])
    lib.sdrk_dev_free(dev, d_out)
    lib.sdrk_dev_free(dev, d_in)
    return rec


def slots(lib, plan, dev, frames, outputs, n_slices, reps):
    d_in = ctypes.c_void_p()
    _ffi.check(lib.sdrk_dev_alloc(dev, frames * NFFT * 8, ctypes.byref(d_in)))
    outs = []
    for _ in range(outputs):
        p = ctypes.c_void_p()
        _ffi.check(lib.sdrk_dev_alloc(dev, frames * NFFT * 4, ctypes.byref(p)))
        outs.append(p)
    _ffi.check(lib.sdrk_synth_fill(dev, 1234, 0, frames, NFFT, d_in, None))
    warm_up_by_time(lambda: plan.exec_device_timed(d_in.value, frames, outs[0].value, 1))

    def med(i_off, o_ptr, n):
        plan.exec_device_timed(d_in.value + i_off, n, o_ptr, 1)                      # one untimed
        return statistics.median(plan.exec_device_timed_each(d_in.value + i_off, n, o_ptr, reps))

    per = frames // n_slices
    rec = {"kind": "slots", "frames": frames, "outputs": outputs, "slices": n_slices, "frames_per_slice": per, "reps": reps,
           "d_in": hex(d_in.value), "d_out": [hex(p.value) for p in outs], "whole_ms": [], "whole_again_ms": [], "slice_ms": []}
    for p in outs:
        rec["whole_ms"].append(round(med(0, p.value, frames), 4))
    for p in outs:
        rec["slice_ms"].append([round(med(k * per * NFFT * 8, p.value + k * per * NFFT * 4, per), 4) for k in range(n_slices)])
    for p in outs:                                                                   # the wholes again: did anything drift?
        rec["whole_again_ms"].append(round(med(0, p.value, frames), 4))
    rec["slice_sum_ms"] = [round(sum(r), 4) for r in rec["slice_ms"]]

    # The same slices in SWEEP order: slice 0, 1, ... S-1 one launch each, the sweep repeated `reps` times, per-slice
    # medians.  No slice is launched twice in a row, so nothing a repeated launch over the same 3 GiB could keep warm
    # (translations, caches) is warm here: a sweep is the whole-pair run cut at S launch boundaries.
    def sweep(p, s):
        n = frames // s
        t = [[] for _ in range(s)]
        for _ in range(reps + 1):                                                    # the first sweep is not counted
            for k in range(s):
                t[k].append(plan.exec_device_timed_each(d_in.value + k * n * NFFT * 8, n, p.value + k * n * NFFT * 4, 1)[0])
        return [round(statistics.median(v[1:]), 4) for v in t]

    rec["sweep_ms"] = [sweep(p, n_slices) for p in outs]
    rec["sweep_sum_ms"] = [round(sum(r), 4) for r in rec["sweep_ms"]]
    rec["coarse"] = {}
    for s in (2, 4):                                                                 # at which scale does the whole's level appear?
        n = frames // s
        rec["coarse"][str(s)] = {
            "repeated_ms": [[round(med(k * n * NFFT * 8, p.value + k * n * NFFT * 4, n), 4) for k in range(s)] for p in outs],
            "sweep_ms": [sweep(p, s) for p in outs]}
    rec["whole_last_ms"] = [round(med(0, p.value, frames), 4) for p in outs]

    # The whole pair as K back-to-back launches of frames/K frames each, enqueued without a host wait between them and timed
    # as ONE span (events around all K on a stream of torch's): what a sweep's sum leaves out (the gaps between launches) is in.
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def split(p, k_parts):
        n = frames // k_parts
        t = []
        for _ in range(reps + 1):
            e0.record(stream)
            for k in range(k_parts):
                plan.exec_device(d_in.value + k * n * NFFT * 8, n, p.value + k * n * NFFT * 4, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return round(statistics.median(t[1:]), 4)

    rec["split_parts"] = [1, 2, 4, 8, 16, 32, 64, 256]
    rec["split_ms"] = [[split(p, k) for k in rec["split_parts"]] for p in outs]
    for p in outs:
        lib.sdrk_dev_free(dev, p)
    lib.sdrk_dev_free(dev, d_in)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--outputs", type=int, default=6)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-call", action="store_true")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    lib = _ffi.lib()
    _ffi.require_device(0)
    with SpectrumPlan(NFFT, window="hann", device=0) as plan:
        rec = pair_call(lib, plan, 0, a.frames, a.outputs) if a.pair_call else slots(lib, plan, 0, a.frames, a.outputs, a.slices, a.reps)
    rec["label"] = a.label
    rec["pid"] = os.getpid()
    append_record(a.out, rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

"""Reader of the flagship kernel's per-frame time line (experiments/f4k_order/build.sh; run with SDRK_LIB pointing at
sdr-iq-visualizer_amd/lib_f4ktl/libsdrk.so).

One process: the 32 GiB input, `--pairs` 16 GiB row buffers, and for each order (SDRK_F4K_ORDER = stride, ticket) and each
pair ONE launch over all 2^20 frames and ONE launch over the first 65536 (SDRK_F4K_PARTS=1: no cut by the host).  Each
launch leaves a record per frame: the 100 MHz real-time counter when the frame's loads were issued, the frame, the workgroup.
Printed per 0.5 ms of the launch: the frames issued in it, the span of their indices (max - min), and the furthest any
workgroup that still has frames to come lags behind the front — the highest frame issued so far minus the last frame that
workgroup issued — in frames and in grids.  One JSON line per launch goes to --out.

    SDRK_LIB=sdr-iq-visualizer_amd/lib_f4ktl/libsdrk.so python experiments/f4k_order/timeline.py --out /tmp/f4k_timeline.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import torch  # noqa: E402  (first: one HIP runtime in the process)
import numpy as np  # noqa: E402
from bench import warm_up_by_time  # noqa: E402
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402

NFFT = 4096
TICK_NS = 10.0          # the real-time counter runs at 100 MHz
BIN_MS = 0.5


def analyse(rec, n_frames):
    """rec: uint32 (n_frames, 4) = time lo, time hi, frame, workgroup."""
    t = rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))
    assert (t > 0).all(), "frames without a record"
    assert np.array_equal(rec[:, 2], np.arange(n_frames, dtype=np.uint32)), "a record names another frame than its own"
    wg = rec[:, 3].astype(np.int64)
    grid = int(wg.max()) + 1
    ms = (t - t.min()).astype(np.float64) * TICK_NS * 1e-6
    frame = np.arange(n_frames, dtype=np.int64)
    last_ms = np.zeros(grid)
    np.maximum.at(last_ms, wg, ms)                       # when each workgroup issued its last frame
    order = np.argsort(ms, kind="stable")
    bins = []
    reached = np.full(grid, -1, dtype=np.int64)          # the last frame each workgroup has issued so far (its latest in time)
    n_bins = int(np.ceil((ms.max() + 1e-9) / BIN_MS))
    cut = np.searchsorted(ms[order], np.arange(n_bins + 1) * BIN_MS, side="left")
    cut[-1] = n_frames
    for b in range(n_bins):
        hi = (b + 1) * BIN_MS
        idx = order[cut[b]:cut[b + 1]]
        if idx.size == 0:
            continue
        reached[wg[idx]] = frame[idx]                    # in time order: the later assignment wins
        active = (last_ms >= hi) & (reached >= 0)
        front = int(reached.max())
        lag = int(front - reached[active].min()) if active.any() else 0
        bins.append({"ms": round(b * BIN_MS, 2), "frames": int(idx.size), "span": int(frame[idx].max() - frame[idx].min()),
                     "lag_frames": lag, "lag_grids": round(lag / grid, 2)})
    return {"grid": grid, "launch_ms_by_records": round(float(ms.max()), 3), "bins": bins}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--short", type=int, default=65536)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--orders", default="stride,ticket",
                    help="comma-separated SDRK_F4K_ORDER values, each optionally with :<SDRK_F4K_TICKET_FORM> (ticket:rot4) and, for a "
                         "rot form, @<SDRK_F4K_ROT_AHEAD>: 3, 2top or 2flow (ticket:rot4@3, ticket:rot4@2flow)")
    a = ap.parse_args()
    lib = _ffi.lib()
    _ffi.require_device(0)
    set_tl = lib.sdrk_f4k_timeline           # only the experiment build has it
    set_tl.argtypes, set_tl.restype = [ctypes.c_void_p], ctypes.c_int
    os.environ["SDRK_F4K_PARTS"] = "1"
    d_in = ctypes.c_void_p()
    _ffi.check(lib.sdrk_dev_alloc(0, a.frames * NFFT * 8, ctypes.byref(d_in)))
    outs = []
    for _ in range(a.pairs):
        p = ctypes.c_void_p()
        _ffi.check(lib.sdrk_dev_alloc(0, a.frames * NFFT * 4, ctypes.byref(p)))
        outs.append(p)
    _ffi.check(lib.sdrk_synth_fill(0, 1234, 0, a.frames, NFFT, d_in, None))
    tl = torch.zeros((a.frames, 4), dtype=torch.int32, device="cuda")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for order in [o for o in a.orders.split(",") if o]:
            os.environ["SDRK_F4K_ORDER"] = order.split(":")[0]
            form, _, ahead = order.partition(":")[2].partition("@")
            for var, value in (("SDRK_F4K_TICKET_FORM", form), ("SDRK_F4K_ROT_AHEAD", ahead)):
                if value:
                    os.environ[var] = value
                else:
                    os.environ.pop(var, None)
            with SpectrumPlan(NFFT, window="hann", device=0) as plan:
                warm_up_by_time(lambda: plan.exec_device_timed(d_in.value, a.frames, outs[0].value, 1))
                for i, p in enumerate(outs):
                    for n in (a.frames, a.short):
                        plan.exec_device_timed(d_in.value, n, p.value, 1)          # one untimed, unrecorded
                        tl.zero_()
                        torch.cuda.synchronize()
                        assert set_tl(tl.data_ptr()) == 0
                        ms = plan.exec_device_timed(d_in.value, n, p.value, 1)
                        assert set_tl(None) == 0
                        rec = tl[:n].cpu().numpy().view(np.uint32)
                        r = {"order": order, "pair": i, "frames": n, "launch_ms_by_events": round(float(ms), 4), **analyse(rec, n)}
                        out.write(json.dumps(r) + "\n")
                        out.flush()
                        print(f"== {order} pair {i} frames {n}: {r['launch_ms_by_events']} ms by events, "
                              f"{r['launch_ms_by_records']} ms first to last issue, grid {r['grid']}")
                        for b in r["bins"]:
                            print(f"   {b['ms']:5.2f} ms  frames {b['frames']:7d}  span {b['span']:8d}  lag {b['lag_frames']:8d} "
                                  f"frames = {b['lag_grids']:7.2f} grids", flush=True)
    for p in outs:
        lib.sdrk_dev_free(0, p)
    lib.sdrk_dev_free(0, d_in)


if __name__ == "__main__":
    main()

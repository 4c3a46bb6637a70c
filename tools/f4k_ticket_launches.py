"""Developer helper (GPU box): how many launches does the ticket order of the N = 4096 kernel want for a long call, and how
does it stand against the grid-stride order on the same buffers?  (tools/placement_slots.py's "one span" method.)

One process: the 32 GiB input, `--outputs` 16 GiB row buffers (all kept), a warm-up by time, then for every row buffer the
Hann plan over all 2^20 frames as K = 1, 2, 4, 8, 16 back-to-back launches of frames/K frames, enqueued without a host wait
between them and timed as ONE span (events around all K) — for a plan of each order, the two orders alternating per buffer.
SDRK_F4K_PARTS=1 keeps the host from cutting a call itself, so K is the number of launches in both orders; the grid-stride
order is also timed as the product issues it ("product": one call, cut by f4k_split_parts).  Every figure is the median of
`--reps` spans.  One record per process is appended to the JSON list in --out (profiles/f4k_ticket/SUMMARY.md).

    python tools/f4k_ticket_launches.py --out profiles/f4k_ticket/launches.json

A form is SDRK_F4K_TICKET_FORM's name, and a rot form may name its look-ahead behind an "@": rot4@3, rot4@2top, rot4@2flow
(SDRK_F4K_ROT_AHEAD; csrc/f4k_rot.h).

--paired FORM,FORM,... (profiles/f4k_window/SUMMARY.md, profiles/f4k_ahead/SUMMARY.md) measures forms of the ticket order
against a control, `--control` (rot4 at look-ahead three, rot4@3), instead: two plans in the process per comparison, the control
and the other form (named at creation), on the same pair; whole calls of 2^20 frames alternate between the two, each timed by
events of its own, and each side is the median of `--reps` (after one uncounted launch each).  The first comparison on every
pair is the control against a second control plan: its largest difference over the pairs and processes is what alternation
alone produces.  (profiles/f4k_window/ was measured with 1x2 as the control: --control 1x2.)

    python tools/f4k_ticket_launches.py --paired rot4@2top --out profiles/f4k_ahead/paired.json
    python tools/f4k_ticket_launches.py --control rot4@2top --paired rot4@2flow --out profiles/f4k_flow/paired.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402  (first: one HIP runtime in the process, see _ffi.py)
from bench import warm_up_by_time  # noqa: E402
from sdr_iq_visualizer_amd import _ffi  # noqa: E402
from sdr_iq_visualizer_amd.spectrum import SpectrumPlan  # noqa: E402
from tools.placement_slots import append_record  # noqa: E402

NFFT = 4096
PARTS = [1, 2, 4, 8, 16]


def name_form(form):
    """SDRK_F4K_TICKET_FORM and SDRK_F4K_ROT_AHEAD from "<form>[@<ahead>]"; None: the defaults."""
    name, _, ahead = (form or "").partition("@")
    for var, value in (("SDRK_F4K_TICKET_FORM", name), ("SDRK_F4K_ROT_AHEAD", ahead)):
        if value:
            os.environ[var] = value
        else:
            os.environ.pop(var, None)


def plan_of(order, parts, form=None):
    os.environ["SDRK_F4K_ORDER"] = order
    name_form(form)
    if parts:
        os.environ["SDRK_F4K_PARTS"] = str(parts)
    else:
        os.environ.pop("SDRK_F4K_PARTS", None)
    return SpectrumPlan(NFFT, window="hann", device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--outputs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--probe", default="", help="comma-separated forms to time the no-arithmetic 2:1 probe under, beside stride and 1x2")
    ap.add_argument("--paired", default="", help="comma-separated forms to time against the control, launches alternating")
    ap.add_argument("--control", default="rot4@3", help="the other side of --paired")
    a = ap.parse_args()
    lib = _ffi.lib()
    _ffi.require_device(0)
    frames = a.frames
    d_in = ctypes.c_void_p()
    _ffi.check(lib.sdrk_dev_alloc(0, frames * NFFT * 8, ctypes.byref(d_in)))
    outs = []
    for _ in range(a.outputs):
        p = ctypes.c_void_p()
        _ffi.check(lib.sdrk_dev_alloc(0, frames * NFFT * 4, ctypes.byref(p)))
        outs.append(p)
    _ffi.check(lib.sdrk_synth_fill(0, 1234, 0, frames, NFFT, d_in, None))
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def span(plan, p, k_parts):
        n = frames // k_parts
        t = []
        for _ in range(a.reps + 1):                                                  # the first span is not counted
            e0.record(stream)
            for k in range(k_parts):
                plan.exec_device(d_in.value + k * n * NFFT * 8, n, p.value + k * n * NFFT * 4, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        return round(statistics.median(t[1:]), 4)

    def alternate(plan_a, plan_b, p):
        ta, tb = [], []
        for _ in range(a.reps + 1):                                                  # the first of each is not counted
            for plan, t in ((plan_a, ta), (plan_b, tb)):
                e0.record(stream)
                plan.exec_device(d_in.value, frames, p.value, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
        return round(statistics.median(ta[1:]), 4), round(statistics.median(tb[1:]), 4)

    if a.probe:
        # the no-arithmetic 2:1 probe (sdrk_stream_ceiling_probe) on every pair, grid-stride and in each form: median of `reps`
        forms = ["stride", "1x2"] + [f for f in a.probe.split(",") if f]
        rec = {"kind": "f4k_probe_forms", "frames": frames, "outputs": a.outputs, "reps": a.reps, "forms": forms,
               "d_in": hex(d_in.value), "d_out": [hex(p.value) for p in outs], "label": a.label, "pid": os.getpid(), "pairs": []}
        ms = (ctypes.c_float * a.reps)()
        os.environ["SDRK_F4K_ORDER"] = "stride"
        warm_up_by_time(lambda: _ffi.check(lib.sdrk_stream_ceiling_probe(0, d_in, outs[0], frames, 1, ms)))
        for p in outs:
            row = {}
            for form in forms:
                os.environ["SDRK_F4K_ORDER"] = "stride" if form == "stride" else "ticket"
                name_form("1x2" if form == "stride" else form)
                _ffi.check(lib.sdrk_stream_ceiling_probe(0, d_in, p, frames, a.reps, ms))
                row[form] = round(statistics.median(ms), 4)
            rec["pairs"].append(row)
        for p in outs:
            lib.sdrk_dev_free(0, p)
        lib.sdrk_dev_free(0, d_in)
        append_record(a.out, rec)
        print(json.dumps(rec), flush=True)
        return

    if a.paired:
        forms = [a.control] + [f for f in a.paired.split(",") if f]
        rec = {"kind": "f4k_ticket_paired", "frames": frames, "outputs": a.outputs, "reps": a.reps, "control": a.control, "forms": forms,
               "d_in": hex(d_in.value), "d_out": [hex(p.value) for p in outs], "label": a.label, "pid": os.getpid(), "pairs": []}
        with plan_of("ticket", 1, a.control) as base:
            warm_up_by_time(lambda: base.exec_device_timed(d_in.value, frames, outs[0].value, 1))
            for p in outs:
                row = {}
                for form in forms:
                    with plan_of("ticket", 1, form) as other:
                        base_ms, form_ms = alternate(base, other, p)
                    row[form] = {"base_ms": base_ms, "form_ms": form_ms, "gain_ms": round(base_ms - form_ms, 4)}
                rec["pairs"].append(row)
        for p in outs:
            lib.sdrk_dev_free(0, p)
        lib.sdrk_dev_free(0, d_in)
        append_record(a.out, rec)
        print(json.dumps(rec), flush=True)
        return

    rec = {"kind": "f4k_ticket_launches", "frames": frames, "outputs": a.outputs, "reps": a.reps, "parts": PARTS,
           "d_in": hex(d_in.value), "d_out": [hex(p.value) for p in outs], "label": a.label, "pid": os.getpid()}
    with plan_of("stride", 0) as product, plan_of("stride", 1) as stride, plan_of("ticket", 1) as ticket:
        warm_up_by_time(lambda: product.exec_device_timed(d_in.value, frames, outs[0].value, 1))
        rec["stride_product_ms"], rec["stride_ms"], rec["ticket_ms"], rec["stride_product_again_ms"] = [], [], [], []
        for p in outs:
            rec["stride_product_ms"].append(span(product, p, 1))
            s_row, t_row = [], []
            for k in PARTS:                                                          # the orders alternate
                t_row.append(span(ticket, p, k))
                s_row.append(span(stride, p, k))
            rec["stride_ms"].append(s_row)
            rec["ticket_ms"].append(t_row)
            rec["stride_product_again_ms"].append(span(product, p, 1))
    for p in outs:
        lib.sdrk_dev_free(0, p)
    lib.sdrk_dev_free(0, d_in)
    append_record(a.out, rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

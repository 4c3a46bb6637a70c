#!/usr/bin/env python3
"""Device-resident throughput of every supported frame length (developer sweep).

    python tools/size_sweep.py [N ...] [--precision double]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.extra_bench import device_run
ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int)
ap.add_argument("--precision", choices=("single", "double"), default="single")
args = ap.parse_args()
double = args.precision == "double"
# double: powers of two only (no chirp-z in double), 2^26 samples per run (1 GiB of complex128 in)
sizes = args.sizes or ([1 << k for k in range(1, 23)] if double else [1 << k for k in range(4, 23)] + [1000, 5000, 100000])
for n in sizes:
    frames = max(1, ((1 << 26) if double else (1 << 27)) // n)
    r = device_run(n, frames, n, None, 5, "sweep", precision=args.precision)
    print(json.dumps({k: r[k] for k in ("nfft", "frames", "ms", "frame_Msamples_per_s", "algorithmic_GBps", "hbm_peak_frac")}),
          flush=True)

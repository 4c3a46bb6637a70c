#!/usr/bin/env python3
"""Generate the randomised reference records the CPU suite checks the oracle and the streamer shim against:

  tests/golden/ref_process_frame_random.json  60 random frames through the REFERENCE's reader loop
                                              (app/sdr/streamer.py:95-133, driven as oracle/make_golden.py drives it):
                                              dtype, shape and SHA-256 of power_db and freqs, the keys of the dict
  tests/golden/ref_streamer_random_scripts.json
                                              300 random failure scripts through the REFERENCE's `_stream_data`
                                              (driven as oracle/make_golden_streamer.py drives it): the event traces
  tests/golden/ref_classifier_random_rows.npz 400 random rows through the REFERENCE's classifier helpers
                                              (app/processing/classifier.py:163-219): the nine scalars and the peaks

TEST INFRASTRUCTURE.  Runs only where the reference is present (SDRK_REFERENCE, as in oracle/make_golden.py); the
committed records — inputs by seeded recipe (the functions below, which the tests call too), the reference's outputs:
data only — are what travels.

    python oracle/make_golden_random.py
"""
from __future__ import annotations

import hashlib
import json
import logging
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
FRAMES_OUT = os.path.join(GOLDEN, "ref_process_frame_random.json")
SCRIPTS_OUT = os.path.join(GOLDEN, "ref_streamer_random_scripts.json")
ROWS_OUT = os.path.join(GOLDEN, "ref_classifier_random_rows.npz")

FRAMES_FS_FC = (2_400_000, 915_000_000)
ROW_FS_FC = (20e6, 2.4e9)


def array_digest(a) -> str:
    """dtype, shape and SHA-256 of the bytes, NaNs made one bit pattern first (equality as np.array_equal(equal_nan=True))."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), np.array(np.nan, dtype=a.dtype), a)
    return f"{a.dtype.str}{a.shape}:{hashlib.sha256(a.tobytes()).hexdigest()}"


def random_frames():
    """Lengths 2 ... 70000, odd and even, complex64 and complex128, amplitudes 1e-9 ... 1e6, with NaNs and exact zeros."""
    rng = np.random.default_rng(95)
    frames = []
    for c in range(60):
        n = int(rng.choice([2, 3, 16, 100, 1000, 4096, 4097, 5000, 65536, 70000]))
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 10.0 ** rng.uniform(-9, 6)
        if c % 7 == 3:
            x[rng.integers(0, n)] = np.nan
        if c % 7 == 5:
            x[:] = 0
        frames.append(x.astype(np.complex64 if c % 2 == 0 else np.complex128))
    return frames


def random_scripts():
    """Good frames, generic exceptions, OSErrors of every errno class the loop distinguishes (9, 10054, 110, 113, others,
    none), frames the transform rejects, reconnects that succeed on the k-th try or never, starting connected or not."""
    rng = np.random.default_rng(83)
    steps = ["ok", {"raise": "Exception"}, {"raise": "ValueError"}, {"raise": "RuntimeError"}, {"raise": "OSError"},
             {"raise": "OSError", "errno": 9}, {"raise": "OSError", "errno": 10054}, {"raise": "OSError", "errno": 110},
             {"raise": "OSError", "errno": 113}, {"raise": "OSError", "errno": 5}, {"return": "garbage"}]
    weights = np.array([6, 2, 1, 1, 1, 1, 1, 2, 1, 1, 1], dtype=float)
    scripts = []
    for c in range(300):
        scripts.append({"name": f"random_{c}",
                        "rx": [steps[i] for i in rng.choice(len(steps), size=int(rng.integers(1, 14)), p=weights / weights.sum())],
                        "reconnect": [bool(b) for b in rng.random(int(rng.integers(0, 6))) < 0.4],
                        "start_connected": bool(rng.random() < 0.85)})
    return scripts


def random_rows():
    """Rows of the kinds tools/stress_features.py and stress_fused.py use (noise, ties, tones, cliffs, far-off
    percentiles, -inf bins, constant tails, ramps, values past 385 dB, NaNs; lengths 16 ... 20000): (kind, row) pairs."""
    rng = np.random.default_rng(400)
    kinds = ["noise", "quantised", "tone", "steps", "wide", "holes", "const_tail", "ramp", "huge", "nans"]
    rows = []
    for c in range(400):
        n = int(rng.choice([16, 64, 100, 257, 1000, 2048, 4096, 4097, 8192, 20000]))
        kind = kinds[c % len(kinds)]
        x = (rng.standard_normal(n) * rng.uniform(1, 9) + rng.uniform(-120, 60)).astype(np.float32)
        if kind == "quantised":
            x = (np.round(x * 2) / 2).astype(np.float32)
        elif kind == "tone":
            x[rng.integers(0, n, 3)] += np.float32(90)
        elif kind == "steps":
            x[: max(1, n // 5 + int(rng.integers(-3, 4)))] -= np.float32(150)
        elif kind == "wide":
            x[rng.random(n) < 0.8] += np.float32(70)
        elif kind == "holes":
            x[rng.random(n) < 0.05] = -np.inf
        elif kind == "const_tail":
            x[n // 2:] = x[0]
        elif kind == "ramp":
            x = np.linspace(-80, 5, n).astype(np.float32) + (rng.standard_normal(n) * 0.01).astype(np.float32)
        elif kind == "huge":
            x[rng.random(n) < 0.3] += np.float32(rng.uniform(400, 3000))
        elif kind == "nans":
            x[rng.integers(0, n, int(rng.integers(1, 4)))] = np.nan
        rows.append((kind, x))
    return rows


def record_frames():
    from oracle import make_golden
    S = make_golden.load_reference_streamer()
    frames = random_frames()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = make_golden.run_reference(S, frames, *FRAMES_FS_FC)
    return {"source": "app/sdr/streamer.py:95-133 driven by oracle/make_golden_random.py on random_frames()",
            "fs_fc": list(FRAMES_FS_FC),
            "frames": [{"keys": sorted(d), "samples_is_input": d["samples"] is x, "power_db": array_digest(d["power_db"]),
                        "freqs": array_digest(d["freqs"])} for x, d in zip(frames, ref)]}


def record_scripts():
    from unittest.mock import MagicMock
    from oracle import make_golden_streamer as G
    from oracle.make_golden import REF
    sys.modules.setdefault("adi", MagicMock())
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import app.sdr.streamer as module
    logging.disable(logging.CRITICAL)
    try:
        traces = [G.run_scenario(module, module.SDRDataStreamer, sc) for sc in random_scripts()]
    finally:
        logging.disable(logging.NOTSET)
    return {"source": "app/sdr/streamer.py:83-174 driven by oracle/make_golden_streamer.py on random_scripts()",
            "traces": traces}


def record_rows():
    from oracle import cpu_ref
    from oracle.make_golden import REF
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from app.processing import classifier as C
    scalars, peaks = [], []
    for _, x in random_rows():
        freqs = cpu_ref.freq_axis(x.shape[0], *ROW_FS_FC)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            nf = C._estimate_noise_floor(x)
            snr = float(np.max(x) - nf)
            thr = max(nf + 5.0, np.max(x) - 0.9 * snr + 5.0)
            pk = C._find_peaks(x, threshold_db=thr, min_distance_bins=max(3, len(x) // 300))
            scalars.append([nf, snr, C._occupied_bandwidth(freqs, x, 3), C._occupied_bandwidth(freqs, x, 10),
                            C._occupied_bandwidth(freqs, x, 20), C._spectral_flatness(x), C._spectral_kurtosis(x), float(thr),
                            C._peak_spacing_std(freqs, pk)])
        peaks.append(np.array(pk, dtype=np.int64))
    return {"scalars": np.array(scalars, dtype=np.float64), "peaks_concat": np.concatenate(peaks),
            "peaks_off": np.cumsum([0] + [p.size for p in peaks]).astype(np.int64)}


def main():
    for path, rec in ((FRAMES_OUT, record_frames()), (SCRIPTS_OUT, record_scripts())):
        with open(path, "w") as f:
            json.dump(rec, f, separators=(",", ":"))
        print("wrote", path, os.path.getsize(path), "bytes")
    np.savez_compressed(ROWS_OUT, **record_rows())
    print("wrote", ROWS_OUT, os.path.getsize(ROWS_OUT), "bytes")


if __name__ == "__main__":
    main()

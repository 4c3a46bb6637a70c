"""Offline PSD of a SigMF recording on the GPU (BASELINE.json config 1).

    python -m sdr_iq_visualizer_amd.cli psd recording.sigmf-meta [--nfft 4096] [--welch 1024] [--integrate K [--sk] [--cross] [--correlate]] [--pfb T] [--out rows.npz]
    python -m sdr_iq_visualizer_amd.cli extract recording.sigmf-meta --offset-hz F [F ...] --decim D [--exact] [--taps M] --out BASE
    python -m sdr_iq_visualizer_amd.cli extract multichannel.sigmf-meta --weights W.npy --offset-hz F --decim D [--exact] --out BASE
    python -m sdr_iq_visualizer_amd.cli synth out_base --frames 8 --nfft 4096      # write a test recording

``psd`` reproduces, for the first ``--nfft`` samples, the reference's live expression
(app/sdr/streamer.py:119-121) and, with ``--welch N``, the averaged Hann PSD its offline script
plots (scripts/process_sigmf_data.py:188-189).  ``extract`` tunes to ``center_freq + F`` (rounded to a bin of
``sample_rate/4096``), low-passes, decimates by D and writes the channel as a cf32_le SigMF recording at ``sample_rate/D``;
several offsets are extracted in one pass over the recording and written as ``BASE_0``, ``BASE_1``, ...  With ``--exact`` the
digital down-converter does it: F is tuned to the nearest 32-bit frequency word (``sample_rate/2^32``) and D is any integer in 1..256.
A ``ci16_le``, ``ci8`` or ``cu8`` recording is pushed as it is stored (4 and 2 bytes per sample), with or without ``--exact``.
All transforms run through libsdrk.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np


def _positive(text: str) -> int:
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {v}")
    return v


EXTRACT_PIECE = 1 << 22            # samples per ChannelStream.push of `extract`


def _extract(args, sigmf_io, spectrum) -> int:
    """One channel of a single-channel recording -> a cf32_le recording at sample_rate / decim.  ci16_le, ci8 and cu8 samples are
    pushed as the recording holds them (4 and 2 bytes per sample), everything else as complex64."""
    if args.weights is not None:
        return _extract_beam(args, sigmf_io, spectrum)
    samples, meta = sigmf_io.read_sigmf(args.path, native="all")
    g = meta.get("global", {})
    if int(g.get("core:num_channels", 1)) != 1:
        print(f"extract takes a single-channel recording; this one has core:num_channels = {g.get('core:num_channels')}",
              file=sys.stderr)
        return 2
    fs, fc = float(meta["sample_rate"]), float(meta["center_freq"])
    if len(args.offset_hz) > 1:
        return _extract_bank(args, sigmf_io, spectrum, samples, fs, fc)
    try:
        if args.exact:
            taps = spectrum.ddc_taps(args.decim, args.taps)
            ch = spectrum.DdcStream(None, taps, args.decim, args.offset_hz[0], fs, device=args.device)
        else:
            taps = spectrum.channel_taps(args.decim, args.taps)
            ch = spectrum.ChannelStream(None, taps, args.decim, args.offset_hz[0], fs, device=args.device)
    except ValueError as err:
        print(f"extract: {err}", file=sys.stderr)
        return 2
    with ch:
        n = int(samples.shape[0])
        out = [ch.push(samples[at:at + EXTRACT_PIECE]) for at in range(0, n, EXTRACT_PIECE)]
    y = np.concatenate(out) if out else np.empty(0, np.complex64)
    paths = sigmf_io.write_sigmf(args.out, y, fs / args.decim, fc + ch.tuned_hz,
                                 description=f"channel at {ch.tuned_hz:+.1f} Hz of {fc:.1f} Hz, decimated by {args.decim}")
    tuning = {"freq_word": ch.freq_word} if args.exact else {"shift_bins": ch.shift_bins}
    print(json.dumps({"wrote": list(paths), "samples_in": n, "samples_out": int(y.shape[0]), "sample_rate": fs / args.decim,
                      "center_freq": fc + ch.tuned_hz, "tuned_offset_hz": ch.tuned_hz, **tuning,
                      "decim": args.decim, "taps": int(taps.shape[0])}))
    return 0


def _extract_beam(args, sigmf_io, spectrum) -> int:
    """--weights W.npy: the channels of a 2..8-channel recording combined by a filter-and-sum beamformer into ONE cf32_le
    recording at sample_rate / decim.  W holds (C,) weights (y = w^H x, then the default ddc_taps(decim) low-pass) or (C, M)
    per-channel taps; the elements are pushed as the recording holds them (8, 4 or 2 bytes per sample)."""
    if len(args.offset_hz) != 1:
        print("extract --weights takes one --offset-hz", file=sys.stderr)
        return 2
    try:
        samples, meta = sigmf_io.read_sigmf_channels(args.path)
        nch = int(meta["num_channels"])
        if not 2 <= nch <= spectrum.BEAM_MAX_CHANNELS:
            raise ValueError(f"--weights needs a recording of 2..{spectrum.BEAM_MAX_CHANNELS} channels in cf32_le, ci16_le, ci8 or "
                             f"cu8; this one has core:num_channels = {nch}")
        w = np.load(args.weights)
        if w.ndim not in (1, 2) or w.shape[0] != nch:
            raise ValueError(f"{args.weights} must hold ({nch},) weights or ({nch}, M) taps, got shape {w.shape}")
        filters = spectrum.beam_taps(w, spectrum.ddc_taps(args.decim, args.taps)) if w.ndim == 1 else w
        fs, fc = float(meta["sample_rate"]), float(meta["center_freq"])
        offset = args.offset_hz[0]
        if not args.exact:                                   # a whole bin of sample_rate / 4096, as without --exact elsewhere
            offset = round(offset / (fs / spectrum.FIR_BLOCK)) * (fs / spectrum.FIR_BLOCK)
        ch = spectrum.BeamStream(None, filters, args.decim, offset, fs, device=args.device)
    except ValueError as err:
        print(f"extract: {err}", file=sys.stderr)
        return 2
    with ch:
        n = int(samples.shape[0])
        out = [ch.push(samples[at:at + EXTRACT_PIECE]) for at in range(0, n, EXTRACT_PIECE)]
    y = np.concatenate(out) if out else np.empty(0, np.complex64)
    paths = sigmf_io.write_sigmf(args.out, y, fs / args.decim, fc + ch.tuned_hz,
                                 description=f"beam of {nch} channels at {ch.tuned_hz:+.1f} Hz of {fc:.1f} Hz, decimated by {args.decim}")
    print(json.dumps({"wrote": list(paths), "samples_in": n, "samples_out": int(y.shape[0]), "sample_rate": fs / args.decim,
                      "center_freq": fc + ch.tuned_hz, "tuned_offset_hz": ch.tuned_hz, "freq_word": ch.freq_word, "channels": nch,
                      "decim": args.decim, "taps": int(filters.shape[1])}))
    return 0


def _extract_bank(args, sigmf_io, spectrum, samples, fs: float, fc: float) -> int:
    """Several offsets: one ChannelBankStream, one pass over the recording, channel c -> the recording BASE_c."""
    try:
        if args.exact:
            taps = spectrum.ddc_taps(args.decim, args.taps)
            bank = spectrum.DdcBankStream(None, taps, args.decim, args.offset_hz, fs, device=args.device)
        else:
            taps = spectrum.channel_taps(args.decim, args.taps)
            bank = spectrum.ChannelBankStream(None, taps, args.decim, args.offset_hz, fs, device=args.device)
    except ValueError as err:
        print(f"extract: {err}", file=sys.stderr)
        return 2
    with bank:
        n = int(samples.shape[0])
        out = [bank.push(samples[at:at + EXTRACT_PIECE]) for at in range(0, n, EXTRACT_PIECE)]
    key, tunings = ("freq_word", bank.freq_words) if args.exact else ("shift_bins", bank.shift_bins)
    y = np.concatenate(out, axis=1) if out else np.empty((len(tunings), 0), np.complex64)
    channels = []
    for c, (tuned, bins) in enumerate(zip(bank.tuned_hz, tunings)):
        paths = sigmf_io.write_sigmf(f"{args.out}_{c}", np.ascontiguousarray(y[c]), fs / args.decim, fc + tuned,
                                     description=f"channel at {tuned:+.1f} Hz of {fc:.1f} Hz, decimated by {args.decim}")
        channels.append({"wrote": list(paths), "center_freq": fc + tuned, "tuned_offset_hz": tuned, key: bins})
    print(json.dumps({"channels": channels, "samples_in": n, "samples_out": int(y.shape[1]), "sample_rate": fs / args.decim,
                      "decim": args.decim, "taps": int(taps.shape[0])}))
    return 0


REAL_DATATYPES = ("rf32_le", "ri16_le", "ri8", "ru8")


def _psd_real(args, sigmf_io, spectrum) -> int:
    """psd on a real-sampled recording: one-sided dB rows of --nfft real samples each (even; default 8192) with their axis."""
    for flag, on in (("--sk", args.sk), ("--cross", args.cross), ("--correlate", args.correlate), ("--pfb", args.pfb),
                     ("--integrate", args.integrate)):
        if on:
            print(f"{flag} is not provided on a real-sampled recording: psd writes its one-sided rows (rows_db), which the "
                  f"caller can reduce", file=sys.stderr)
            return 2
    nfft = 8192 if args.nfft is None else int(args.nfft)
    if nfft < 32 or nfft & (nfft - 1):
        print(f"--nfft {nfft}: on a real-sampled recording it is the real frame length, a power of two 32 ... 2^21",
              file=sys.stderr)
        return 2
    samples, meta = sigmf_io.read_sigmf_real(args.path)
    n_samples = int(samples.shape[0])
    if n_samples < nfft:
        print(f"recording has {n_samples} samples, need {nfft}", file=sys.stderr)
        return 2
    fs, fc = meta["sample_rate"], meta["center_freq"]
    frames = n_samples // nfft
    rows = spectrum.rspectrum_db(np.ascontiguousarray(samples[: frames * nfft]).reshape(frames, nfft), nfft, args.window,
                                 device=args.device)
    freqs = spectrum.rfreq_axis(nfft, fs, fc)
    k = int(np.argmax(rows[0]))
    report = {"samples": n_samples, "sample_rate": fs, "center_freq": fc, "nfft": nfft, "real": True,
              "datatype": meta.get("global", {}).get("core:datatype"), "rows": frames, "bins": int(rows.shape[1]),
              "peak_db": float(rows[0, k]), "peak_freq_hz": float(freqs[k]), "median_db": float(np.median(rows[0]))}
    if args.out:
        np.savez_compressed(args.out, power_db=rows[0], rows_db=rows, freqs=freqs)
        report["out"] = args.out
    print(json.dumps(report))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="sdr_iq_visualizer_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("psd")
    p.add_argument("path")
    p.add_argument("--nfft", type=int, default=None,
                   help="frame length (default 4096); on a real-sampled recording (rf32_le, ri16_le, ri8, ru8) the real frame "
                        "length, even (default 8192): psd then writes one-sided rows of nfft/2 + 1 bins")
    p.add_argument("--welch", type=int, default=0, help="also compute the averaged PSD with this NFFT (Hann)")
    p.add_argument("--integrate", type=_positive, default=0, metavar="K",
                   help="also write one dB row per K frames of --nfft samples (integrated_db)")
    p.add_argument("--detector", choices=["mean", "max", "min"], default="mean", help="what --integrate keeps per bin")
    p.add_argument("--sk", action="store_true",
                   help="with --integrate K (K >= 2): also write the spectral kurtosis per bin and group (array sk) and the mean "
                        "power it was formed beside (sk_mean_db), behind the filter bank with --pfb T; the report counts the "
                        "bins outside the 3-sigma band of Gaussian noise")
    p.add_argument("--cross", action="store_true",
                   help="with --integrate K, on a two-channel cf32_le or ci16_le recording (core:num_channels = 2): also write "
                        "the auto and cross power of the two channels per K frames (arrays cross_paa, cross_pbb, cross, coherence, "
                        "phase); the report has the peak-coherence bin, its phase and the median coherence.  The other rows are "
                        "then channel 0's")
    p.add_argument("--correlate", action="store_true",
                   help="with --integrate K, on a recording of 2..8 channels (core:num_channels; cf32_le, ci16_le, ci8 or cu8): "
                        "also write the correlation matrix of the channels per K frames (array corr_planes: channels^2 planes per "
                        "row, spectrum.plane_index); the report has per pair the peak-coherence bin, its phase and the median "
                        "coherence.  The other rows are then channel 0's")
    p.add_argument("--pfb", type=_positive, default=0, metavar="T",
                   help="also write polyphase-filter-bank dB rows: T blocks of --nfft samples folded under the default "
                        "prototype (spectrum.pfb_prototype), one row per --nfft samples (pfb_db); with --integrate K also one "
                        "row per K folded frames (pfb_integrated_db)")
    p.add_argument("--window", default=None)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default=None, help="write results to this .npz")
    e = sub.add_parser("extract")
    e.add_argument("path")
    e.add_argument("--offset-hz", type=float, nargs="+", required=True,
                   help="the channel's centre, relative to the recording's centre; several: one pass, recordings OUT_0, OUT_1, ...")
    e.add_argument("--decim", type=_positive, required=True,
                   help="decimation: a power of two in 1..256 (with --exact: any integer in 1..256)")
    e.add_argument("--exact", action="store_true",
                   help="digital down-converter: tune each offset to the nearest 32-bit frequency word (sample_rate/2^32) instead "
                        "of a bin of sample_rate/4096, and allow any integer --decim; the report has freq_word for shift_bins")
    e.add_argument("--taps", type=_positive, default=None, help="filter length (default min(16*decim + 1, 2049))")
    e.add_argument("--weights", default=None, metavar="W.npy",
                   help="on a recording of 2..8 channels (core:num_channels; cf32_le, ci16_le, ci8 or cu8): combine the channels by "
                        "a filter-and-sum beamformer into one recording.  W.npy holds (C,) complex weights (y = w^H x, then the "
                        "default low-pass) or (C, M) per-channel taps; one --offset-hz, any integer --decim in 1..256")
    e.add_argument("--out", required=True, help="base name of the cf32_le SigMF recording to write")
    e.add_argument("--device", type=int, default=0)
    s = sub.add_parser("synth")
    s.add_argument("base")
    s.add_argument("--frames", type=int, default=8)
    s.add_argument("--nfft", type=int, default=4096)
    s.add_argument("--sample-rate", type=float, default=1_000_000)
    s.add_argument("--center-freq", type=float, default=2_400_000_000)
    s.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args(argv)
    if args.cmd == "psd" and args.sk and args.integrate < 2:
        ap.error("--sk needs --integrate K with K >= 2")
    if args.cmd == "psd" and args.cross and args.integrate < 1:
        ap.error("--cross needs --integrate K")
    if args.cmd == "psd" and args.correlate and args.integrate < 1:
        ap.error("--correlate needs --integrate K")

    from . import sigmf_io, synth
    if args.cmd == "synth":
        x = synth.synth_iq(args.seed, 0, args.frames, args.nfft).reshape(-1)
        paths = sigmf_io.write_sigmf(args.base, x, args.sample_rate, args.center_freq,
                                     description="synthetic 12-bit IQ (sdr_iq_visualizer_amd.synth)")
        print(json.dumps({"wrote": paths, "samples": int(x.size)}))
        return 0

    from . import spectrum
    if args.cmd == "extract":
        return _extract(args, sigmf_io, spectrum)
    if not args.path.endswith(".zip") and sigmf_io.sigmf_datatype(args.path) in REAL_DATATYPES:
        return _psd_real(args, sigmf_io, spectrum)
    if args.nfft is None:
        args.nfft = 4096
    # one read; an int16 recording stays int16 (the spectrum row and the --integrate / --pfb rows are computed from the int16 samples
    # themselves: the same bits from half the bytes) and is widened only if the Welch leg, which stays on complex64, is asked for.
    # A ci8 / cu8 recording stays 8-bit for the spectrum row and the --integrate, --pfb and --sk rows (2 bytes per sample over the
    # link and into the kernels); only the Welch leg widens it on the host, for itself.
    samples, meta = sigmf_io.read_sigmf(args.path, native="all")
    pair = None
    if args.cross:   # both channels as they are stored (element n: sample n of channel 0, then of channel 1); the rest: channel 0
        g = meta.get("global", {})
        if int(g.get("core:num_channels", 1)) != 2 or g.get("core:datatype", "cf32_le") not in ("cf32_le", "ci16_le") \
                or args.path.endswith(".zip"):
            print(f"--cross needs a two-channel cf32_le or ci16_le recording (core:num_channels = 2, not zipped); this one has "
                  f"core:num_channels = {g.get('core:num_channels', 1)}, core:datatype = {g.get('core:datatype', 'cf32_le')!r}",
                  file=sys.stderr)
            return 2
        pair, _ = sigmf_io.read_sigmf_channels(args.path)
        samples = np.ascontiguousarray(pair[:, 0])
    multi = None
    if args.correlate:   # every channel as stored (element n: sample n of channel 0, 1, ...); the rest: channel 0
        g = meta.get("global", {})
        nch, dt = int(g.get("core:num_channels", 1)), g.get("core:datatype", "cf32_le")
        if not 2 <= nch <= 8 or dt not in ("cf32_le", "ci16_le", "ci8", "cu8") or args.path.endswith(".zip"):
            print(f"--correlate needs a recording of 2..8 channels in cf32_le, ci16_le, ci8 or cu8 (core:num_channels, not "
                  f"zipped); this one has core:num_channels = {nch}, core:datatype = {dt!r}", file=sys.stderr)
            return 2
        multi, _ = sigmf_io.read_sigmf_channels(args.path)
        samples = np.ascontiguousarray(multi[:, 0])
    raw16 = samples if samples.dtype == np.int16 else None
    raw8 = np.ascontiguousarray(samples) if samples.dtype in (np.int8, np.uint8) else None
    if raw8 is not None:
        samples = raw8
    n_samples = int(samples.shape[0])
    if n_samples < args.nfft:
        print(f"recording has {n_samples} samples, need {args.nfft}", file=sys.stderr)
        return 2
    fs, fc = meta["sample_rate"], meta["center_freq"]
    if raw16 is not None:
        power_db = spectrum.spectrum_db_ci16(np.ascontiguousarray(raw16[: args.nfft]), window=args.window, device=args.device)
    elif raw8 is not None:
        power_db = spectrum.spectrum_db_ci8(raw8[: args.nfft], window=args.window, device=args.device)
    else:
        power_db = spectrum.spectrum_db(samples[: args.nfft], window=args.window, device=args.device)
    freqs = spectrum.freq_axis(args.nfft, fs, fc)
    k = int(np.argmax(power_db))
    report = {"samples": n_samples, "sample_rate": fs, "center_freq": fc, "nfft": args.nfft,
              "peak_db": float(power_db[k]), "peak_freq_hz": float(freqs[k]),
              "median_db": float(np.median(power_db))}
    results = {"power_db": power_db, "freqs": freqs}
    if args.welch:
        if raw16 is not None:
            samples = raw16.astype(np.float32).view(np.complex64).reshape(-1)
        elif raw8 is not None:
            samples = spectrum.iq8_to_c64(raw8)
        pxx = spectrum.welch_psd(samples, args.welch, fs, device=args.device)
        results["welch_pxx"] = pxx
        results["welch_freqs"] = spectrum.freq_axis(args.welch, fs, fc)
        report["welch_nfft"] = args.welch
        report["welch_segments"] = 1 + (samples.size - args.welch) // args.welch
        report["welch_peak_db_per_hz"] = float(10 * np.log10(pxx.max()))
    if args.integrate:
        if raw16 is not None:   # the int16 samples as they are: the same rows from half the bytes, nothing widened on the host
            rows = spectrum.integrated_db_ci16(np.ascontiguousarray(raw16), args.nfft, args.integrate, detector=args.detector,
                                               window=args.window, device=args.device)
        elif raw8 is not None:   # ... and the bytes of a ci8 / cu8 recording as they are
            rows = spectrum.integrated_db_ci8(raw8, args.nfft, args.integrate, detector=args.detector, window=args.window,
                                              device=args.device)
        else:
            rows = spectrum.integrated_db(samples, args.nfft, args.integrate, detector=args.detector, window=args.window,
                                          device=args.device)
        results["integrated_db"] = rows
        report["integrate_k"] = args.integrate
        report["integrate_detector"] = args.detector
        report["integrated_rows"] = int(rows.shape[0])
        if rows.shape[0] == 0:
            print(f"recording holds fewer than {args.integrate} frames of {args.nfft} samples: no integrated row", file=sys.stderr)
    if args.pfb:   # the prototype is the window: --window does not apply; an int16 or 8-bit recording goes in as it is
        if raw16 is not None:
            rows = spectrum.pfb_db_ci16(np.ascontiguousarray(raw16), args.nfft, args.pfb, device=args.device)
        elif raw8 is not None:
            rows = spectrum.pfb_db_ci8(raw8, args.nfft, args.pfb, device=args.device)
        else:
            rows = spectrum.pfb_db(samples, args.nfft, args.pfb, device=args.device)
        results["pfb_db"] = rows
        report["pfb_taps"] = args.pfb
        report["pfb_rows"] = int(rows.shape[0])
        if rows.shape[0] == 0:
            print(f"recording holds fewer than {args.pfb} blocks of {args.nfft} samples: no PFB row", file=sys.stderr)
        if args.integrate:   # both: the spectrometer form as well, one row per K folded frames
            if raw16 is not None:
                rows = spectrum.pfb_integrated_db_ci16(np.ascontiguousarray(raw16), args.nfft, args.pfb, args.integrate,
                                                       detector=args.detector, device=args.device)
            elif raw8 is not None:
                rows = spectrum.pfb_integrated_db_ci8(raw8, args.nfft, args.pfb, args.integrate, detector=args.detector,
                                                      device=args.device)
            else:
                rows = spectrum.pfb_integrated_db(samples, args.nfft, args.pfb, args.integrate, detector=args.detector,
                                                  device=args.device)
            results["pfb_integrated_db"] = rows
            report["pfb_integrated_rows"] = int(rows.shape[0])
    if args.sk:   # (behind the filter bank with --pfb; an int16 or 8-bit recording goes in as it is)
        x = np.ascontiguousarray(raw16) if raw16 is not None else raw8 if raw8 is not None else samples
        if args.pfb:
            mean_db, sk = spectrum.pfb_spectral_kurtosis(x, args.nfft, args.pfb, args.integrate, device=args.device)
        elif raw16 is not None:
            mean_db, sk = spectrum.spectral_kurtosis_ci16(x, args.nfft, args.integrate, window=args.window, device=args.device)
        elif raw8 is not None:
            mean_db, sk = spectrum.spectral_kurtosis_ci8(x, args.nfft, args.integrate, window=args.window, device=args.device)
        else:
            mean_db, sk = spectrum.spectral_kurtosis(x, args.nfft, args.integrate, window=args.window, device=args.device)
        lo, hi = spectrum.sk_limits(args.integrate)
        results["sk"] = sk
        results["sk_mean_db"] = mean_db
        report["sk_rows"] = int(sk.shape[0])
        report["sk_limits"] = [lo, hi]
        report["sk_flagged_fraction"] = float(np.mean((sk < lo) | (sk > hi))) if sk.size else 0.0
    if pair is not None:
        plan = spectrum._cached_plan(args.nfft, args.window, 1e-12, True, args.device)
        xs = (plan.cross_spectrum_ci16 if pair.dtype == np.int16 else plan.cross_spectrum)(pair, args.integrate)
        coh, phase = xs.coherence, xs.phase
        results.update(cross_paa=xs.paa, cross_pbb=xs.pbb, cross=xs.cross, coherence=coh, phase=phase)
        report["cross_rows"] = int(coh.shape[0])
        if coh.size:
            g, b = np.unravel_index(int(np.argmax(coh)), coh.shape)
            report["cross_peak_coherence"] = float(coh[g, b])
            report["cross_peak_row"] = int(g)
            report["cross_peak_freq_hz"] = float(freqs[b])
            report["cross_peak_phase_rad"] = float(phase[g, b])
            report["cross_median_coherence"] = float(np.median(coh))
        else:
            print(f"recording holds fewer than {args.integrate} frames of {args.nfft} samples: no cross-spectrum row", file=sys.stderr)
    if multi is not None:
        plan = spectrum._cached_plan(args.nfft, args.window, 1e-12, True, args.device)
        multi = np.ascontiguousarray(multi)
        cm = (plan.correlate_ci16 if multi.dtype == np.int16 else plan.correlate_ci8 if multi.dtype in (np.int8, np.uint8)
              else plan.correlate)(multi, args.integrate)
        results["corr_planes"] = cm.planes
        report["corr_channels"] = cm.channels
        report["corr_rows"] = int(cm.planes.shape[0])
        report["corr_pairs"] = []
        if cm.planes.shape[0] == 0:
            print(f"recording holds fewer than {args.integrate} frames of {args.nfft} samples: no correlation row", file=sys.stderr)
        for i in range(cm.channels if cm.planes.shape[0] else 0):
            for j in range(i + 1, cm.channels):
                coh, phase = cm.coherence(i, j), cm.phase(i, j)
                g, b = np.unravel_index(int(np.argmax(coh)), coh.shape)
                report["corr_pairs"].append({"pair": [i, j], "peak_coherence": float(coh[g, b]), "peak_row": int(g),
                                             "peak_freq_hz": float(freqs[b]), "peak_phase_rad": float(phase[g, b]),
                                             "median_coherence": float(np.median(coh))})
    if args.out:
        np.savez_compressed(args.out, **results)
        report["out"] = args.out
    if args.cross:
        report["wrote"] = [args.out] if args.out else []
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())

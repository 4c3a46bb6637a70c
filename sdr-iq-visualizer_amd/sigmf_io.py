"""Minimal SigMF reader/writer for ``cf32_le`` recordings (BASELINE.json config 1), and for ``ci16_le`` ones in their own
format (``write_sigmf(..., datatype="ci16_le")``, ``read_sigmf(..., native=True)`` -> the ``(n, 2)`` int16 array the
``*_ci16`` spectrum functions take).  The 8-bit formats of the common radios, ``ci8`` (signed: a HackRF) and ``cu8``
(unsigned, mid-scale 127.5: an RTL-SDR), are written from and — with ``native="all"`` — read back as ``(n, 2)`` int8 / uint8
arrays for the ``*_ci8`` functions.

Format = what the reference's dashboard exports (app/dashboard/callbacks.py:285-319):
a ``.sigmf-data`` file of interleaved little-endian float32 I,Q and a ``.sigmf-meta``
JSON with ``global.core:datatype = "cf32_le"``, ``core:sample_rate``, ``core:version`` and
``captures[0].core:frequency`` / ``core:sample_start`` / ``core:datetime``, optionally
zipped together with a README.  The reference's offline reader
(scripts/process_sigmf_data.py:20-62) goes through the ``sigmf`` package, which is not a
dependency here: the format is simple enough to read directly.  File I/O only — no
signal processing in this module.

Multi-channel recordings (``core:num_channels = C``, the channels' samples interleaved per sample instant, as a 2 x 2 front
end delivers them): ``write_sigmf(..., num_channels=C)`` and ``read_sigmf_channels`` -> ``(n, C)`` (``(n, C, 2)`` for the
integer formats, ci8 / cu8 included).  ``read_sigmf`` itself
reads the data file as one stream whatever the channel count says.

Real-sampled recordings (``rf32_le``, ``ri16_le``, ``ri8``, ``ru8``): ``write_sigmf(..., datatype=...)`` from a flat array of
the matching dtype, ``read_sigmf_real`` -> the flat array in the file's own dtype, for the ``r*`` spectrum functions.
``read_sigmf`` refuses them: it returns complex samples.
"""
from __future__ import annotations

import io
import json
import os
import zipfile
from datetime import datetime, timezone
from typing import Optional, Tuple

import numpy as np

_DTYPES = {"cf32_le": np.dtype("<c8"), "cf64_le": np.dtype("<c16"),
           "ci16_le": np.dtype("<i2"), "ci8": np.dtype("i1"), "cu8": np.dtype("u1")}
_CU8_MID = np.float32(127.5)          # mid-scale of 0 ... 255: cu8 decodes to (I - 127.5) + 1j*(Q - 127.5)
_NATIVE = {"ci16_le": np.int16, "ci8": np.int8, "cu8": np.uint8}   # the (n, 2) dtype read_sigmf(native=...) gives back
# real-sampled recordings: read_sigmf_real / write_sigmf only (read_sigmf refuses them); the flat array's dtype
_REAL = {"rf32_le": np.dtype("<f4"), "ri16_le": np.dtype("<i2"), "ri8": np.dtype("i1"), "ru8": np.dtype("u1")}


def make_metadata(sample_rate: float, center_freq: float, *, description: str = "IQ recording",
                  author: str = "sdr_iq_visualizer_amd", hw: str = "", when: Optional[datetime] = None,
                  datatype: str = "cf32_le", num_channels: int = 1) -> dict:
    """Metadata dict with the keys of app/dashboard/callbacks.py:285-304 (and ``core:num_channels`` where it is not 1)."""
    when = when or datetime.now(timezone.utc)
    meta = {
        "global": {
            "core:datatype": datatype,
            "core:sample_rate": int(sample_rate),
            "core:version": "1.0.0",
            "core:description": description,
            "core:author": author,
            "core:hw": hw,
            "core:license": "CC0-1.0",
        },
        "captures": [{
            "core:sample_start": 0,
            "core:frequency": int(center_freq),
            "core:datetime": when.strftime("%Y-%m-%dT%H:%M:%S.%f") + "Z",
        }],
        "annotations": [],
    }
    if int(num_channels) != 1:
        meta["global"]["core:num_channels"] = int(num_channels)
    return meta


def _to_ci16(samples) -> np.ndarray:
    """``(n, 2)`` little-endian int16 from an int16 ``(..., 2)`` array (as is) or from complex / integer samples whose
    parts are whole numbers in the int16 range (anything else would lose information: ValueError)."""
    x = np.asarray(samples)
    if x.dtype == np.int16 and x.ndim >= 2 and x.shape[-1] == 2:
        return np.ascontiguousarray(x.reshape(-1, 2)).astype("<i2", copy=False)
    z = x.reshape(-1).astype(np.complex128)
    parts = np.stack([z.real, z.imag], axis=-1)
    if not np.all(parts == np.rint(parts)) or parts.min(initial=0) < -32768 or parts.max(initial=0) > 32767:
        raise ValueError("datatype='ci16_le' needs samples whose I and Q are integers in [-32768, 32767]")
    return parts.astype("<i2")


def _to_iq8(samples, datatype: str) -> np.ndarray:
    """``(n, 2)`` int8 (``ci8``) / uint8 (``cu8``) from an array of that dtype and shape ``(..., 2)`` (as is), or from complex
    samples that the format holds exactly: whole I and Q in [-128, 127] for ci8; I + 127.5 and Q + 127.5 whole and in
    [0, 255] for cu8 (what the reader gives back).  Anything else would lose information: ValueError."""
    dt = _NATIVE[datatype]
    x = np.asarray(samples)
    if x.dtype == dt and x.ndim >= 2 and x.shape[-1] == 2:
        return np.ascontiguousarray(x.reshape(-1, 2))
    if x.dtype in (np.int8, np.uint8):
        raise ValueError(f"datatype={datatype!r} takes an (n, 2) {np.dtype(dt).name} array, got {x.dtype} of shape {x.shape}")
    z = x.reshape(-1).astype(np.complex128)
    parts = np.stack([z.real, z.imag], axis=-1) + (127.5 if datatype == "cu8" else 0.0)
    lo, hi = (0, 255) if datatype == "cu8" else (-128, 127)
    if not np.all(parts == np.rint(parts)) or parts.min(initial=lo) < lo or parts.max(initial=hi) > hi:
        raise ValueError(f"datatype={datatype!r} needs samples whose I and Q" + (" + 127.5" if datatype == "cu8" else "")
                         + f" are integers in [{lo}, {hi}]")
    return parts.astype(dt)


def write_sigmf(base_path: str, samples, sample_rate: float, center_freq: float, datatype: str = "cf32_le",
                num_channels: int = 1, **meta_kw) -> Tuple[str, str]:
    """Write ``<base>.sigmf-data`` (cf32_le, or ci16_le on request: interleaved int16 I,Q from an int16 ``(n, 2)`` array or
    from integer-valued complex samples; or ci8 / cu8: interleaved bytes from an ``(n, 2)`` int8 / uint8 array or from complex
    samples the format holds exactly) and ``<base>.sigmf-meta``; returns both paths.
    ``num_channels=C`` (> 1): ``samples`` is ``(n, C)`` complex (or ``(n, C, 2)`` int16; for ci8 / cu8 ``(n, C, 2)`` int8 /
    uint8, nothing else), stored with the channels interleaved per sample instant and ``core:num_channels = C`` in the metadata."""
    if datatype in _REAL:
        x = np.asarray(samples)
        if x.dtype != _REAL[datatype].newbyteorder("=") or x.ndim != 1 or int(num_channels) != 1:
            raise ValueError(f"datatype={datatype!r} takes a flat {_REAL[datatype].newbyteorder('=').name} array of one channel, got "
                             f"{x.dtype} of shape {x.shape}")
        data_path, meta_path = base_path + ".sigmf-data", base_path + ".sigmf-meta"
        np.ascontiguousarray(x).astype(_REAL[datatype], copy=False).tofile(data_path)
        with open(meta_path, "w") as fh:
            json.dump(make_metadata(sample_rate, center_freq, datatype=datatype, **meta_kw), fh, indent=2)
        return data_path, meta_path
    if datatype not in ("cf32_le", "ci16_le", "ci8", "cu8"):
        raise ValueError(f"write_sigmf writes 'cf32_le', 'ci16_le', 'ci8', 'cu8' or the real 'rf32_le', 'ri16_le', 'ri8', 'ru8', "
                         f"not {datatype!r}")
    num_channels = int(num_channels)
    if num_channels < 1:
        raise ValueError("num_channels must be >= 1")
    if num_channels > 1:
        shape = np.shape(samples)
        int16 = getattr(samples, "dtype", None) == np.int16
        if datatype in ("ci8", "cu8"):   # the bytes as they are: (n, C, 2) of the format's own dtype
            if getattr(samples, "dtype", None) != _NATIVE[datatype] or len(shape) != 3 or shape[1:] != (num_channels, 2):
                raise ValueError(f"datatype={datatype!r} with num_channels={num_channels} needs an (n, {num_channels}, 2) "
                                 f"{np.dtype(_NATIVE[datatype]).name} array, got {getattr(samples, 'dtype', None)} of shape {shape}")
        elif len(shape) != (3 if int16 else 2) or shape[1] != num_channels:
            raise ValueError(f"num_channels={num_channels} needs samples of shape (n, {num_channels})"
                             f"{' (or (n, C, 2) int16)' if int16 else ''}, got {shape}")
        meta_kw["num_channels"] = num_channels   # (C-order flattening below interleaves the channels)
    data_path, meta_path = base_path + ".sigmf-data", base_path + ".sigmf-meta"
    if datatype != "cf32_le":
        (_to_ci16(samples) if datatype == "ci16_le" else _to_iq8(samples, datatype)).tofile(data_path)
        with open(meta_path, "w") as fh:
            json.dump(make_metadata(sample_rate, center_freq, datatype=datatype, **meta_kw), fh, indent=2)
        return data_path, meta_path
    x = np.asarray(samples)
    if x.dtype != np.complex64:                       # callbacks.py:307-308
        x = x.astype(np.complex64)
    x.astype("<c8", copy=False).tofile(data_path)     # callbacks.py:310 (tobytes)
    with open(meta_path, "w") as fh:
        json.dump(make_metadata(sample_rate, center_freq, **meta_kw), fh, indent=2)
    return data_path, meta_path


def _decode(raw: bytes, datatype: str) -> np.ndarray:
    if datatype not in _DTYPES:
        raise ValueError(f"unsupported core:datatype {datatype!r} (supported: {sorted(_DTYPES)})")
    a = np.frombuffer(raw, dtype=_DTYPES[datatype])
    if datatype == "cu8":                             # unsigned bytes around mid-scale 127.5 -> complex64 (exact)
        a = (a[: a.size // 2 * 2].astype(np.float32) - _CU8_MID).view(np.complex64)
    elif datatype.startswith("ci"):                   # interleaved integers -> complex64
        a = a[: a.size // 2 * 2].astype(np.float32).view(np.complex64)
    return a.astype(np.complex64, copy=False)


def _native_types(native) -> tuple:
    """The datatypes ``read_sigmf(native=...)`` returns raw: ``True`` keeps its first meaning (``ci16_le`` alone), ``"all"``
    is every integer format with entry points of its own, a name or a collection of names is those."""
    if native is True:
        return ("ci16_le",)
    if not native:
        return ()
    if native == "all":
        return tuple(_NATIVE)
    names = (native,) if isinstance(native, str) else tuple(native)
    for n in names:
        if n not in _NATIVE:
            raise ValueError(f"native={native!r}: {n!r} is none of {sorted(_NATIVE)}")
    return names


def read_sigmf(path: str, max_samples: Optional[int] = None, native=False) -> Tuple[np.ndarray, dict]:
    """Read a recording given its ``.sigmf-meta``, ``.sigmf-data``, base name, or the
    ``.zip`` the dashboard's download button produces.  Returns ``(samples complex64, meta)``;
    ``meta['sample_rate']`` and ``meta['center_freq']`` are lifted out for convenience.
    ``native=True``: a ``ci16_le`` recording comes back as its own ``(n, 2)`` int16 array, not widened (for the ``*_ci16``
    spectrum functions); every other datatype as without it.  ``native="all"``, or a collection of datatype names (``"ci16_le"``,
    ``"ci8"``, ``"cu8"``): ``ci8`` / ``cu8`` recordings too come back raw, ``(n, 2)`` int8 / uint8, for the ``*_ci8`` functions."""
    raw_types = _native_types(native)
    if path.endswith(".zip"):
        with zipfile.ZipFile(path) as z:
            names = z.namelist()
            meta_name = next(n for n in names if n.endswith(".sigmf-meta"))
            data_name = next(n for n in names if n.endswith(".sigmf-data"))
            meta = json.loads(z.read(meta_name))
            raw = z.read(data_name)
    else:
        base = path
        for ext in (".sigmf-meta", ".sigmf-data"):
            if base.endswith(ext):
                base = base[: -len(ext)]
        with open(base + ".sigmf-meta") as fh:
            meta = json.load(fh)
        itemsize = _DTYPES.get(meta.get("global", {}).get("core:datatype", "cf32_le"), np.dtype("<c8")).itemsize
        with open(base + ".sigmf-data", "rb") as fh:
            raw = fh.read() if max_samples is None else fh.read(int(max_samples) * itemsize * 2)
    g = meta.get("global", {})
    if g.get("core:datatype") in raw_types:
        a = np.frombuffer(raw, dtype=_DTYPES[g["core:datatype"]])
        samples = a[: a.size // 2 * 2].reshape(-1, 2).astype(_NATIVE[g["core:datatype"]], copy=False)
    else:
        samples = _decode(raw, g.get("core:datatype", "cf32_le"))
    if max_samples is not None:
        samples = samples[: int(max_samples)]
    caps = meta.get("captures") or [{}]
    out = dict(meta)
    out["sample_rate"] = float(g.get("core:sample_rate", 1.0))
    out["center_freq"] = float(caps[0].get("core:frequency", 0.0))
    return samples, out


def sigmf_datatype(path: str) -> str:
    """``core:datatype`` of a recording given its ``.sigmf-meta``, ``.sigmf-data`` or base name (default ``cf32_le``)."""
    base = path
    for ext in (".sigmf-meta", ".sigmf-data"):
        if base.endswith(ext):
            base = base[: -len(ext)]
    with open(base + ".sigmf-meta") as fh:
        return json.load(fh).get("global", {}).get("core:datatype", "cf32_le")


def read_sigmf_real(path: str, max_samples: Optional[int] = None) -> Tuple[np.ndarray, dict]:
    """Read a real-sampled recording (``rf32_le``, ``ri16_le``, ``ri8``, ``ru8``) given its ``.sigmf-meta``, ``.sigmf-data``
    or base name: ``(samples, meta)`` with the samples flat and in the file's own dtype (float32, int16, int8, uint8) — what
    ``rspectrum_db`` / ``rfft`` / ``SpectrumPlan.rstft_db`` take.  ``meta`` as from ``read_sigmf``.  Any other datatype is a
    ValueError."""
    base = path
    for ext in (".sigmf-meta", ".sigmf-data"):
        if base.endswith(ext):
            base = base[: -len(ext)]
    with open(base + ".sigmf-meta") as fh:
        meta = json.load(fh)
    g = meta.get("global", {})
    datatype = g.get("core:datatype", "cf32_le")
    if datatype not in _REAL:
        raise ValueError(f"read_sigmf_real reads {sorted(_REAL)}, not {datatype!r} (read_sigmf reads the complex datatypes)")
    a = np.fromfile(base + ".sigmf-data", dtype=_REAL[datatype], count=-1 if max_samples is None else int(max_samples))
    samples = a.astype(_REAL[datatype].newbyteorder("="), copy=False)
    caps = meta.get("captures") or [{}]
    out = dict(meta)
    out["sample_rate"] = float(g.get("core:sample_rate", 1.0))
    out["center_freq"] = float(caps[0].get("core:frequency", 0.0))
    return samples, out


def read_sigmf_channels(path: str) -> Tuple[np.ndarray, dict]:
    """Read a recording (``.sigmf-meta``, ``.sigmf-data`` or base name) honouring ``core:num_channels = C`` (default 1):
    ``(samples, meta)`` with the samples in their own format and the channels de-interleaved by a reshape, not a copy —
    ``(n, C)`` complex64 for ``cf32_le``, ``(n, C, 2)`` int16 for ``ci16_le``, ``(n, C, 2)`` int8 / uint8 for ``ci8`` /
    ``cu8``; a trailing partial sample instant is dropped.
    ``meta`` as from ``read_sigmf``, plus ``meta['num_channels']``."""
    base = path
    for ext in (".sigmf-meta", ".sigmf-data"):
        if base.endswith(ext):
            base = base[: -len(ext)]
    with open(base + ".sigmf-meta") as fh:
        meta = json.load(fh)
    g = meta.get("global", {})
    datatype, nch = g.get("core:datatype", "cf32_le"), int(g.get("core:num_channels", 1))
    if datatype not in ("cf32_le", "ci16_le", "ci8", "cu8"):
        raise ValueError(f"read_sigmf_channels reads 'cf32_le', 'ci16_le', 'ci8' or 'cu8', not {datatype!r}")
    if nch < 1:
        raise ValueError(f"core:num_channels is {nch}")
    per = nch if datatype == "cf32_le" else 2 * nch          # values of the file's dtype per sample instant
    a = np.fromfile(base + ".sigmf-data", dtype=_DTYPES[datatype])
    a = a[: a.size // per * per]
    if datatype == "cf32_le":
        samples = a.reshape(-1, nch).astype(np.complex64, copy=False)
    else:
        samples = a.reshape(-1, nch, 2).astype(_NATIVE[datatype], copy=False)
    caps = meta.get("captures") or [{}]
    out = dict(meta)
    out["sample_rate"] = float(g.get("core:sample_rate", 1.0))
    out["center_freq"] = float(caps[0].get("core:frequency", 0.0))
    out["num_channels"] = nch
    return samples, out


def to_zip_bytes(samples, sample_rate: float, center_freq: float, base_name: str = "sdr_sample") -> bytes:
    """The dashboard's download payload (callbacks.py:313-341): a zip of data + meta."""
    x = np.asarray(samples).astype(np.complex64)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr(f"{base_name}.sigmf-data", x.tobytes())
        z.writestr(f"{base_name}.sigmf-meta", json.dumps(make_metadata(sample_rate, center_freq), indent=2))
    return buf.getvalue()

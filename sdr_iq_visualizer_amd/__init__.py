"""Import name of the MI355X-native IQ spectrum path.

The project layout keeps the package sources in ``sdr-iq-visualizer_amd/`` (the
repository's name for it, with a hyphen, which Python cannot import directly).
This shim package gives it an importable name by putting that directory on its
``__path__``; every submodule (``spectrum``, ``waterfall``, ``synth``,
``sharding``, ``processing``, ``_ffi``) lives there, next to ``csrc/`` (the HIP
kernels and the C ABI) and ``lib/libsdrk.so`` (the built library).
"""
import os as _os

_SRC_DIR = _os.path.join(
    _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "sdr-iq-visualizer_amd"
)
if not _os.path.isdir(_SRC_DIR):  # pragma: no cover - broken checkout
    raise ImportError(f"package sources not found at {_SRC_DIR}")
__path__.append(_SRC_DIR)

from .spectrum import (  # noqa: E402
    ChannelBankStream,
    ChannelStream,
    CrossSpectrum,
    DdcBankStream,
    DdcStream,
    SpectrumPlan,
    channel_taps,
    cross_spectrum,
    ddc,
    ddc_bank,
    ddc_bank_ci8,
    ddc_ci8,
    ddc_taps,
    fft_c64,
    fft_c128,
    fft_ci16,
    fft_ci8,
    fir_bank,
    fir_filter,
    freq_axis,
    freq_word,
    freq_word_hz,
    integrated_db,
    integrated_db_ci16,
    integrated_db_ci8,
    pfb_db,
    pfb_db_ci16,
    pfb_integrated_db,
    pfb_integrated_db_ci16,
    pfb_prototype,
    pfb_spectral_kurtosis,
    process_frame,
    sk_limits,
    spectral_kurtosis,
    spectral_kurtosis_ci16,
    spectrum_db,
    spectrum_db_ci16,
    spectrum_db_ci8,
    stft_db,
    stft_db_ci16,
    stft_db_ci8,
    welch_psd,
    welch_psd_streamed,
    welch_psd_streamed_ci16,
    welch_psd_streamed_ci8,
)
from .waterfall import WaterfallBuffer  # noqa: E402
from .hostmem import is_pinned, pinned_empty, registered  # noqa: E402
from ._ffi import SdrkError, device_count, device_info, library_path  # noqa: E402

__all__ = [
    "ChannelBankStream",
    "ChannelStream",
    "CrossSpectrum",
    "DdcBankStream",
    "DdcStream",
    "SpectrumPlan",
    "WaterfallBuffer",
    "SdrkError",
    "channel_taps",
    "cross_spectrum",
    "ddc",
    "ddc_bank",
    "ddc_bank_ci8",
    "ddc_ci8",
    "ddc_taps",
    "device_count",
    "device_info",
    "fft_c64",
    "fft_c128",
    "fft_ci16",
    "fft_ci8",
    "fir_bank",
    "fir_filter",
    "freq_axis",
    "freq_word",
    "freq_word_hz",
    "integrated_db",
    "integrated_db_ci16",
    "integrated_db_ci8",
    "is_pinned",
    "library_path",
    "pfb_db",
    "pfb_db_ci16",
    "pfb_integrated_db",
    "pfb_integrated_db_ci16",
    "pfb_prototype",
    "pfb_spectral_kurtosis",
    "pinned_empty",
    "process_frame",
    "registered",
    "sk_limits",
    "spectral_kurtosis",
    "spectral_kurtosis_ci16",
    "spectrum_db",
    "spectrum_db_ci16",
    "spectrum_db_ci8",
    "stft_db",
    "stft_db_ci16",
    "stft_db_ci8",
    "welch_psd",
    "welch_psd_streamed",
    "welch_psd_streamed_ci16",
    "welch_psd_streamed_ci8",
]

"""``processing`` — the numpy-in / numpy-out module BASELINE.json's north-star
describes for the streamed-IQ FFT / PSD / waterfall path.

The reference's ``app/processing`` holds only the classifier (a consumer of
``power_db``); the spectrum itself is inline at app/sdr/streamer.py:119-121 and
the waterfall at app/dashboard/callbacks.py:176-182.  A maintainer switching to
this build imports these names there (INTEGRATION.md shows the three-line
change); the Dash callbacks keep reading the same ``plot_data`` dict.
"""
from .spectrum import (fft_c64, fft_ci16, freq_axis, integrated_db, integrated_db_ci16, process_frame,  # noqa: F401
                       spectrum_db, spectrum_db_ci16, stft_db, stft_db_ci16, welch_psd, welch_psd_streamed,
                       welch_psd_streamed_ci16)
from .spectrum import (fft_ci8, integrated_db_ci8, spectrum_db_ci8, stft_db_ci8, welch_psd_streamed_ci8)  # noqa: F401
from .spectrum import ddc_bank_ci8, ddc_ci8  # noqa: F401
from .waterfall import WaterfallBuffer  # noqa: F401

__all__ = ["spectrum_db", "fft_c64", "freq_axis", "process_frame", "stft_db", "welch_psd", "WaterfallBuffer",
           "spectrum_db_ci16", "fft_ci16", "stft_db_ci16", "integrated_db", "welch_psd_streamed",
           "integrated_db_ci16", "welch_psd_streamed_ci16",
           "spectrum_db_ci8", "fft_ci8", "stft_db_ci8", "integrated_db_ci8", "welch_psd_streamed_ci8",
           "ddc_ci8", "ddc_bank_ci8"]

/*
 * sdrk.h — C ABI of the MI355X-native IQ spectrum path ("sdrk" = SDR kernels).
 *
 * This is the drop-in boundary of the build.  The reference (a pure-Python Dash
 * app) has no FFI for this path: the work is three inline numpy expressions in
 * its SDR reader thread and a deque in its dashboard callback.  Each entry point
 * below names the reference expression it replaces (paths relative to the
 * reference checkout):
 *
 *   app/sdr/streamer.py:119   fft_data = np.fft.fftshift(np.fft.fft(samples))
 *   app/sdr/streamer.py:121   power_db = 20 * np.log10(np.abs(fft_data) + 1e-12)
 *   app/dashboard/callbacks.py:19    waterfall_data = deque(maxlen=100)
 *   app/dashboard/callbacks.py:176   waterfall_data.append(power_db)
 *   app/dashboard/callbacks.py:182   waterfall_array = np.array(waterfall_data)
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - every function returns SDRK_OK (0) or a negative sdrk_status; nothing
 *     throws; sdrk_last_error() returns a thread-local message for the last
 *     failure on the calling thread;
 *   - the caller owns every host buffer; the library owns plans, rings, device
 *     scratch, pinned staging and streams, released by the matching _destroy;
 *   - a plan or a waterfall is used by one thread at a time; distinct handles
 *     (e.g. one per GPU) may be used concurrently from different threads;
 *   - there is NO CPU fallback behind any of these symbols: with no usable
 *     gfx950 device they fail with SDRK_ERR_NO_DEVICE.
 */
#ifndef SDRK_H
#define SDRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRK_VERSION 500 /* 0.5.0: _ffi.py refuses a library of another version.  A change to an existing entry point bumps it;
                           * additions (new symbols) do not: _ffi.py checks that every symbol it declares is present. */

typedef enum sdrk_status {
    SDRK_OK = 0,
    SDRK_ERR_INVALID = -1,     /* bad argument (NULL, size, unsupported nfft …)   */
    SDRK_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range        */
    SDRK_ERR_HIP = -3,         /* a HIP runtime call failed; see sdrk_last_error() */
    SDRK_ERR_NOMEM = -4,       /* host or device allocation failed                 */
    SDRK_ERR_UNSUPPORTED = -5  /* valid request this build has no kernel for       */
} sdrk_status;

/* Window applied to each frame before the transform.  The reference applies
 * none (streamer.py:119): SDRK_WINDOW_RECT reproduces it.  SDRK_WINDOW_HANN is
 * numpy.hanning(nfft) (symmetric; w[0]=w[nfft-1]=0), the window matplotlib's
 * psd() uses in scripts/process_sigmf_data.py:188.  SDRK_WINDOW_CUSTOM takes
 * nfft float32 coefficients from the caller. */
typedef enum sdrk_window {
    SDRK_WINDOW_RECT = 0,
    SDRK_WINDOW_HANN = 1,
    SDRK_WINDOW_CUSTOM = 2
} sdrk_window;

typedef struct sdrk_plan sdrk_plan;           /* opaque */
typedef struct sdrk_waterfall sdrk_waterfall; /* opaque */

/* ---- library / device ---------------------------------------------------- */

int sdrk_version(void);
/* Thread-local, never NULL; valid until the next failing call on this thread. */
const char* sdrk_last_error(void);
/* Number of HIP devices visible to the process (0 if none). */
int sdrk_device_count(void);
/* Short device description ("gfx950 … 256 CUs …") into buf. */
int sdrk_device_info(int device, char* buf, size_t buf_len);

/* ---- device memory helpers (so callers need no other GPU runtime) -------- */

int sdrk_dev_alloc(int device, size_t bytes, void** d_ptr);
int sdrk_dev_free(int device, void* d_ptr);
/* Free and total device memory in bytes (what the runtime reports for `device` right now). */
int sdrk_dev_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* A long-lived input/output pair for the device-resident path, with the output placed where the two streams
 * interfere least.  On MI355X the achieved rate of a kernel that streams one buffer in and another out (the
 * spectrum path: 8 B in, 4 B out per sample) has two or three discrete levels ~6 % apart that depend on WHICH
 * two allocations are paired — read-only and (with rare exceptions) write-only rates do not depend on the buffer, and the level is
 * stable for the life of the pair (experiments/probes/placeprobe.hip).  This call allocates the input,
 * then up to `candidates` outputs (earlier ones stay allocated meanwhile, so each lands elsewhere), times a
 * probe over each pairing (after a warm-up by time; candidate 0 is timed again at the end and counts with the better of
 * its two timings: sdrk_placement_report) and keeps the fastest.  The probe is `plan`'s own transform over the pair (packed
 * frames; the input need not be initialised) or, with plan = NULL, a no-arithmetic kernel with the 2:1 traffic
 * shape.  probe_ms (may be NULL): `candidates` floats, the median probe time of each candidate (0 = not tried);
 * chosen (may be NULL): index kept.  Pairs too small for the effect to show (< 2^13 frame-equivalents of 4096
 * samples) are allocated without probing.  Free both with sdrk_dev_free. */
int sdrk_dev_alloc_stream_pair(int device, size_t in_bytes, size_t out_bytes, int candidates,
                               sdrk_plan* plan, void** d_in, void** d_out, float* probe_ms, int* chosen);
int sdrk_memcpy_h2d(int device, void* d_dst, const void* h_src, size_t bytes);
int sdrk_memcpy_d2h(int device, void* h_dst, const void* d_src, size_t bytes);

/* ---- pinned host memory for the numpy boundary ---------------------------------
 * sdrk_exec_host / sdrk_exec_fft_host stage pageable caller arrays through pinned slots with a pool of copy
 * threads (host_pool.h) — about 100 GB/s per process however many GPUs it drives.  Arrays that live in PINNED
 * host memory skip that: their chunks are DMA'd straight from / to the caller's memory, no host copy and no
 * host thread involved, so the boundary scales with the number of GPUs ("host gather via per-GPU
 * D2H into slices of one pinned array").  Either let the library allocate (sdrk_host_alloc: page-locked, visible
 * to every device) or register memory of your own (sdrk_host_register: the range must stay mapped until
 * sdrk_host_unregister — a numpy array must outlive its registration).  exec_host recognises any range that lies
 * inside such an allocation; input and output are decided independently. */
int sdrk_host_alloc(size_t bytes, void** h_ptr);
int sdrk_host_free(void* h_ptr);
int sdrk_host_register(void* h_ptr, size_t bytes);
int sdrk_host_unregister(void* h_ptr);
/* 1 if [h_ptr, h_ptr + bytes) lies inside memory made known by the calls above, else 0. */
int sdrk_host_is_pinned(const void* h_ptr, size_t bytes);

/* ---- spectrum plan -------------------------------------------------------
 * Replaces streamer.py:119,121 for frames of nfft complex64 samples:
 *     out_db[k] = 20*log10( | fftshift( fft( w * x ) ) |[k] + eps )     (float32)
 * nfft: 2 <= nfft <= 2^22 (2^SDRK_MAX_LOG2_NFFT) for powers of two (direct kernels);
 *       any other length 2 <= nfft <= 2^21 goes through a chirp-z (Bluestein) convolution
 *       built from the power-of-two kernels — the reference transforms whatever
 *       len(samples) is (streamer.py:119).
 * max_batch: largest n_frames a single sdrk_exec_host() call will be given
 *            (sizes the plan's device staging; exec_device has no such limit).
 * window_kind / window: see sdrk_window; `window` is read only for CUSTOM.
 * eps: additive floor on |X| (reference: 1e-12; legacy script 1e-10; 0 allowed).
 * shift: non-zero = fftshift order (DC at index nfft/2), as the reference. */
#define SDRK_MAX_LOG2_NFFT 22
int sdrk_plan_create(int device, int nfft, size_t max_batch, int window_kind,
                     const float* window, float eps, int shift, sdrk_plan** out);
/* Same with option flags.  nfft = 65536 has two forms: ONE persistent launch whose per-frame intermediate stays in each
 * XCD's L2 (fft_fused64k.hip), and the two tiled launches through a scratch buffer (fft_tiled2.hip); bit-identical rows.
 * Without a flag a plan takes the persistent launch for calls of 512 frames or more (BASELINE config 3: 3.9 ms against
 * 5.0 ms) and the two launches below that (they are faster there: the persistent grid costs ~30 us to set up); if a persistent launch ever reports a failed hand-over (its
 * workgroups must all be resident at once — another process's kernels can prevent that), the call returns SDRK_ERR_HIP and
 * the plan takes the two launches from then on.  SDRK_PLAN_FUSED64K: the persistent launch for every call (A/B work, tests).
 * SDRK_PLAN_TILED64K: never the persistent launch (a device shared with other processes' long-running kernels). */
#define SDRK_PLAN_FUSED64K 0x1u
#define SDRK_PLAN_TILED64K 0x8u
/* SDRK_PLAN_OVERLAP_PASSES (power-of-two nfft >= 2^15): run the row pass of chunk i on a second stream beside the
 * col pass of chunk i + 1, each on its own half of the scratch and on its own share of the CUs.  Bit-identical
 * rows; kept for A/B work like the flag above — measured 20-35 % SLOWER than the serial two-launch form on
 * BASELINE configs 3 and 5 (profiles/r03/overlap_probe.log). */
#define SDRK_PLAN_OVERLAP_PASSES 0x2u
/* SDRK_PLAN_TUNE_STAGING: allocate the device staging of the numpy boundary (sdrk_exec_host's chunk slots) at plan
 * creation and place each slot's row buffer as sdrk_dev_alloc_stream_pair places a resident pair — the fastest of three
 * candidates under the plan's own transform over one chunk.  Plans whose max_batch needs no chunking are unaffected.
 * sdrk_plan_staging_probe returns the probe times (3 per slot; n = 0 when nothing was tuned).  Measured on MI355X:
 * no effect at the shipped chunk size (the 24 MiB pairs are cache resident and the call is PCIe-bound). */
#define SDRK_PLAN_TUNE_STAGING 0x4u
int sdrk_plan_create_ex(int device, int nfft, size_t max_batch, int window_kind,
                        const float* window, float eps, int shift, unsigned flags, sdrk_plan** out);
int sdrk_plan_staging_probe(const sdrk_plan* plan, float* probe_ms, int capacity, int* n);
/* nfft = 65536 plans: how many persistent (fused) launches the plan has made so far, and whether one of them reported a
 * failed hand-over so that the plan now takes the two tiled launches (see SDRK_PLAN_FUSED64K above).  Either pointer may be
 * NULL.  Other plans: 0 / 0. */
int sdrk_plan_fused_status(const sdrk_plan* plan, unsigned* launches, int* fallen_back);
/* Large-frame plans (nfft >= 2^15) keep their two-pass intermediate in a scratch buffer, and — like the resident
 * input / output pair, see sdrk_dev_alloc_stream_pair — their speed depends a few per cent on WHERE that buffer
 * landed relative to the data (N = 65536 STFT over the same buffers with six different scratch allocations:
 * 5.02 ... 5.34 ms, stable per allocation).  This call times the plan's own transform of (d_iq, n_frames,
 * frame_stride) -> d_out_db with the present scratch and with up to `candidates` - 1 freshly allocated ones,
 * keeps the fastest and frees the others.  probe_ms (or NULL) receives `candidates` times (0 = not tried);
 * chosen (or NULL) the index kept (0 = the original).  d_out_db is overwritten with the transform's result.
 * Plans without a scratch return at once.  Not to be called while the plan is in use by another thread.
 * The probe warms up by time first (>= 60 ms of the plan's own launches: an idle MI355X needs tens of milliseconds of load
 * to reach its sustained shader clock, and a probe that starts cold measures that ramp instead of the placement), times
 * candidate 0 AGAIN after the last candidate, and replaces the present scratch only by a candidate that beats both of its
 * timings by one per cent (sdrk_placement_report has the re-timed figure). */
int sdrk_plan_tune_scratch(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames, size_t frame_stride_samples,
                           float* d_out_db, int candidates, float* probe_ms, int* chosen);
/* What the LAST placement probe on the calling thread did (sdrk_dev_alloc_stream_pair, sdrk_plan_tune_scratch): the wall
 * time and number of its warm-up launches, candidate 0 as first timed and as timed again after the last candidate, and the
 * kept candidate's time, all in milliseconds (any pointer may be NULL).  Returns the number of candidates it tried (0: no
 * probe has run on this thread, or the last one had nothing to place).  A first / re-timed pair that differs by more than
 * the candidates do says the probe measured drift, not placement. */
int sdrk_placement_report(float* warm_ms, int* warm_launches, float* first_ms, float* retimed_first_ms, float* chosen_ms);
int sdrk_plan_destroy(sdrk_plan* plan);
int sdrk_plan_nfft(const sdrk_plan* plan);
int sdrk_plan_device(const sdrk_plan* plan);

/* Host in / host out (the numpy boundary).  iq_c64: interleaved float32 I,Q,
 * frame f starts at sample f*frame_stride (frame_stride == nfft for packed
 * frames, == hop for an overlapped STFT over one contiguous stream; the buffer
 * must hold (n_frames-1)*frame_stride + nfft samples).  out_db: n_frames*nfft
 * float32, row-major.  Blocks until out_db is complete.
 * Calls of up to 256 KiB (the reference's live shape: one 4096-sample buffer,
 * streamer.py:114-121) are served by a kernel that reads and writes pinned host
 * memory directly; larger calls stream through pinned staging in ~16 MiB chunks,
 * three in flight (staging memcpys by a small helper-thread pool, H2D, transform
 * and D2H overlapped).  The caller's arrays may be ordinary pageable memory. */
int sdrk_exec_host(sdrk_plan* plan, const void* iq_c64, size_t n_frames,
                   size_t frame_stride, float* out_db);

/* Device in / device out, asynchronous on `stream` (a hipStream_t, or NULL for
 * the plan's own stream).  Same layout rules as sdrk_exec_host.  An nfft = 4096
 * call of about 10^5 frames or more is enqueued as several back-to-back launches of
 * about 65536 frames each (same rows; the kernel's time per frame grows with the
 * length of a launch: csrc/f4k_split.h). */
int sdrk_exec_device(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames,
                     size_t frame_stride, float* d_out_db, void* stream);

/* Complex spectrum (no |.|, no log): out_c64[f][k] = fft(w*x)[k], optionally
 * fftshifted as the plan says.  Replaces np.fft.fft at streamer.py:119 alone;
 * used by the parity tests to check the transform before the log epilogue. */
int sdrk_exec_fft_host(sdrk_plan* plan, const void* iq_c64, size_t n_frames,
                       size_t frame_stride, void* out_c64);

/* Averaged periodogram (Welch, no detrend): out_psd[k] = scale * sum_f |fft(w*x_f)|^2[k]
 * over n_frames frames cut from one host stream at spacing frame_stride, in the plan's
 * shift order.  With scale = 1/(n_frames * Fs * sum(w^2)) this is matplotlib's
 * mlab.psd(..., window=hanning, noverlap=nfft-frame_stride) as plotted by the reference's
 * offline script (scripts/process_sigmf_data.py:188-189).  out_psd: nfft float32. */
int sdrk_welch_psd_host(sdrk_plan* plan, const void* iq_c64, size_t n_frames, size_t frame_stride,
                        float scale, float* out_psd);

/* Block until everything queued on the plan's own stream has finished. */
int sdrk_plan_sync(sdrk_plan* plan);

/* Timed replay for the bench harness: runs `launches` back-to-back
 * sdrk_exec_device() calls on the plan's stream bracketed by HIP events on that
 * stream and returns the elapsed milliseconds (all launches together). */
int sdrk_exec_device_timed(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames,
                           size_t frame_stride, float* d_out_db, int launches,
                           float* elapsed_ms);

/* The same, returning the elapsed milliseconds of each of the `launches` launches
 * (events between consecutive launches; each_ms holds `launches` floats). */
int sdrk_exec_device_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames,
                                size_t frame_stride, float* d_out_db, int launches, float* each_ms);

/* ---- double precision: the reference's own dtypes ----------------------------
 * app/sdr/streamer.py:119-121 computes in float64 on the complex128 samples pyadi-iio delivers:
 *     out_db[k] = 20*log10( | fftshift( fft( w * x ) ) |[k] + eps )     (float64, complex128 in)
 * in that order (abs, + eps, log10, * 20), with library hypot / log10 / sincospi in double on the device.
 * An f64 plan is an ordinary sdrk_plan: sdrk_plan_destroy, _sync, _nfft and _device take it.  It serves ONLY the
 * _f64 entry points below; every float32 entry point (exec, Welch, features, waterfall) given an f64 plan returns
 * SDRK_ERR_INVALID, and so does an _f64 entry point given a float32 plan.
 * nfft: powers of two 2 ... 2^SDRK_MAX_LOG2_NFFT (other lengths: SDRK_ERR_UNSUPPORTED).  window: nfft doubles for
 * SDRK_WINDOW_CUSTOM; SDRK_WINDOW_HANN is numpy.hanning(nfft) in float64.  eps >= 0 (0: exact zeros give -inf).
 * Layout rules as sdrk_exec_host / sdrk_exec_device, with 16-byte samples (interleaved float64 I,Q) and 8-byte rows. */
/* streamer.py:119-121 */
int sdrk_plan_create_f64(int device, int nfft, size_t max_batch, int window_kind,
                         const double* window, double eps, int shift, sdrk_plan** out);
/* streamer.py:119-121 (which arithmetic a plan does): 32 (sdrk_plan_create*) or 64 (sdrk_plan_create_f64) */
int sdrk_plan_precision(const sdrk_plan* plan);
/* streamer.py:119-121, host in / host out, any batch in bounded device memory (pageable or pinned caller arrays) */
int sdrk_exec_host_f64(sdrk_plan* plan, const void* iq_c128, size_t n_frames, size_t frame_stride, double* out_db);
/* streamer.py:119 alone: complex128 fft(w*x), fftshifted if the plan shifts */
int sdrk_exec_fft_host_f64(sdrk_plan* plan, const void* iq_c128, size_t n_frames, size_t frame_stride, void* out_c128);
/* streamer.py:119-121, device in / device out, asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_f64(sdrk_plan* plan, const void* d_iq_c128, size_t n_frames, size_t frame_stride,
                         double* d_out_db, void* stream);
/* streamer.py:119-121, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_f64_timed_each(sdrk_plan* plan, const void* d_iq_c128, size_t n_frames, size_t frame_stride,
                                    double* d_out_db, int launches, float* each_ms);

/* ---- int16 input: what the radio delivers -----------------------------------------
 * The AD936x behind app/sdr/streamer.py:114 (self.sdr.rx()) produces 12-bit integers in int16 pairs; pyadi-iio widens them to
 * complex128 only because numpy needs it, and "ci16_le" is the most common SigMF datatype.  These entry points take that
 * format as it is: interleaved little-endian int16 I,Q, 4 bytes per sample, frame f at sample f*frame_stride (layout rules as
 * sdrk_exec_host / sdrk_exec_device; the buffer need only be 4-byte aligned).  Semantics:
 *     x[n] = float32(I[n]) + i*float32(Q[n])          (exact)
 * then exactly what the plan's complex64 entry point computes — the same bits, not the same values within a tolerance.  No
 * scale is applied: a caller who wants full-scale normalisation folds 1/32768 (1/2048 for 12-bit data) into a custom window or
 * adds the constant 20*log10(scale) to the dB rows.  Served by ordinary float32 plans of any nfft; an f64 plan returns
 * SDRK_ERR_INVALID.  nfft = 256 ... 16384 are read as int16 by the transform itself (half the input bytes of the complex64
 * call); other lengths are widened on the device in chunks of at most 64 MiB first.  The integrated spectra have an int16
 * form (sdrk_exec_*_integrated_ci16, below); sdrk_welch_psd_host, the feature entry points and the waterfall appends have
 * none. */
/* streamer.py:114-121, host in / host out: the numpy boundary of sdrk_exec_host with 4-byte samples */
int sdrk_exec_host_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db);
/* streamer.py:114-119: complex64 fft(w*x) of int16 samples, fftshifted if the plan shifts */
int sdrk_exec_fft_host_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64);
/* streamer.py:114-121, device in / device out, asynchronous on `stream` (NULL: the plan's stream); any number of frames */
int sdrk_exec_device_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                          void* stream);
/* streamer.py:114-121, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                     float* d_out_db, int launches, float* each_ms);
/* streamer.py:114: sdrk_synth_fill's values (below) as int16 pairs, n_frames*nfft*4 bytes; equal to synth.py's int16 form */
int sdrk_synth_fill_ci16(int device, uint32_t seed, uint64_t first_frame, size_t n_frames, int nfft, void* d_iq_ci16,
                         void* stream);

/* ---- integrated spectra: one row per K frames ---------------------------------------
 * What a spectrum analyser does with the rows of streamer.py:119-121 before anybody looks at them: average the power of K
 * consecutive frames (video averaging; Welch, scripts/process_sigmf_data.py:188-189), or hold the maximum (peak hold) or
 * the minimum (noise floor) per bin.  Frames are cut as for sdrk_exec_device — frame f at sample f*frame_stride, any stride
 * >= 1 — and group g is the frames [g*k_frames, (g+1)*k_frames).  With p_f[k] = |fft(w*x_f)[k]|^2,
 *     SDRK_DET_MEAN  R[k] = (1/K) sum_f p_f[k]        SDRK_DET_MAX  R[k] = max_f p_f[k]        SDRK_DET_MIN  R[k] = min_f p_f[k]
 * and the row of a group, float32[nfft] in the plan's shift order, is
 *     SDRK_INT_OUT_DB     20*log10(sqrt(R[k]) + eps)    (the plan's own expression on the RMS / largest / smallest magnitude;
 *                                                        K = 1 is the ordinary row)
 *     SDRK_INT_OUT_POWER  scale * R[k]                  (with scale = 1/(Fs*sum(w^2)) and MEAN: matplotlib's mlab.psd)
 * `scale` is ignored for SDRK_INT_OUT_DB.  Any k_frames >= 1 and n_groups >= 1; the device entry has no frame limit (the
 * plan's max_batch does not apply) and the host entry runs in device memory that does not depend on the stream length.
 * The mean is a compensated sum; there are no floating-point atomics: the same input gives the same bits, from the device
 * entry and from the host entry alike.  Served by float32 plans of every nfft (N = 4096 inside the transform's registers,
 * other lengths through plan-owned staging of at most 64 MiB); an f64 plan, an unknown detector or form and zero counts
 * return SDRK_ERR_INVALID. */
enum sdrk_detector { SDRK_DET_MEAN = 0, SDRK_DET_MAX = 1, SDRK_DET_MIN = 2 };
enum sdrk_int_out { SDRK_INT_OUT_DB = 0, SDRK_INT_OUT_POWER = 1 };
/* device in / device out (d_out: n_groups * nfft float32), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_integrated(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                int detector, int out_form, float scale, float* d_out, void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` calls (bench harness) */
int sdrk_exec_device_integrated_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                           size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                           int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked through pinned staging */
int sdrk_exec_host_integrated(sdrk_plan* plan, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                              int detector, int out_form, float scale, float* out);
/* The same three from int16 I,Q (the int16 section above: 4 bytes per sample, frame starts 4-byte aligned, any frame_stride
 * >= 1, no scale applied to the samples): x[n] = float32(I[n]) + i*float32(Q[n]) exactly, then the same bits as the entry
 * point above returns for those widened samples — every nfft of a float32 plan (chirp-z included), every detector, form,
 * k_frames, n_groups and stride, device and host entry alike; the same refusals.  N = 4096 reads the int16 samples inside the
 * reducing transform (4 + 4/K bytes per sample through device memory); other lengths run the plan's int16 transform into the
 * same staging of at most 64 MiB. */
int sdrk_exec_device_integrated_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                     size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_integrated_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                int launches, float* each_ms);
int sdrk_exec_host_integrated_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                   int detector, int out_form, float scale, float* out);

/* ---- 8-bit input: SigMF ci8 and cu8 -------------------------------------------------
 * What the two most common radios write: a HackRF signed 8-bit pairs (SigMF "ci8"), an RTL-SDR unsigned ones ("cu8").  A
 * sample is 2 bytes, I then Q; frame f at sample f*frame_stride (layout rules as the int16 entry points; the buffer need only
 * be 2-byte aligned).  `iq8_format`, right after the input pointer, says which:
 *     SDRK_IQ8_SIGNED    (int8)    x[n] = float32(I[n]) + i*float32(Q[n])
 *     SDRK_IQ8_UNSIGNED  (uint8)   x[n] = (float32(I[n]) - 127.5f) + i*(float32(Q[n]) - 127.5f)     (127.5: mid-scale of 0...255)
 * both exact in float32 (no -0.0 arises), then exactly what the plan's complex64 entry point computes on those values — the
 * same bits, at every nfft, stride, window, epilogue and detector, device and host entry alike.  No scale is applied, as with
 * int16.  Per-frame rows / spectra and the integrated spectra have an 8-bit form; nfft = 4096 reads the bytes inside the
 * transform (2 bytes per sample in), every other length is widened on the device in chunks of at most 64 MiB first.  Each
 * entry point has the signature and the refusals of its _ci16 twin, and refuses an f64 plan and a format other than the two
 * with SDRK_ERR_INVALID; a plan that has refused still works.  The down-converter has an 8-bit form in a section of its own
 * (sdrk_exec_*_downconv_iq8, below), the filter bank and spectral kurtosis in another (sdrk_exec_*_pfb_iq8, _kurtosis_iq8,
 * below); the cross-spectra, bin-tuned FIR / channel bank, Welch, features and waterfall entry points have none. */
enum sdrk_iq8_format { SDRK_IQ8_SIGNED = 0, SDRK_IQ8_UNSIGNED = 1 };
int sdrk_exec_host_ci8(sdrk_plan* plan, const void* iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride, float* out_db);
int sdrk_exec_fft_host_ci8(sdrk_plan* plan, const void* iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride,
                           void* out_c64);
int sdrk_exec_device_ci8(sdrk_plan* plan, const void* d_iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride,
                         float* d_out_db, void* stream);
int sdrk_exec_device_ci8_timed_each(sdrk_plan* plan, const void* d_iq_ci8, int iq8_format, size_t n_frames, size_t frame_stride,
                                    float* d_out_db, int launches, float* each_ms);
int sdrk_exec_device_integrated_ci8(sdrk_plan* plan, const void* d_iq_ci8, int iq8_format, size_t n_groups, size_t k_frames,
                                    size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_integrated_ci8_timed_each(sdrk_plan* plan, const void* d_iq_ci8, int iq8_format, size_t n_groups,
                                               size_t k_frames, size_t frame_stride, int detector, int out_form, float scale,
                                               float* d_out, int launches, float* each_ms);
int sdrk_exec_host_integrated_ci8(sdrk_plan* plan, const void* iq_ci8, int iq8_format, size_t n_groups, size_t k_frames,
                                  size_t frame_stride, int detector, int out_form, float scale, float* out);

/* ---- real-sampled input: SigMF rf32_le / ri16_le / ri8 / ru8 --------------------------
 * One-sided spectra of real sample streams (a direct-sampling receiver, an ADC behind an IF, audio-rate baseband).  For a
 * float32 plan of power-of-two length N = nfft, 16 <= N <= 2^20, a real frame has L = 2 N samples and a row N + 1 bins: bin k
 * at k * fs / L, ascending from 0 to fs / 2, no fftshift, whatever the plan's `shift`.  The plan's own window (window_kind at
 * creation) plays no part; the mode has a real window of L coefficients of its own, rectangular until one is set.
 *     SDRK_REAL_F32 float32          SDRK_REAL_S16 int16 -> float32(v)
 *     SDRK_REAL_S8  int8 -> float32(v)          SDRK_REAL_U8  uint8 -> float32(v) - 127.5f        (all exact)
 * Arithmetic: y[n] = w[n] * x[n] (one float32 product; no window: none), z[m] = y[2m] + i y[2m+1], Z = the plan's rectangular
 * transform of z, and for k = 0 ... N with Z[N] = Z[0]:
 *     E = (Z[k] + conj Z[N-k]) / 2,   O = -(i/2) (Z[k] - conj Z[N-k]),   X[k] = E + exp(-i pi k / N) * O
 * X[0] = Re Z[0] + Im Z[0] and X[N] = Re Z[0] - Im Z[0], both with imaginary part +0.0; exp(-i pi k / N) comes from a table
 * computed in float64 and rounded once (at N = 4096 times a constant exp(-i pi k2 / 16)).  Rows are complex64 X[k]
 * (SDRK_REAL_OUT_COMPLEX) or float32 20*log10(|X[k]| + eps) with the plan's eps (SDRK_REAL_OUT_DB).
 * sdrk_plan_set_real_window: n must be 2 * nfft; the coefficients are copied; NULL / 0 returns to rectangular.  Not with work
 * of the plan in flight.
 * Calls: frame_stride counts REAL samples and must be even (frames may overlap or leave gaps); the input pointer must be
 * aligned to a pair of samples (8 / 4 / 2 bytes); out_stride counts output elements between rows: 0 = packed (nfft + 1),
 * otherwise >= nfft + 1, and what lies between rows is not written.  The host entries write packed rows and chunk as
 * sdrk_exec_host does.  N = 4096 is one kernel on the caller's data; other lengths stage complex64 pairs in plan-owned memory
 * (at most 2 x 64 MiB).
 * Promised: the integer formats return the bits of the float32 call on the widened samples; a host entry returns the bits of
 * the device entry however it is chunked; a frame's row does not depend on where in a call it stands.
 * Refused, nothing launched: an f64 plan, an odd frame_stride, a misaligned pointer, a window of another length, an unknown
 * real_format or out_form, out_stride in 1 ... nfft, NULL pointers (SDRK_ERR_INVALID); a chirp-z (non-power-of-two) plan and
 * nfft < 16 or > 2^20 (SDRK_ERR_UNSUPPORTED); each with a message.  A plan that has refused still works.
 * Integrated form (sdrk_exec_*_real_integrated): ONE row of nfft + 1 float32 per group of k_frames consecutive frames, group g
 * the frames [g * k_frames, (g + 1) * k_frames); rows packed, n_groups x (nfft + 1), ascending from 0 to fs/2, never shifted.
 * The frame, format, window, alignment and stride rules are those above.  With X_f[k] the complex64 row of frame f as
 * SDRK_REAL_OUT_COMPLEX returns it and p_f[k] = fmaf(re, re, im * im), the row is the reduction of p_f[k] over the group's
 * frames by `detector` (SDRK_DET_MEAN: compensated sum times float32(1 / k_frames); SDRK_DET_MAX; SDRK_DET_MIN), given as
 * 20*log10(sqrt(R) + eps) (SDRK_INT_OUT_DB) or scale * R (SDRK_INT_OUT_POWER) — the detectors, forms and splitting of few
 * long groups are those of sdrk_exec_device_integrated.  N = 4096 reduces inside the transform's kernel on the caller's data;
 * other lengths run the per-frame route into at most 64 MiB more of plan-owned staging and reduce down its columns.
 * Promised: an unsplit group's row carries the bits of that reduction applied to the per-frame complex rows; k_frames = 1 in
 * dB is the per-frame SDRK_REAL_OUT_DB row bit for bit; the integer formats give the bits of the float32 call on the widened
 * samples; the host entry gives the device entry's bits however it is chunked; a group's row does not depend on its place
 * in a call.  Refused, nothing launched: everything the per-frame entries refuse, and an unknown detector or out_form,
 * n_groups or k_frames of 0, a frame_stride of 0 (SDRK_ERR_INVALID).
 * Not provided: filter-bank / kurtosis / cross forms and the FIR family on real input, double precision, odd hops, the
 * inverse transform. */
enum sdrk_real_format { SDRK_REAL_F32 = 0, SDRK_REAL_S16 = 1, SDRK_REAL_S8 = 2, SDRK_REAL_U8 = 3 };
enum sdrk_real_out { SDRK_REAL_OUT_DB = 0, SDRK_REAL_OUT_COMPLEX = 1 };
int sdrk_plan_set_real_window(sdrk_plan* plan, const float* w, size_t n);
int sdrk_exec_device_real(sdrk_plan* plan, const void* d_x, int real_format, size_t n_frames, size_t frame_stride, int out_form,
                          void* d_out, size_t out_stride, void* stream);
int sdrk_exec_device_real_timed_each(sdrk_plan* plan, const void* d_x, int real_format, size_t n_frames, size_t frame_stride,
                                     int out_form, void* d_out, size_t out_stride, int launches, float* each_ms);
int sdrk_exec_host_real(sdrk_plan* plan, const void* x, int real_format, size_t n_frames, size_t frame_stride, float* out_db);
int sdrk_exec_fft_host_real(sdrk_plan* plan, const void* x, int real_format, size_t n_frames, size_t frame_stride, void* out_c64);
int sdrk_exec_device_real_integrated(sdrk_plan* plan, const void* d_x, int real_format, size_t n_groups, size_t k_frames,
                                     size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_real_integrated_timed_each(sdrk_plan* plan, const void* d_x, int real_format, size_t n_groups,
                                                size_t k_frames, size_t frame_stride, int detector, int out_form, float scale,
                                                float* d_out, int launches, float* each_ms);
int sdrk_exec_host_real_integrated(sdrk_plan* plan, const void* x, int real_format, size_t n_groups, size_t k_frames,
                                   size_t frame_stride, int detector, int out_form, float scale, float* out);

/* ---- polyphase filter bank spectra: a T-tap weighted fold in front of the transform ------
 * A plain windowed FFT gives every bin the window's response: a wide main lobe, side lobes that fall slowly.  A polyphase
 * filter bank (weighted overlap-add) applies a prototype filter h of T*nfft coefficients (typically a windowed sinc) to T*nfft
 * consecutive samples, folds the T blocks into nfft samples and transforms those: the bins become nearly rectangular channels.
 * It sits in front of app/sdr/streamer.py:119-121 (`samples` becomes the folded frame); the reference has no counterpart (a
 * build-side extension, like the decimated waterfall read-out).
 * With N = nfft, frame f starts at sample s = f*frame_stride (any stride >= 1) and reads T*N samples; the buffer holds
 * (n_frames-1)*frame_stride + T*N samples:
 *     y_f[n] = (((h[n]*x[s+n]) + h[N+n]*x[s+N+n]) + h[2N+n]*x[s+2N+n]) + ...        (taps in ascending order)
 * per real component in float32, every product rounded to float32, then every sum: no fused multiply-add — what numpy computes
 * on float32 arrays.  The row is then exactly what the plan's complex64 entry point returns for the frame y_f with a rectangular
 * window: the same bits at every length (chirp-z and the two-pass lengths included), as dB rows or as the complex spectrum, in
 * the plan's shift order and with its eps.
 * The prototype is the window: these entry points serve float32 plans created with SDRK_WINDOW_RECT only.  A windowed plan, an
 * f64 plan, a plan with no prototype set, taps < 1 or > 32, NULL pointers and n_frames = 0 return SDRK_ERR_INVALID.  T = 1 is
 * the rectangular transform of numpy's float32 h*x.  Every other entry point of a plan with a prototype set behaves as before.
 * N = 4096 folds inside the transform's registers (8 B/sample from device memory at frame_stride = nfft, 4 B/sample out); other
 * lengths fold into plan-owned staging of at most 64 MiB and run the plan's own transform.
 * Integration over K folded frames is the next section, int16 I,Q input the one after it.  Not provided: double precision,
 * waterfall appends. */
/* the prototype: taps*nfft float32 from host memory into a plan-owned device copy; may be called again with another prototype
 * or another T (not while work of this plan is in flight) */
int sdrk_plan_set_pfb(sdrk_plan* plan, int taps, const float* h);
/* taps of the prototype set on the plan; 0 = none */
int sdrk_plan_pfb_taps(const sdrk_plan* plan);
/* device in / device out (d_out_db: n_frames*nfft float32), asynchronous on `stream` (NULL: the plan's stream); any number of frames */
int sdrk_exec_device_pfb(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames, size_t frame_stride, float* d_out_db,
                         void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_pfb_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames, size_t frame_stride,
                                    float* d_out_db, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked through pinned staging in device memory that does not depend
 * on the stream length (n_frames <= the plan's max_batch, as for sdrk_exec_host) */
int sdrk_exec_host_pfb(sdrk_plan* plan, const void* iq_c64, size_t n_frames, size_t frame_stride, float* out_db);
/* the complex spectrum of the folded frames: out_c64[f][k] = fft(y_f)[k], fftshifted if the plan shifts */
int sdrk_exec_fft_host_pfb(sdrk_plan* plan, const void* iq_c64, size_t n_frames, size_t frame_stride, void* out_c64);

/* ---- integrated polyphase filter bank spectra: one row per K folded frames ---------------
 * The form a filter bank is used in (spectrometer back ends, monitoring receivers): fold, transform, |.|^2, and accumulate K
 * spectra per output row.  Frames are cut as in the section above — frame f starts at sample f*frame_stride (any stride >= 1)
 * and covers T*nfft samples; the buffer holds (n_groups*k_frames - 1)*frame_stride + T*nfft samples — and folded to y_f by the
 * same float32 arithmetic; group g is the frames [g*k_frames, (g+1)*k_frames).  The row of a group is, bit for bit, what
 * sdrk_exec_device_integrated returns on the same plan for the packed frames y_f (frame_stride = nfft) with the same n_groups,
 * k_frames, detector, out_form and scale: SDRK_DET_MEAN (compensated), _MAX or _MIN of |fft(y_f)[k]|^2 as SDRK_INT_OUT_DB or
 * SDRK_INT_OUT_POWER, in the plan's shift order and with its eps — at every nfft of a float32 plan (chirp-z and the two-pass
 * lengths included), every T in [1, 32], K, number of groups and stride, from the device entry and the host entry alike.
 * The refusals are those of the two sections together, each SDRK_ERR_INVALID with a message: a windowed plan, an f64 plan, a
 * plan with no prototype set; an unknown detector or out_form; n_groups or k_frames = 0 or their product out of range;
 * frame_stride = 0; NULL pointers.  A plan that has refused a call still works.
 * N = 4096 folds and reduces inside the transform's registers: 8 B/sample read from device memory at frame_stride = nfft, 4/K
 * written.  Other lengths fold into the PFB staging, transform into the integrate staging (each at most 64 MiB) and reduce
 * from there.  The device entry has no frame limit; the host entry runs in device memory that does not grow with the stream. */
/* device in / device out (d_out: n_groups * nfft float32), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_pfb_integrated(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                    int detector, int out_form, float scale, float* d_out, void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` calls (bench harness) */
int sdrk_exec_device_pfb_integrated_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                               size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                               int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked through pinned staging */
int sdrk_exec_host_pfb_integrated(sdrk_plan* plan, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                  int detector, int out_form, float scale, float* out);

/* ---- polyphase filter bank spectra from int16 I,Q: per frame and integrated, 4 bytes per sample ----
 * The two sections above on interleaved little-endian int16 I,Q (SigMF ci16_le), as a radio delivers it:
 * x[n] = float32(I[n]) + i*float32(Q[n]) exactly, and every entry point returns the bits its complex64 counterpart above
 * returns for those widened samples — at every nfft of a float32 rectangular plan, every T in [1, 32], stride, frame or group
 * count, K, detector, out_form, scale and shift, from the device entries and the host entries alike.  The argument lists are
 * the counterparts'; frame_stride counts samples; the buffer holds (frames - 1)*frame_stride + T*nfft samples of 4 bytes each;
 * frame starts need 4-byte alignment only.  The refusals are the counterparts' too, each SDRK_ERR_INVALID with a message.
 * N = 4096 folds the int16 samples inside the transform's registers: 4 B/sample read from device memory at frame_stride = nfft
 * (4*T with the cached re-reads, half the complex64 form's), 4 or 4/K written.  Other lengths fold the int16 samples straight
 * into the PFB staging (no widened copy of the stream) and go on as above.  The host entries move 4 B/sample over the link. */
int sdrk_exec_device_pfb_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                              void* stream);
int sdrk_exec_device_pfb_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                         float* d_out_db, int launches, float* each_ms);
int sdrk_exec_host_pfb_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db);
int sdrk_exec_fft_host_pfb_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64);
int sdrk_exec_device_pfb_integrated_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                         size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_pfb_integrated_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                                    size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                                    int launches, float* each_ms);
int sdrk_exec_host_pfb_integrated_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                       int detector, int out_form, float scale, float* out);

/* ---- spectral kurtosis: per-bin SK and mean power over K frames in one pass ------------
 * What a spectrometer accumulates beside the power: the sum of squared powers, and from both the spectral kurtosis estimator of
 * Nita & Gary, the usual per-channel interference flag of monitoring receivers and radio-astronomy back ends.  Frames and
 * groups are cut exactly as for sdrk_exec_device_integrated (frame f at sample f*frame_stride, any stride >= 1; group g is the
 * frames [g*k_frames, (g+1)*k_frames)); the PFB forms cut and fold them as sdrk_exec_device_pfb_integrated does.  With
 * p_f[k] = |fft(w*x_f)[k]|^2 and M = k_frames,
 *     S1 = sum_f p_f        S2 = sum_f p_f^2        SK = (M+1)/(M-1) * (M*S2/S1^2 - 1)
 * Gaussian noise gives SK = 1 with variance 4M^2/((M-1)(M+2)(M+3)) whatever its level; a CW carrier drives SK towards 0, pulsed
 * or bursty interference well above 1.
 * Output: per group TWO planes of nfft float32, d_out[n_groups][2][nfft], in the plan's shift order.  Plane 0 is the group's
 * mean power R = S1/K through the epilogue of the integrated section (SDRK_INT_OUT_DB: 20*log10(sqrt(R) + eps);
 * SDRK_INT_OUT_POWER: scale * R).  Plane 1 is SK, dimensionless; out_form and scale do not touch it.
 * Sums: S1 and S2 are plain float32 running sums in frame order, S1 += p and S2 = fmaf(p, p, S2) with p = fmaf(re, re, im*im) as
 * the integrating kernels form it.  No floating-point atomics.  A group that was cut into slices (few groups on a large device)
 * has its slices' sums added in slice order in float64 and rounded to float32 once.  SK is then one float32 expression of S1, S2
 * and M — IEEE division, no fast reciprocal — that every route shares.  S1 == 0 (a dead bin; also S1^2 below the float32 range,
 * mean |X| under roughly 1e-10) gives SK = 0, never NaN: a bin without power is as non-Gaussian as a carrier.
 * Accuracy of plane 0: it is NOT the compensated mean of SDRK_DET_MEAN.  Its relative power error may grow as K * 2^-24 on bins
 * whose power hardly changes from frame to frame; callers who need the 1e-5 amplitude bound at large K take SDRK_DET_MEAN.
 * Overflow: S2 (and S1^2) leave float32 where p^2 does, |X| above about 4e9; that is not guarded.
 * Determinism: the same input gives the same bits, from the device entry and the host entry alike, however the host call is
 * chunked.  The int16 forms return the bits of the complex64 forms on float32(I) + i*float32(Q); the PFB forms the bits of the
 * complex64 form on the packed folded frames wherever both take the same route (every nfft but 4096).
 * Refusals, each SDRK_ERR_INVALID with a message: k_frames < 2 (the estimator divides by M - 1); everything the integrated
 * entry points refuse apart from the detector (an f64 plan, an unknown out_form, n_groups = 0 or the product out of range,
 * frame_stride = 0, NULL pointers); for the PFB forms a windowed plan or one without a prototype.  A plan that has refused
 * still works.
 * N = 4096 keeps both sums in the transform's registers: 8 + 8/K bytes per sample through device memory from complex64,
 * 4 + 8/K from int16, where reducing per-frame rows afterwards moves 12.  Other lengths reduce the plan's complex spectra from
 * staging of at most 64 MiB.  The PFB forms fold and transform through the per-frame PFB route into that staging at every
 * nfft, 4096 included: there is no folding SK kernel.  Not provided: double precision, the generalised estimator for
 * pre-accumulated spectra, waterfall appends. */
/* device in / device out (d_out: n_groups * 2 * nfft float32), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_sk(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                        int out_form, float scale, float* d_out, void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` calls (bench harness) */
int sdrk_exec_device_sk_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                                   int out_form, float scale, float* d_out, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked through pinned staging */
int sdrk_exec_host_sk(sdrk_plan* plan, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride, int out_form,
                      float scale, float* out);
/* the same three from int16 I,Q (4 bytes per sample, frame starts 4-byte aligned) */
int sdrk_exec_device_sk_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                             int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_sk_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                        size_t frame_stride, int out_form, float scale, float* d_out, int launches,
                                        float* each_ms);
int sdrk_exec_host_sk_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                           int out_form, float scale, float* out);
/* behind the plan's polyphase filter bank (float32 rectangular plans with a prototype set; a frame covers T*nfft samples) */
int sdrk_exec_device_pfb_sk(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                            int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_pfb_sk_timed_each(sdrk_plan* plan, const void* d_iq_c64, size_t n_groups, size_t k_frames,
                                       size_t frame_stride, int out_form, float scale, float* d_out, int launches,
                                       float* each_ms);
int sdrk_exec_host_pfb_sk(sdrk_plan* plan, const void* iq_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                          int out_form, float scale, float* out);
int sdrk_exec_device_pfb_sk_ci16(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                 int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_pfb_sk_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, size_t n_groups, size_t k_frames,
                                            size_t frame_stride, int out_form, float scale, float* d_out, int launches,
                                            float* each_ms);
int sdrk_exec_host_pfb_sk_ci16(sdrk_plan* plan, const void* iq_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                               int out_form, float scale, float* out);

/* ---- filter bank and spectral kurtosis from 8-bit I,Q: ci8 / cu8, 2 bytes per sample ------
 * The polyphase-filter-bank sections (per frame and integrated) and the spectral-kurtosis section (plain and behind the filter
 * bank) on interleaved 8-bit I,Q as the 8-bit section above defines it: `iq8_format` (SDRK_IQ8_SIGNED / SDRK_IQ8_UNSIGNED)
 * right after the samples pointer, x[n] the exact float32 conversion given there (mid-scale 127.5 for unsigned bytes, no
 * scale), and every entry point returns the bits its complex64 counterpart returns for those widened samples — at every nfft
 * of a float32 plan, every T in [1, 32], stride, frame or group count, K, detector, out_form, scale and shift, from the device
 * entries and the host entries alike, however a host call is chunked.  Each entry point has the argument list of its _ci16
 * twin plus the format; frame_stride counts samples; a PFB buffer holds (frames - 1)*frame_stride + T*nfft samples of 2 bytes
 * each; frame starts need 2-byte alignment only, so any stride serves.  The refusals are the twins' (for the PFB forms a
 * windowed plan, an f64 plan, a plan without a prototype; k_frames < 2 for the kurtosis forms), and a format other than the two,
 * each SDRK_ERR_INVALID with a message; a plan that has refused still works.  (The kurtosis entries spell the word out: _sk names
 * the complex64 / int16 family.)
 * N = 4096 reads the bytes inside the transform: the filter bank folds them in the transform's registers (2 B/sample read from
 * device memory at frame_stride = nfft, 4 or 4/K written), plain spectral kurtosis keeps both sums there (2 + 8/K).  Other
 * lengths fold the bytes straight into the PFB staging (no widened copy of the stream), or widen chunks of at most 64 MiB for
 * the plain kurtosis, and go on as the complex64 forms do.  Behind the filter bank the kurtosis folds and transforms through
 * the per-frame route at every nfft, as its twins do.  The host entries move 2 B/sample over the link, through the copy
 * engines.  Not provided: cross-spectra, Welch, waterfall appends, double precision. */
int sdrk_exec_device_pfb_iq8(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_frames, size_t frame_stride,
                             float* d_out_db, void* stream);
int sdrk_exec_device_pfb_iq8_timed_each(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_frames, size_t frame_stride,
                                        float* d_out_db, int launches, float* each_ms);
int sdrk_exec_host_pfb_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, size_t n_frames, size_t frame_stride, float* out_db);
int sdrk_exec_fft_host_pfb_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, size_t n_frames, size_t frame_stride,
                               void* out_c64);
int sdrk_exec_device_pfb_integrated_iq8(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                        size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_pfb_integrated_iq8_timed_each(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups,
                                                   size_t k_frames, size_t frame_stride, int detector, int out_form, float scale,
                                                   float* d_out, int launches, float* each_ms);
int sdrk_exec_host_pfb_integrated_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                      size_t frame_stride, int detector, int out_form, float scale, float* out);
int sdrk_exec_device_kurtosis_iq8(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                  size_t frame_stride, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_kurtosis_iq8_timed_each(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                             size_t frame_stride, int out_form, float scale, float* d_out, int launches,
                                             float* each_ms);
int sdrk_exec_host_kurtosis_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                size_t frame_stride, int out_form, float scale, float* out);
int sdrk_exec_device_pfb_kurtosis_iq8(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                      size_t frame_stride, int out_form, float scale, float* d_out, void* stream);
int sdrk_exec_device_pfb_kurtosis_iq8_timed_each(sdrk_plan* plan, const void* d_iq8, int iq8_format, size_t n_groups,
                                                 size_t k_frames, size_t frame_stride, int out_form, float scale, float* d_out,
                                                 int launches, float* each_ms);
int sdrk_exec_host_pfb_kurtosis_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, size_t n_groups, size_t k_frames,
                                    size_t frame_stride, int out_form, float scale, float* out);

/* ---- two-channel cross-spectra: auto and cross power over K frames in one pass ----------
 * What two coherent receive channels give that one cannot: the cross term, and from it coherence (a common signal under
 * uncorrelated receiver noise) and the phase difference per bin (delay, direction, interferometry).
 * Input: a stream of ELEMENTS.  Element n holds sample n of channel 0, then sample n of channel 1 — what a 2 x 2 front end
 * delivers with both receive channels enabled, and what SigMF stores for core:num_channels = 2.  complex64 form: 4 float32
 * I0 Q0 I1 Q1, 16 bytes.  int16 form (_ci16): 4 little-endian int16, 8 bytes, x = float32(I) + i*float32(Q) exactly.  The
 * pointer is aligned to an element.  Frame f starts at ELEMENT f*frame_stride (any stride >= 1) and covers nfft elements;
 * group g is the frames [g*k_frames, (g+1)*k_frames); the buffer holds (n_groups*k_frames - 1)*frame_stride + nfft elements.
 * Sums: with A_f = fft(w*x0_f), B_f = fft(w*x1_f) (the plan's window, twiddles and shift order), A = (ar, ai), B = (br, bi)
 * per bin,
 *     paa = fmaf(ar, ar, ai*ai)      pbb = fmaf(br, br, bi*bi)          (as the integrating kernels form p)
 *     cre = (ar*br) + (ai*bi)        cim = (ai*br) - (ar*bi)            (A * conj(B); every product rounded to float32 first)
 * Saa, Sbb, Sre, Sim are plain float32 running sums of these in frame order.  No floating-point atomics.  A group that was cut
 * into slices (few groups on a large device) has its slices' sums added in slice order in float64 and rounded to float32 once.
 * Output: per group FOUR planes of nfft float32, d_out[n_groups][4][nfft], in the plan's shift order:
 *     scale*Saa/K     scale*Sbb/K     scale*Sre/K     scale*Sim/K
 * each formed as SDRK_INT_OUT_POWER forms its row from the mean.  There is no dB form and no out_form argument; the plan's eps
 * is not used.  With the same scale and k_frames >= 2, planes 0 and 1 carry the bits of plane 0 of sdrk_exec_device_sk
 * (SDRK_INT_OUT_POWER) on the de-interleaved channel, at every nfft.  Like that plane they are NOT the compensated mean of
 * SDRK_DET_MEAN.
 * Because the products are rounded on their own, swapping the channels returns the exact conjugate: planes 0 and 1 exchanged,
 * plane 2 with the same bits, plane 3 negated (as values: a zero's sign may differ).  Two identical channels give plane 3 = 0.
 * Determinism: the same input gives the same bits, from the device entry and the host entry alike, however the host call is
 * chunked.  The int16 forms return the bits of the complex64 forms on the widened elements.
 * Every float32 plan is served at every nfft, chirp-z lengths included, with the plan's window.  A prototype set with
 * sdrk_plan_set_pfb is ignored.  k_frames = 1 is allowed.
 * Refusals, each SDRK_ERR_INVALID with a message: an f64 plan, n_groups = 0 or k_frames = 0 or their product out of range,
 * frame_stride = 0, NULL pointers.  A plan that has refused still works.
 * N = 4096 transforms both channels of a frame in one kernel and keeps the four sums in its registers: 16 + 16/K bytes per
 * element through device memory from complex64, 8 + 16/K from int16.  Other lengths de-interleave chunks of frames, run the
 * plan's transform once per channel and reduce both spectra, in plan-owned staging of at most 64 MiB of spectra and 64 MiB of
 * split samples however long the stream is.
 * Not provided: filter-bank forms, double precision, waterfall appends; more than two channels and 8-bit elements are the
 * correlation-matrix calls' (sdrk_exec_*_corrmat*, the next section). */
/* device in / device out (d_out: n_groups * 4 * nfft float32), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_xspec(sdrk_plan* plan, const void* d_iq2_c64, size_t n_groups, size_t k_frames, size_t frame_stride,
                           float scale, float* d_out, void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` calls (bench harness) */
int sdrk_exec_device_xspec_timed_each(sdrk_plan* plan, const void* d_iq2_c64, size_t n_groups, size_t k_frames,
                                      size_t frame_stride, float scale, float* d_out, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked through pinned staging */
int sdrk_exec_host_xspec(sdrk_plan* plan, const void* iq2_c64, size_t n_groups, size_t k_frames, size_t frame_stride, float scale,
                         float* out);
/* the same three from int16 elements (8 bytes per element) */
int sdrk_exec_device_xspec_ci16(sdrk_plan* plan, const void* d_iq2_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                                float scale, float* d_out, void* stream);
int sdrk_exec_device_xspec_ci16_timed_each(sdrk_plan* plan, const void* d_iq2_ci16, size_t n_groups, size_t k_frames,
                                           size_t frame_stride, float scale, float* d_out, int launches, float* each_ms);
int sdrk_exec_host_xspec_ci16(sdrk_plan* plan, const void* iq2_ci16, size_t n_groups, size_t k_frames, size_t frame_stride,
                              float scale, float* out);

/* ---- correlation matrix: 2..8 coherent channels per bin over K frames ----------------------
 * What direction finding and interference nulling start from: the C x C cross-spectral matrix per bin,
 * R[i][j] = <X_i * conj(X_j)> over K frames, for the four-channel transceiver boards and the five-dongle arrays on one clock
 * that a two-channel call does not reach.  Every channel is transformed ONCE per frame (the F-X split of a correlator), where
 * C(C-1)/2 two-channel calls transform each C - 1 times.
 * Input: a stream of ELEMENTS.  Element n holds sample n of channel 0, then of channel 1, ... up to channel C - 1, for
 * `channels` = C in 2..8 — what SigMF stores for core:num_channels = C.  complex64 form: 8*C bytes per element.  int16 form
 * (_ci16): 4*C bytes, widened as the int16 calls do.  8-bit form (_iq8): 2*C bytes, `iq8_format` (SDRK_IQ8_SIGNED /
 * SDRK_IQ8_UNSIGNED) right after the samples pointer, widened exactly as the package's iq8_to_c64 and the other 8-bit modes do (cu8:
 * float32(byte) - 127.5).  The pointer is aligned to one sample of one channel — 8, 4 or 2 bytes — NOT to an element: C = 3
 * or 5 make elements of 24, 12, 6 and 40, 20, 10 bytes.  Frame f starts at ELEMENT f*frame_stride (any stride >= 1) and covers
 * nfft elements; group g is the frames [g*k_frames, (g+1)*k_frames); the buffer holds
 * (n_groups*k_frames - 1)*frame_stride + nfft elements.
 * Sums: X_c,f is the plan's transform of channel c of frame f (the plan's window, twiddles and shift order; the bits of the
 * plan's own complex spectrum of the de-interleaved channel).  Per bin the C auto sums S_cc of fmaf(r, r, i*i), and for every
 * pair i < j the sums Sre_ij + i*Sim_ij of X_i * conj(X_j) with every product rounded to float32 on its own — the expressions
 * of the two-channel section above, written once in the library.  Plain float32 running sums in frame order, no floating-point
 * atomics.  A group cut into slices has its slices' sums added in slice order in float64 and rounded to float32 once; the cut
 * is the one the two-channel call makes for the same plan, n_groups and k_frames.
 * Output: per group C*C planes of nfft float32, d_out[n_groups][C*C][nfft], in the plan's shift order: planes 0..C-1 are
 * scale*S_cc/K; after them, for the pairs (0,1), (0,2), ..., (0,C-1), (1,2), ..., (C-2,C-1) in that order, two planes each:
 * scale*Sre_ij/K, then scale*Sim_ij/K.  For C = 2 this is the two-channel layout.  There is no dB form; the plan's eps is
 * not used; k_frames = 1 is allowed; a prototype set with sdrk_plan_set_pfb is ignored.
 * Identities, as bit equalities: C = 2 returns what sdrk_exec_*_xspec returns for the same buffer; for any C and pair i < j the
 * planes (i, j, re_ij, im_ij) are the two-channel call's on the stream built from channels i and j; the int16 and 8-bit forms
 * return what the complex64 form returns for the widened elements; the host entry equals the device entry however it is
 * chunked; permuting the channels permutes the planes, im negated (as a value) where a pair's order flips.
 * Every float32 plan is served at every nfft, chirp-z lengths included.  N = 4096 reads the channels of a frame straight from
 * the element stream, one workgroup per frame, and writes their spectra to staging (complex64 above 5 channels de-interleaves
 * first: that measured faster); other lengths de-interleave chunks of frames and run the plan's transform once per channel.  A column kernel with the C*C sums of a bin in one thread's registers
 * reduces the staged spectra.  Staging is plan-owned and bounded however long the stream is: at most 64 MiB of spectra and
 * 64 MiB of split frames, or one frame of all C channels where that is larger.
 * Refusals, each SDRK_ERR_INVALID with a message: channels outside 2..8, an f64 plan, n_groups = 0 or k_frames = 0 or their
 * product out of range, frame_stride = 0, an element count or its byte size out of range, NULL pointers, an iq8_format that is
 * neither.  A plan that has refused still works.
 * Not provided: a filter-bank front end, double precision, waterfall appends, more than 8 channels, and direction-finding
 * estimators (MUSIC, Capon, ...: numpy on the matrix). */
/* device in / device out (d_out: n_groups * channels * channels * nfft float32), asynchronous on `stream` (NULL: the plan's) */
int sdrk_exec_device_corrmat(sdrk_plan* plan, const void* d_iq_c64, int channels, size_t n_groups, size_t k_frames,
                             size_t frame_stride, float scale, float* d_out, void* stream);
/* the same, timed on the plan's stream: the milliseconds of each of `launches` calls (bench harness) */
int sdrk_exec_device_corrmat_timed_each(sdrk_plan* plan, const void* d_iq_c64, int channels, size_t n_groups, size_t k_frames,
                                        size_t frame_stride, float scale, float* d_out, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays), chunked at element boundaries through pinned staging */
int sdrk_exec_host_corrmat(sdrk_plan* plan, const void* iq_c64, int channels, size_t n_groups, size_t k_frames,
                           size_t frame_stride, float scale, float* out);
/* the same three from int16 elements (4 * channels bytes per element) */
int sdrk_exec_device_corrmat_ci16(sdrk_plan* plan, const void* d_iq_ci16, int channels, size_t n_groups, size_t k_frames,
                                  size_t frame_stride, float scale, float* d_out, void* stream);
int sdrk_exec_device_corrmat_ci16_timed_each(sdrk_plan* plan, const void* d_iq_ci16, int channels, size_t n_groups,
                                             size_t k_frames, size_t frame_stride, float scale, float* d_out, int launches,
                                             float* each_ms);
int sdrk_exec_host_corrmat_ci16(sdrk_plan* plan, const void* iq_ci16, int channels, size_t n_groups, size_t k_frames,
                                size_t frame_stride, float scale, float* out);
/* the same three from 8-bit elements (2 * channels bytes per element) */
int sdrk_exec_device_corrmat_iq8(sdrk_plan* plan, const void* d_iq8, int iq8_format, int channels, size_t n_groups,
                                 size_t k_frames, size_t frame_stride, float scale, float* d_out, void* stream);
int sdrk_exec_device_corrmat_iq8_timed_each(sdrk_plan* plan, const void* d_iq8, int iq8_format, int channels, size_t n_groups,
                                            size_t k_frames, size_t frame_stride, float scale, float* d_out, int launches,
                                            float* each_ms);
int sdrk_exec_host_corrmat_iq8(sdrk_plan* plan, const void* iq8, int iq8_format, int channels, size_t n_groups, size_t k_frames,
                               size_t frame_stride, float scale, float* out);

/* ---- FIR filtering and channel extraction: tune, filter, decimate in one pass --------------
 * The way back from a spectrum to samples: tune to a channel seen in the waterfall, band-limit it, lower the rate, and hand the
 * IQ to a demodulator or to a smaller recording.  Overlap-save fast convolution in blocks of 4096 samples: forward transform,
 * multiply by the filter's frequency response, inverse transform, keep the valid samples — in one kernel, 8*4096/L bytes read
 * and 8/D written per input sample (4*4096/L from int16).  The reference has no counterpart.
 * The filter belongs to the plan, as the PFB prototype does: sdrk_plan_set_fir takes M = ntaps complex64 taps h from host
 * memory, 1 <= M <= 2049, and keeps H = DFT_4096(h zero-padded), computed once in float64 and rounded once to complex64, as a
 * plan-owned device copy of 4096 complex64 in natural bin order.  It may be set again (not while work of the plan is in
 * flight) and coexists with a prototype set by sdrk_plan_set_pfb; neither disturbs the other.
 * With D = decim (a power of two in 1..256), s = shift_bins (-2048..2047) and W4096^q = exp(-2 pi i q / 4096) from the plan's
 * own twiddle table, the device entry computes, in "valid" form,
 *     n_out  = (n_in - M)/D + 1                                  (integer division)
 *     h_s[t] = h[t] exp(+2 pi i s t / 4096)                      (realised as H rotated by s bins, H_s[k] = H[(k - s) mod 4096]: exact)
 *     v[i]   = sum_t h_s[t] x[i + M - 1 - t]                     i = 0 .. n_in - M
 *     out[m] = v[m D] W4096^((phase0 + s m D) mod 4096)          (s = 0: no mixer)
 * so the band centred on bin s of 4096 is filtered by the low-pass h, moved to DC and decimated; the phase is continuous from
 * call to call as long as the caller carries phase0 (any int, taken mod 4096).
 * Blocks: L is the largest multiple of 256 with L <= 4097 - M; block b reads input samples b L .. b L + 4095 (past n_in: zeros)
 * and yields outputs i = b L .. b L + L - 1 from its positions M - 1 .. M - 2 + L.  The inverse transform is the forward one on
 * the conjugated product, conjugated again, scaled by the exact 2^-12.
 * The host entries are the device entry applied to the virtual stream prefix || iq (prefix: M - 1 samples, NULL = zeros; with a
 * zero prefix this is lfilter(h, 1, x)): n outputs before decimation, of which those whose stream index sample0 + j is a multiple
 * of D are kept, with the mixer phase s (sample0 + j) mod 4096; *n_out receives their number.  out_c64 holds at least
 * (n + D - 1)/D complex64.  Chunked in whole blocks through the plan's pinned staging, in device memory that does not grow with
 * n; every block is the same 4096 samples as in one device call on the same virtual stream from its first kept sample.
 * Promised: the host entries return the bits of that device call however they are chunked; the int16 entries return the bits
 * of the complex64 entries on the widened samples (x = float32(I) + i float32(Q)); repeated calls return the same bits.  Not
 * promised: equal bits between different cuts of one stream into calls (the blocks differ).
 * Served: float32 plans with nfft = 4096 only; the plan's window, shift and eps are ignored.  Plans of another length return
 * SDRK_ERR_UNSUPPORTED with a message.  An f64 plan, no filter set, NULL pointers, n_in < M, decim not a power of two in 1..256
 * and shift_bins outside -2048..2047 return SDRK_ERR_INVALID with a message.  A plan that has refused still works.
 * Not provided: other block lengths, double precision, rational resampling.  Not provided by THESE entry points: fine (sub-bin) tuning
 * and decimation by an integer that is no power of two; both are the digital down-converter's (sdrk_exec_*_ddc, below). */
int sdrk_plan_set_fir(sdrk_plan* plan, int ntaps, const void* taps_c64);
/* taps of the filter set on the plan; 0 = none */
int sdrk_plan_fir_taps(const sdrk_plan* plan);
/* device in / device out (d_out_c64: n_out complex64), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_fir(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int decim, int shift_bins, int phase0,
                         void* d_out_c64, void* stream);
int sdrk_exec_device_fir_ci16(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, int decim, int shift_bins, int phase0,
                              void* d_out_c64, void* stream);
/* the complex64 form, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_fir_timed_each(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int decim, int shift_bins, int phase0,
                                    void* d_out_c64, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays) */
int sdrk_exec_host_fir(sdrk_plan* plan, const void* prefix_c64, const void* iq_c64, size_t n, int decim, int shift_bins,
                       uint64_t sample0, void* out_c64, size_t* n_out);
int sdrk_exec_host_fir_ci16(sdrk_plan* plan, const void* prefix_ci16, const void* iq_ci16, size_t n, int decim, int shift_bins,
                            uint64_t sample0, void* out_c64, size_t* n_out);

/* ---- channel bank: C tuned channels from one pass over the input ---------------------------
 * A wide-band capture rarely holds one signal of interest: six carriers in the waterfall want six narrow IQ streams.  With the
 * single call above that is six calls, each re-reading the capture and each repeating the forward transform of every block.
 * The bank call reads the input once and transforms each block once; per channel only the channel-dependent half runs (H rotated
 * by that channel's offset, the inverse transform, the mixer, the decimated store): 1 + C transforms per block instead of 2 C.
 * The filter is the one set by sdrk_plan_set_fir, shared by all channels; D = decim is common; channel c is tuned to
 * shift_bins[c] (-2048..2047, duplicates allowed) and starts its mixer at phase0[c] (any int, taken mod 4096; phase0 = NULL:
 * zeros).  1 <= n_chan <= 64.  Both arrays are host memory and are read before the call returns.
 * Channel c lies at d_out_c64 + c * out_stride complex64 (out_stride >= n_out) and holds n_out = (n_in - M)/D + 1 samples:
 * EXACTLY THE BITS of sdrk_exec_device_fir(plan, d_in, n_in, D, shift_bins[c], phase0[c], ...) on the same input — for every C,
 * M, D, set of offsets and length, from complex64 and from int16 (the bits of sdrk_exec_device_fir_ci16), and a channel with
 * offset 0 runs no mixer, as there.  Elements between n_out and out_stride are not written.
 * The host entries are the device entry on the virtual stream prefix || iq exactly as sdrk_exec_host_fir is (same prefix,
 * sample0, kept samples and *n_out, the same for every channel; channel c's mixer phase is shift_bins[c] (sample0 + j) mod 4096),
 * plane c at out_c64 + c * out_stride with out_stride >= (n + D - 1)/D; chunked in whole blocks through the same pinned staging
 * (SDRK_FIR_CHUNK_BLOCKS honoured), in device memory that does not grow with n, and returning the device entry's bits however
 * they are chunked.
 * Served and refused as the single call is, and in addition SDRK_ERR_INVALID with a message for n_chan outside 1..64, a NULL
 * shift_bins, an offset outside -2048..2047 and an out_stride below the outputs of a channel.  A plan that has refused still works.
 * Not provided: per-channel filters or decimation, more than 64 channels (the critically sampled many-channel case is the
 * polyphase filter bank's), a smaller inverse transform for D > 1.  Channels tuned finer than a bin, or decimated by another
 * integer: sdrk_exec_*_ddcbank, below. */
int sdrk_exec_device_chanbank(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int decim, int n_chan, const int* shift_bins,
                              const int* phase0, void* d_out_c64, size_t out_stride, void* stream);
int sdrk_exec_device_chanbank_ci16(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, int decim, int n_chan, const int* shift_bins,
                                   const int* phase0, void* d_out_c64, size_t out_stride, void* stream);
/* the complex64 form, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_chanbank_timed_each(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int decim, int n_chan,
                                         const int* shift_bins, const int* phase0, void* d_out_c64, size_t out_stride, int launches,
                                         float* each_ms);
/* host in / host out (pageable or pinned caller arrays) */
int sdrk_exec_host_chanbank(sdrk_plan* plan, const void* prefix_c64, const void* iq_c64, size_t n, int decim, int n_chan,
                            const int* shift_bins, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out);
int sdrk_exec_host_chanbank_ci16(sdrk_plan* plan, const void* prefix_ci16, const void* iq_ci16, size_t n, int decim, int n_chan,
                                 const int* shift_bins, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out);

/* ---- digital down-converter (DDC): exact-frequency tuning and any integer decimation, one pass ----
 * The two calls above tune to a bin of fs/4096 and decimate by a power of two.  A DDC tunes to a frequency, low-passes and
 * decimates: here by a 32-bit frequency word (steps of fs/2^32: 0.014 Hz at 61.44 Msps) and by any integer D = decim in 1..256
 * (2.4 Msps -> 48 kHz is D = 50), in the same single pass, as a single call and as the C-channel bank, from complex64 and from
 * int16.  The filter is the one sdrk_plan_set_fir sets (M taps, L as above); block b reads samples b L .. b L + 4095 and the
 * forward and inverse transforms, the product with H and the exact 2^-12 scaling are those of the FIR call, in its order.
 *   freq_word  uint32_t: the tuned frequency is int32(freq_word) / 2^32 cycles per input sample.
 *   decim      D, any integer 1 <= D <= 256.
 *   index0     uint64_t: the stream index of valid-convolution output i = 0.
 * Filter centre: s = ((freq_word + 0x80000) >> 20) & 4095, the nearest bin; H is rotated by s bins as above.  So the FILTER is
 * centred within fs/8192 of the tuned frequency (half a bin: leave the pass band that much room), while the SIGNAL at the tuned
 * frequency lands at DC exactly.
 * Kept samples: with v[i] the filtered sample as above, i = 0 .. n_in - M, output i is kept iff (index0 + i) % D == 0, and the
 * kept samples are stored in ascending i.  With i_first = (D - index0 % D) % D,
 *     n_out = i_first > n_in - M ? 0 : (n_in - M - i_first)/D + 1
 * which sdrk_ddc_outputs(n_in, taps, decim, index0) returns (0 for taps < 1, n_in < taps or decim outside 1..256).  n_out = 0
 * is a successful no-op.
 * Mixer: out = v[i] f, f = exp(-2 pi i phase / 2^32) formed as
 *     phase = freq_word * (uint32)(index0 + i)             (uint32 wrap-around: exact mod 2^32)
 *     q = phase >> 20;  r = phase & 0xFFFFF;  W = W4096^q  (the plan's twiddle table)
 *     r == 0:  f = W
 *     else:    a = (float)r * 0x1.921fb6p-30f              (2 pi 2^-32 rounded to float32)
 *              c = fmaf(-0.5f a, a, 1.0f);  t = (a a) (1.0f/6.0f);  sn = fmaf(-t, a, a);  f = W (c - i sn)
 * with the complex products of the FIR call's mixer (c is within 2^-25 of cos a and sn within 1.6e-10 of sin a for every r).
 * freq_word == 0 runs no mixer at all: -0.0, Inf and NaN pass as they are.  A freq_word that is a multiple of 2^20, with D a
 * power of two and index0 a multiple of D, gives the bits of sdrk_exec_device_fir with shift_bins = int32(freq_word) >> 20 and
 * phase0 = shift_bins index0 mod 4096.
 * Host entries: the device entry on the virtual stream prefix || iq (prefix: M - 1 samples, NULL = zeros) with index0 = sample0:
 * output j has stream index sample0 + j; out holds at least (n + D - 1)/D samples; *n_out receives the count.  Chunked in whole
 * blocks through the same pinned staging slots (SDRK_FIR_CHUNK_BLOCKS honoured); device memory does not grow with n.
 * Bank: 1 <= n_chan <= 64, freq_word[c] per channel (host memory, read before the call returns), D and index0 shared, plane c at
 * out + c out_stride (out_stride >= n_out; the host entries: >= (n + D - 1)/D); elements behind n_out are not written.
 * Promised: the host entries return the bits of the device entry however they are chunked; the int16 entries return the bits of
 * the complex64 entries on the widened samples; plane c of the bank carries the bits of the single call with freq_word[c];
 * repeated calls return the same bits.  Not promised: equal bits between different cuts of one stream into calls.
 * Served and refused as the FIR call is (float32 plans with nfft = 4096 only); in addition decim outside 1..256, n_chan outside
 * 1..64, a NULL freq_word array and a short out_stride return SDRK_ERR_INVALID with a message.  A plan that has refused still
 * works.  Not provided: rational (non-integer) resampling, per-channel filters or decimation, D above 256, double precision. */
size_t sdrk_ddc_outputs(size_t n_in, int taps, int decim, uint64_t index0);
/* device in / device out (d_out_c64: n_out complex64), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_ddc(sdrk_plan* plan, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                         void* d_out_c64, void* stream);
int sdrk_exec_device_ddc_ci16(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                              void* d_out_c64, void* stream);
/* the complex64 form, timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_ddc_timed_each(sdrk_plan* plan, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim,
                                    uint64_t index0, void* d_out_c64, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays) */
int sdrk_exec_host_ddc(sdrk_plan* plan, const void* prefix_c64, const void* iq_c64, size_t n, uint32_t freq_word, int decim,
                       uint64_t sample0, void* out_c64, size_t* n_out);
int sdrk_exec_host_ddc_ci16(sdrk_plan* plan, const void* prefix_ci16, const void* iq_ci16, size_t n, uint32_t freq_word, int decim,
                            uint64_t sample0, void* out_c64, size_t* n_out);
/* the bank */
int sdrk_exec_device_ddcbank(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                             uint64_t index0, void* d_out_c64, size_t out_stride, void* stream);
int sdrk_exec_device_ddcbank_ci16(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, int n_chan, const uint32_t* freq_word,
                                  int decim, uint64_t index0, void* d_out_c64, size_t out_stride, void* stream);
int sdrk_exec_device_ddcbank_timed_each(sdrk_plan* plan, const void* d_in_c64, size_t n_in, int n_chan, const uint32_t* freq_word,
                                        int decim, uint64_t index0, void* d_out_c64, size_t out_stride, int launches,
                                        float* each_ms);
int sdrk_exec_host_ddcbank(sdrk_plan* plan, const void* prefix_c64, const void* iq_c64, size_t n, int n_chan,
                           const uint32_t* freq_word, int decim, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out);
int sdrk_exec_host_ddcbank_ci16(sdrk_plan* plan, const void* prefix_ci16, const void* iq_ci16, size_t n, int n_chan,
                                const uint32_t* freq_word, int decim, uint64_t sample0, void* out_c64, size_t out_stride,
                                size_t* n_out);

/* ---- the down-converter from 8-bit input: ci8 / cu8 recordings, 2 bytes per sample ----
 * The single call and the bank of the section above reading interleaved 8-bit I,Q as a HackRF (ci8) or an RTL-SDR (cu8) writes
 * it, the bytes read inside the overlap-save transform: 2*4096/L + 8/D bytes per input sample, where int16 moves 4*4096/L and
 * complex64 8*4096/L.  `iq8_format` (SDRK_IQ8_SIGNED / SDRK_IQ8_UNSIGNED, as for the 8-bit spectra) sits right after the samples
 * pointer; every other argument, sdrk_ddc_outputs and every refusal are those of the _ci16 twin (the timed entries: of the
 * complex64 ones), and a format other than the two returns SDRK_ERR_INVALID with the message of the 8-bit spectra.  Buffers need
 * 2-byte alignment only.
 * Promised: an 8-bit call returns the bits of the complex64 call on the widened samples (x[n] as the 8-bit section defines it),
 * for every tap count, freq_word, decim, index0 and n_chan, device and host entries alike, however a host call is chunked.  That
 * includes the last block of a call: positions past n_in count as +0.0 + 0.0i for both formats, as they do for complex64 (and
 * not as byte 0, which is -127.5 for cu8).
 * Host entries, NULL prefix: M - 1 samples of byte value 0 for SDRK_IQ8_SIGNED and of byte value 0x80 for SDRK_IQ8_UNSIGNED.
 * No cu8 byte widens to zero; 0x80 is the nearer mid-scale byte and widens to +0.5 + 0.5i (byte 0 would mean -127.5 - 127.5i).
 * So a cu8 host call with a NULL prefix equals the complex64 host call given M - 1 samples of 0.5 + 0.5i as its prefix, and a
 * ci8 one the complex64 call with a NULL prefix.
 * The bin-tuned FIR / channel-bank calls have no 8-bit form: a freq_word on a bin with a power-of-two decim gives their bits. */
int sdrk_exec_device_downconv_iq8(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word, int decim,
                                  uint64_t index0, void* d_out_c64, void* stream);
int sdrk_exec_device_downconv_iq8_timed_each(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word,
                                             int decim, uint64_t index0, void* d_out_c64, int launches, float* each_ms);
int sdrk_exec_host_downconv_iq8(sdrk_plan* plan, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n,
                                uint32_t freq_word, int decim, uint64_t sample0, void* out_c64, size_t* n_out);
int sdrk_exec_device_downconvbank_iq8(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, int n_chan,
                                      const uint32_t* freq_word, int decim, uint64_t index0, void* d_out_c64, size_t out_stride,
                                      void* stream);
int sdrk_exec_device_downconvbank_iq8_timed_each(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, int n_chan,
                                                 const uint32_t* freq_word, int decim, uint64_t index0, void* d_out_c64,
                                                 size_t out_stride, int launches, float* each_ms);
int sdrk_exec_host_downconvbank_iq8(sdrk_plan* plan, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n, int n_chan,
                                    const uint32_t* freq_word, int decim, uint64_t sample0, void* out_c64, size_t out_stride,
                                    size_t* n_out);

/* ---- measurement probes (bench harness; no reference counterpart) ----------
 * sdrk_stream_ceiling_probe: a plain streaming kernel with the spectrum path's traffic
 *   shape at N = 4096 (32 KiB read + 16 KiB written per frame, no arithmetic), timed per
 *   launch on device buffers the caller provides (d_in: n*32 KiB, d_out: n*16 KiB) — the
 *   "measured-copy" ceiling SURVEY.md §8(d) asks to be reported next to the nominal 8 TB/s.
 * sdrk_copy_probe: a plain 1:1 copy of `bytes` (16 bytes per lane each way, non-temporal) from d_in to
 *   d_out, timed per launch — the shape MI355X_MICROARCH.md quotes 6.29 TB/s for; run on the same buffers it
 *   anchors the 2:1 probe above to a published figure (fastest of three grid sizes).  Bandwidth = 2 * bytes / time.
 *   Both probes deal their frames (the copy: 16 KiB units) to the workgroups in the order an N = 4096 plan created
 *   at that moment would take for a full grid (by ticket; SDRK_F4K_ORDER=stride keeps their grid-stride loops).
 * sdrk_host_link_probe: pinned-memory DMA rates in GB/s — `bytes` host-to-device, bytes/2
 *   device-to-host, and both at once (quoted on the upstream bytes): what the numpy
 *   boundary could reach at best.
 * sdrk_host_threads: helper threads of the host staging pool (SDRK_HOST_THREADS overrides). */
int sdrk_stream_ceiling_probe(int device, const void* d_in, void* d_out, size_t n_frames4096,
                              int launches, float* each_ms);
int sdrk_copy_probe(int device, const void* d_in, void* d_out, size_t bytes, int launches, float* each_ms);
int sdrk_host_link_probe(int device, size_t bytes, double* h2d_gbps, double* d2h_gbps,
                         double* duplex_gbps);
int sdrk_host_threads(void);

/* ---- synthetic IQ generator (bench / parity input, device resident) ------
 * Sample n of frame F (F = first_frame + f, 64-bit) is
 *     h = fmix32( fmix32(seed ^ lo32(F)) ^ fmix32(hi32(F) + 0x9E3779B1) ^ n )
 *     I = (h & 0xFFF) - 2048,  Q = ((h >> 12) & 0xFFF) - 2048      (as float32)
 * i.e. 12-bit integers like the AD9363 behind streamer.py:114, bit-identical
 * to the numpy generator in the host package (synth.py). */
int sdrk_synth_fill(int device, uint32_t seed, uint64_t first_frame, size_t n_frames,
                    int nfft, void* d_iq_c64, void* stream);

/* ---- per-row reductions for the spectrum's first consumer ------------------
 * The O(N) measurements of the reference's classifier helpers
 * (app/processing/classifier.py:163-212) computed next to the rows, so that a
 * consumer needs ~20 scalars per row instead of the row.  `rows` is n_rows*nfft
 * float32, on the host (rows_on_device = 0) or already on `device` (non-zero, e.g.
 * the output of sdrk_exec_device).
 *
 * stats: out[r*16 + i] (double), i =
 *   0 max | 1 sorted[rank] | 2 sorted[rank+1] (order statistics of the row, for the
 *   percentile noise floor, classifier.py:179-181) | 3 mean | 4 mean (x-mean)^2 |
 *   5 mean (x-mean)^4 (:191-198) | 6 mean ln p | 7 mean p, p = max(10^(x/10), 1e-15)
 *   (:183-189) | 8,9 first,last index with x >= max-3 | 10,11 ... max-10 | 12,13 ...
 *   max-20 (:163-170) | 14 argmax | 15 nfft.
 * thr: the adaptive peak threshold of classifier.py:55, max(noise_floor + 5,
 *   max - 0.9*snr + 5), with the percentile interpolated as numpy.percentile does on a
 *   float32 row: noise_floor = sorted[rank] + (sorted[rank+1]-sorted[rank])*gamma
 *   (`rank`, `gamma` = floor and fraction of float32(nfft-1)*float32(q/100)).
 * peaks: strict local maxima above the threshold, accepted left to right when
 *   >= min_distance bins after the previous accepted one (:200-212).
 *   out_idx: n_rows*max_peaks int32 (first max_peaks peaks of each row; the host entry points
 *   sdrk_row_features / sdrk_frame_features_host fill the unused slots with -1),
 *   out_count: n_rows int32 (may exceed max_peaks: the total found).
 *
 * sdrk_row_features: everything in ONE launch that reads each row from HBM once (rows up
 *   to 32768 bins are staged in LDS; longer rows are scanned in place); out_thr, out_idx
 *   and out_count may be NULL (then only the stats are produced).
 * sdrk_row_stats / sdrk_row_peaks: the two halves separately (sdrk_row_peaks takes the
 *   thresholds from the caller). */
int sdrk_row_features(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft,
                      int rank, float gamma, int min_distance, int max_peaks, double* out_stats,
                      double* out_thr, int32_t* out_idx, int32_t* out_count);
int sdrk_row_stats(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft,
                   int rank, double* out);
int sdrk_row_peaks(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft,
                   const double* thresholds, int min_distance, int max_peaks, int32_t* out_idx,
                   int32_t* out_count);

/* IQ frames -> those measurements, the rows staying on the device (streamer.py:119,121
 * followed by classifier.py:163-212).  For nfft = 4096 the reductions run as the epilogue
 * of the transform kernel itself: the row exists only in LDS unless the caller passes a
 * buffer for it.  _device: every pointer is device memory, asynchronous on `stream` (or
 * the plan's stream); d_out_db, d_thr, d_idx/d_count may be NULL.  _host: host pointers,
 * blocking; out_db (the rows) may be NULL; batches of more than 32 MiB of IQ stream through the
 * pinned staging of sdrk_exec_host in chunks (pinned caller arrays are read in place). */
int sdrk_frame_features_device(sdrk_plan* plan, const void* d_iq_c64, size_t n_frames,
                               size_t frame_stride, float* d_out_db, int rank, float gamma,
                               int min_distance, int max_peaks, double* d_stats, double* d_thr,
                               int32_t* d_idx, int32_t* d_count, void* stream);
int sdrk_frame_features_host(sdrk_plan* plan, const void* iq_c64, size_t n_frames,
                             size_t frame_stride, int rank, float gamma, int min_distance,
                             int max_peaks, double* out_stats, double* out_thr, int32_t* out_idx,
                             int32_t* out_count, float* out_db);

/* The same measurements FINISHED on the device, for a whole batch: what classify_signal_advanced forms from its helpers'
 * results before the rule ladder (classifier.py:45-58) as planes of n_rows 8-byte words — the host receives arrays, not
 * packed per-row records that it then has to post-process row by row.  out_planes: SDRK_FEAT_PLANES * n_rows words;
 * plane P, row r at out_planes[P * n_rows + r]:
 *   double planes   SDRK_FEAT_MAX_DB                np.max(power_db)                                    (:46)
 *                   SDRK_FEAT_NOISE_FLOOR_DB        np.percentile(power_db, q) as numpy forms it on a float32 row (:179-181)
 *                   SDRK_FEAT_SNR_DB                float32(max - noise floor)                          (:46)
 *                   SDRK_FEAT_FLATNESS              clip(exp(mean ln p) / mean p, 0, 1)                 (:183-189)
 *                   SDRK_FEAT_KURTOSIS              0 if sigma < 1e-9 else m4 / m2^2                    (:191-198)
 *                   SDRK_FEAT_THRESHOLD_DB          the adaptive peak threshold                         (:55)
 *                   SDRK_FEAT_PEAK_SPACING_STD_HZ   np.std(np.diff(freqs[peaks])) over the kept peaks, 0 for < 3 (:214-219)
 *                   SDRK_FEAT_PEAK_DENSITY          peak_count / nfft                                   (:58)
 *                   SDRK_FEAT_BANDWIDTH_HZ + j      freqs[last] - freqs[first] of the bins within 3 / 10 / 20 dB (j = 0, 1, 2)
 *                                                   of the maximum, 0.0 when no bin qualifies           (:163-170)
 *   int64 planes    SDRK_FEAT_ARGMAX, SDRK_FEAT_PEAK_COUNT (total found; may exceed max_peaks)
 *                   SDRK_FEAT_OCCUPIED_BINS + 2 j   the (first, last) bin pairs behind bandwidth j: 2 * n_rows words,
 *                                                   row r at [2 r], [2 r + 1]
 * freqs: the nfft float64 bin frequencies (streamer.py:120), host memory; NULL: the three Hz quantities are 0.
 * out_idx (n_rows * max_peaks int32, unused slots -1) may be NULL: then no peaks are looked for (count 0). */
enum {
    SDRK_FEAT_MAX_DB = 0, SDRK_FEAT_NOISE_FLOOR_DB, SDRK_FEAT_SNR_DB, SDRK_FEAT_FLATNESS, SDRK_FEAT_KURTOSIS,
    SDRK_FEAT_THRESHOLD_DB, SDRK_FEAT_PEAK_SPACING_STD_HZ, SDRK_FEAT_PEAK_DENSITY, SDRK_FEAT_BANDWIDTH_HZ /* 3 planes */,
    SDRK_FEAT_ARGMAX = 11, SDRK_FEAT_PEAK_COUNT, SDRK_FEAT_OCCUPIED_BINS /* 6 planes */, SDRK_FEAT_PLANES = 19
};
int sdrk_row_features_planes(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft,
                             int rank, float gamma, int min_distance, int max_peaks, const double* freqs,
                             void* out_planes, int32_t* out_idx);
int sdrk_frame_features_host_planes(sdrk_plan* plan, const void* iq_c64, size_t n_frames, size_t frame_stride,
                                    int rank, float gamma, int min_distance, int max_peaks, const double* freqs,
                                    void* out_planes, int32_t* out_idx, float* out_db);

/* ---- waterfall ring -------------------------------------------------------
 * Replaces deque(maxlen=100) / append / np.array(deque) at
 * dashboard/callbacks.py:19,176,182: a device-resident ring of the last
 * `maxlen` rows of nfft float32, read out oldest row first. */
int sdrk_waterfall_create(int device, int nfft, int maxlen, sdrk_waterfall** out);
int sdrk_waterfall_destroy(sdrk_waterfall* wf);
/* Append n_rows precomputed rows (host float32, n_rows*nfft). */
int sdrk_waterfall_append_rows(sdrk_waterfall* wf, const float* rows, size_t n_rows);
/* Transform n_frames host IQ frames with `plan` and append the resulting rows
 * without a host round trip of the rows (plan nfft/device must match). */
int sdrk_waterfall_append_iq(sdrk_waterfall* wf, sdrk_plan* plan, const void* iq_c64,
                             size_t n_frames, size_t frame_stride);
/* Same, IQ already on the device. */
int sdrk_waterfall_append_iq_device(sdrk_waterfall* wf, sdrk_plan* plan,
                                    const void* d_iq_c64, size_t n_frames,
                                    size_t frame_stride);
/* The same without waiting: the transforms are only enqueued on the ring's stream.  Every later call on this
 * waterfall (append, read, read_decimated, sync, destroy) is ordered behind them; d_iq_c64 must stay valid and
 * unmodified until one of those has returned after waiting (read, read_decimated, _end, sync). */
int sdrk_waterfall_append_iq_device_async(sdrk_waterfall* wf, sdrk_plan* plan, const void* d_iq_c64,
                                          size_t n_frames, size_t frame_stride);
/* Wait for everything enqueued on the ring's stream (`plan`, if not NULL: also report its launches' errors). */
int sdrk_waterfall_sync(sdrk_waterfall* wf, sdrk_plan* plan);
/* Number of valid rows (<= maxlen). */
int sdrk_waterfall_rows(const sdrk_waterfall* wf);
/* Copy the valid rows, oldest first, into out (capacity max_rows rows); the
 * number written is returned through n_rows.  If fewer than rows() fit, the
 * NEWEST max_rows are returned (still oldest-of-those first). */
int sdrk_waterfall_read(sdrk_waterfall* wf, float* out, size_t max_rows, size_t* n_rows);
/* Decimated read-out for display: like sdrk_waterfall_read, but every run of `factor`
 * consecutive bins is reduced on the device to one value — mode 0 = max (peak hold),
 * mode 1 = mean of the dB values — so `out` holds rows of nfft/factor float32.  factor
 * must divide nfft.  (Build-side extension: the reference plots full rows,
 * dashboard/callbacks.py:182-190, which is unusable at nfft = 2^20.) */
int sdrk_waterfall_read_decimated(sdrk_waterfall* wf, float* out, size_t max_rows, int factor, int mode,
                                  size_t* n_rows);
/* For nfft = 2^20 ... 2^22 the transform behind sdrk_waterfall_append_iq* also leaves every row max-hold-decimated by 16
 * beside the ring (1/16 of its size; the row pass has the sixteen neighbouring bins in LDS anyway), and a max-mode read-out
 * whose factor is a multiple of 16 is served from those — it reads 1/16 of the bytes instead of every 4 MiB row again, with
 * bit-identical results (a maximum does not depend on the order).  Rows appended as finished rows carry no such companion;
 * a read-out that touches one falls back to the full rows.  Returns how many of the valid rows carry one. */
int sdrk_waterfall_maxhold16_rows(const sdrk_waterfall* wf);
/* sdrk_waterfall_read_decimated in two halves, for a continuous channel (BASELINE config 5): _begin enqueues the
 * reduction behind everything appended so far and the device-to-host copy of its result on a second stream, and
 * returns; _end waits for that copy.  Between the two the caller can enqueue the next batch of frames
 * (sdrk_waterfall_append_iq_device_async), whose transform then runs while the previous batch's rows cross PCIe.
 * `out` must stay valid until _end (pinned memory makes the copy truly asynchronous).  The reduction itself runs on that
 * second stream too (behind an event), so the transform stream goes straight on; a later append waits for it only if it
 * overwrites ring rows still being reduced.  Up to TWO reads may be in flight per waterfall — _end completes the OLDEST —
 * so that a channel can enqueue batch i + 1 and begin its read-out before it collects batch i - 1 (the GPU then never
 * waits for the host); a third _begin is refused.  n_rows is known at _begin. */
int sdrk_waterfall_read_decimated_begin(sdrk_waterfall* wf, float* out, size_t max_rows, int factor, int mode,
                                        size_t* n_rows);
int sdrk_waterfall_read_decimated_end(sdrk_waterfall* wf);
int sdrk_waterfall_clear(sdrk_waterfall* wf);

/* ---- filter-and-sum beamformer: 1..8 coherent channels in, one channel out, one pass ----------
 * Applies per-channel filters to a stream of C-channel ELEMENTS (one sample of every channel: I0 Q0 I1 Q1 ..., the layout of the
 * correlation matrix calls) and returns the SUM, tuned and decimated as the down-converter does it:
 *     v[i] = sum_c sum_t h_c,s[t] x_c[i + M - 1 - t]           h_c,s: channel c's taps, rotated to s as the DDC section says
 * followed by that section's mixer and keeping.  A single complex weight per channel is h_c = conj(w_c) h (y = w^H x, then the
 * shared filter h); per-channel taps also serve true-time-delay and frequency-dependent weights.  Per block of 4096 elements
 * every channel is transformed once and ONE transform comes back: C + 1 transforms where C down-converter calls run 2 C, the
 * stream read once at 8, 4 or 2 bytes per sample, nothing staged in device memory.
 * The plan owns the filters: sdrk_plan_set_beam(plan, channels, ntaps, taps_c64) takes `channels` x `ntaps` complex64,
 * row-major, 1 <= channels <= 8, 1 <= ntaps <= 2049, on float32 plans with nfft = 4096 (others: as sdrk_plan_set_fir refuses
 * them).  Row c goes through sdrk_plan_set_fir's own computation, so H_c carries the bits that call gives h_c.  The beam filters
 * and the FIR filter are separate state: neither call touches the other's.  sdrk_plan_beam_channels / sdrk_plan_beam_taps
 * return C and M, 0 while no beam is set.  Not with work of the plan in flight.
 * Calls: the argument lists of sdrk_exec_*_ddc / _ddc_ci16 / _downconv_iq8, with n_in, n and the prefix counted in ELEMENTS
 * (a prefix is M - 1 elements); n_out = sdrk_ddc_outputs(n_in, M, decim, index0).  The stream needs the alignment of one sample.
 * Arithmetic, per block and in this order for c = 0 .. C - 1: X_c = the plan's transform of channel c (widened), z_c = the
 * product with H_c rotated by s, ROUNDED as the single-channel call rounds it; u = z_0, then u = u + z_c as plain float32 adds
 * per component; then the transform again, the 2^-12 scaling, the mixer (none for freq_word == 0) and the keeping of the DDC.
 * Positions at or past n_in count as +0.0 + 0.0i in every channel, for cu8 too.  Host entries, NULL prefix: M - 1 elements of
 * byte 0, of byte 0x80 for SDRK_IQ8_UNSIGNED.
 * Promised: C = 1 returns the bits of sdrk_exec_*_ddc* on a plan whose FIR filter is h_0; the int16 and 8-bit entries return
 * the bits of the complex64 entry on the widened elements; a host entry returns the bits of the device entry on prefix || iq
 * however it is chunked (SDRK_FIR_CHUNK_BLOCKS honoured; device memory does not grow with n); repeated calls return the same
 * bits.  Not promised: equal bits between different cuts of one stream into calls, or between channel orders for C > 2.
 * Refused with SDRK_ERR_INVALID and a message: no beam set (the message names sdrk_plan_set_beam), channels outside 1..8,
 * ntaps outside 1..2049, decim outside 1..256, n_in < M, NULL pointers, an iq8_format other than the two (the 8-bit spectra's
 * message), launches < 1; other plans as for the FIR call.  A plan that has refused still works.
 * Not provided: several beams per call, more than 8 channels, other lengths, double precision. */
int sdrk_plan_set_beam(sdrk_plan* plan, int channels, int ntaps, const void* taps_c64);
int sdrk_plan_beam_channels(const sdrk_plan* plan);
int sdrk_plan_beam_taps(const sdrk_plan* plan);
/* device in / device out (d_out_c64: n_out complex64), asynchronous on `stream` (NULL: the plan's stream) */
int sdrk_exec_device_beam(sdrk_plan* plan, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                          void* d_out_c64, void* stream);
int sdrk_exec_device_beam_ci16(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                               void* d_out_c64, void* stream);
int sdrk_exec_device_beam_iq8(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word, int decim,
                              uint64_t index0, void* d_out_c64, void* stream);
/* timed on the plan's stream: the milliseconds of each of `launches` launches (bench harness) */
int sdrk_exec_device_beam_timed_each(sdrk_plan* plan, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim,
                                     uint64_t index0, void* d_out_c64, int launches, float* each_ms);
int sdrk_exec_device_beam_ci16_timed_each(sdrk_plan* plan, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim,
                                          uint64_t index0, void* d_out_c64, int launches, float* each_ms);
int sdrk_exec_device_beam_iq8_timed_each(sdrk_plan* plan, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word,
                                         int decim, uint64_t index0, void* d_out_c64, int launches, float* each_ms);
/* host in / host out (pageable or pinned caller arrays) */
int sdrk_exec_host_beam(sdrk_plan* plan, const void* prefix_c64, const void* iq_c64, size_t n, uint32_t freq_word, int decim,
                        uint64_t sample0, void* out_c64, size_t* n_out);
int sdrk_exec_host_beam_ci16(sdrk_plan* plan, const void* prefix_ci16, const void* iq_ci16, size_t n, uint32_t freq_word, int decim,
                             uint64_t sample0, void* out_c64, size_t* n_out);
int sdrk_exec_host_beam_iq8(sdrk_plan* plan, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n,
                            uint32_t freq_word, int decim, uint64_t sample0, void* out_c64, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* SDRK_H */

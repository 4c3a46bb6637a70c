// sdrk_waterfall.hip — the waterfall ring of include/sdrk.h (sdrk_waterfall_*): rows resident on the device, appended as
// finished rows or written in place by a plan's transform, read out whole or decimated on a second stream.  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "kernels.h"
#include "plan_internal.h"

using namespace sdrk_host;

struct sdrk_waterfall {
    int device = 0;
    int nfft = 0;
    int maxlen = 0;
    float* d_ring = nullptr;  // maxlen * nfft float32
    size_t head = 0;          // slot the next row is written to
    size_t count = 0;         // valid rows (<= maxlen)
    hipStream_t stream = nullptr;
    // decimated read-out staging (only grows).  Slot 0 also serves the one-call form (sdrk_waterfall_read_decimated).
    void* d_dec[2] = {nullptr, nullptr};
    size_t dec_cap[2] = {0, 0};
    // two-phase decimated read-out, up to TWO in flight (a channel that enqueues batch i + 1 before it collects batch i - 1 keeps
    // the transform stream fed): the reduction AND the copy run on a second stream behind the transform that produced the rows
    // (ev_dec = "rows written", recorded on `stream`), so the transform stream goes straight on with the next batch;
    // ev_dec_done[k] = "reduction k finished with the ring" (recorded on s_copy): a later write into ring slots [dec_start[k],
    // dec_start[k] + dec_rows[k]) waits for it (wf_before_write) — in a running channel those are the newest rows and the next
    // batch lands elsewhere, so nothing waits; ev_copy_done[k] = its rows are in the caller's array.
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_dec = nullptr, ev_dec_done[2] = {nullptr, nullptr}, ev_copy_done[2] = {nullptr, nullptr};
    int reads_in_flight = 0, oldest_read = 0;
    bool dec_guard[2] = {false, false};
    size_t dec_start[2] = {0, 0}, dec_rows[2] = {0, 0};
    // frame lengths whose transform can write them (sdrk::fft_tiled2_has_mip): every ring row max-hold-decimated by 16,
    // maxlen * nfft / 16 float32, written by the row pass beside the row itself; mip_ok[slot] = that slot's row came from
    // sdrk_waterfall_append_iq* (rows appended as finished rows have none)
    float* d_mip_ring = nullptr;
    std::vector<unsigned char> mip_ok;
};

extern "C" {

int sdrk_waterfall_create(int device, int nfft, int maxlen, sdrk_waterfall** out) {
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (nfft < 1) return fail(SDRK_ERR_INVALID, "nfft must be >= 1");
    if (maxlen < 1) return fail(SDRK_ERR_INVALID, "maxlen must be >= 1");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    sdrk_waterfall* wf = new (std::nothrow) sdrk_waterfall();
    if (!wf) return fail(SDRK_ERR_NOMEM, "out of host memory");
    wf->device = device;
    wf->nfft = nfft;
    wf->maxlen = maxlen;
    hipError_t e = hipMalloc((void**)&wf->d_ring, (size_t)maxlen * nfft * sizeof(float));
    if (e == hipSuccess && sdrk::fft_tiled2_has_mip(nfft, sdrk::EPI_LOGPSD)) {
        // 1/16 of the ring again: the rows max-hold-decimated by 16, written by the transform beside the rows (N >= 2^20)
        e = hipMalloc((void**)&wf->d_mip_ring, (size_t)maxlen * (nfft / 16) * sizeof(float));
        // -inf everywhere: should a slot ever be read before the transform has written it, a maximum over it is harmless
        if (e == hipSuccess) e = hipMemsetD32(wf->d_mip_ring, (int)0xFF800000u, (size_t)maxlen * (size_t)(nfft / 16));
        wf->mip_ok.assign((size_t)maxlen, 0);
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&wf->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        int s = fail(e == hipErrorOutOfMemory ? SDRK_ERR_NOMEM : SDRK_ERR_HIP,
                     "waterfall allocation failed: %s", hipGetErrorString(e));
        sdrk_waterfall_destroy(wf);
        return s;
    }
    *out = wf;
    return SDRK_OK;
}

int sdrk_waterfall_destroy(sdrk_waterfall* wf) {
    if (!wf) return SDRK_OK;
    (void)hipSetDevice(wf->device);
    if (wf->s_copy) {
        (void)hipStreamSynchronize(wf->s_copy);
        (void)hipStreamDestroy(wf->s_copy);
    }
    if (wf->ev_dec) (void)hipEventDestroy(wf->ev_dec);
    for (int k = 0; k < 2; ++k) {
        if (wf->ev_dec_done[k]) (void)hipEventDestroy(wf->ev_dec_done[k]);
        if (wf->ev_copy_done[k]) (void)hipEventDestroy(wf->ev_copy_done[k]);
    }
    if (wf->stream) {
        (void)hipStreamSynchronize(wf->stream);
        (void)hipStreamDestroy(wf->stream);
    }
    if (wf->d_ring) (void)hipFree(wf->d_ring);
    if (wf->d_mip_ring) (void)hipFree(wf->d_mip_ring);
    for (int k = 0; k < 2; ++k)
        if (wf->d_dec[k]) (void)hipFree(wf->d_dec[k]);
    delete wf;
    return SDRK_OK;
}

int sdrk_waterfall_rows(const sdrk_waterfall* wf) {
    return wf ? (int)wf->count : fail(SDRK_ERR_INVALID, "waterfall is NULL");
}

int sdrk_waterfall_maxhold16_rows(const sdrk_waterfall* wf) {
    if (!wf) return fail(SDRK_ERR_INVALID, "waterfall is NULL");
    if (wf->mip_ok.empty()) return 0;
    int n = 0;
    const size_t L = (size_t)wf->maxlen, start = (wf->head + L - wf->count % L) % L;
    for (size_t r = 0; r < wf->count; ++r) n += wf->mip_ok[(start + r) % L] ? 1 : 0;
    return n;
}

int sdrk_waterfall_clear(sdrk_waterfall* wf) {
    if (!wf) return fail(SDRK_ERR_INVALID, "waterfall is NULL");
    wf->head = 0;
    wf->count = 0;
    return SDRK_OK;
}

// Before `run` ring slots from wf->head are overwritten on wf->stream: if the second stream's reduction may still be reading
// any of them, the write waits for it.
static hipError_t wf_before_write(sdrk_waterfall* wf, size_t run) {
    if (run == 0) return hipSuccess;
    const size_t L = (size_t)wf->maxlen;
    for (int k = 0; k < 2; ++k) {
        if (!wf->dec_guard[k]) continue;
        const size_t a0 = wf->head, b0 = wf->dec_start[k];    // both ranges may wrap: compare slot by modular distance
        const bool overlap = ((b0 + L - a0) % L) < run || ((a0 + L - b0) % L) < wf->dec_rows[k];
        if (!overlap) continue;
        wf->dec_guard[k] = false;                             // (a stream waits for an event once; later writes are behind it)
        const hipError_t e = hipStreamWaitEvent(wf->stream, wf->ev_dec_done[k], 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static void wf_advance(sdrk_waterfall* wf, size_t rows) {
    wf->head = (wf->head + rows) % (size_t)wf->maxlen;
    wf->count = wf->count + rows > (size_t)wf->maxlen ? (size_t)wf->maxlen : wf->count + rows;
}

int sdrk_waterfall_append_rows(sdrk_waterfall* wf, const float* rows, size_t n_rows) {
    if (!wf) return fail(SDRK_ERR_INVALID, "waterfall is NULL");
    if (n_rows == 0) return SDRK_OK;
    if (!rows) return fail(SDRK_ERR_INVALID, "rows is NULL");
    HIP_TRY(hipSetDevice(wf->device));
    // deque(maxlen) semantics (dashboard/callbacks.py:19,176): only the newest maxlen survive.
    size_t skip = n_rows > (size_t)wf->maxlen ? n_rows - (size_t)wf->maxlen : 0;
    if (skip) wf_advance(wf, skip);
    const size_t row_bytes = (size_t)wf->nfft * sizeof(float);
    size_t done = skip;
    while (done < n_rows) {
        size_t run = (size_t)wf->maxlen - wf->head;
        if (run > n_rows - done) run = n_rows - done;
        HIP_TRY(wf_before_write(wf, run));
        HIP_TRY(hipMemcpyAsync(wf->d_ring + wf->head * (size_t)wf->nfft, rows + done * (size_t)wf->nfft,
                               run * row_bytes, hipMemcpyHostToDevice, wf->stream));
        if (!wf->mip_ok.empty()) std::fill(wf->mip_ok.begin() + (long)wf->head, wf->mip_ok.begin() + (long)(wf->head + run), 0);
        wf_advance(wf, run);
        done += run;
    }
    HIP_TRY(hipStreamSynchronize(wf->stream));
    return SDRK_OK;
}

int sdrk_waterfall_append_iq_device_async(sdrk_waterfall* wf, sdrk_plan* p, const void* d_iq,
                                          size_t n_frames, size_t frame_stride) {
    if (!wf || !p) return fail(SDRK_ERR_INVALID, "waterfall or plan is NULL");
    if (int st = check_precision(p, 32); st != SDRK_OK) return st;
    if (p->nfft != wf->nfft || p->device != wf->device)
        return fail(SDRK_ERR_INVALID, "plan (nfft %d, device %d) does not match waterfall (nfft %d, device %d)",
                    p->nfft, p->device, wf->nfft, wf->device);
    if (n_frames == 0) return SDRK_OK;
    if (!d_iq) return fail(SDRK_ERR_INVALID, "d_iq is NULL");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1 for more than one frame");
    HIP_TRY(hipSetDevice(wf->device));
    size_t skip = n_frames > (size_t)wf->maxlen ? n_frames - (size_t)wf->maxlen : 0;
    if (skip) wf_advance(wf, skip);
    size_t done = skip;
    while (done < n_frames) {
        size_t run = (size_t)wf->maxlen - wf->head;
        if (run > n_frames - done) run = n_frames - done;
        // the transform writes its rows straight into the ring slots
        // ... and, where the row pass can, the by-16 max-hold of each row beside it.  Whether it did is reported by the
        // launcher itself (with_mip); a plan that cannot — chirp-z, N = 65536, the pair-kernel builds — leaves the slots marked
        // as having none, and max-mode read-outs of those slots reduce the rows themselves.
        bool with_mip = false;
        HIP_TRY(wf_before_write(wf, run));
        int st = plan_launch(p, static_cast<const float2*>(d_iq) + done * frame_stride, run, frame_stride,
                             wf->d_ring + wf->head * (size_t)wf->nfft, sdrk::EPI_LOGPSD, wf->stream,
                             wf->d_mip_ring ? wf->d_mip_ring + wf->head * (size_t)(wf->nfft / 16) : nullptr, &with_mip);
        if (st != SDRK_OK) return st;
        if (!wf->mip_ok.empty()) std::fill(wf->mip_ok.begin() + (long)wf->head, wf->mip_ok.begin() + (long)(wf->head + run), with_mip ? 1 : 0);
        wf_advance(wf, run);
        done += run;
    }
    return SDRK_OK;
}

int sdrk_waterfall_sync(sdrk_waterfall* wf, sdrk_plan* p) {
    if (!wf) return fail(SDRK_ERR_INVALID, "waterfall is NULL");
    HIP_TRY(hipSetDevice(wf->device));
    HIP_TRY(hipStreamSynchronize(wf->stream));
    return p ? fused_check(p) : SDRK_OK;
}

int sdrk_waterfall_append_iq_device(sdrk_waterfall* wf, sdrk_plan* p, const void* d_iq,
                                    size_t n_frames, size_t frame_stride) {
    int st = sdrk_waterfall_append_iq_device_async(wf, p, d_iq, n_frames, frame_stride);
    if (st != SDRK_OK || n_frames == 0) return st;
    return sdrk_waterfall_sync(wf, p);
}

int sdrk_waterfall_append_iq(sdrk_waterfall* wf, sdrk_plan* p, const void* iq, size_t n_frames,
                             size_t frame_stride) {
    if (!wf || !p) return fail(SDRK_ERR_INVALID, "waterfall or plan is NULL");
    if (int st = check_precision(p, 32); st != SDRK_OK) return st;
    if (n_frames == 0) return SDRK_OK;
    if (!iq) return fail(SDRK_ERR_INVALID, "iq is NULL");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1");
    if (n_frames > p->max_batch)
        return fail(SDRK_ERR_INVALID, "n_frames %zu exceeds the plan's max_batch %zu", n_frames, p->max_batch);
    HIP_TRY(hipSetDevice(p->device));
    const size_t in_bytes = ((n_frames - 1) * frame_stride + (size_t)p->nfft) * sizeof(float2);
    int st = grow(p->device, &p->d_in, &p->in_cap, in_bytes);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipMemcpyAsync(p->d_in, iq, in_bytes, hipMemcpyHostToDevice, wf->stream));
    return sdrk_waterfall_append_iq_device(wf, p, p->d_in, n_frames, frame_stride);
}

int sdrk_waterfall_read(sdrk_waterfall* wf, float* out, size_t max_rows, size_t* n_rows) {
    if (!wf || !n_rows) return fail(SDRK_ERR_INVALID, "waterfall or n_rows is NULL");
    *n_rows = 0;
    size_t rows = wf->count < max_rows ? wf->count : max_rows;
    if (rows == 0) return SDRK_OK;
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(wf->device));
    const size_t L = (size_t)wf->maxlen, nf = (size_t)wf->nfft;
    // newest row is at head-1; the `rows` newest start at head-rows (mod L)
    size_t start = (wf->head + L - rows % L) % L;
    size_t first = L - start < rows ? L - start : rows;
    HIP_TRY(hipMemcpyAsync(out, wf->d_ring + start * nf, first * nf * sizeof(float),
                           hipMemcpyDeviceToHost, wf->stream));
    if (first < rows)
        HIP_TRY(hipMemcpyAsync(out + first * nf, wf->d_ring, (rows - first) * nf * sizeof(float),
                               hipMemcpyDeviceToHost, wf->stream));
    HIP_TRY(hipStreamSynchronize(wf->stream));
    *n_rows = rows;
    return SDRK_OK;
}

// the reduction of `rows` ring rows starting at slot `start` to nfft / factor bins each, into wf->d_dec[slot]: from the by-16
// rows when every requested slot has one (max mode, factor a multiple of 16) — 1/16 of the bytes —, else from the rows
static hipError_t wf_launch_decimate(sdrk_waterfall* wf, size_t start, size_t rows, int factor, int mode, hipStream_t stream,
                                     int slot) {
    bool mip = wf->d_mip_ring && mode == 0 && factor % 16 == 0;
    for (size_t r = 0; r < rows && mip; ++r) mip = wf->mip_ok[(start + r) % (size_t)wf->maxlen] != 0;
    if (mip)
        return sdrk::launch_decimate_mip(wf->d_mip_ring, wf->nfft, wf->maxlen, (int)start, (int)rows, factor,
                                         static_cast<float*>(wf->d_dec[slot]), stream);
    return sdrk::launch_decimate_rows(wf->d_ring, wf->nfft, wf->maxlen, (int)start, (int)rows, factor, mode,
                                      static_cast<float*>(wf->d_dec[slot]), stream);
}

int sdrk_waterfall_read_decimated(sdrk_waterfall* wf, float* out, size_t max_rows, int factor, int mode,
                                  size_t* n_rows) {
    if (!wf || !n_rows) return fail(SDRK_ERR_INVALID, "waterfall or n_rows is NULL");
    *n_rows = 0;
    if (factor < 1 || wf->nfft % factor != 0) return fail(SDRK_ERR_INVALID, "factor %d must divide nfft %d", factor, wf->nfft);
    if (mode != 0 && mode != 1) return fail(SDRK_ERR_INVALID, "mode must be 0 (max) or 1 (mean)");
    if (wf->reads_in_flight) return fail(SDRK_ERR_INVALID, "a two-phase decimated read is in flight (call _end first)");
    size_t rows = wf->count < max_rows ? wf->count : max_rows;
    if (rows == 0) return SDRK_OK;
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(wf->device));
    const size_t L = (size_t)wf->maxlen;
    const size_t start = (wf->head + L - rows % L) % L;
    const size_t bins = (size_t)(wf->nfft / factor);
    int st = grow(wf->device, &wf->d_dec[0], &wf->dec_cap[0], rows * bins * sizeof(float));
    if (st != SDRK_OK) return st;
    hipError_t e = wf_launch_decimate(wf, start, rows, factor, mode, wf->stream, 0);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "decimate launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, wf->d_dec[0], rows * bins * sizeof(float), hipMemcpyDeviceToHost, wf->stream));
    HIP_TRY(hipStreamSynchronize(wf->stream));
    *n_rows = rows;
    return SDRK_OK;
}

int sdrk_waterfall_read_decimated_begin(sdrk_waterfall* wf, float* out, size_t max_rows, int factor, int mode,
                                        size_t* n_rows) {
    if (!wf || !n_rows) return fail(SDRK_ERR_INVALID, "waterfall or n_rows is NULL");
    *n_rows = 0;
    if (wf->reads_in_flight >= 2) return fail(SDRK_ERR_INVALID, "two decimated reads are already in flight (call _end first)");
    if (factor < 1 || wf->nfft % factor != 0) return fail(SDRK_ERR_INVALID, "factor %d must divide nfft %d", factor, wf->nfft);
    if (mode != 0 && mode != 1) return fail(SDRK_ERR_INVALID, "mode must be 0 (max) or 1 (mean)");
    size_t rows = wf->count < max_rows ? wf->count : max_rows;
    if (rows == 0) return SDRK_OK;
    if (!out) return fail(SDRK_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(wf->device));
    if (!wf->s_copy) {
        HIP_TRY(hipStreamCreateWithFlags(&wf->s_copy, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&wf->ev_dec, hipEventDisableTiming));
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&wf->ev_dec_done[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&wf->ev_copy_done[k], hipEventDisableTiming));
        }
    }
    const int k = (wf->oldest_read + wf->reads_in_flight) & 1;
    const size_t L = (size_t)wf->maxlen;
    const size_t start = (wf->head + L - rows % L) % L;
    const size_t bins = (size_t)(wf->nfft / factor);
    if (rows * bins * sizeof(float) > wf->dec_cap[k]) HIP_TRY(hipStreamSynchronize(wf->s_copy));   // the staging is about to move
    int st = grow(wf->device, &wf->d_dec[k], &wf->dec_cap[k], rows * bins * sizeof(float));
    if (st != SDRK_OK) return st;
    // the rows are complete once everything enqueued on the transform stream so far has run; from there on the second stream
    HIP_TRY(hipEventRecord(wf->ev_dec, wf->stream));
    HIP_TRY(hipStreamWaitEvent(wf->s_copy, wf->ev_dec, 0));
    hipError_t e = wf_launch_decimate(wf, start, rows, factor, mode, wf->s_copy, k);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "decimate launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipEventRecord(wf->ev_dec_done[k], wf->s_copy));
    wf->dec_start[k] = start;
    wf->dec_rows[k] = rows;
    wf->dec_guard[k] = true;
    HIP_TRY(hipMemcpyAsync(out, wf->d_dec[k], rows * bins * sizeof(float), hipMemcpyDeviceToHost, wf->s_copy));
    HIP_TRY(hipEventRecord(wf->ev_copy_done[k], wf->s_copy));
    ++wf->reads_in_flight;
    *n_rows = rows;
    return SDRK_OK;
}

// Waits for the OLDEST read in flight (its rows are then in the caller's array); no-op when none is.
int sdrk_waterfall_read_decimated_end(sdrk_waterfall* wf) {
    if (!wf) return fail(SDRK_ERR_INVALID, "waterfall is NULL");
    if (!wf->reads_in_flight) return SDRK_OK;
    HIP_TRY(hipSetDevice(wf->device));
    const int k = wf->oldest_read;
    wf->oldest_read ^= 1;
    --wf->reads_in_flight;
    wf->dec_guard[k] = false;                                  // (its copy is behind its reduction on the same stream)
    HIP_TRY(hipEventSynchronize(wf->ev_copy_done[k]));
    return SDRK_OK;
}

}  // extern "C"

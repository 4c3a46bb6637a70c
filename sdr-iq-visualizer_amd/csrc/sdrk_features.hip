// sdrk_features.hip — the per-row reductions of include/sdrk.h (sdrk_row_*, sdrk_frame_features_*): statistics, thresholds
// and peaks of finished rows, or of frames on their way through a plan (fused with the transform at nfft = 4096).  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <mutex>

#include "kernels.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

// Device scratch of the plan-less row entry points: one buffer per device, only ever grown, used under the
// device's lock (calls on one device serialise; different devices run concurrently).
struct RowScratch {
    std::mutex lock;
    void* buf = nullptr;
    size_t cap = 0;
};
RowScratch g_row_scratch[64];

struct RowScratchGuard {
    RowScratch* rs;
    explicit RowScratchGuard(int device) : rs(&g_row_scratch[device & 63]) { rs->lock.lock(); }
    ~RowScratchGuard() { rs->lock.unlock(); }
    int reserve(int device, size_t bytes) { return grow(device, &rs->buf, &rs->cap, bytes); }
};

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// layout of the packed per-row results in a scratch buffer
struct FeatLayout {
    size_t rows_off, stats_off, thr_off, idx_off, cnt_off, planes_off, freqs_off, total;
    FeatLayout(size_t n_rows, int nfft, int max_peaks, bool stage_rows, bool peaks, bool planes = false) {
        size_t o = 0;
        rows_off = o;  o += stage_rows ? align256(n_rows * (size_t)nfft * sizeof(float)) : 0;
        stats_off = o; o += align256(n_rows * 16 * sizeof(double));
        thr_off = o;   o += align256(n_rows * sizeof(double));
        idx_off = o;   o += peaks ? align256(n_rows * (size_t)max_peaks * sizeof(int)) : 0;
        cnt_off = o;   o += peaks ? align256(n_rows * sizeof(int)) : 0;
        planes_off = o; o += planes ? align256(n_rows * SDRK_FEAT_PLANES * sizeof(double)) : 0;
        freqs_off = o;  o += planes ? align256((size_t)nfft * sizeof(double)) : 0;
        total = o;
    }
};

// the packed results of a batch -> finished planes (feature_finalize_kernel) -> the caller's host arrays
int planes_to_host(char* base, const FeatLayout& L, bool peaks, size_t n_rows, int nfft, float gamma, int max_peaks,
                   const double* freqs, void* out_planes, int32_t* out_idx, hipStream_t s) {
    const double* d_freqs = nullptr;
    if (freqs) {
        HIP_TRY(hipMemcpyAsync(base + L.freqs_off, freqs, (size_t)nfft * sizeof(double), hipMemcpyHostToDevice, s));
        d_freqs = reinterpret_cast<const double*>(base + L.freqs_off);
    }
    hipError_t e = sdrk::launch_feature_finalize(reinterpret_cast<const double*>(base + L.stats_off),
                                                 reinterpret_cast<const double*>(base + L.thr_off),
                                                 peaks ? reinterpret_cast<const int*>(base + L.idx_off) : nullptr,
                                                 peaks ? reinterpret_cast<const int*>(base + L.cnt_off) : nullptr, n_rows, nfft,
                                                 gamma, max_peaks, d_freqs, reinterpret_cast<double*>(base + L.planes_off), s);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "feature finalize launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out_planes, base + L.planes_off, n_rows * SDRK_FEAT_PLANES * sizeof(double), hipMemcpyDeviceToHost, s));
    if (peaks)
        HIP_TRY(hipMemcpyAsync(out_idx, base + L.idx_off, n_rows * (size_t)max_peaks * sizeof(int), hipMemcpyDeviceToHost, s));
    return SDRK_OK;
}

int device_cus(int device, int* cus) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    *cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return SDRK_OK;
}

int row_features_impl(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft, int rank,
                      float gamma, int min_distance, int max_peaks, double* out_stats, double* out_thr,
                      int32_t* out_idx, int32_t* out_count, const double* freqs, void* out_planes) {
    if (n_rows == 0) return SDRK_OK;
    if (!rows || (!out_stats && !out_planes)) return fail(SDRK_ERR_INVALID, "rows or the result pointer is NULL");
    if (nfft < 1) return fail(SDRK_ERR_INVALID, "nfft must be >= 1");
    const bool peaks = out_idx != nullptr || out_count != nullptr;
    if (peaks && (!out_idx || (!out_count && !out_planes) || max_peaks < 1 || min_distance < 1))
        return fail(SDRK_ERR_INVALID, "peaks need out_idx, out_count and max_peaks, min_distance >= 1");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    int cus = 256;
    st = device_cus(device, &cus);
    if (st != SDRK_OK) return st;
    RowScratchGuard g(device);
    const FeatLayout L(n_rows, nfft, max_peaks, !rows_on_device, peaks, out_planes != nullptr);
    st = g.reserve(device, L.total);
    if (st != SDRK_OK) return st;
    char* base = static_cast<char*>(g.rs->buf);
    const float* d_rows = rows;
    if (!rows_on_device) {
        HIP_TRY(hipMemcpy(base + L.rows_off, rows, n_rows * (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
        d_rows = reinterpret_cast<const float*>(base + L.rows_off);
    }
    if (peaks) HIP_TRY(hipMemsetAsync(base + L.idx_off, 0xFF, n_rows * (size_t)max_peaks * sizeof(int), nullptr));   // unused slots: -1
    hipError_t e = sdrk::launch_row_features(d_rows, n_rows, nfft, rank, gamma, min_distance, max_peaks,
                                             reinterpret_cast<double*>(base + L.stats_off),
                                             reinterpret_cast<double*>(base + L.thr_off),
                                             peaks ? reinterpret_cast<int*>(base + L.idx_off) : nullptr,
                                             peaks ? reinterpret_cast<int*>(base + L.cnt_off) : nullptr, cus, nullptr);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "row_features launch failed: %s", hipGetErrorString(e));
    if (out_planes) {
        st = planes_to_host(base, L, peaks, n_rows, nfft, gamma, max_peaks, freqs, out_planes, out_idx, nullptr);
        if (st != SDRK_OK) return st;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return SDRK_OK;
    }
    HIP_TRY(hipMemcpy(out_stats, base + L.stats_off, n_rows * 16 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_thr) HIP_TRY(hipMemcpy(out_thr, base + L.thr_off, n_rows * sizeof(double), hipMemcpyDeviceToHost));
    if (peaks) {
        HIP_TRY(hipMemcpy(out_idx, base + L.idx_off, n_rows * (size_t)max_peaks * sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_count, base + L.cnt_off, n_rows * sizeof(int), hipMemcpyDeviceToHost));
    }
    return SDRK_OK;
}

}  // namespace

extern "C" {

int sdrk_row_features(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft, int rank,
                      float gamma, int min_distance, int max_peaks, double* out_stats, double* out_thr,
                      int32_t* out_idx, int32_t* out_count) {
    return row_features_impl(device, rows, rows_on_device, n_rows, nfft, rank, gamma, min_distance, max_peaks, out_stats,
                             out_thr, out_idx, out_count, nullptr, nullptr);
}

int sdrk_row_features_planes(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft, int rank,
                             float gamma, int min_distance, int max_peaks, const double* freqs, void* out_planes,
                             int32_t* out_idx) {
    if (n_rows && !out_planes) return fail(SDRK_ERR_INVALID, "out_planes is NULL");
    return row_features_impl(device, rows, rows_on_device, n_rows, nfft, rank, gamma, min_distance, max_peaks, nullptr,
                             nullptr, out_idx, nullptr, freqs, out_planes);
}

int sdrk_row_stats(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft, int rank,
                   double* out) {
    return sdrk_row_features(device, rows, rows_on_device, n_rows, nfft, rank, 0.0f, 1, 1, out, nullptr, nullptr, nullptr);
}

int sdrk_row_peaks(int device, const float* rows, int rows_on_device, size_t n_rows, int nfft,
                   const double* thresholds, int min_distance, int max_peaks, int32_t* out_idx,
                   int32_t* out_count) {
    if (n_rows == 0) return SDRK_OK;
    if (!rows || !thresholds || !out_idx || !out_count) return fail(SDRK_ERR_INVALID, "NULL pointer");
    if (nfft < 1 || max_peaks < 1 || min_distance < 1)
        return fail(SDRK_ERR_INVALID, "nfft, max_peaks and min_distance must be >= 1");
    int st = check_device(device);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(device));
    RowScratchGuard g(device);
    const FeatLayout L(n_rows, nfft, max_peaks, !rows_on_device, true);
    st = g.reserve(device, L.total);
    if (st != SDRK_OK) return st;
    char* base = static_cast<char*>(g.rs->buf);
    const float* d_rows = rows;
    if (!rows_on_device) {
        HIP_TRY(hipMemcpy(base + L.rows_off, rows, n_rows * (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
        d_rows = reinterpret_cast<const float*>(base + L.rows_off);
    }
    HIP_TRY(hipMemcpy(base + L.thr_off, thresholds, n_rows * sizeof(double), hipMemcpyHostToDevice));
    hipError_t e = sdrk::launch_row_peaks(d_rows, n_rows, nfft, reinterpret_cast<const double*>(base + L.thr_off),
                                          min_distance, max_peaks, reinterpret_cast<int*>(base + L.idx_off),
                                          reinterpret_cast<int*>(base + L.cnt_off), nullptr);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "row_peaks launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpy(out_idx, base + L.idx_off, n_rows * (size_t)max_peaks * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_count, base + L.cnt_off, n_rows * sizeof(int), hipMemcpyDeviceToHost));
    return SDRK_OK;
}

int sdrk_frame_features_device(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride,
                               float* d_out_db, int rank, float gamma, int min_distance, int max_peaks,
                               double* d_stats, double* d_thr, int32_t* d_idx, int32_t* d_count, void* stream) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (int st = check_precision(p, 32); st != SDRK_OK) return st;
    if (n_frames == 0) return SDRK_OK;
    if (!d_iq || !d_stats) return fail(SDRK_ERR_INVALID, "d_iq or d_stats is NULL");
    const bool peaks = d_idx != nullptr || d_count != nullptr;
    if (peaks && (!d_idx || !d_count || max_peaks < 1 || min_distance < 1))
        return fail(SDRK_ERR_INVALID, "peaks need d_idx, d_count and max_peaks, min_distance >= 1");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1");
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : p->stream;
    if (p->nfft == 4096) {
        // fused: the rows never leave the chip unless d_out_db asks for them (fft4096_features.hip)
        const sdrk::LaunchArgs a = plan_launch_args(p, d_iq, n_frames, frame_stride, d_out_db, sdrk::EPI_LOGPSD, s);
        hipError_t e = sdrk::launch_fft4096_features(a, rank, gamma, min_distance, max_peaks > 0 ? max_peaks : 1, d_stats,
                                                     d_thr, peaks ? d_idx : nullptr, peaks ? d_count : nullptr);
        if (e != hipSuccess) return fail(SDRK_ERR_HIP, "fused feature launch failed: %s", hipGetErrorString(e));
        return SDRK_OK;
    }
    // other frame lengths: the transform writes its rows (to the caller's buffer, or to plan staging in
    // chunks), then one single-read reduction launch per chunk
    const size_t nfft = (size_t)p->nfft;
    size_t per = n_frames;
    float* rows = d_out_db;
    if (!rows) {
        per = ((size_t)256 << 20) / (nfft * sizeof(float));
        if (per < 1) per = 1;
        if (per > n_frames) per = n_frames;
        int st = grow(p->device, &p->d_out, &p->out_cap, per * nfft * sizeof(float));
        if (st != SDRK_OK) return st;
        rows = static_cast<float*>(p->d_out);
    }
    for (size_t f0 = 0; f0 < n_frames; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        float* dst = d_out_db ? d_out_db + f0 * nfft : rows;
        int st = plan_launch(p, static_cast<const float2*>(d_iq) + f0 * frame_stride, nf, frame_stride, dst,
                             sdrk::EPI_LOGPSD, s);
        if (st != SDRK_OK) return st;
        hipError_t e = sdrk::launch_row_features(dst, nf, p->nfft, rank, gamma, min_distance, max_peaks > 0 ? max_peaks : 1,
                                                 d_stats + f0 * 16, d_thr ? d_thr + f0 : nullptr,
                                                 peaks ? d_idx + f0 * (size_t)max_peaks : nullptr,
                                                 peaks ? d_count + f0 : nullptr, p->num_cus, s);
        if (e != hipSuccess) return fail(SDRK_ERR_HIP, "row_features launch failed: %s", hipGetErrorString(e));
    }
    return SDRK_OK;
}

namespace {
int frame_features_host_impl(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, int rank,
                             float gamma, int min_distance, int max_peaks, double* out_stats, double* out_thr,
                             int32_t* out_idx, int32_t* out_count, float* out_db, const double* freqs, void* out_planes) {
    int st = check_exec_args(p, iq, n_frames, frame_stride, out_planes ? out_planes : static_cast<void*>(out_stats));
    if (st != SDRK_OK || n_frames == 0) return st;
    const bool peaks = out_idx != nullptr || out_count != nullptr;
    if (peaks && (!out_idx || (!out_count && !out_planes) || max_peaks < 1 || min_distance < 1))
        return fail(SDRK_ERR_INVALID, "peaks need out_idx, out_count and max_peaks, min_distance >= 1");
    HIP_TRY(hipSetDevice(p->device));
    const size_t nfft = (size_t)p->nfft;
    const size_t in_bytes = ((n_frames - 1) * frame_stride + nfft) * sizeof(float2);
    // results (and the rows, when the caller wants them or the frame length has no fused kernel) in a second
    // staging buffer that only grows
    const bool need_rows = out_db != nullptr;
    const FeatLayout L(n_frames, p->nfft, max_peaks, need_rows, peaks, out_planes != nullptr);
    void*& fbuf = p->d_feat;
    st = grow(p->device, &fbuf, &p->feat_cap, L.total);
    if (st != SDRK_OK) return st;
    char* base = static_cast<char*>(fbuf);
    float* d_rows = need_rows ? reinterpret_cast<float*>(base + L.rows_off) : nullptr;
    double* d_stats = reinterpret_cast<double*>(base + L.stats_off);
    double* d_thr = reinterpret_cast<double*>(base + L.thr_off);
    int32_t* d_idx = peaks ? reinterpret_cast<int32_t*>(base + L.idx_off) : nullptr;
    int32_t* d_cnt = peaks ? reinterpret_cast<int32_t*>(base + L.cnt_off) : nullptr;
    if (peaks) HIP_TRY(hipMemsetAsync(d_idx, 0xFF, n_frames * (size_t)max_peaks * sizeof(int), p->stream));        // unused slots: -1
    if (in_bytes <= 2 * HOST_CHUNK_BYTES) {
        st = grow(p->device, &p->d_in, &p->in_cap, in_bytes);
        if (st != SDRK_OK) return st;
        HIP_TRY(hipMemcpyAsync(p->d_in, iq, in_bytes, hipMemcpyHostToDevice, p->stream));
        st = sdrk_frame_features_device(p, p->d_in, n_frames, frame_stride, d_rows, rank, gamma, min_distance, max_peaks,
                                        d_stats, d_thr, d_idx, d_cnt, nullptr);
        if (st != SDRK_OK) return st;
    } else {
        // Large batches: the frames go through the pinned slots of the sdrk_exec_host pipeline in ~16 MiB chunks —
        // helper threads stage chunk c+1 (or the copy engine reads the caller's pinned array directly) while chunk
        // c crosses PCIe and chunk c-1 is measured.  The per-row results stay on the device until the end (they are
        // ~1 % of the input).
        // A slot is free once its chunk is measured (ChunkOut::None): nothing comes back per chunk, and no drain — the one
        // stream sync behind the results below covers every chunk.
        SlotPipe pipe;
        st = pipe.open(p, "feature pipeline");
        if (st != SDRK_OK) return st;
        const size_t stride_bytes = (frame_stride ? frame_stride : 1) * sizeof(float2);
        size_t per = HOST_CHUNK_BYTES / stride_bytes;
        if (per < 1) per = 1;
        const size_t chunk_in = ((per - 1) * frame_stride + nfft) * sizeof(float2);
        const bool in_pinned = pinned_ranges().covers(iq, in_bytes);
        for (size_t f0 = 0; f0 < n_frames; f0 += per) {
            const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
            const size_t cin = ((nf - 1) * frame_stride + nfft) * sizeof(float2);
            HostSlot* s = nullptr;
            st = pipe.acquire(chunk_in, 0, s);
            if (st != SDRK_OK) return st;
            const void* src = static_cast<const float2*>(iq) + f0 * frame_stride;
            st = pipe.upload(*s, chunk_pinned_src(*s, src, cin, in_pinned), cin);
            if (st == SDRK_OK)
                st = pipe.submit(*s, sdrk_frame_features_device(p, s->d_in, nf, frame_stride, d_rows ? d_rows + f0 * nfft : nullptr,
                                                                rank, gamma, min_distance, max_peaks, d_stats + f0 * 16, d_thr + f0,
                                                                d_idx ? d_idx + f0 * (size_t)max_peaks : nullptr,
                                                                d_cnt ? d_cnt + f0 : nullptr, nullptr),
                                 ChunkOut{});
            if (st != SDRK_OK) return st;
        }
    }
    // the results come back through ONE exit: whatever fails from here on, no chunk of the pipelined form may still be
    // using its staging slot when the call returns (a later sdrk_exec_host would restage it under the copy engine)
    auto results = [&]() -> int {
        if (out_planes) {
            int r = planes_to_host(base, L, peaks, n_frames, p->nfft, gamma, max_peaks, freqs, out_planes, out_idx, p->stream);
            if (r != SDRK_OK) return r;
        } else {
            HIP_TRY(hipMemcpyAsync(out_stats, base + L.stats_off, n_frames * 16 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
            if (out_thr) HIP_TRY(hipMemcpyAsync(out_thr, base + L.thr_off, n_frames * sizeof(double), hipMemcpyDeviceToHost, p->stream));
            if (peaks) {
                HIP_TRY(hipMemcpyAsync(out_idx, base + L.idx_off, n_frames * (size_t)max_peaks * sizeof(int), hipMemcpyDeviceToHost, p->stream));
                HIP_TRY(hipMemcpyAsync(out_count, base + L.cnt_off, n_frames * sizeof(int), hipMemcpyDeviceToHost, p->stream));
            }
        }
        if (need_rows)
            HIP_TRY(hipMemcpyAsync(out_db, base + L.rows_off, n_frames * nfft * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SDRK_OK;
    };
    st = results();
    if (st != SDRK_OK) {
        if (p->s_h2d) slots_abandon(p);
        else (void)hipStreamSynchronize(p->stream);
        for (auto& s : p->slot) s.busy = false;
        return st;
    }
    for (auto& s : p->slot) s.busy = false;                      // the pipelined form's chunks are all through
    return fused_check(p);
}
}  // namespace

int sdrk_frame_features_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, int rank,
                             float gamma, int min_distance, int max_peaks, double* out_stats, double* out_thr,
                             int32_t* out_idx, int32_t* out_count, float* out_db) {
    if (p && n_frames && !out_stats) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    return frame_features_host_impl(p, iq, n_frames, frame_stride, rank, gamma, min_distance, max_peaks, out_stats, out_thr,
                                    out_idx, out_count, out_db, nullptr, nullptr);
}

int sdrk_frame_features_host_planes(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, int rank,
                                    float gamma, int min_distance, int max_peaks, const double* freqs, void* out_planes,
                                    int32_t* out_idx, float* out_db) {
    if (p && n_frames && !out_planes) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    return frame_features_host_impl(p, iq, n_frames, frame_stride, rank, gamma, min_distance, max_peaks, nullptr, nullptr,
                                    out_idx, nullptr, out_db, freqs, out_planes);
}

}  // extern "C"

// pfb_api.hip — host side of the per-frame polyphase-filter-bank entry points of include/sdrk.h (sdrk_plan_set_pfb,
// sdrk_plan_pfb_taps, sdrk_exec_*_pfb, sdrk_exec_*_pfb_ci16): a prototype filter of T * nfft coefficients folds T consecutive
// blocks of a stream into each frame in front of the plan's transform (kernels_pfb.h has the exact arithmetic).  The stream is
// complex64, or interleaved little-endian int16 I,Q at 4 bytes per sample: x[n] = float32(I[n]) + i float32(Q[n]) exactly, then
// the bits of the complex64 call.  Sits in front of app/sdr/streamer.py:119-121; the reference has no counterpart.
//
// N = 4096 is one launch on the caller's stream (pfb4096.hip, pfb4096_i16.hip: the fold in the transform's registers).  Every
// other length (single-pass, two-pass with the persistent N = 65536 form, chirp-z) runs "fold a chunk of frames into plan-owned
// complex64 staging (pfb_fold.hip, pfb_fold_i16.hip: no widened copy of an int16 stream), then plan_launch" on the same stream,
// the staging capped at 64 MiB and cut at frame boundaries however many frames the call has.  The numpy boundary is
// sdrk_host_pipeline.hip's exec_host with an input span of T * nfft samples per frame: a chunk carries its (T - 1) * nfft
// samples of overlap.
// Integration over K folded frames is integrate_api.hip, with this file's launchers and checks.  Out of scope: double
// precision, waterfall appends.
// The last part of the file is the host side of "FIR filtering and channel extraction" (sdrk_plan_set_fir, sdrk_exec_*_fir*):
// overlap-save fast convolution in blocks of 4096 through ols4096.hip, the filter held by the plan as the prototype is, and of
// the channel bank (sdrk_exec_*_chanbank*): C tuned channels from one pass through ols_bank.hip, on the same chunk loop.
// Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels_ols_bank.h"
#include "kernels_pfb.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace {

constexpr size_t PFB_STAGE_BYTES = (size_t)64 << 20;   // folded complex64 frames of the generic route, per plan

// How pfb4096_kernel shares the frames among its workgroups: SDRK_PFB_ASSIGN = 0 / 1 / 2 (kernels_pfb.h) for A/B work,
// read when the prototype is set; the default is what measured fastest (profiles/pfb/SUMMARY.md).
int pfb_assign_default() {
    if (const char* env = getenv("SDRK_PFB_ASSIGN")) {
        const long v = atol(env);
        if (v >= sdrk::PFB_ASSIGN_STRIDE && v <= sdrk::PFB_ASSIGN_RUNS) return (int)v;
    }
    return sdrk::PFB_ASSIGN_XCD;
}

}  // namespace

// Which plans the PFB entry points serve: float32, rectangular window (the prototype is the window), taps set.
int sdrk_host::check_pfb_plan(const sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "the polyphase filter bank serves float32 plans only (this is a float64 plan)");
    if (p->d_window)
        return fail(SDRK_ERR_INVALID, "the polyphase filter bank needs a plan created with SDRK_WINDOW_RECT: the prototype is the window");
    return SDRK_OK;
}

int sdrk_host::check_pfb_ready(const sdrk_plan* p) {
    int st = check_pfb_plan(p);
    if (st != SDRK_OK) return st;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    return SDRK_OK;
}

int sdrk_host::check_pfb_exec(const sdrk_plan* p, const void* in, size_t n_frames, size_t frame_stride, const void* out) {
    int st = check_pfb_ready(p);
    if (st != SDRK_OK) return st;
    if (n_frames == 0) return fail(SDRK_ERR_INVALID, "n_frames must be >= 1");
    if (!in || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (frame_stride == 0 && n_frames > 1) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1 for more than one frame");
    return SDRK_OK;
}

namespace {

// The generic route of a PFB transform, for samples of in_elem bytes and the fold kernel that reads them (kernels_pfb.h's
// launch_pfb_fold or its int16 form).
using PfbFoldFn = hipError_t (*)(const void* d_iq, size_t frame_stride, size_t n_frames, int nfft, const float* d_h, int taps,
                                 void* d_out, int num_cus, hipStream_t stream);
int pfb_fold_route(sdrk_plan* p, const void* d_in, size_t in_elem, PfbFoldFn fold, size_t n_frames, size_t stride, void* d_out,
                   int epilogue, hipStream_t stream) {
    const size_t nfft = (size_t)p->nfft;
    const size_t out_elem = epilogue == sdrk::EPI_LOGPSD ? sizeof(float) : sizeof(float2);
    size_t per = PFB_STAGE_BYTES / (nfft * sizeof(float2));   // one frame is at most 2^22 samples = 32 MiB
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    sdrk_host::Staging& sg = p->pfb;   // one staging per plan: a call on another stream waits for the last one's reads
    int st = sg.reserve(0, per * nfft * sizeof(float2));
    if (st == SDRK_OK) st = sg.enter(stream);
    if (st != SDRK_OK) return st;
    void* const d_stage = sg.buf[0].d;
    // N = 65536: the form is chosen for the call, not for its chunks (plan_launch's call_frames), as in the int16 route
    for (size_t f0 = 0; f0 < n_frames && st == SDRK_OK; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        const hipError_t e = fold(static_cast<const char*>(d_in) + f0 * stride * in_elem, stride, nf, p->nfft, p->d_pfb_h, p->pfb_taps,
                                  d_stage, p->num_cus, stream);
        if (e != hipSuccess) {
            st = fail(SDRK_ERR_HIP, "pfb fold launch failed: %s", hipGetErrorString(e));
            break;
        }
        st = plan_launch(p, d_stage, nf, nfft, static_cast<char*>(d_out) + f0 * nfft * out_elem, epilogue, stream,
                         nullptr, nullptr, nullptr, n_frames);
    }
    return sg.leave(stream, st);   // (also after a failed launch: earlier chunks are in flight)
}

// One PFB transform of the plan on a raw stream of in_elem-byte samples: the folding N = 4096 kernel `flagship`, else the
// generic route with `fold`.
template <class Flagship>
int launch_pfb_any(sdrk_plan* p, const void* d_in, size_t in_elem, PfbFoldFn fold, Flagship flagship, size_t n_frames, size_t stride,
                   void* d_out, int epilogue, hipStream_t stream) {
    if (n_frames == 0) return SDRK_OK;
    if (p->pfb_taps < 1 || !p->d_pfb_h) return fail(SDRK_ERR_INVALID, "no prototype filter set: call sdrk_plan_set_pfb first");
    if (p->nfft != 4096 || p->blu_inner) return pfb_fold_route(p, d_in, in_elem, fold, n_frames, stride, d_out, epilogue, stream);
    const sdrk::LaunchArgs a = plan_launch_args(p, d_in, n_frames, stride, d_out, epilogue, stream);
    const hipError_t e = flagship(a, p->d_pfb_h, p->pfb_taps, p->pfb_assign);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "pfb kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

// The numpy boundary of a PFB mode: T * nfft samples of in_elem bytes per frame in; float32 rows or complex64 out; always
// through the copy engines (every sample is read T times: over PCIe it would cross T times)
int exec_host_pfb(size_t in_elem, LaunchFn launch, int epilogue, sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride,
                  void* out) {
    int st = check_pfb_exec(p, iq, n_frames, frame_stride, out);
    if (st != SDRK_OK) return st;
    const size_t span = (size_t)p->pfb_taps * (size_t)p->nfft;
    return exec_host(p, iq, n_frames, frame_stride, out, frames_io(in_elem, span, launch, epilogue));
}

}  // namespace

// The LaunchFns of the two PFB modes (the transforms of the numpy boundary and of integrate_api.hip's generic route too;
// declared in plan_internal.h).
int sdrk_host::launch_pfb(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t stream) {
    return launch_pfb_any(p, d_in, sizeof(float2), sdrk::launch_pfb_fold, sdrk::launch_pfb4096, n_frames, stride, d_out, epilogue, stream);
}

int sdrk_host::launch_pfb_ci16(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue,
                               hipStream_t stream) {
    return launch_pfb_any(p, d_in, 4, sdrk::launch_pfb_fold_i16, sdrk::launch_pfb4096_i16, n_frames, stride, d_out, epilogue, stream);
}

extern "C" {

int sdrk_plan_set_pfb(sdrk_plan* p, int taps, const float* h) {
    int st = check_pfb_plan(p);
    if (st != SDRK_OK) return st;
    if (taps < 1 || taps > sdrk::PFB_MAX_TAPS) return fail(SDRK_ERR_INVALID, "taps=%d: must be in [1, %d]", taps, sdrk::PFB_MAX_TAPS);
    if (!h) return fail(SDRK_ERR_INVALID, "prototype pointer is NULL");
    HIP_TRY(hipSetDevice(p->device));
    // not with work in flight, says the header; make it safe all the same for work on the plan's own stream and staging
    HIP_TRY(hipStreamSynchronize(p->stream));
    st = p->pfb.wait();
    if (st == SDRK_OK) st = p->integ.wait();   // sdrk_exec_*_pfb_integrated reads the prototype too
    if (st != SDRK_OK) return st;
    const size_t bytes = (size_t)taps * (size_t)p->nfft * sizeof(float);
    p->pfb_taps = 0;
    if (p->d_pfb_h) {
        HIP_TRY(hipFree(p->d_pfb_h));
        p->d_pfb_h = nullptr;
    }
    HIP_TRY(hipMalloc((void**)&p->d_pfb_h, bytes));
    HIP_TRY(hipMemcpy(p->d_pfb_h, h, bytes, hipMemcpyHostToDevice));
    p->pfb_taps = taps;
    p->pfb_assign = pfb_assign_default();
    return SDRK_OK;
}

int sdrk_plan_pfb_taps(const sdrk_plan* p) { return p ? p->pfb_taps : fail(SDRK_ERR_INVALID, "plan is NULL"); }

int sdrk_exec_device_pfb(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db, void* stream) {
    return exec_device_frames(check_pfb_exec, launch_pfb, p, d_iq, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_pfb_timed_each(sdrk_plan* p, const void* d_iq, size_t n_frames, size_t frame_stride, float* d_out_db,
                                    int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_pfb_exec, launch_pfb, p, d_iq, n_frames, frame_stride, d_out_db, launches, each_ms);
}

int sdrk_exec_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host_pfb(sizeof(float2), launch_pfb, sdrk::EPI_LOGPSD, p, iq, n_frames, frame_stride, out_db);
}

int sdrk_exec_fft_host_pfb(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out_c64) {
    return exec_host_pfb(sizeof(float2), launch_pfb, sdrk::EPI_COMPLEX, p, iq, n_frames, frame_stride, out_c64);
}

int sdrk_exec_device_pfb_ci16(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride, float* d_out_db,
                              void* stream) {
    return exec_device_frames(check_pfb_exec, launch_pfb_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, stream);
}

int sdrk_exec_device_pfb_ci16_timed_each(sdrk_plan* p, const void* d_iq_ci16, size_t n_frames, size_t frame_stride,
                                         float* d_out_db, int launches, float* each_ms) {
    return exec_device_frames_timed_each(check_pfb_exec, launch_pfb_ci16, p, d_iq_ci16, n_frames, frame_stride, d_out_db, launches,
                                         each_ms);
}

int sdrk_exec_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host_pfb(4, launch_pfb_ci16, sdrk::EPI_LOGPSD, p, iq_ci16, n_frames, frame_stride, out_db);
}

int sdrk_exec_fft_host_pfb_ci16(sdrk_plan* p, const void* iq_ci16, size_t n_frames, size_t frame_stride, void* out_c64) {
    return exec_host_pfb(4, launch_pfb_ci16, sdrk::EPI_COMPLEX, p, iq_ci16, n_frames, frame_stride, out_c64);
}

}  // extern "C"

// ---- FIR filtering and channel extraction: tune, filter, decimate (include/sdrk.h; kernels_ols.h has the block geometry) ----
namespace {

// How ols4096_kernel shares the blocks among its workgroups: SDRK_OLS_ASSIGN = 0 / 1 (kernels_ols.h) for A/B work, read when
// the filter is set.
int fir_assign_default() {
    if (const char* env = getenv("SDRK_OLS_ASSIGN")) {
        const long v = atol(env);
        if (v >= sdrk::OLS_ASSIGN_STRIDE && v <= sdrk::OLS_ASSIGN_RUNS) return (int)v;
    }
    return sdrk::OLS_ASSIGN_STRIDE;
}

// Which plans the FIR entry points serve: float32, nfft = 4096 (the block length is the plan's transform).
int check_fir_plan(const sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (p->precision != 32) return fail(SDRK_ERR_INVALID, "FIR filtering serves float32 plans only (this is a float64 plan)");
    if (p->nfft != 4096 || p->blu_inner)
        return fail(SDRK_ERR_UNSUPPORTED, "FIR filtering serves plans with nfft = 4096 only (this plan has nfft = %d)", p->nfft);
    return SDRK_OK;
}

int check_fir_call(const sdrk_plan* p, int decim, int shift_bins) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (p->fir_taps < 1 || !p->d_fir_h) return fail(SDRK_ERR_INVALID, "no FIR filter set: call sdrk_plan_set_fir first");
    if (decim < 1 || decim > sdrk::OLS_MAX_DECIM || (decim & (decim - 1)))
        return fail(SDRK_ERR_INVALID, "decim=%d: must be a power of two in [1, %d]", decim, sdrk::OLS_MAX_DECIM);
    if (shift_bins < -sdrk::OLS_N / 2 || shift_bins >= sdrk::OLS_N / 2)
        return fail(SDRK_ERR_INVALID, "shift_bins=%d: must be in [%d, %d]", shift_bins, -sdrk::OLS_N / 2, sdrk::OLS_N / 2 - 1);
    return SDRK_OK;
}

int check_fir_device(const sdrk_plan* p, const void* d_in, size_t n_in, int decim, int shift_bins, const void* d_out) {
    int st = check_fir_call(p, decim, shift_bins);
    if (st != SDRK_OK) return st;
    if (!d_in || !d_out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (n_in < (size_t)p->fir_taps) return fail(SDRK_ERR_INVALID, "n_in=%zu: a valid convolution needs at least the %d taps", n_in, p->fir_taps);
    return SDRK_OK;
}

// One launch: the first max_blocks blocks (0: all) of the valid convolution of n_in samples.
int fir_launch(sdrk_plan* p, bool i16, const void* d_in, size_t n_in, int decim, int shift_bins, int phase0, void* d_out,
               size_t max_blocks, hipStream_t stream) {
    sdrk::OlsArgs a;
    a.d_in = d_in;
    a.n_in = n_in;
    a.taps = p->fir_taps;
    a.decim = decim;
    a.shift_bins = shift_bins;
    a.phase0 = phase0;
    a.d_h = p->d_fir_h;
    a.d_twiddle = p->d_twiddle;
    a.d_out = static_cast<float2*>(d_out);
    a.max_blocks = max_blocks;
    a.num_cus = p->num_cus;
    a.assign = p->fir_assign;
    a.stream = stream;
    const hipError_t e = i16 ? sdrk::launch_ols4096_i16(a) : sdrk::launch_ols4096(a);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "FIR kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

int exec_device_fir(bool i16, sdrk_plan* p, const void* d_in, size_t n_in, int decim, int shift_bins, int phase0, void* d_out,
                    void* stream) {
    int st = check_fir_device(p, d_in, n_in, decim, shift_bins, d_out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return fir_launch(p, i16, d_in, n_in, decim, shift_bins, phase0, d_out, 0, stream ? static_cast<hipStream_t>(stream) : p->stream);
}

// Blocks per chunk of the host entries: ~HOST_CHUNK_BYTES of input (SDRK_FIR_CHUNK_BLOCKS overrides it: tests reach several
// chunks with short streams).
size_t fir_chunk_blocks(size_t L, size_t in_elem) {
    if (const char* env = getenv("SDRK_FIR_CHUNK_BLOCKS")) {
        const long v = atol(env);
        if (v >= 1) return (size_t)v;
    }
    const size_t per = HOST_CHUNK_BYTES / (L * in_elem);
    return per < 1 ? 1 : per;
}

// The numpy boundary: the device entry on the virtual stream prefix || iq, from its first sample whose stream index is a
// multiple of D, in chunks of whole blocks through the plan's three pinned staging slots.  Every block sees the 4096 samples it
// sees in one device call on the whole virtual stream (a chunk carries its last block's 4096 - L samples of overlap, and a
// launch is cut at its chunk's blocks), so the chunking does not show in the bits.
// One loop for the single call and the channel bank: `planes` output planes, out_stride complex64 apart in the caller's array
// and packed in a slot's staging; launch(d_in, cn, index, d_out, nb, co) runs the first nb blocks of a chunk of cn samples,
// whose first valid output has stream index `index` mod 4096 (the mixer's phase is s * index) and which keeps co outputs a plane.
template <class Launch>
int host_fir_chunks(size_t in_elem, sdrk_plan* p, const void* prefix, const void* iq, size_t n, int decim, uint64_t sample0,
                    size_t planes, void* out, size_t out_stride, size_t* n_out, Launch launch) {
    if (!n_out) return fail(SDRK_ERR_INVALID, "n_out pointer is NULL");
    *n_out = 0;
    if (n == 0) return SDRK_OK;
    if (!iq || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    const size_t D = (size_t)decim, M = (size_t)p->fir_taps, L = (size_t)sdrk::ols_block_len(p->fir_taps), N = sdrk::OLS_N;
    const size_t j0 = (size_t)((D - sample0 % D) % D);   // the first kept sample of iq
    if (j0 >= n) return SDRK_OK;
    const size_t n_virt = n - j0 + M - 1;                 // the virtual stream from there: sample t is V[j0 + t], V = prefix || iq
    const size_t total_out = (n - j0 - 1) / D + 1;
    const size_t n_blocks = sdrk::ols_blocks(n_virt, p->fir_taps);
    const size_t per = fir_chunk_blocks(L, in_elem), opb = L / D;
    const size_t chunk_in = ((per - 1) * L + N) * in_elem, chunk_out = planes * per * opb * sizeof(float2);
    HIP_TRY(hipSetDevice(p->device));
    int st = ensure_copy_streams(p);
    if (st != SDRK_OK) return st;
    auto retire = [planes, out_stride](HostSlot& s) -> int {   // out_bytes: of one plane
        if (!s.busy) return SDRK_OK;
        s.busy = false;
        HIP_TRY(hipEventSynchronize(s.ev_done));
        for (size_t c = 0; c < planes; ++c)
            memcpy(static_cast<char*>(s.user_out) + c * out_stride * sizeof(float2), static_cast<char*>(s.h_out) + c * s.out_bytes, s.out_bytes);
        return SDRK_OK;
    };
    size_t c = 0;
    for (size_t b0 = 0; b0 < n_blocks; b0 += per, ++c) {
        HostSlot& s = p->slot[c % HOST_SLOTS];
        const size_t nb = n_blocks - b0 < per ? n_blocks - b0 : per;
        const size_t t0 = b0 * L;
        const size_t cn = (nb - 1) * L + N < n_virt - t0 ? (nb - 1) * L + N : n_virt - t0;
        const size_t o0 = b0 * opb, co = nb * opb < total_out - o0 ? nb * opb : total_out - o0;
        st = retire(s);
        if (st == SDRK_OK) st = slot_reserve(p, s, chunk_in, chunk_out);
        if (st != SDRK_OK) { slots_abandon(p); return st; }
        // samples V[v0 .. v0 + cn): the part below M - 1 from the prefix (NULL: zeros), the rest from iq
        const size_t v0 = j0 + t0;
        char* dst = static_cast<char*>(s.h_in);
        size_t done = 0;
        if (v0 < M - 1) {
            done = M - 1 - v0 < cn ? M - 1 - v0 : cn;
            if (prefix) memcpy(dst, static_cast<const char*>(prefix) + v0 * in_elem, done * in_elem);
            else memset(dst, 0, done * in_elem);
        }
        if (done < cn)
            memcpy(dst + done * in_elem, static_cast<const char*>(iq) + (v0 + done - (M - 1)) * in_elem, (cn - done) * in_elem);
        hipError_t e = stage_chunk_in(p, s, s.h_in, cn * in_elem);
        if (e == hipSuccess) {
            st = launch(s.d_in, cn, (unsigned)((sample0 + j0 + t0) & (N - 1)), s.d_out, nb, co);
            if (st != SDRK_OK) { slots_abandon(p); return st; }
            e = hipEventRecord(s.ev_k, p->stream);
        }
        if (e == hipSuccess) e = hipStreamWaitEvent(p->s_d2h, s.ev_k, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(s.h_out, s.d_out, planes * co * sizeof(float2), hipMemcpyDeviceToHost, p->s_d2h);
        if (e == hipSuccess) e = hipEventRecord(s.ev_done, p->s_d2h);
        if (e != hipSuccess) {
            slots_abandon(p);
            return fail(SDRK_ERR_HIP, "host pipeline failed: %s", hipGetErrorString(e));
        }
        s.busy = true;
        s.user_out = static_cast<char*>(out) + o0 * sizeof(float2);
        s.out_bytes = co * sizeof(float2);
    }
    for (size_t i = 0; i < HOST_SLOTS; ++i) {   // drain in submission order
        st = retire(p->slot[(c + i) % HOST_SLOTS]);
        if (st != SDRK_OK) { slots_abandon(p); return st; }
    }
    *n_out = total_out;
    return SDRK_OK;
}

int exec_host_fir(size_t in_elem, sdrk_plan* p, const void* prefix, const void* iq, size_t n, int decim, int shift_bins,
                  uint64_t sample0, void* out, size_t* n_out) {
    int st = check_fir_call(p, decim, shift_bins);
    if (st != SDRK_OK) return st;
    const unsigned s_mod = (unsigned)shift_bins & (unsigned)(sdrk::OLS_N - 1);
    return host_fir_chunks(in_elem, p, prefix, iq, n, decim, sample0, 1, out, 0, n_out,
                           [&](const void* d_in, size_t cn, unsigned index, void* d_out, size_t nb, size_t) {
                               const unsigned phase = (s_mod * index) & (unsigned)(sdrk::OLS_N - 1);
                               return fir_launch(p, in_elem == 4, d_in, cn, decim, shift_bins, (int)phase, d_out, nb, p->stream);
                           });
}

// ---- channel bank: C tuned channels from one pass over the input (kernels_ols_bank.h) ----
int check_bank_call(const sdrk_plan* p, int decim, int n_chan, const int* shift_bins) {
    int st = check_fir_call(p, decim, 0);
    if (st != SDRK_OK) return st;
    if (n_chan < 1 || n_chan > sdrk::OLS_BANK_MAX_CHAN)
        return fail(SDRK_ERR_INVALID, "n_chan=%d: must be in [1, %d]", n_chan, sdrk::OLS_BANK_MAX_CHAN);
    if (!shift_bins) return fail(SDRK_ERR_INVALID, "shift_bins pointer is NULL");
    for (int c = 0; c < n_chan; ++c)
        if (shift_bins[c] < -sdrk::OLS_N / 2 || shift_bins[c] >= sdrk::OLS_N / 2)
            return fail(SDRK_ERR_INVALID, "shift_bins[%d]=%d: must be in [%d, %d]", c, shift_bins[c], -sdrk::OLS_N / 2, sdrk::OLS_N / 2 - 1);
    return SDRK_OK;
}

int check_bank_device(const sdrk_plan* p, const void* d_in, size_t n_in, int decim, int n_chan, const int* shift_bins,
                      const void* d_out, size_t out_stride) {
    int st = check_bank_call(p, decim, n_chan, shift_bins);
    if (st == SDRK_OK) st = check_fir_device(p, d_in, n_in, decim, 0, d_out);
    if (st != SDRK_OK) return st;
    const size_t n_out = sdrk::ols_outputs(n_in, p->fir_taps, decim);
    if (out_stride < n_out) return fail(SDRK_ERR_INVALID, "out_stride=%zu: a plane holds the %zu outputs of a channel", out_stride, n_out);
    return SDRK_OK;
}

// One launch: the first max_blocks blocks (0: all) of every channel; phase0 == nullptr: zeros.
int bank_launch(sdrk_plan* p, bool i16, const void* d_in, size_t n_in, int decim, int n_chan, const int* shift_bins, const int* phase0,
                void* d_out, size_t out_stride, size_t max_blocks, hipStream_t stream) {
    static const int zeros[sdrk::OLS_BANK_MAX_CHAN] = {};
    sdrk::OlsBankArgs a;
    a.d_in = d_in;
    a.n_in = n_in;
    a.taps = p->fir_taps;
    a.decim = decim;
    a.n_chan = n_chan;
    a.shift_bins = shift_bins;
    a.phase0 = phase0 ? phase0 : zeros;
    a.d_h = p->d_fir_h;
    a.d_twiddle = p->d_twiddle;
    a.d_out = static_cast<float2*>(d_out);
    a.out_stride = out_stride;
    a.max_blocks = max_blocks;
    a.num_cus = p->num_cus;
    a.stream = stream;
    const hipError_t e = i16 ? sdrk::launch_chanbank_i16(a) : sdrk::launch_chanbank(a);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "channel bank kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

int exec_device_bank(bool i16, sdrk_plan* p, const void* d_in, size_t n_in, int decim, int n_chan, const int* shift_bins,
                     const int* phase0, void* d_out, size_t out_stride, void* stream) {
    int st = check_bank_device(p, d_in, n_in, decim, n_chan, shift_bins, d_out, out_stride);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return bank_launch(p, i16, d_in, n_in, decim, n_chan, shift_bins, phase0, d_out, out_stride, 0,
                       stream ? static_cast<hipStream_t>(stream) : p->stream);
}

// The chunk loop of the single call with C planes: per chunk, channel c's phase is s_c times the chunk's stream index.
int exec_host_bank(size_t in_elem, sdrk_plan* p, const void* prefix, const void* iq, size_t n, int decim, int n_chan,
                   const int* shift_bins, uint64_t sample0, void* out, size_t out_stride, size_t* n_out) {
    int st = check_bank_call(p, decim, n_chan, shift_bins);
    if (st != SDRK_OK) return st;
    const size_t need = (n + (size_t)decim - 1) / (size_t)decim;
    if (out_stride < need) return fail(SDRK_ERR_INVALID, "out_stride=%zu: a plane holds up to %zu outputs of a channel", out_stride, need);
    return host_fir_chunks(in_elem, p, prefix, iq, n, decim, sample0, (size_t)n_chan, out, out_stride, n_out,
                           [&](const void* d_in, size_t cn, unsigned index, void* d_out, size_t nb, size_t co) {
                               int phase[sdrk::OLS_BANK_MAX_CHAN];
                               for (int c = 0; c < n_chan; ++c) {
                                   const unsigned s_mod = (unsigned)shift_bins[c] & (unsigned)(sdrk::OLS_N - 1);
                                   phase[c] = (int)((s_mod * index) & (unsigned)(sdrk::OLS_N - 1));
                               }
                               return bank_launch(p, in_elem == 4, d_in, cn, decim, n_chan, shift_bins, phase, d_out, co, nb, p->stream);
                           });
}

}  // namespace

extern "C" {

int sdrk_plan_set_fir(sdrk_plan* p, int ntaps, const void* taps_c64) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (ntaps < 1 || ntaps > sdrk::OLS_MAX_TAPS) return fail(SDRK_ERR_INVALID, "ntaps=%d: must be in [1, %d]", ntaps, sdrk::OLS_MAX_TAPS);
    if (!taps_c64) return fail(SDRK_ERR_INVALID, "taps pointer is NULL");
    // H = DFT_4096(taps zero-padded) in float64, rounded once: exact table angles, H[k] = sum_t h[t] W4096^((k t) mod 4096)
    constexpr int N = sdrk::OLS_N;
    std::vector<double> wr(N), wi(N);
    for (int m = 0; m < N; ++m) {
        const double ang = -2.0 * 3.14159265358979323846 * (double)m / (double)N;
        wr[m] = cos(ang);
        wi[m] = sin(ang);
    }
    const float* h = static_cast<const float*>(taps_c64);
    std::vector<float2> H(N);
    for (int k = 0; k < N; ++k) {
        double re = 0.0, im = 0.0;
        for (int t = 0; t < ntaps; ++t) {
            const int m = (k * t) & (N - 1);
            const double hr = h[2 * t], hi = h[2 * t + 1];
            re += hr * wr[m] - hi * wi[m];
            im += hr * wi[m] + hi * wr[m];
        }
        H[k] = make_float2((float)re, (float)im);
    }
    HIP_TRY(hipSetDevice(p->device));
    // not with work in flight, says the header; make it safe all the same for work on the plan's own stream
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->fir_taps = 0;
    if (!p->d_fir_h) HIP_TRY(hipMalloc((void**)&p->d_fir_h, N * sizeof(float2)));
    HIP_TRY(hipMemcpy(p->d_fir_h, H.data(), N * sizeof(float2), hipMemcpyHostToDevice));
    p->fir_taps = ntaps;
    p->fir_assign = fir_assign_default();
    return SDRK_OK;
}

int sdrk_plan_fir_taps(const sdrk_plan* p) { return p ? p->fir_taps : fail(SDRK_ERR_INVALID, "plan is NULL"); }

int sdrk_exec_device_fir(sdrk_plan* p, const void* d_in_c64, size_t n_in, int decim, int shift_bins, int phase0, void* d_out_c64,
                         void* stream) {
    return exec_device_fir(false, p, d_in_c64, n_in, decim, shift_bins, phase0, d_out_c64, stream);
}

int sdrk_exec_device_fir_ci16(sdrk_plan* p, const void* d_in_ci16, size_t n_in, int decim, int shift_bins, int phase0,
                              void* d_out_c64, void* stream) {
    return exec_device_fir(true, p, d_in_ci16, n_in, decim, shift_bins, phase0, d_out_c64, stream);
}

int sdrk_exec_device_fir_timed_each(sdrk_plan* p, const void* d_in_c64, size_t n_in, int decim, int shift_bins, int phase0,
                                    void* d_out_c64, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_fir_device(p, d_in_c64, n_in, decim, shift_bins, d_out_c64);
    if (st != SDRK_OK) return st;
    return timed_each(p, launches, each_ms,
                      [&] { return fir_launch(p, false, d_in_c64, n_in, decim, shift_bins, phase0, d_out_c64, 0, p->stream); });
}

int sdrk_exec_host_fir(sdrk_plan* p, const void* prefix_c64, const void* iq_c64, size_t n, int decim, int shift_bins,
                       uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_fir(sizeof(float2), p, prefix_c64, iq_c64, n, decim, shift_bins, sample0, out_c64, n_out);
}

int sdrk_exec_host_fir_ci16(sdrk_plan* p, const void* prefix_ci16, const void* iq_ci16, size_t n, int decim, int shift_bins,
                            uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_fir(4, p, prefix_ci16, iq_ci16, n, decim, shift_bins, sample0, out_c64, n_out);
}

int sdrk_exec_device_chanbank(sdrk_plan* p, const void* d_in_c64, size_t n_in, int decim, int n_chan, const int* shift_bins,
                              const int* phase0, void* d_out_c64, size_t out_stride, void* stream) {
    return exec_device_bank(false, p, d_in_c64, n_in, decim, n_chan, shift_bins, phase0, d_out_c64, out_stride, stream);
}

int sdrk_exec_device_chanbank_ci16(sdrk_plan* p, const void* d_in_ci16, size_t n_in, int decim, int n_chan, const int* shift_bins,
                                   const int* phase0, void* d_out_c64, size_t out_stride, void* stream) {
    return exec_device_bank(true, p, d_in_ci16, n_in, decim, n_chan, shift_bins, phase0, d_out_c64, out_stride, stream);
}

int sdrk_exec_device_chanbank_timed_each(sdrk_plan* p, const void* d_in_c64, size_t n_in, int decim, int n_chan, const int* shift_bins,
                                         const int* phase0, void* d_out_c64, size_t out_stride, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_bank_device(p, d_in_c64, n_in, decim, n_chan, shift_bins, d_out_c64, out_stride);
    if (st != SDRK_OK) return st;
    return timed_each(p, launches, each_ms, [&] {
        return bank_launch(p, false, d_in_c64, n_in, decim, n_chan, shift_bins, phase0, d_out_c64, out_stride, 0, p->stream);
    });
}

int sdrk_exec_host_chanbank(sdrk_plan* p, const void* prefix_c64, const void* iq_c64, size_t n, int decim, int n_chan,
                            const int* shift_bins, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out) {
    return exec_host_bank(sizeof(float2), p, prefix_c64, iq_c64, n, decim, n_chan, shift_bins, sample0, out_c64, out_stride, n_out);
}

int sdrk_exec_host_chanbank_ci16(sdrk_plan* p, const void* prefix_ci16, const void* iq_ci16, size_t n, int decim, int n_chan,
                                 const int* shift_bins, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out) {
    return exec_host_bank(4, p, prefix_ci16, iq_ci16, n, decim, n_chan, shift_bins, sample0, out_c64, out_stride, n_out);
}

}  // extern "C"

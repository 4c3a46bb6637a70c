// integrate_call.h — the machinery of an integrated-spectrum call (one row per K frames), shared by the four modes of
// integrate_api.hip: complex64 or int16 I,Q samples, plain frames or frames folded by the plan's polyphase filter bank.  An
// IntIo says what differs between them, the way HostIo (plan_internal.h) does for exec_host: the bytes per input sample, the
// launcher of the N = 4096 kernel that reduces inside the transform, and the plan's own transform for every other length.
// The spectral-kurtosis calls (sdrk_exec_*_sk*) are the same call with other kernels behind it: an IntIo also names the
// reduction down the columns of staged spectra, the finalize of split groups, and how many planes of nfft floats a group gives.
// The two-channel cross-spectrum calls (sdrk_exec_*_xspec*) are the same call once more: their input is a stream of elements
// (both channels' sample n side by side), their unit state is four floats per bin, and their staged route de-interleaves a chunk
// of frames (kernels_xspec.h) and runs the plan's transform once per channel before the column kernel takes both spectra.
// The correlation-matrix calls (sdrk_exec_*_corrmat*) carry that to C = 2..8 channels per element: C * C floats of unit state
// and as many planes, C spectra per frame in staging — written by corrmat4096.hip straight from the element stream at N = 4096,
// by the split and the plan's transform elsewhere — and the column kernel of corrmat_rows.hip over them (kernels_corrmat.h).
//
// N = 4096 runs the fused kernel on the caller's samples: one launch, plus a finalize when the groups are too few to fill the
// device and were cut into slices (integrate_split.h).  Every other length (chirp-z included) runs "the plan's own transform
// with EPI_COMPLEX into at most 64 MiB of plan-owned staging, then integrate_rows.hip down the columns", chunk by chunk at
// frame boundaries.  A unit that a chunk boundary cuts is carried: its accumulator state goes to one of two carry rows
// (launch i writes row (i + 1) & 1, launch i + 1 reads it) and the next launch continues from it, so the result does not
// depend on where the chunks were cut.  The numpy boundary feeds the same machinery through the three pinned staging slots of
// sdrk_host_pipeline.hip, in device memory that does not grow with the stream.  Host code only; not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernels_corrmat.h"
#include "kernels_integrate.h"
#include "kernels_xspec.h"
#include "plan_internal.h"

namespace sdrk_host {

struct IntIo {
    size_t in_elem = 0;                                            // bytes per input sample: 8 (complex64) or 4 (int16 I,Q)
    hipError_t (*fused)(const sdrk::IntegrateArgs&) = nullptr;     // N = 4096: the reduction inside the transform
    LaunchFn transform = nullptr;                                  // every other length: the plan's transform (EPI_COMPLEX)
    size_t in_span = 0;                                            // input samples a frame reads from its start (0: nfft;
                                                                   // the filter bank: taps * nfft)
    // the reduction over staged spectra and the finalize of split groups; planes of nfft float32 per output group; the fewest
    // frames a group may have (spectral kurtosis: launch_sk_rows, launch_sk_finalize, 2 planes, 2 frames; no fused kernel
    // behind the filter bank: N = 4096 then takes the staged route)
    hipError_t (*rows)(const sdrk::IntegrateArgs&) = sdrk::launch_integrate_rows;
    decltype(&sdrk::launch_integrate_finalize) finalize = sdrk::launch_integrate_finalize;
    size_t planes = 1;
    size_t min_k = 1;
    // floats of unit state per bin: the size of the carry rows and the partial rows (cross-spectra: 4)
    size_t state = 2;
    // two-channel element input (in_elem 16: complex64, 8: int16): the column kernel over both channels' staged spectra; the
    // staged route then splits each chunk's frames into packed complex64 frames per channel first, at most INT_STAGE_BYTES of
    // them beside at most INT_STAGE_BYTES of spectra, and `rows` is not used
    hipError_t (*rows2)(const sdrk::IntegrateArgs&, const float2*) = nullptr;
    // C-channel element input (the correlation matrix; in_elem = channels * bytes of a sample of format `fmt`, a sdrk::CmFormat):
    // state and planes are channels * channels, every route is staged — channels spectra per frame share the INT_STAGE_BYTES (one
    // frame of all channels where that is more), N = 4096 fills them with launch_corrmat4096_spectra from the caller's elements,
    // every other length splits into as much again and runs `transform` per channel — and launch_corrmat_rows /
    // launch_corrmat_finalize stand where rows / rows2 / finalize do, which are not used
    int channels = 0;
    int fmt = 0;
    // elements of a row, a state row and a staged spectrum (0: nfft).  Real-sampled input (ci16_api.hip): nfft + 1 bins from 0 to
    // fs/2; in_elem is then a pair of samples, `transform` writes packed complex64 rows of `bins`, and real_fmt (a
    // sdrk::REAL_* value) tells the fused launcher what the pairs are
    size_t bins = 0;
    int real_fmt = 0;
};

constexpr size_t INT_STAGE_BYTES = (size_t)64 << 20;   // complex64 spectra of the generic route, per plan

struct IntCall {
    sdrk_plan* p = nullptr;
    IntIo io;
    size_t n_groups = 0, k = 0, stride = 0;
    int detector = 0, out_form = 0;
    float scale = 1.0f;
    sdrk::IntSplit sp{1, 1};
    bool fused = false;          // the N = 4096 kernel of io.fused
    bool direct = false;         // io.channels at N = 4096: the spectra kernel that reads the element stream itself
    size_t bins = 0;             // elements of a row: io.bins, or nfft
    size_t group_floats = 0;     // float32 per output group: io.planes * bins
    size_t stage_frames = 0;     // generic route: frames per staging chunk
    unsigned launches = 0;       // reduction launches so far: picks the carry rows
    hipStream_t stream = nullptr;
    float2* carry[2] = {nullptr, nullptr};
    float2* partials = nullptr;
};

inline int check_int_args(const sdrk_plan* p, const void* in, size_t n_groups, size_t k, size_t stride, int detector, int out_form,
                          const void* out) {
    if (detector != SDRK_DET_MEAN && detector != SDRK_DET_MAX && detector != SDRK_DET_MIN)
        return fail(SDRK_ERR_INVALID, "detector %d is none of SDRK_DET_MEAN / _MAX / _MIN", detector);
    if (out_form != SDRK_INT_OUT_DB && out_form != SDRK_INT_OUT_POWER)
        return fail(SDRK_ERR_INVALID, "out_form %d is neither SDRK_INT_OUT_DB nor SDRK_INT_OUT_POWER", out_form);
    if (n_groups == 0 || k == 0) return fail(SDRK_ERR_INVALID, "n_groups and k_frames must be >= 1");
    if (k > ((size_t)1 << 40) || n_groups > (~(size_t)0 >> 1) / k)
        return fail(SDRK_ERR_INVALID, "n_groups * k_frames is out of range");
    if (stride == 0) return fail(SDRK_ERR_INVALID, "frame_stride must be >= 1");
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    if (int st = check_precision(p, 32); st != SDRK_OK) return st;
    if (!in || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    return SDRK_OK;
}

// ... of a call through `io`: the detector is the caller's where the mode has one
inline int check_call_args(const IntIo& io, const sdrk_plan* p, const void* in, size_t n_groups, size_t k, size_t stride, int detector,
                           int out_form, const void* out) {
    int st = check_int_args(p, in, n_groups, k, stride, detector, out_form, out);
    if (st == SDRK_OK && k < io.min_k)
        return fail(SDRK_ERR_INVALID, "k_frames must be >= %zu: the spectral-kurtosis estimator divides by k_frames - 1", io.min_k);
    return st;
}

inline int call_begin(IntCall& c, const IntIo& io, sdrk_plan* p, size_t n_groups, size_t k, size_t stride, int detector,
                      int out_form, float scale, hipStream_t stream) {
    c.p = p;
    c.io = io;
    c.n_groups = n_groups;
    c.k = k;
    c.stride = stride;
    c.detector = detector;
    c.out_form = out_form;
    c.scale = scale;
    c.stream = stream;
    const size_t nfft = (size_t)p->nfft;
    const bool f4k = p->nfft == 4096 && !p->blu_inner;
    c.fused = f4k && io.fused != nullptr;
    // N = 4096 with channels: the spectra kernel that reads the elements itself, except where the split route measured faster
    // (cm4k_reads_directly, kernels_corrmat.h).  SDRK_CORRMAT_ROUTE=split / =direct picks one for tools/bench_corrmat.py, which
    // measures both; the bits are the same either way.
    const char* const route = io.channels ? std::getenv("SDRK_CORRMAT_ROUTE") : nullptr;
    c.direct = f4k && io.channels &&
               (route && std::strcmp(route, "split") == 0    ? false
                : route && std::strcmp(route, "direct") == 0 ? true
                                                             : sdrk::cm4k_reads_directly(io.fmt, io.channels));
    c.bins = io.bins ? io.bins : nfft;
    const size_t bins = c.bins;
    c.group_floats = io.planes * bins;
    // the generic route has nfft / 256 workgroups per unit to spread: it splits later than the fused kernel.  The C-channel
    // calls make the two-channel call's cut at every length, so that a pair's planes are that call's bits.
    const size_t ways = c.fused || (f4k && io.channels) ? 1 : (nfft + 255) / 256;
    c.sp = n_groups > (~(size_t)0) / ways ? sdrk::IntSplit{1, k} : sdrk::integrate_split(n_groups * ways, k, p->num_cus);
    const size_t row = bins * sizeof(float2);              // a staged spectrum
    const size_t state_row = bins * io.state * sizeof(float);
    const size_t n_partials = c.sp.slices > 1 ? n_groups * c.sp.slices : 0;
    Staging& sg = p->integ;   // buf[0]: carry and partial rows; buf[1]: spectra of the generic route
    int st = sg.reserve(0, (2 + n_partials) * state_row);
    if (st != SDRK_OK) return st;
    if (!c.fused) {
        // (two channels: both spectra of a frame share the 64 MiB, and the split frames take as much again behind them)
        const size_t chans = io.channels ? (size_t)io.channels : io.rows2 ? 2 : 1;
        const size_t per_frame = chans * row;
        c.stage_frames = INT_STAGE_BYTES / per_frame ? INT_STAGE_BYTES / per_frame : 1;
        if (c.stage_frames > n_groups * k) c.stage_frames = n_groups * k;
        // (element input: the split frames behind the spectra, unless the spectra kernel reads the elements itself)
        st = sg.reserve(1, c.stage_frames * per_frame * (chans > 1 && !c.direct ? 2 : 1));
        if (st != SDRK_OK) return st;
    }
    c.carry[0] = static_cast<float2*>(sg.buf[0].d);
    // (rows of bins * state floats: counted in floats, an odd length times an odd state is no whole number of float2)
    float* const rows = static_cast<float*>(sg.buf[0].d);
    c.carry[1] = reinterpret_cast<float2*>(rows + bins * io.state);
    c.partials = reinterpret_cast<float2*>(rows + 2 * bins * io.state);
    return sg.enter(stream);   // one state and one staging per plan: a call on another stream waits for the last one's work
}

// The frames [f0, f1) of the call, d_in at frame f0's first sample.  Rows of the groups that end in the range go to
// d_out + (group - out_row0) * group_floats (unsplit calls only).
inline int call_range(IntCall& c, const void* d_in, size_t f0, size_t f1, float* d_out, size_t out_row0) {
    sdrk_plan* p = c.p;
    sdrk::IntegrateArgs a;
    a.k = c.k;
    a.slices = c.sp.slices;
    a.slice_len = c.sp.len;
    a.detector = c.detector;
    a.out_form = c.out_form;
    a.scale = c.scale;
    a.eps = p->eps;
    a.d_out = d_out;
    a.out_row0 = out_row0;
    a.d_partials = c.partials;
    a.nfft = (int)c.bins;
    a.d_window = p->d_window;
    a.d_twiddle = p->d_twiddle;
    a.shift = p->shift;
    a.num_cus = p->num_cus;
    a.stream = c.stream;
    a.d_pfb_h = p->d_pfb_h;   // (read by the polyphase-filter-bank launcher alone)
    a.pfb_taps = p->pfb_taps;
    a.d_real_window = p->d_real_win;   // (read by the real-input launcher alone)
    a.d_real_tab = p->d_real_tab;
    a.real_fmt = c.io.real_fmt;
    const size_t step = c.fused ? f1 - f0 : c.stage_frames;
    for (size_t s0 = f0; s0 < f1; s0 += step) {
        const size_t s1 = f1 - s0 < step ? f1 : s0 + step;
        const void* src = static_cast<const char*>(d_in) + (s0 - f0) * c.stride * c.io.in_elem;
        a.f0 = s0;
        a.f1 = s1;
        a.d_carry_in = c.carry[c.launches & 1];
        a.d_carry_out = c.carry[(c.launches + 1) & 1];
        ++c.launches;
        hipError_t e;
        if (c.fused) {
            a.d_in = src;
            a.in_stride = c.stride;
            e = c.io.fused(a);
        } else if (c.io.rows2) {   // [spectra 0][spectra 1][frames 0][frames 1], stage_frames frames each
            const size_t n = s1 - s0, plane = c.stage_frames * (size_t)p->nfft;
            float2* const spec0 = static_cast<float2*>(p->integ.buf[1].d);
            float2 *const spec1 = spec0 + plane, *const x0 = spec1 + plane, *const x1 = x0 + plane;
            e = sdrk::launch_xspec_split(src, c.io.in_elem == 8, n, c.stride, p->nfft, x0, x1, p->num_cus, c.stream);
            if (e != hipSuccess) return fail(SDRK_ERR_HIP, "cross-spectrum split launch failed: %s", hipGetErrorString(e));
            int st = c.io.transform(p, x0, n, (size_t)p->nfft, spec0, sdrk::EPI_COMPLEX, c.stream);
            if (st == SDRK_OK) st = c.io.transform(p, x1, n, (size_t)p->nfft, spec1, sdrk::EPI_COMPLEX, c.stream);
            if (st != SDRK_OK) return st;
            a.d_in = spec0;
            a.in_stride = (size_t)p->nfft;
            e = c.io.rows2(a, spec1);
        } else if (c.io.channels) {   // [spectra 0 .. C-1][frames 0 .. C-1 (split route)], stage_frames frames each
            const size_t n = s1 - s0, plane = c.stage_frames * (size_t)p->nfft, chans = (size_t)c.io.channels;
            float2* const spec = static_cast<float2*>(p->integ.buf[1].d);
            if (c.direct) {
                a.d_in = src;
                a.in_stride = c.stride;
                e = sdrk::launch_corrmat4096_spectra(a, c.io.fmt, c.io.channels, spec, plane);
                if (e != hipSuccess) return fail(SDRK_ERR_HIP, "correlation-matrix spectra launch failed: %s", hipGetErrorString(e));
            } else {
                float2* const x = spec + chans * plane;
                e = sdrk::launch_corrmat_split(src, c.io.fmt, c.io.channels, n, c.stride, p->nfft, x, plane, p->num_cus, c.stream);
                if (e != hipSuccess) return fail(SDRK_ERR_HIP, "correlation-matrix split launch failed: %s", hipGetErrorString(e));
                for (size_t ch = 0; ch < chans; ++ch) {
                    int st = c.io.transform(p, x + ch * plane, n, (size_t)p->nfft, spec + ch * plane, sdrk::EPI_COMPLEX, c.stream);
                    if (st != SDRK_OK) return st;
                }
            }
            a.d_in = spec;
            a.in_stride = (size_t)p->nfft;
            e = sdrk::launch_corrmat_rows(a, c.io.channels, plane);
        } else {
            void* const d_stage = p->integ.buf[1].d;
            int st = c.io.transform(p, src, s1 - s0, c.stride, d_stage, sdrk::EPI_COMPLEX, c.stream);
            if (st != SDRK_OK) return st;
            a.d_in = d_stage;
            a.in_stride = c.bins;
            e = c.io.rows(a);
        }
        if (e != hipSuccess) return fail(SDRK_ERR_HIP, "integrate kernel launch failed: %s", hipGetErrorString(e));
    }
    return SDRK_OK;
}

// Split calls: every group's partial rows -> its row.
inline int call_finalize(IntCall& c, float* d_out) {
    if (c.sp.slices == 1) return SDRK_OK;
    const hipError_t e =
        c.io.channels ? sdrk::launch_corrmat_finalize(reinterpret_cast<const float*>(c.partials), c.io.channels, c.n_groups, c.k,
                                                      c.sp.slices, c.p->nfft, c.scale, d_out, c.p->num_cus, c.stream)
                      : c.io.finalize(c.partials, c.n_groups, c.k, c.sp.slices, (int)c.bins, c.detector, c.out_form, c.scale,
                                      c.p->eps, d_out, c.p->num_cus, c.stream);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "integrate finalize launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

inline int call_end(IntCall& c, int st) {   // (also after a failed launch: earlier launches are in flight)
    return c.p->integ.leave(c.stream, st);
}

inline int device_call(const IntIo& io, sdrk_plan* p, const void* d_iq, size_t n_groups, size_t k, size_t stride, int detector,
                       int out_form, float scale, float* d_out, hipStream_t stream) {
    IntCall c;
    int st = call_begin(c, io, p, n_groups, k, stride, detector, out_form, scale, stream);
    if (st != SDRK_OK) return st;
    st = call_range(c, d_iq, 0, n_groups * k, d_out, 0);
    if (st == SDRK_OK) st = call_finalize(c, d_out);
    return call_end(c, st);
}

// ---- the three entry points of a format, behind their names ----

inline int exec_device_integrated(const IntIo& io, sdrk_plan* p, const void* d_iq, size_t n_groups, size_t k_frames,
                                  size_t frame_stride, int detector, int out_form, float scale, float* d_out, void* stream) {
    int st = check_call_args(io, p, d_iq, n_groups, k_frames, frame_stride, detector, out_form, d_out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return device_call(io, p, d_iq, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out,
                       stream ? static_cast<hipStream_t>(stream) : p->stream);
}

inline int exec_device_integrated_timed_each(const IntIo& io, sdrk_plan* p, const void* d_iq, size_t n_groups, size_t k_frames,
                                             size_t frame_stride, int detector, int out_form, float scale, float* d_out,
                                             int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_call_args(io, p, d_iq, n_groups, k_frames, frame_stride, detector, out_form, d_out);
    if (st != SDRK_OK) return st;
    st = timed_each(p, launches, each_ms, [&] {
        return device_call(io, p, d_iq, n_groups, k_frames, frame_stride, detector, out_form, scale, d_out, p->stream);
    });
    return st == SDRK_OK ? fused_check(p) : st;
}

// The numpy boundary.  Chunks of about HOST_CHUNK_BYTES of input, cut at frame boundaries wherever they fall within a group,
// go through the three staging slots: (helper threads: pageable -> pinned) -> H2D on the copy stream -> reduction on the plan's
// stream -> the rows of the groups that ended in the chunk D2H on the other copy stream.  Everything is asynchronous, so the
// H2D of chunk c + 1 runs beside the transform of chunk c; a slot is reused once its chunk's rows have arrived.
inline int exec_host_integrated(const IntIo& io, sdrk_plan* p, const void* iq, size_t n_groups, size_t k_frames,
                                size_t frame_stride, int detector, int out_form, float scale, float* out) {
    int st = check_call_args(io, p, iq, n_groups, k_frames, frame_stride, detector, out_form, out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    SlotPipe pipe;
    st = pipe.open(p, "host pipeline");
    if (st != SDRK_OK) return st;
    IntCall c;
    st = call_begin(c, io, p, n_groups, k_frames, frame_stride, detector, out_form, scale, p->stream);
    if (st != SDRK_OK) return st;
    const size_t nfft = (size_t)p->nfft, K = k_frames, n_frames = n_groups * K, elem = io.in_elem;
    const size_t group_bytes = c.group_floats * sizeof(float);
    const size_t span = io.in_span ? io.in_span : nfft;   // a chunk carries its span - nfft samples of overlap
    const bool direct = c.sp.slices == 1;   // rows leave per chunk; split calls finalize once at the end
    // frames per chunk: bounded by the input bytes and, through the rows a chunk can complete, by the output bytes
    size_t per = HOST_CHUNK_BYTES / (frame_stride * elem);
    size_t rows_cap = HOST_CHUNK_BYTES / group_bytes;
    if (rows_cap < 1) rows_cap = 1;
    if (per / K >= rows_cap) per = rows_cap * K;
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    const size_t chunk_in = ((per - 1) * frame_stride + span) * elem;
    const size_t chunk_out = direct ? (per / K + 1) * group_bytes : 0;
    const size_t in_bytes = ((n_frames - 1) * frame_stride + span) * elem;
    const size_t out_bytes = n_groups * group_bytes;
    const bool in_pinned = pinned_ranges().covers(iq, in_bytes), out_pinned = pinned_ranges().covers(out, out_bytes);
    const ChunkOut::Rows via = out_pinned ? ChunkOut::Direct : ChunkOut::Pooled;
    for (size_t f0 = 0; f0 < n_frames; f0 += per) {
        const size_t f1 = n_frames - f0 < per ? n_frames : f0 + per;
        const size_t cin = ((f1 - f0 - 1) * frame_stride + span) * elem;
        // (a chunk in which no group ends brings back 0 bytes: its slot still completes through the D2H stream)
        const size_t row0 = f0 / K, rows = direct ? f1 / K - row0 : 0, cout = rows * group_bytes;
        HostSlot* s = nullptr;
        st = pipe.acquire(chunk_in, chunk_out, s);
        if (st != SDRK_OK) return call_end(c, st);
        const void* src = chunk_pinned_src(*s, static_cast<const char*>(iq) + f0 * frame_stride * elem, cin, in_pinned);
        st = pipe.upload(*s, src, cin);
        if (st == SDRK_OK)
            st = pipe.submit(*s, call_range(c, s->d_in, f0, f1, static_cast<float*>(s->d_out), row0),
                             {via, out + row0 * c.group_floats, cout});
        if (st != SDRK_OK) return call_end(c, st);
    }
    st = pipe.drain();
    if (st != SDRK_OK) return call_end(c, st);
    if (!direct) {   // fewer groups than the device has workgroups: a handful of rows
        auto bail = [&](int status) { slots_abandon(p); return call_end(c, status); };
        HostSlot& s = p->slot[0];
        st = slot_reserve(p, s, 0, out_bytes);
        if (st == SDRK_OK) st = call_finalize(c, static_cast<float*>(s.d_out));
        if (st != SDRK_OK) return bail(st);
        hipError_t e = hipMemcpyAsync(out, s.d_out, out_bytes, hipMemcpyDeviceToHost, p->stream);
        if (e != hipSuccess) return bail(fail(SDRK_ERR_HIP, "host pipeline failed: %s", hipGetErrorString(e)));
    }
    st = call_end(c, SDRK_OK);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->integ.busy = false;
    return fused_check(p);
}

}  // namespace sdrk_host

// sdrk_host_pipeline.hip — the numpy boundary of include/sdrk.h (sdrk_exec_host, sdrk_exec_fft_host, sdrk_welch_psd_host and,
// through sdrk_host::exec_host, their float64 forms): the small mapped call, zero-copy chunks, and SlotPipe — the order in which
// a chunk goes through the three pinned staging slots — which the chunked paths of sdrk_features.hip, integrate_call.h and
// fir_api.hip run on as well.  Host code only.
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_pool.h"
#include "kernels.h"
#include "plan_internal.h"

using namespace sdrk_host;

namespace sdrk_host {

int slot_reserve(sdrk_plan* p, HostSlot& s, size_t in_bytes, size_t out_bytes) {
    if (!s.ev_in) {
        HIP_TRY(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.ev_k, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    }
    if (in_bytes > s.in_cap) {
        if (s.h_in) HIP_TRY(hipHostFree(s.h_in));
        if (s.d_in) HIP_TRY(hipFree(s.d_in));
        s.h_in = s.d_in = nullptr;
        s.in_cap = 0;
        HIP_TRY(hipHostMalloc(&s.h_in, in_bytes, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&s.d_in, in_bytes));
        s.in_cap = in_bytes;
    }
    if (out_bytes > s.out_cap) {
        if (s.h_out) HIP_TRY(hipHostFree(s.h_out));
        if (s.d_out) HIP_TRY(hipFree(s.d_out));
        s.h_out = s.d_out = nullptr;
        s.out_cap = 0;
        HIP_TRY(hipHostMalloc(&s.h_out, out_bytes, hipHostMallocDefault));
        HIP_TRY(hipMalloc(&s.d_out, out_bytes));
        s.out_cap = out_bytes;
    }
    (void)p;
    return SDRK_OK;
}

void slots_abandon(sdrk_plan* p) {   // error path: nothing may still be writing into the staging buffers
    (void)hipStreamSynchronize(p->s_h2d);
    (void)hipStreamSynchronize(p->stream);
    (void)hipStreamSynchronize(p->s_d2h);
    for (auto& s : p->slot) s.busy = false;
}

const void* chunk_pinned_src(HostSlot& s, const void* src, size_t bytes, bool in_pinned) {
    if (in_pinned) return src;
    sdrk::CopyPool::get().copy(s.h_in, src, bytes);
    return s.h_in;
}

int SlotPipe::open(sdrk_plan* plan, const char* name) {
    p = plan;
    what = name;
    if (!p->s_h2d) {
        HIP_TRY(hipStreamCreateWithFlags(&p->s_h2d, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&p->s_d2h, hipStreamNonBlocking));
    }
    return SDRK_OK;
}

int SlotPipe::hip_failed(hipError_t e) {
    slots_abandon(p);
    return fail(SDRK_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// Wait for the chunk in flight in slot `s` and hand what it brought back to the caller's array.
int SlotPipe::retire(HostSlot& s) {
    if (!s.busy) return SDRK_OK;
    s.busy = false;
    const ChunkOut& o = s.out;
    if (mark) mark(mark_ctx, 0);
    const hipError_t e = hipEventSynchronize(o.rows == ChunkOut::None ? s.ev_k : s.ev_done);
    if (e != hipSuccess) return hip_failed(e);
    if (mark) mark(mark_ctx, 1);
    if (o.rows == ChunkOut::Planes) {
        for (size_t i = 0; i < o.planes; ++i)
            memcpy(static_cast<char*>(o.user) + i * o.plane_stride, static_cast<char*>(s.h_out) + i * o.bytes, o.bytes);
    } else if ((o.rows == ChunkOut::Pooled || o.rows == ChunkOut::Kernel) && o.bytes) {
        sdrk::CopyPool::get().copy(o.user, s.h_out, o.bytes);
    }
    if (mark) mark(mark_ctx, 2);
    return SDRK_OK;
}

int SlotPipe::acquire(size_t chunk_in, size_t chunk_out, HostSlot*& s) {
    s = &p->slot[n % HOST_SLOTS];
    int st = retire(*s);                                       // chunk n - HOST_SLOTS: delivered, slot free
    if (st != SDRK_OK) return st;
    st = slot_reserve(p, *s, chunk_in, chunk_out);
    if (st != SDRK_OK) slots_abandon(p);
    return st;
}

int SlotPipe::upload(HostSlot& s, const void* pinned_src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(s.d_in, pinned_src, bytes, hipMemcpyHostToDevice, p->s_h2d);
    if (e == hipSuccess) e = hipEventRecord(s.ev_in, p->s_h2d);
    if (e == hipSuccess) e = hipStreamWaitEvent(p->stream, s.ev_in, 0);
    return e == hipSuccess ? SDRK_OK : hip_failed(e);
}

int SlotPipe::submit(HostSlot& s, int launch_st, const ChunkOut& out) {
    if (launch_st != SDRK_OK) {
        slots_abandon(p);
        return launch_st;
    }
    hipError_t e;
    if (out.rows == ChunkOut::Kernel) {
        e = hipEventRecord(s.ev_done, p->stream);
    } else {
        e = hipEventRecord(s.ev_k, p->stream);
        if (out.rows != ChunkOut::None) {
            if (e == hipSuccess) e = hipStreamWaitEvent(p->s_d2h, s.ev_k, 0);
            if (e == hipSuccess && out.bytes)
                e = hipMemcpyAsync(out.rows == ChunkOut::Direct ? out.user : s.h_out, s.d_out, out.planes * out.bytes,
                                   hipMemcpyDeviceToHost, p->s_d2h);
            if (e == hipSuccess) e = hipEventRecord(s.ev_done, p->s_d2h);
        }
    }
    if (e != hipSuccess) return hip_failed(e);
    s.busy = true;
    s.out = out;
    ++n;
    return SDRK_OK;
}

int SlotPipe::drain() {
    for (size_t i = 0; i < HOST_SLOTS; ++i)
        if (int st = retire(p->slot[(n + i) % HOST_SLOTS]); st != SDRK_OK) return st;
    return SDRK_OK;
}

namespace {

struct HostTrace {   // SDRK_HOST_TRACE=1: where a pipelined sdrk_exec_host call spends its wall time (stderr)
    bool on = false;
    double t_in = 0, t_wait = 0, t_out = 0, t_mark = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    static void mark(void* ctx, int point) {   // SlotPipe's hook: a retire's wait ends at point 1, its delivery at point 2
        HostTrace& tr = *static_cast<HostTrace*>(ctx);
        const double t = now();
        if (point == 1) tr.t_wait += t - tr.t_mark;
        if (point == 2) tr.t_out += t - tr.t_mark;
        tr.t_mark = t;
    }
};

}  // namespace

// The numpy boundary.  Small calls (the live app's one 4096-sample buffer, streamer.py:114-121): the
// kernel reads and writes pinned mapped host memory, no DMA copies.  Everything else: the frames go
// through in chunks of ~16 MiB, HOST_SLOTS of them in flight — helper threads copy the caller's pageable
// memory into a pinned slot, then H2D (copy stream) -> transform (plan stream) -> D2H (copy stream) run
// asynchronously, chained by events, while the host stages the next chunk and drains finished ones.
// H2D of chunk c+1 overlaps D2H of chunk c (PCIe is full duplex) and both overlap the staging memcpys.
// Element sizes, the launch and the kernels that may read host memory themselves come from `io` (float32 and float64 plans).
int exec_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, void* out, const HostIo& io) {
    int st = check_exec_args(p, iq, n_frames, frame_stride, out, io.precision);
    if (st != SDRK_OK || n_frames == 0) return st;
    if (n_frames > p->max_batch)
        return fail(SDRK_ERR_INVALID, "n_frames %zu exceeds the plan's max_batch %zu", n_frames,
                    p->max_batch);
    HIP_TRY(hipSetDevice(p->device));
    const size_t nfft = (size_t)p->nfft;
    const size_t span = io.in_span ? io.in_span : nfft;   // samples a frame reads from its start
    const size_t bins = io.out_bins ? io.out_bins : nfft;   // output bins of a frame's row
    const size_t in_samples = (n_frames - 1) * frame_stride + span;
    const size_t in_elem = io.in_elem, out_elem = io.out_elem;
    const int epilogue = io.epilogue;
    const size_t in_bytes = in_samples * in_elem;
    const size_t out_bytes = n_frames * bins * out_elem;
    if (in_bytes <= SMALL_IN_BYTES && out_bytes <= SMALL_IN_BYTES && p->nfft <= 4096 && !p->blu_inner && !io.out_bins) {
        if (!p->h_small_in) {
            HIP_TRY(hipHostMalloc(&p->h_small_in, SMALL_IN_BYTES, hipHostMallocMapped));
            HIP_TRY(hipHostMalloc(&p->h_small_out, SMALL_IN_BYTES, hipHostMallocMapped));
            void* f = nullptr;
            if (hipHostMalloc(&f, 64, hipHostMallocMapped) == hipSuccess) {
                memset(f, 0, 64);
                p->h_small_flag = static_cast<uint32_t*>(f);
                if (hipHostGetDevicePointer(&p->d_small_flag, f, 0) != hipSuccess) {
                    (void)hipHostFree(f);
                    p->h_small_flag = nullptr;
                }
            }
            (void)hipGetLastError();
        }
        void *d_si = nullptr, *d_so = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&d_si, p->h_small_in, 0));
        HIP_TRY(hipHostGetDevicePointer(&d_so, p->h_small_out, 0));
        memcpy(p->h_small_in, iq, in_bytes);
        st = io.launch(p, d_si, n_frames, frame_stride, d_so, epilogue, p->stream);
        if (st != SDRK_OK) return st;
        // Completion: the stream writes a sequence number into mapped host memory behind the kernel and the caller
        // polls it — for a 10 us job the wake-up path of hipStreamSynchronize costs as much as the job.  Falls back
        // to the synchronize after ~200 us of polling (or if the stream memory operation is not available).
        static const bool poll_ok = getenv("SDRK_SMALL_NOPOLL") == nullptr;
        bool done = false;
        if (poll_ok && p->h_small_flag) {
            const uint32_t seq = ++p->small_seq;
            if (hipStreamWriteValue32(p->stream, p->d_small_flag, seq, 0) == hipSuccess) {
                const uint32_t* flag = p->h_small_flag;
                for (int spins = 0; spins < 200000; ++spins) {
                    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) { done = true; break; }   // (a plain mov on x86: the acquire only binds the compiler)
                    __builtin_ia32_pause();
                }
            } else {
                (void)hipGetLastError();
            }
        }
        if (!done) HIP_TRY(hipStreamSynchronize(p->stream));
        memcpy(out, p->h_small_out, out_bytes);
        return SDRK_OK;
    }
    SlotPipe pipe;
    st = pipe.open(p, "host pipeline");
    if (st != SDRK_OK) return st;
    // frames per chunk: ~HOST_CHUNK_BYTES of input, but at least 4 chunks per call when the call is big
    // enough for the overlap to matter, and never less than one frame
    const size_t stride_bytes = (frame_stride ? frame_stride : 1) * in_elem;
    size_t target = HOST_CHUNK_BYTES;
    if (in_bytes / 4 < target) target = in_bytes / 4 > ((size_t)1 << 20) ? in_bytes / 4 : ((size_t)1 << 20);
    size_t per = target / stride_bytes;
    if (per > target / (bins * out_elem)) per = target / (bins * out_elem);   // heavily overlapped frames: bound the rows too
    if (per < 1) per = 1;
    if (per > n_frames) per = n_frames;
    const size_t chunk_in = ((per - 1) * frame_stride + span) * in_elem;   // (with the span's overlap into the next chunk)
    const size_t chunk_out = per * bins * out_elem;
    sdrk::CopyPool& pool = sdrk::CopyPool::get();
    HostTrace tr;
    { const char* env = getenv("SDRK_HOST_TRACE"); tr.on = env && env[0] == '1'; }
    // Mid-size calls of packed frames on the single-pass kernels: let the transform read the pinned chunk and
    // write the pinned rows itself over PCIe (measured on MI355X, N = 4096: B = 16 48 vs 81 us, B = 256 0.34 vs
    // 0.44 ms against the DMA form; equal at 32 MiB).  Large calls, overlapped frames (the halo would cross PCIe
    // twice) and the two-pass kernels (their 128-byte column segments read host memory at half the DMA rate:
    // 26 vs 48 GB/s at N = 65536) use the copy engines.
    // Caller arrays in pinned memory (sdrk_host_alloc / sdrk_host_register) are not staged: the copy engines read
    // and write them directly.  Decided per side.
    const bool in_pinned = pinned_ranges().covers(iq, in_bytes), out_pinned = pinned_ranges().covers(out, out_bytes);
    const bool zc_length = p->nfft <= io.zero_copy_max_nfft && p->nfft >= io.zero_copy_min_nfft && !io.out_bins;
    const bool zero_copy = zc_length && !p->blu_inner && frame_stride >= nfft && in_bytes <= ZERO_COPY_MAX_BYTES &&
                           !in_pinned && !out_pinned;
    if (in_pinned && out_pinned && zc_length && !p->blu_inner && frame_stride >= nfft &&
        in_bytes <= ZERO_COPY_MAX_BYTES) {
        // both arrays pinned, a call small enough that the link's latency matters more than its last 10 %: ONE launch
        // that reads the caller's frames and writes the caller's rows over PCIe — no staging, no copy engine, no chunks
        void *d_src = nullptr, *d_dst = nullptr;
        if (hipHostGetDevicePointer(&d_src, const_cast<void*>(iq), 0) == hipSuccess &&
            hipHostGetDevicePointer(&d_dst, out, 0) == hipSuccess) {
            st = io.launch(p, d_src, n_frames, frame_stride, d_dst, epilogue, p->stream);
            if (st != SDRK_OK) return st;
            HIP_TRY(hipStreamSynchronize(p->stream));
            return fused_check(p);
        }
        (void)hipGetLastError();   // no device view of the range: take the copy-engine path below
    }
    const double t_call = tr.on ? HostTrace::now() : 0;
    if (tr.on) { pipe.mark = HostTrace::mark; pipe.mark_ctx = &tr; }
    const ChunkOut::Rows rows = zero_copy ? ChunkOut::Kernel : out_pinned ? ChunkOut::Direct : ChunkOut::Pooled;
    for (size_t f0 = 0; f0 < n_frames; f0 += per) {
        const size_t nf = n_frames - f0 < per ? n_frames - f0 : per;
        const size_t cin = ((nf - 1) * frame_stride + span) * in_elem;
        const size_t cout = nf * bins * out_elem;
        HostSlot* sp = nullptr;
        st = pipe.acquire(chunk_in, chunk_out, sp);
        if (st != SDRK_OK) return st;
        HostSlot& s = *sp;
        const double t0 = tr.on ? HostTrace::now() : 0;
        const void* src = static_cast<const char*>(iq) + f0 * frame_stride * in_elem;
        src = chunk_pinned_src(s, src, cin, in_pinned);
        void* user_rows = static_cast<char*>(out) + f0 * bins * out_elem;
        if (tr.on) tr.t_in += HostTrace::now() - t0;
        if (zero_copy) {
            // the transform reads the pinned chunk and writes the pinned rows itself, over PCIe: no DMA-engine
            // copies, two API calls per chunk
            st = pipe.submit(s, io.launch(p, s.h_in, nf, frame_stride, s.h_out, epilogue, p->stream), {rows, user_rows, cout});
        } else {
            st = pipe.upload(s, src, cin);
            if (st == SDRK_OK)
                st = pipe.submit(s, io.launch(p, s.d_in, nf, frame_stride, s.d_out, epilogue, p->stream), {rows, user_rows, cout});
        }
        if (st != SDRK_OK) return st;
    }
    st = pipe.drain();
    if (st != SDRK_OK) return st;
    if (tr.on) {
        const double t = HostTrace::now() - t_call;
        fprintf(stderr, "[sdrk host] %zu chunks of %zu frames, %.1f MiB in: total %.3f ms = stage-in %.3f + wait %.3f + "
                "stage-out %.3f + other %.3f (%.1f GB/s of input, %d helper threads)\n", pipe.n, per,
                in_bytes / 1048576.0, t * 1e3, tr.t_in * 1e3, tr.t_wait * 1e3, tr.t_out * 1e3,
                (t - tr.t_in - tr.t_wait - tr.t_out) * 1e3, in_bytes / t / 1e9, pool.helpers());
    }
    return fused_check(p);
}

// plan_launch as a LaunchFn (declared in plan_internal.h)
int launch_f32(sdrk_plan* p, const void* d_in, size_t n_frames, size_t stride, void* d_out, int epilogue, hipStream_t s) {
    return plan_launch(p, d_in, n_frames, stride, d_out, epilogue, s);
}

namespace {

// the float32 numpy boundary: complex64 in; float32 rows or complex64 out; the single-pass kernels (nfft <= 16384) may read and
// write pinned host memory themselves
HostIo f32_io(int epilogue) {
    HostIo io = frames_io(sizeof(float2), 0, launch_f32, epilogue);
    io.zero_copy_max_nfft = 16384;
    return io;
}

}  // namespace
}  // namespace sdrk_host

extern "C" {

int sdrk_exec_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride, float* out_db) {
    return exec_host(p, iq, n_frames, frame_stride, out_db, f32_io(sdrk::EPI_LOGPSD));
}

int sdrk_exec_fft_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride,
                       void* out_c64) {
    return exec_host(p, iq, n_frames, frame_stride, out_c64, f32_io(sdrk::EPI_COMPLEX));
}

int sdrk_welch_psd_host(sdrk_plan* p, const void* iq, size_t n_frames, size_t frame_stride,
                        float scale, float* out_psd) {
    int st = check_exec_args(p, iq, n_frames, frame_stride, out_psd);
    if (st != SDRK_OK) return st;
    if (n_frames == 0) return fail(SDRK_ERR_INVALID, "welch needs at least one frame");
    if (n_frames > p->max_batch)
        return fail(SDRK_ERR_INVALID, "n_frames %zu exceeds the plan's max_batch %zu", n_frames, p->max_batch);
    HIP_TRY(hipSetDevice(p->device));
    const size_t nfft = (size_t)p->nfft;
    const size_t in_bytes = ((n_frames - 1) * frame_stride + nfft) * sizeof(float2);
    // spectra are produced in chunks into d_out; the column sums accumulate per chunk on the host side
    // of the call only through `scale` (each chunk adds scale * sum), so one small device row suffices.
    const size_t chunk = ((size_t)256 << 20) / (nfft * sizeof(float2)) ? ((size_t)256 << 20) / (nfft * sizeof(float2)) : 1;
    const size_t spec_frames = n_frames < chunk ? n_frames : chunk;
    st = grow(p->device, &p->d_in, &p->in_cap, in_bytes);
    if (st != SDRK_OK) return st;
    st = grow(p->device, &p->d_out, &p->out_cap, spec_frames * nfft * sizeof(float2) + nfft * sizeof(float));
    if (st != SDRK_OK) return st;
    float* d_row = reinterpret_cast<float*>(static_cast<char*>(p->d_out) + spec_frames * nfft * sizeof(float2));
    HIP_TRY(hipMemcpyAsync(p->d_in, iq, in_bytes, hipMemcpyHostToDevice, p->stream));
    std::vector<float> row(nfft), total(nfft, 0.0f);
    for (size_t f0 = 0; f0 < n_frames; f0 += spec_frames) {
        const size_t nf = n_frames - f0 < spec_frames ? n_frames - f0 : spec_frames;
        st = plan_launch(p, static_cast<const float2*>(p->d_in) + f0 * frame_stride, nf, frame_stride, p->d_out,
                         sdrk::EPI_COMPLEX, p->stream);
        if (st != SDRK_OK) return st;
        hipError_t e = sdrk::launch_power_mean(p->d_out, nf, p->nfft, scale, d_row, p->stream);
        if (e != hipSuccess) return fail(SDRK_ERR_HIP, "power_mean launch failed: %s", hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(row.data(), d_row, nfft * sizeof(float), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        st = fused_check(p);
        if (st != SDRK_OK) return st;
        for (size_t k = 0; k < nfft; ++k) total[k] += row[k];   // <= a handful of chunks
    }
    memcpy(out_psd, total.data(), nfft * sizeof(float));
    return SDRK_OK;
}

}  // extern "C"

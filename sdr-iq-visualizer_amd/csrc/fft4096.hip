// fft4096.hip — the flagship kernel: window * x -> 4096-point complex FFT ->
// fftshift -> 20*log10(|X| + eps), one HBM read (8 B/sample) and one HBM write
// (4 B/sample) per frame, everything in between in registers and LDS.
//
// Replaces, per frame, the reference's
//   app/sdr/streamer.py:119  fft_data = np.fft.fftshift(np.fft.fft(samples))
//   app/sdr/streamer.py:121  power_db = 20 * np.log10(np.abs(fft_data) + 1e-12)
//
// Decomposition (N = 4096 = 16*16*16, one 256-thread workgroup per frame, each
// thread owns 16 points; three in-register radix-16 passes, two LDS exchanges):
//   n = n0 + 16 n1 + 256 n2,   k = k0 + 16 k1 + 256 k2
//   pass 1  thread r=(n0,n1): DFT-16 over n2, times W4096^(r k0)   -> (n0,n1,k0)
//   pass 2  thread q=(n0,k0): DFT-16 over n1, times W256^(n0 k1)   -> (n0,k0,k1)
//   pass 3  thread p=(k0,k1): DFT-16 over n0                       -> X[p + 256 k2]
// Loads are x[r + 256 j]: every wave instruction reads 64 consecutive complex64
// (512 B); stores are out[p + 256 j]: 64 consecutive float32 (256 B).
// The fftshift of streamer.py:119 is a half rotation for even N: k2 ^= 8.
//
// LDS exchange layouts (complex64 units), every ds_read_b64 / ds_write_b64
// bank-conflict free on gfx950 (64 dword banks for b64 reads, 32 for writes) and
// every address of the form (one of two per-thread bases) + immediate:
//   exchange 1:  a1(n0,n1,k0) = n0 + 16 (n1 ^ (k0 & 1)) + 256 k0       (XOR swizzle)
//   exchange 2:  a2(n0,k0,k1) = k0 + 16 k1 + 257 n0                    (+1 padding)
//
// Global traffic goes through buffer instructions (wave-uniform descriptor on
// the frame, one VGPR byte offset, SGPR row offsets): no 64-bit address VGPRs.
// The kernel is persistent (grid-stride over frames) and software-pipelined:
// the next frame's 16 loads per thread are in flight while the current frame is
// transformed, so each resident workgroup keeps 32 KiB of HBM reads outstanding.
// fft4096_ticket_kernel is the same frame body under another order of the frames: a workgroup takes its next frame
// from a counter in device memory (f4k_ticket.h) instead of stepping by the grid; fft4096_rot_kernel takes one frame per
// ticket from several such counters in rotation (f4k_rot.h), three tickets ahead, fft4096_rot2_kernel two, and
// fft4096_flow2_kernel, what a full grid runs, two with the row stores left in flight across the turn.
#include "f4k_deal.h"
#include "fft4096_core.h"

namespace sdrk {

#ifdef SDRK_F4K_TIMELINE
// Experiment build only (experiments/f4k_order): one 16-byte record per frame — the shared real-time counter (100 MHz) when
// the frame's loads were issued, the frame, the workgroup — into the buffer sdrk_f4k_timeline() names, if it names one.
__device__ uint4* f4k_timeline_buf = nullptr;
#define F4K_TIMELINE_LOAD() uint4* const f4k_tl = f4k_timeline_buf
#define F4K_TIMELINE_MARK(fr)                                                                                   \
    do {                                                                                                        \
        if (f4k_tl && tid == 0 && (fr) < n_frames) {                                                            \
            const unsigned long long f4k_t = wall_clock64();                                                    \
            f4k_tl[fr] = make_uint4((unsigned)f4k_t, (unsigned)(f4k_t >> 32), (unsigned)(fr), blockIdx.x);      \
        }                                                                                                       \
    } while (0)
#else
#define F4K_TIMELINE_LOAD() (void)0
#define F4K_TIMELINE_MARK(fr) (void)0
#endif

// fft4096_ci16_kernel (fft4096_ci16.hip) and the ci8 kernel are this function with another input policy: a change here is made
// there too — except the ticket order of fft4096_ticket_kernel below, which only the complex64 input has so far.
//
// (Tried and dropped, A/B on the same buffers: two frames prefetched (2 % slower, again in round 5 at 140 VGPRs), a sqrt-free
// log epilogue (1.5 % slower), and sending the row through LDS once more so that it leaves as four 16-byte stores
// per thread instead of sixteen 4-byte ones (1.0-1.5 % slower: two more barriers per frame cost more than the
// narrower stores do); issuing the prefetch through inline asm with an exact `s_waitcnt vmcnt(16)` in front of its first
// use — hipcc waits vmcnt(0) there, i.e. also for the previous frame's stores — changed nothing either ON THIS KERNEL, the
// grid-stride order at 9.2 ms, which then ran faster than its no-arithmetic probe (0.95-0.98) and whose pace the disorder
// among its workgroups set.  In the rot order at 7.7-7.9 ms the same wait costs 0.11-0.22 ms: fft4096_flow2_kernel below,
// profiles/f4k_flow/SUMMARY.md.  This loop, and the other N = 4096 kernels', still drain their stores.  The window coefficients
// in 16 VGPRs per thread instead of the 16 KiB LDS copy were a build switch, F4K_WINREG, that nothing set; it is gone.)
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift) {
    typedef F4kInC64 In;
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;

    const size_t first = blockIdx.x;
    const size_t step = gridDim.x;
    F4K_TIMELINE_LOAD();

    // Software pipeline: each workgroup keeps the loads of its next frame in flight while it transforms the
    // current one.  (Two frames ahead — 64 KiB per workgroup in flight — measured 2.5 % slower against the
    // same-buffers copy: 1.055x instead of 1.030x its time.)
    auto issue = [&](In::word (&x)[16], size_t fr) {
        F4K_TIMELINE_MARK(fr);
        if (fr >= n_frames) fr = first;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    auto process = [&](In::word (&x)[16], size_t f) {
        In::to_owners(x, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(x[j]);
        issue(x, f + step);
        f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + f * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
    };
    In::word nxt[16];
    issue(nxt, first);
    for (size_t f = first; f < n_frames; f += step) process(nxt, f);
}

// The same frames in ticket order (f4k_ticket.h): workgroup b draws from head b % heads, and a ticket is `frames` consecutive
// frames.  One lane draws: f4k_ticket_depth tickets with the first atomic, before the prologue's barrier, and one more at the
// top of every iteration whose prefetch reaches the last frame of a ticket, ahead of that iteration's prefetch loads, so that
// the wait for those loads at the top of the next iteration has covered it.  At the next such iteration the lane puts the value
// into one of two LDS slots (alternating: a wave that is through the frame's last barrier may write the next slot while another
// still reads this one); every wave reads it behind the transform's four barriers and makes it wave-uniform.  A ticket is thus
// drawn some iterations before its first frame is prefetched, nothing waits or polls for it, and the frame body has no barrier
// more than the grid-stride form.  A workgroup leaves at its first frame at or past the end; the draws that remain in flight
// are part of what the host expects of the heads.
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_ticket_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift, unsigned* __restrict__ heads, const sdrk_host::F4kTicketBases bases,
    const sdrk_host::F4kTicketForm form) {
    typedef F4kInC64 In;
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    __shared__ unsigned ticket_slot[2];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    const unsigned hx = blockIdx.x & (form.heads - 1);
    const unsigned depth = sdrk_host::f4k_ticket_depth(form);
    // (+ the lane: 0 in the one lane that draws.  An address the compiler takes for wave-uniform makes it rewrite the atomic as
    // "one elected lane adds, then everybody reads the first lane", which waits for the returned value where it is issued.)
    unsigned* const head = heads + hx * sdrk_host::F4K_TICKET_HEAD_WORDS + __lane_id();
    const unsigned base = bases.base[hx];
    unsigned drawn = 0;   // lane 0: the head's value at the youngest ticket this workgroup holds
    if (tid == 0) drawn = __hip_atomic_fetch_add(head, depth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    if (tid == 0) {
        ticket_slot[0] = drawn;
        drawn += depth - 1;
    }
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;
    F4K_TIMELINE_LOAD();

    auto first_of = [&](unsigned head_value) { return sdrk_host::f4k_ticket_first_frame(form, head_value - base, hx); };
    const unsigned h0 = __builtin_amdgcn_readfirstlane(ticket_slot[0]);
    const size_t in_ticket = form.frames - 1;
    // cur: the frame to transform, its loads in flight; nx: the frame to prefetch; tn: the first frame of the ticket behind nx's
    size_t cur = first_of(h0), nx = in_ticket ? cur + 1 : first_of(h0 + 1), tn = first_of(h0 + depth - 2);
    unsigned par = 1;

    auto issue = [&](In::word (&x)[16], size_t fr) {
        F4K_TIMELINE_MARK(fr);
        if (fr >= n_frames) fr = 0;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    In::word nxt[16];
    issue(nxt, cur);
    while (cur < n_frames) {
        const bool last_of_ticket = ((nx + 1) & in_ticket) == 0;   // the prefetch reaches the end of a ticket: tn is next, and a draw
        if (last_of_ticket && tid == 0) {
            ticket_slot[par] = drawn;
            drawn = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        In::to_owners(nxt, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
        issue(nxt, nx);
        f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
        size_t after = nx + 1;
        if (last_of_ticket) {
            after = tn;
            tn = first_of(__builtin_amdgcn_readfirstlane(ticket_slot[par]));
            par ^= 1;
        }
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + cur * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
        cur = nx;
        nx = after;
    }
}

// The same frames in the "rot H" order (f4k_rot.h, dealt by F4kRotDeal of f4k_deal.h): one frame per ticket, `n_heads` heads
// that start at zero, and the workgroup's draws go round the heads.  Lane 0 draws three tickets in the prologue and one more
// at the top of every iteration, ahead of that iteration's prefetch loads; at the top of the next iteration the ticket is in
// its register, goes into an LDS slot as a frame number and is read by every wave behind that iteration's barriers: three
// tickets ahead of the frame transformed, and nothing waits or polls.  A frame at or past the end is skipped (one barrier in
// place of the transform's, for the slot), F4K_ROT_NONE ends the loop, and the last workgroup out zeroes the heads.
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_rot_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift, unsigned* __restrict__ heads, const unsigned n_heads) {
    typedef F4kInC64 In;
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    __shared__ unsigned deal_slot[F4K_DEAL_SLOTS];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kRotDeal deal(heads, n_heads, n_frames, deal_slot, tid);
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    deal.publish(tid);
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;
    F4K_TIMELINE_LOAD();

    auto issue = [&](In::word (&x)[16], size_t fr) {
        F4K_TIMELINE_MARK(fr);
        if (fr >= n_frames) fr = 0;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    In::word nxt[16];
    deal.begin();
    issue(nxt, deal.frame());   // the frame to transform has its loads in flight; deal.next() is the frame to prefetch
    while (deal.more()) {
        deal.top(tid);
        const size_t cur = deal.frame();
        if (cur < n_frames) {
            In::to_owners(nxt, lds, tid);
            cf v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
            issue(nxt, deal.next());
            f4k_windowed_transform<HAS_WINDOW>(v, lds, tw256, tw1, lds_win, A, tid);
            deal.step();
            f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + cur * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                    voff_out, xor_k2, eps);
        } else {
            issue(nxt, deal.next());
            __syncthreads();
            deal.step();
        }
    }
    deal.leave(tid);
}

// The rot order at look-ahead two (f4k_rot.h, F4kRotDeal2 of f4k_deal.h), the product's form until fft4096_flow2_kernel below and
// now its selectable control (SDRK_F4K_ROT_AHEAD=2top): the ticket that is in lane 0's
// register at the top of an iteration names the prefetch of that same iteration, with the barriers the frame body has anyway.
// The transform's first barrier — it only orders the previous frame's pass-3 LDS reads before this frame's exchange-1 writes —
// stands at the top of the iteration, behind lane 0's slot write; every wave reads the slot there, and the prefetch goes out
// where it does in fft4096_rot_kernel.  An iteration has the four barriers it had, a skipped frame has one.  The next draw
// goes out behind the row stores; hipcc waits vmcnt(0) at the top of the loop (for the prefetched loads), which covers it.
// The rows are fft4096_rot_kernel's bits: only the order of the frames differs.
// (Built and dropped, profiles/f4k_ahead/SUMMARY.md: the barrier left where it was and the slot read, and the prefetch issued,
// behind it, one radix-16 pass later — 92 VGPRs, 0.07 ms slower than look-ahead three; and the draw at the top of the
// iteration, ahead of the prefetch loads — 0.16 ms slower than behind the stores.)
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_rot2_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift, unsigned* __restrict__ heads, const unsigned n_heads) {
    typedef F4kInC64 In;
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    __shared__ unsigned deal_slot[F4K_DEAL_SLOTS];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kRotDeal2 deal(heads, n_heads, n_frames, deal_slot, tid);
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    deal.publish(tid);
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;
    F4K_TIMELINE_LOAD();

    auto issue = [&](In::word (&x)[16], size_t fr) {
        F4K_TIMELINE_MARK(fr);
        if (fr >= n_frames) fr = 0;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    In::word nxt[16];
    deal.begin();
    issue(nxt, deal.frame());   // the frame to transform has its loads in flight
    while (deal.more()) {
        deal.top(tid);
        __syncthreads();        // the slot; and the previous frame's pass-3 reads are done
        deal.read();            // deal.next() is the frame to prefetch
        const size_t cur = deal.frame();
        if (cur < n_frames) {
            In::to_owners(nxt, lds, tid);
            cf v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
            issue(nxt, deal.next());
            f4k_windowed_transform<HAS_WINDOW, false>(v, lds, tw256, tw1, lds_win, A, tid);
            f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + cur * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                    voff_out, xor_k2, eps);
        } else {
            issue(nxt, deal.next());
        }
        deal.tail(tid);
        deal.step();
    }
    deal.leave(tid);
}

// fft4096_rot2_kernel's order, dealer and frame body with the row stores left in flight across the turn ("2flow",
// F4K_AHEAD_2FLOW of f4k_rot.h, what a full grid runs; profiles/f4k_flow/SUMMARY.md: 0.11-0.22 ms faster on every pair).
// There every wave waits vmcnt(0) on its way back to the loop header — for the acknowledgement of the sixteen row stores it has just issued, and in wave 0 for the draw behind them —
// before it may touch words that were loaded a whole turn earlier: the header is also reached from the prologue and from a
// skipped frame, where no stores follow the loads, and hipcc takes the count of the worst path.  Here
//   - the draw goes out behind the transform and AHEAD of the row stores, so that sixteen stores stand between the atomic
//     and the loop top (the dealer's rule holds: a draw goes out only after the one before was taken in top());
//   - the steady loop is entered and re-entered only behind a transformed frame, i.e. with "16 loads, the draw, 16 stores"
//     outstanding: the first frame runs ahead of the loop, and a workgroup whose frame is at or past the end leaves for a
//     drain loop of fft4096_rot2_kernel's shape (skipped frames, and the frame or two that may still follow one);
// and hipcc counts by itself: no wait in the steady loop names fewer than 16 outstanding (tests/test_f4k_flow_code_objects.py).
// The barriers are those of fft4096_rot2_kernel, four per transformed frame and one per skipped one, and the rows its bits.
// What is left at the loop's latch is `s_waitcnt vmcnt(16)` — the loads and the draw, not the stores — in front of the sixteen
// register copies from the prefetch registers.  (Built and dropped: the steady loop unrolled over two turns with two sets of
// prefetch registers, which removes those copies, takes 152-154 VGPRs where the budget of the N = 4096 kernels is 128.)
template <bool HAS_WINDOW, int EPILOGUE>
__global__ __launch_bounds__(F4K_THREADS, F4K_WAVES) void fft4096_flow2_kernel(
    const float2* __restrict__ iq, size_t frame_stride, void* __restrict__ out_raw,
    size_t n_frames, const float* __restrict__ window, const float2* __restrict__ tw4096,
    float eps, int shift, unsigned* __restrict__ heads, const unsigned n_heads) {
    typedef F4kInC64 In;
    __shared__ float2 lds[f4k_lds_elems(HAS_WINDOW)];
    __shared__ unsigned deal_slot[F4K_DEAL_SLOTS];
    float2* __restrict__ tw256 = lds + F4K_XCH_ELEMS;  // [k][n] = W256^(n k)
    float2* __restrict__ tw1 = tw256 + 256;            // W4096^tid
    float* __restrict__ lds_win = reinterpret_cast<float*>(tw1 + 256);

    const int tid = threadIdx.x;
    F4kRotDeal2 deal(heads, n_heads, n_frames, deal_slot, tid);
    F4kAddr A = f4k_addr(tid);
    f4k_init_tables(tw256, tw1, tw4096, tid);
    if (HAS_WINDOW) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds_win[tid + 256 * j] = window[tid + 256 * j];
    }
    deal.publish(tid);
    __syncthreads();

    const int xor_k2 = shift ? 8 : 0;
    constexpr int OUT_ELEM = (EPILOGUE == EPI_LOGPSD ? 4 : 8);
    const int voff_out = tid * OUT_ELEM;
    F4K_TIMELINE_LOAD();

    auto issue = [&](In::word (&x)[16], size_t fr) {
        F4K_TIMELINE_MARK(fr);
        if (fr >= n_frames) fr = 0;  // harmless re-read past the end
        In::issue(x, iq + fr * frame_stride, tid);
    };
    In::word nxt[16];
    // one turn on a frame below the end: slot, prefetch, transform, draw, row stores
    auto turn = [&]() {
        deal.top(tid);
        __syncthreads();        // the slot; and the previous frame's pass-3 reads are done
        deal.read();            // deal.next() is the frame to prefetch
        const size_t cur = deal.frame();
        In::to_owners(nxt, lds, tid);
        cf v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = In::widen(nxt[j]);
        issue(nxt, deal.next());
        f4k_windowed_transform<HAS_WINDOW, false>(v, lds, tw256, tw1, lds_win, A, tid);
        deal.tail(tid);
        f4k_store_row<EPILOGUE>(v, frame_rsrc(static_cast<char*>(out_raw) + cur * (size_t)(F4K_N * OUT_ELEM), F4K_N * OUT_ELEM),
                                voff_out, xor_k2, eps);
        deal.step();
    };
    deal.begin();
    issue(nxt, deal.frame());   // the frame to transform has its loads in flight
    if (deal.frame() < n_frames) {
        turn();                                    // the first frame: behind it the state is the steady loop's
        while (deal.frame() < n_frames) turn();    // the steady loop
    }
    while (deal.more()) {                          // the drain: at most a few turns
        if (deal.frame() < n_frames) {
            turn();
        } else {
            deal.top(tid);
            __syncthreads();
            deal.read();
            issue(nxt, deal.next());
            deal.tail(tid);
            deal.step();
        }
    }
    deal.leave(tid);
}

unsigned f4k_max_blocks(int num_cus) { return f4k_grid(num_cus, F4K_WAVES, (size_t)-1); }

hipError_t launch_fft4096(const LaunchArgs& a) {
    if (a.n_frames == 0) return hipSuccess;
    dim3 g(f4k_grid(a.num_cus, F4K_WAVES, a.n_frames)), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, E)                                                                            \
    hipLaunchKernelGGL((fft4096_kernel<W, E>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,           \
                       a.n_frames, a.d_window, tw, a.eps, a.shift)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_fft4096_ticket(const LaunchArgs& a, unsigned* d_heads, const sdrk_host::F4kTicketBases& bases,
                                 sdrk_host::F4kTicketForm form, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_ticket_form_ok(form)) return hipErrorInvalidValue;
    dim3 g(grid), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, E)                                                                            \
    hipLaunchKernelGGL((fft4096_ticket_kernel<W, E>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,    \
                       a.n_frames, a.d_window, tw, a.eps, a.shift, d_heads, bases, form)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_fft4096_rot(const LaunchArgs& a, unsigned* d_heads, unsigned n_heads, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_rot_heads_ok(n_heads) ||
        a.n_frames > sdrk_host::F4K_TICKET_MAX_FRAMES)
        return hipErrorInvalidValue;
    dim3 g(grid), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, E)                                                                            \
    hipLaunchKernelGGL((fft4096_rot_kernel<W, E>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,       \
                       a.n_frames, a.d_window, tw, a.eps, a.shift, d_heads, n_heads)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_fft4096_rot2(const LaunchArgs& a, unsigned* d_heads, unsigned n_heads, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_rot_heads_ok(n_heads) ||
        a.n_frames > sdrk_host::F4K_TICKET_MAX_FRAMES)
        return hipErrorInvalidValue;
    dim3 g(grid), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, E)                                                                            \
    hipLaunchKernelGGL((fft4096_rot2_kernel<W, E>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,      \
                       a.n_frames, a.d_window, tw, a.eps, a.shift, d_heads, n_heads)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

hipError_t launch_fft4096_flow2(const LaunchArgs& a, unsigned* d_heads, unsigned n_heads, unsigned grid) {
    if (a.n_frames == 0) return hipSuccess;
    if (!d_heads || grid == 0 || grid % sdrk_host::F4K_TICKET_MAX_HEADS || !sdrk_host::f4k_rot_heads_ok(n_heads) ||
        a.n_frames > sdrk_host::F4K_TICKET_MAX_FRAMES)
        return hipErrorInvalidValue;
    dim3 g(grid), b(F4K_THREADS);
    const float2* iq = static_cast<const float2*>(a.d_iq);
    const float2* tw = static_cast<const float2*>(a.d_twiddle);
#define SDRK_LAUNCH(W, E)                                                                            \
    hipLaunchKernelGGL((fft4096_flow2_kernel<W, E>), g, b, 0, a.stream, iq, a.frame_stride, a.d_out,     \
                       a.n_frames, a.d_window, tw, a.eps, a.shift, d_heads, n_heads)
    if (a.epilogue == EPI_LOGPSD) {
        if (a.d_window) SDRK_LAUNCH(true, EPI_LOGPSD); else SDRK_LAUNCH(false, EPI_LOGPSD);
    } else {
        if (a.d_window) SDRK_LAUNCH(true, EPI_COMPLEX); else SDRK_LAUNCH(false, EPI_COMPLEX);
    }
#undef SDRK_LAUNCH
    return hipGetLastError();
}

}  // namespace sdrk

#ifdef SDRK_F4K_TIMELINE
// Experiment build only: the device buffer (one uint4 per frame of the launches to come) the time line goes to; NULL ends it.
extern "C" int sdrk_f4k_timeline(void* d_records) {
    uint4* p = static_cast<uint4*>(d_records);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(sdrk::f4k_timeline_buf), &p, sizeof p);
}
#endif

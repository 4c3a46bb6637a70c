// f4k_deal.h — device side of the orders in which a persistent grid of workgroups takes "frames" (units of work numbered
// 0 .. n - 1) from counters in device memory: the ticket forms of f4k_ticket.h and the "rot H" form of f4k_rot.h, behind one
// shape so that a kernel's loop reads the same in either:
//
//     Deal deal(...);            // the first draws go out
//     ... the kernel's own prologue ...
//     deal.publish(tid);
//     __syncthreads();
//     deal.begin();
//     while (deal.more()) {
//         deal.top(tid);                                  // the drawing lane: last draw into the slot, next draw out
//         if (deal.frame() < n) ... work on deal.frame(), deal.next() is the one after ...
//         ... at least one __syncthreads() ...
//         deal.step();                                    // every wave reads the slot
//     }
//     deal.leave(tid);
//
// F4kRotDeal2 (look-ahead two) has a shape of its own, see there; Deal::TWO_AHEAD tells a templated loop which one it has.
// The dealers keep their slots in LDS words the kernel hands them (F4K_DEAL_SLOTS).  fft4096_rot_kernel (fft4096.hip) and the
// no-arithmetic probes (aux_kernels.hip) are built on them; fft4096_ticket_kernel carries F4kTicketDeal's steps written out.
#pragma once
#include <hip/hip_runtime.h>

#include "f4k_rot.h"
#include "f4k_ticket.h"

namespace sdrk {

constexpr int F4K_DEAL_SLOTS = 4;

__device__ __forceinline__ unsigned f4k_deal_draw(unsigned* word, unsigned n) {
    return __hip_atomic_fetch_add(word, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// f4k_ticket.h: `form.heads` heads found at `bases`, `form.frames` consecutive frames per ticket (see fft4096_ticket_kernel)
struct F4kTicketDeal {
    static constexpr bool TWO_AHEAD = false;
    sdrk_host::F4kTicketForm form;
    size_t n_frames, cur, nx, tn, in_ticket;
    unsigned* head;      // (+ the lane: 0 in the one lane that draws, see fft4096_ticket_kernel)
    unsigned* slot;
    unsigned hx, base, depth, drawn, par;
    bool last_of_ticket;

    __device__ __forceinline__ F4kTicketDeal(unsigned* heads, const sdrk_host::F4kTicketBases& bases, sdrk_host::F4kTicketForm f,
                                             size_t n, unsigned* lds_slots, int tid)
        : form(f), n_frames(n), in_ticket(f.frames - 1), slot(lds_slots), hx(blockIdx.x & (f.heads - 1)),
          depth(sdrk_host::f4k_ticket_depth(f)), drawn(0), par(1), last_of_ticket(false) {
        head = heads + hx * sdrk_host::F4K_TICKET_HEAD_WORDS + __lane_id();
        base = bases.base[hx];
        if (tid == 0) drawn = f4k_deal_draw(head, depth);
    }
    static __device__ __forceinline__ F4kTicketDeal make(const sdrk_host::F4kDealArgs& a, size_t n, unsigned* lds_slots, int tid) {
        return F4kTicketDeal(a.heads, a.bases, a.form, n, lds_slots, tid);
    }
    __device__ __forceinline__ size_t first_of(unsigned head_value) const {
        return sdrk_host::f4k_ticket_first_frame(form, head_value - base, hx);
    }
    __device__ __forceinline__ void publish(int tid) {
        if (tid == 0) {
            slot[0] = drawn;
            drawn += depth - 1;
        }
    }
    __device__ __forceinline__ void begin() {
        const unsigned h0 = __builtin_amdgcn_readfirstlane(slot[0]);
        cur = first_of(h0);
        nx = in_ticket ? cur + 1 : first_of(h0 + 1);
        tn = first_of(h0 + depth - 2);
    }
    __device__ __forceinline__ bool more() const { return cur < n_frames; }
    __device__ __forceinline__ void top(int tid) {
        last_of_ticket = ((nx + 1) & in_ticket) == 0;
        if (last_of_ticket && tid == 0) {
            slot[par] = drawn;
            drawn = f4k_deal_draw(head, 1u);
        }
    }
    __device__ __forceinline__ size_t frame() const { return cur; }
    __device__ __forceinline__ size_t next() const { return nx; }
    __device__ __forceinline__ void step() {
        size_t after = nx + 1;
        if (last_of_ticket) {
            after = tn;
            tn = first_of(__builtin_amdgcn_readfirstlane(slot[par]));
            par ^= 1;
        }
        cur = nx;
        nx = after;
    }
    __device__ __forceinline__ void leave(int) {}
};

// f4k_rot.h: `n_heads` heads found and left at zero, one frame per ticket, the draws go round the heads.  slot[0], [1]: the
// prologue's first two frames; [2], [3]: the loop's, alternating (a wave that is through an iteration's last barrier may
// write the next slot while another still reads this one).
struct F4kRotDeal {
    static constexpr bool TWO_AHEAD = false;
    sdrk_host::F4kRotDrawer dr;
    size_t n_frames;
    unsigned* lane_heads;   // (+ the lane, as above)
    unsigned* slot;
    unsigned drawn, d0, d1, h0, h1;   // lane 0: the ticket of the last draw; the prologue's first two and their heads
    unsigned cur, nx, par;

    __device__ __forceinline__ F4kRotDeal(unsigned* heads, unsigned n_heads, size_t n, unsigned* lds_slots, int tid)
        : dr(sdrk_host::f4k_rot_drawer(n_heads, blockIdx.x)), n_frames(n), lane_heads(heads + __lane_id()), slot(lds_slots),
          drawn(0), d0(0), d1(0), h0(0), h1(0), par(2) {
        if (tid == 0) {
            h0 = dr.head;
            d0 = f4k_deal_draw(word(h0), 1u);
            h1 = (h0 + 1) & (n_heads - 1);
            d1 = f4k_deal_draw(word(h1), 1u);
            dr.head = (h1 + 1) & (n_heads - 1);
            drawn = f4k_deal_draw(word(dr.head), 1u);
            dr.pending = true;
        }
    }
    static __device__ __forceinline__ F4kRotDeal make(const sdrk_host::F4kDealArgs& a, size_t n, unsigned* lds_slots, int tid) {
        return F4kRotDeal(a.heads, a.rot_heads, n, lds_slots, tid);
    }
    __device__ __forceinline__ unsigned* word(unsigned head) const { return lane_heads + head * sdrk_host::F4K_TICKET_HEAD_WORDS; }
    __device__ __forceinline__ void publish(int tid) {
        if (tid == 0) {
            const unsigned h2 = dr.head;
            dr.head = h0;
            slot[0] = sdrk_host::f4k_rot_take(dr, d0, n_frames);
            dr.head = h1;
            slot[1] = sdrk_host::f4k_rot_take(dr, d1, n_frames);
            dr.head = h2;
        }
    }
    __device__ __forceinline__ void begin() {
        cur = __builtin_amdgcn_readfirstlane(slot[0]);
        nx = __builtin_amdgcn_readfirstlane(slot[1]);
    }
    __device__ __forceinline__ bool more() const { return cur != sdrk_host::F4K_ROT_NONE; }
    __device__ __forceinline__ void top(int tid) {
        if (tid == 0) {
            slot[par] = dr.pending ? sdrk_host::f4k_rot_take(dr, drawn, n_frames) : sdrk_host::F4K_ROT_NONE;
            if (sdrk_host::f4k_rot_advance(dr)) drawn = f4k_deal_draw(word(dr.head), 1u);
        }
    }
    __device__ __forceinline__ size_t frame() const { return cur; }   // at or past the end (F4K_ROT_NONE too): skip
    __device__ __forceinline__ size_t next() const { return nx; }
    __device__ __forceinline__ void step() {
        const unsigned after = __builtin_amdgcn_readfirstlane(slot[par]);
        par ^= 1;
        cur = nx;
        nx = after;
    }
    // Every draw of this workgroup has come back (its ticket went through the slots ahead of F4K_ROT_NONE), so behind
    // grid - 1 other exits no draw is out anywhere: the last one out leaves the heads and the counter at zero.
    __device__ __forceinline__ void leave(int tid) {
        if (tid == 0) {
            unsigned* const exits = lane_heads + sdrk_host::F4K_ROT_EXIT_WORD;
            if (f4k_deal_draw(exits, 1u) == gridDim.x - 1) {
                for (unsigned x = 0; x < dr.heads; ++x) __hip_atomic_store(word(x), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(exits, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};

// f4k_rot.h at look-ahead two: the same heads, rotation and exit; two draws in the prologue, and the ticket that comes back at
// the top of an iteration names the prefetch of that same iteration:
//
//     deal.top(tid);  ... one __syncthreads() ...  deal.read();      // deal.next() is now the frame to prefetch
//     ... work on deal.frame(), prefetch deal.next() ...
//     deal.tail(tid);  deal.step();
//
// The next draw goes out in tail(), behind the iteration's stores (at the top, ahead of the prefetch loads, it measured 0.16 ms
// slower on 2^20 frames, profiles/f4k_ahead/SUMMARY.md); fft4096_flow2_kernel calls tail() behind the transform and ahead of
// the stores, so that the stores are the youngest operations at the loop top (profiles/f4k_flow/SUMMARY.md).  slot[0]: the prologue's frame; [2], [3]: the loop's, alternating (the
// one barrier between top() and read() also orders this iteration's read before the write of the iteration after the next).
struct F4kRotDeal2 {
    static constexpr bool TWO_AHEAD = true;
    sdrk_host::F4kRotDrawer dr;
    size_t n_frames;
    unsigned* lane_heads;   // (+ the lane, as above)
    unsigned* slot;
    unsigned drawn, d0, h0;   // lane 0: the ticket of the last draw; the prologue's first and its head
    unsigned cur, nx, par;

    __device__ __forceinline__ F4kRotDeal2(unsigned* heads, unsigned n_heads, size_t n, unsigned* lds_slots, int tid)
        : dr(sdrk_host::f4k_rot_drawer(n_heads, blockIdx.x)), n_frames(n), lane_heads(heads + __lane_id()), slot(lds_slots),
          drawn(0), d0(0), h0(0), cur(0), nx(sdrk_host::F4K_ROT_NONE), par(2) {
        if (tid == 0) {
            h0 = dr.head;
            d0 = f4k_deal_draw(word(h0), 1u);
            dr.head = (h0 + 1) & (n_heads - 1);
            drawn = f4k_deal_draw(word(dr.head), 1u);
            dr.pending = true;
        }
    }
    static __device__ __forceinline__ F4kRotDeal2 make(const sdrk_host::F4kDealArgs& a, size_t n, unsigned* lds_slots, int tid) {
        return F4kRotDeal2(a.heads, a.rot_heads, n, lds_slots, tid);
    }
    __device__ __forceinline__ unsigned* word(unsigned head) const { return lane_heads + head * sdrk_host::F4K_TICKET_HEAD_WORDS; }
    __device__ __forceinline__ void publish(int tid) {
        if (tid == 0) {
            const unsigned h1 = dr.head;
            dr.head = h0;
            slot[0] = sdrk_host::f4k_rot_take(dr, d0, n_frames);
            dr.head = h1;
        }
    }
    __device__ __forceinline__ void begin() { cur = __builtin_amdgcn_readfirstlane(slot[0]); }
    __device__ __forceinline__ bool more() const { return cur != sdrk_host::F4K_ROT_NONE; }
    __device__ __forceinline__ void top(int tid) {
        if (tid == 0) slot[par] = dr.pending ? sdrk_host::f4k_rot_take(dr, drawn, n_frames) : sdrk_host::F4K_ROT_NONE;
    }
    // behind a barrier that follows top()
    __device__ __forceinline__ void read() {
        nx = __builtin_amdgcn_readfirstlane(slot[par]);
        par ^= 1;
    }
    __device__ __forceinline__ size_t frame() const { return cur; }   // at or past the end (F4K_ROT_NONE too): skip
    __device__ __forceinline__ size_t next() const { return nx; }
    __device__ __forceinline__ void tail(int tid) {
        if (tid == 0 && sdrk_host::f4k_rot_advance(dr)) drawn = f4k_deal_draw(word(dr.head), 1u);
    }
    __device__ __forceinline__ void step() { cur = nx; }
    // (as F4kRotDeal::leave: F4K_ROT_NONE has followed this workgroup's last ticket through the slot)
    __device__ __forceinline__ void leave(int tid) {
        if (tid == 0) {
            unsigned* const exits = lane_heads + sdrk_host::F4K_ROT_EXIT_WORD;
            if (f4k_deal_draw(exits, 1u) == gridDim.x - 1) {
                for (unsigned x = 0; x < dr.heads; ++x) __hip_atomic_store(word(x), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(exits, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
};

}  // namespace sdrk

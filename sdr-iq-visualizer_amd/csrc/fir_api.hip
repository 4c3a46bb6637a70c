// fir_api.hip — host side of "FIR filtering and channel extraction" of include/sdrk.h (sdrk_plan_set_fir, sdrk_plan_fir_taps,
// sdrk_exec_*_fir*): tune, filter, decimate by overlap-save fast convolution in blocks of 4096 through ols4096.hip, the filter
// held by the plan as the polyphase prototype is (kernels_ols.h has the block geometry); and of the channel bank
// (sdrk_exec_*_chanbank*): C tuned channels from one pass over the input through ols_bank.hip (kernels_ols_bank.h); and of the
// digital down-converter (sdrk_ddc_outputs, sdrk_exec_*_ddc*, sdrk_exec_*_ddcbank*): the same two calls tuned by a 32-bit frequency
// word and decimated by any integer, through ddc4096.hip (kernels_ddc.h), with a chunk loop of its own on the same SlotPipe; and of
// the same from interleaved 8-bit I,Q (sdrk_exec_*_downconv_iq8, sdrk_exec_*_downconvbank_iq8) through downconv_iq8.hip: one more
// input format of that loop and of ddc_launch; and of the filter-and-sum beamformer (sdrk_plan_set_beam, sdrk_exec_*_beam*): C coherent
// channels in, one down-converted channel out, through beamsum.hip (kernels_beam.h) and the down-converter's chunk loop.
//
// A device call is one launch on the caller's stream.  The numpy boundary runs the same launches on the virtual stream
// prefix || iq in chunks of whole blocks through sdrk_host_pipeline.hip's SlotPipe, one loop (host_fir_chunks) for the single
// call and the bank: a chunk's input is assembled in a slot's pinned staging, its planes come back packed and are scattered
// to the caller's array when the slot retires.
// Host code only (g++ builds it against tests/fake_hip for the sanitizer legs).
#include "../../include/sdrk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels_beam.h"
#include "kernels_ddc.h"
#include "kernels_ols_bank.h"
#include "plan_internal.h"

using namespace sdrk_host;

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
// The staging is always filled and emptied by plain memcpy on the calling thread, whatever memory the caller's arrays are in.
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
    SlotPipe pipe;
    int st = pipe.open(p, "host pipeline");
    if (st != SDRK_OK) return st;
    for (size_t b0 = 0; b0 < n_blocks; b0 += per) {
        const size_t nb = n_blocks - b0 < per ? n_blocks - b0 : per;
        const size_t t0 = b0 * L;
        const size_t cn = (nb - 1) * L + N < n_virt - t0 ? (nb - 1) * L + N : n_virt - t0;
        const size_t o0 = b0 * opb, co = nb * opb < total_out - o0 ? nb * opb : total_out - o0;
        HostSlot* s = nullptr;
        st = pipe.acquire(chunk_in, chunk_out, s);
        if (st != SDRK_OK) return st;
        // samples V[v0 .. v0 + cn): the part below M - 1 from the prefix (NULL: zeros), the rest from iq
        const size_t v0 = j0 + t0;
        char* dst = static_cast<char*>(s->h_in);
        size_t done = 0;
        if (v0 < M - 1) {
            done = M - 1 - v0 < cn ? M - 1 - v0 : cn;
            if (prefix) memcpy(dst, static_cast<const char*>(prefix) + v0 * in_elem, done * in_elem);
            else memset(dst, 0, done * in_elem);
        }
        if (done < cn)
            memcpy(dst + done * in_elem, static_cast<const char*>(iq) + (v0 + done - (M - 1)) * in_elem, (cn - done) * in_elem);
        st = pipe.upload(*s, s->h_in, cn * in_elem);
        if (st == SDRK_OK)
            st = pipe.submit(*s, launch(s->d_in, cn, (unsigned)((sample0 + j0 + t0) & (N - 1)), s->d_out, nb, co),
                             {ChunkOut::Planes, static_cast<char*>(out) + o0 * sizeof(float2), co * sizeof(float2), planes,
                              out_stride * sizeof(float2)});
        if (st != SDRK_OK) return st;
    }
    st = pipe.drain();
    if (st != SDRK_OK) return st;
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

// ---- digital down-converter: a 32-bit frequency word, any integer decimation (kernels_ddc.h) ----
int check_ddc_call(const sdrk_plan* p, int decim) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (p->fir_taps < 1 || !p->d_fir_h) return fail(SDRK_ERR_INVALID, "no FIR filter set: call sdrk_plan_set_fir first");
    if (decim < 1 || decim > sdrk::DDC_MAX_DECIM) return fail(SDRK_ERR_INVALID, "decim=%d: must be in [1, %d]", decim, sdrk::DDC_MAX_DECIM);
    return SDRK_OK;
}

int check_ddc_chans(int n_chan, const uint32_t* freq_word) {
    if (n_chan < 1 || n_chan > sdrk::DDC_MAX_CHAN) return fail(SDRK_ERR_INVALID, "n_chan=%d: must be in [1, %d]", n_chan, sdrk::DDC_MAX_CHAN);
    if (!freq_word) return fail(SDRK_ERR_INVALID, "freq_word pointer is NULL");
    return SDRK_OK;
}

// bank: n_chan planes out_stride apart; !bank: one channel, freq_word points at its word
int check_ddc_device(const sdrk_plan* p, bool bank, const void* d_in, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                     uint64_t index0, const void* d_out, size_t out_stride) {
    int st = check_ddc_call(p, decim);
    if (st == SDRK_OK && bank) st = check_ddc_chans(n_chan, freq_word);
    if (st != SDRK_OK) return st;
    if (!d_in || !d_out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (n_in < (size_t)p->fir_taps) return fail(SDRK_ERR_INVALID, "n_in=%zu: a valid convolution needs at least the %d taps", n_in, p->fir_taps);
    const size_t n_out = sdrk::ddc_outputs(n_in, p->fir_taps, decim, index0);
    if (bank && out_stride < n_out) return fail(SDRK_ERR_INVALID, "out_stride=%zu: a plane holds the %zu outputs of a channel", out_stride, n_out);
    return SDRK_OK;
}

// What a down-converter call reads: complex64, int16 pairs, or byte pairs of an 8-bit format (in >= 0: the SDRK_IQ8_* value).
constexpr int DDC_IN_C64 = -2, DDC_IN_CI16 = -1;
size_t ddc_in_elem(int in) { return in == DDC_IN_C64 ? sizeof(float2) : in == DDC_IN_CI16 ? 4 : 2; }

// One launch: the outputs i < max_blocks L (0: all) of the valid convolution of n_in samples, for every channel.
int ddc_launch(sdrk_plan* p, int in, bool bank, const void* d_in, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
               uint64_t index0, void* d_out, size_t out_stride, size_t max_blocks, hipStream_t stream) {
    sdrk::DdcArgs a;
    a.d_in = d_in;
    a.n_in = n_in;
    a.taps = p->fir_taps;
    a.decim = decim;
    a.n_chan = n_chan;
    a.freq_word = freq_word;
    a.index0 = index0;
    a.d_h = p->d_fir_h;
    a.d_twiddle = p->d_twiddle;
    a.d_out = static_cast<float2*>(d_out);
    a.out_stride = out_stride;
    a.max_blocks = max_blocks;
    a.num_cus = p->num_cus;
    a.stream = stream;
    if (sdrk::ddc_launch_outputs(a) == 0) return SDRK_OK;   // nothing kept: a successful no-op
    hipError_t e;
    if (in == DDC_IN_C64) e = bank ? sdrk::launch_ddcbank(a) : sdrk::launch_ddc(a);
    else if (in == DDC_IN_CI16) e = bank ? sdrk::launch_ddcbank_i16(a) : sdrk::launch_ddc_i16(a);
    else e = bank ? sdrk::launch_downconvbank_iq8(a, in) : sdrk::launch_downconv_iq8(a, in);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "DDC kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

int exec_device_ddc(int in, bool bank, sdrk_plan* p, const void* d_in, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                    uint64_t index0, void* d_out, size_t out_stride, void* stream) {
    int st = check_ddc_device(p, bank, d_in, n_in, n_chan, freq_word, decim, index0, d_out, out_stride);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return ddc_launch(p, in, bank, d_in, n_in, n_chan, freq_word, decim, index0, d_out, out_stride, 0,
                      stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int exec_device_ddc_timed(int in, bool bank, sdrk_plan* p, const void* d_in, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                          uint64_t index0, void* d_out, size_t out_stride, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_ddc_device(p, bank, d_in, n_in, n_chan, freq_word, decim, index0, d_out, out_stride);
    if (st != SDRK_OK) return st;
    return timed_each(p, launches, each_ms, [&] {
        return ddc_launch(p, in, bank, d_in, n_in, n_chan, freq_word, decim, index0, d_out, out_stride, 0, p->stream);
    });
}

// The chunk loop of the down-converter's host entries and of the beamformer's (below): the virtual stream V = prefix || iq of n + M - 1
// units of in_elem bytes (a sample; for the beamformer an element, one sample of every channel), cut into chunks of whole blocks.
// launch(d_in, cn, index0, d_out, co, nb) runs the first nb blocks of a chunk of cn units whose valid-convolution output 0 has
// stream index index0, and writes co outputs a plane, packed; `pad` is the byte of a NULL prefix.
template <class Launch>
int host_ddc_chunks(size_t in_elem, int pad, int taps, sdrk_plan* p, const void* prefix, const void* iq, size_t n, size_t planes, int decim,
                    uint64_t sample0, void* out, size_t out_stride, size_t* n_out, Launch launch) {
    const size_t D = (size_t)decim, M = (size_t)taps, L = (size_t)sdrk::ols_block_len(taps), N = sdrk::OLS_N;
    const size_t n_virt = n + M - 1, total_out = sdrk::ddc_count(n, decim, sample0);
    if (total_out == 0) return SDRK_OK;
    const size_t n_blocks = sdrk::ols_blocks(n_virt, taps), per = fir_chunk_blocks(L, in_elem);
    const size_t chunk_in = ((per - 1) * L + N) * in_elem, chunk_out = planes * (per * L / D + 1) * sizeof(float2);
    HIP_TRY(hipSetDevice(p->device));
    SlotPipe pipe;
    int st = pipe.open(p, "host pipeline");
    if (st != SDRK_OK) return st;
    for (size_t b0 = 0; b0 < n_blocks; b0 += per) {
        const size_t nb = n_blocks - b0 < per ? n_blocks - b0 : per;
        const size_t t0 = b0 * L;
        const size_t cn = (nb - 1) * L + N < n_virt - t0 ? (nb - 1) * L + N : n_virt - t0;
        const size_t valid = nb * L < cn - M + 1 ? nb * L : cn - M + 1;
        const size_t o0 = sdrk::ddc_count(t0, decim, sample0), co = sdrk::ddc_count(valid, decim, sample0 + t0);
        HostSlot* s = nullptr;
        st = pipe.acquire(chunk_in, chunk_out, s);
        if (st != SDRK_OK) return st;
        // units V[t0 .. t0 + cn): the part below M - 1 from the prefix (NULL: zeros; 0x80 bytes for cu8), the rest from iq
        char* dst = static_cast<char*>(s->h_in);
        size_t done = 0;
        if (t0 < M - 1) {
            done = M - 1 - t0 < cn ? M - 1 - t0 : cn;
            if (prefix) memcpy(dst, static_cast<const char*>(prefix) + t0 * in_elem, done * in_elem);
            else memset(dst, pad, done * in_elem);
        }
        if (done < cn)
            memcpy(dst + done * in_elem, static_cast<const char*>(iq) + (t0 + done - (M - 1)) * in_elem, (cn - done) * in_elem);
        st = pipe.upload(*s, s->h_in, cn * in_elem);
        if (st == SDRK_OK)
            st = pipe.submit(*s, launch(s->d_in, cn, sample0 + t0, s->d_out, co, nb),
                             {ChunkOut::Planes, static_cast<char*>(out) + o0 * sizeof(float2), co * sizeof(float2), planes,
                              out_stride * sizeof(float2)});
        if (st != SDRK_OK) return st;
    }
    st = pipe.drain();
    if (st != SDRK_OK) return st;
    *n_out = total_out;
    return SDRK_OK;
}

// The numpy boundary: the device entry on the virtual stream V = prefix || iq with index0 = sample0 (output j of the valid
// convolution has stream index sample0 + j), in chunks of whole blocks through the plan's pinned staging slots.  Every block is
// the 4096 samples it is in one device call on V (a chunk carries its last block's overlap and its launch is cut at
// max_blocks L outputs) and the mixer's phase and the keeping follow the stream index, which the chunk's launch is handed as its
// index0, so the chunking does not show in the bits.  A block yields L / D outputs or one more, so the outputs of a chunk are
// counted, not multiplied out: chunk [b0, b0 + nb) starts at output ddc_count(b0 L) and holds ddc_count of its own.
int exec_host_ddc(int in, bool bank, sdrk_plan* p, const void* prefix, const void* iq, size_t n, int n_chan,
                  const uint32_t* freq_word, int decim, uint64_t sample0, void* out, size_t out_stride, size_t* n_out) {
    int st = check_ddc_call(p, decim);
    if (st == SDRK_OK && bank) st = check_ddc_chans(n_chan, freq_word);
    if (st != SDRK_OK) return st;
    if (!n_out) return fail(SDRK_ERR_INVALID, "n_out pointer is NULL");
    *n_out = 0;
    const size_t D = (size_t)decim, need = (n + D - 1) / D;
    if (bank && out_stride < need) return fail(SDRK_ERR_INVALID, "out_stride=%zu: a plane holds up to %zu outputs of a channel", out_stride, need);
    if (n == 0) return SDRK_OK;
    if (!iq || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    const size_t in_elem = ddc_in_elem(in);
    const int pad = in == SDRK_IQ8_UNSIGNED ? 0x80 : 0;   // the byte of a NULL prefix: 0x80 is mid-scale for unsigned bytes (+0.5)
    uint32_t words[sdrk::DDC_MAX_CHAN];   // read before the call returns: the launches below see this copy
    memcpy(words, freq_word, (size_t)n_chan * sizeof(uint32_t));
    return host_ddc_chunks(in_elem, pad, p->fir_taps, p, prefix, iq, n, (size_t)n_chan, decim, sample0, out, out_stride, n_out,
                           [&](const void* d_in, size_t cn, uint64_t index0, void* d_out, size_t co, size_t nb) {
                               return ddc_launch(p, in, bank, d_in, cn, n_chan, words, decim, index0, d_out, co, nb, p->stream);
                           });
}

// H = DFT_4096(taps zero-padded) in float64, rounded once: exact table angles, H[k] = sum_t h[t] W4096^((k t) mod 4096).
// `rows` filters of ntaps complex64 taps each, row-major -> rows x 4096 responses: sdrk_plan_set_fir's filter (one row) and every
// row of sdrk_plan_set_beam's go through this one loop.
std::vector<float2> fir_responses(const void* taps_c64, int rows, int ntaps) {
    constexpr int N = sdrk::OLS_N;
    std::vector<double> wr(N), wi(N);
    for (int m = 0; m < N; ++m) {
        const double ang = -2.0 * 3.14159265358979323846 * (double)m / (double)N;
        wr[m] = cos(ang);
        wi[m] = sin(ang);
    }
    std::vector<float2> H((size_t)rows * N);
    for (int r = 0; r < rows; ++r) {
        const float* h = static_cast<const float*>(taps_c64) + (size_t)r * 2 * (size_t)ntaps;
        for (int k = 0; k < N; ++k) {
            double re = 0.0, im = 0.0;
            for (int t = 0; t < ntaps; ++t) {
                const int m = (k * t) & (N - 1);
                const double hr = h[2 * t], hi = h[2 * t + 1];
                re += hr * wr[m] - hi * wi[m];
                im += hr * wi[m] + hi * wr[m];
            }
            H[(size_t)r * N + k] = make_float2((float)re, (float)im);
        }
    }
    return H;
}

// ---- filter-and-sum beamformer: C coherent channels in, one channel out (kernels_beam.h) ----
int check_beam_call(const sdrk_plan* p, int decim) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (p->beam_channels < 1 || !p->d_beam_h) return fail(SDRK_ERR_INVALID, "no beam filters set: call sdrk_plan_set_beam first");
    if (decim < 1 || decim > sdrk::DDC_MAX_DECIM) return fail(SDRK_ERR_INVALID, "decim=%d: must be in [1, %d]", decim, sdrk::DDC_MAX_DECIM);
    return SDRK_OK;
}

int check_beam_device(const sdrk_plan* p, const void* d_in, size_t n_in, int decim, const void* d_out) {
    int st = check_beam_call(p, decim);
    if (st != SDRK_OK) return st;
    if (!d_in || !d_out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    if (n_in < (size_t)p->beam_taps)
        return fail(SDRK_ERR_INVALID, "n_in=%zu: a valid convolution needs at least the %d taps", n_in, p->beam_taps);
    return SDRK_OK;
}

// One launch: the outputs i < max_blocks L (0: all) of the valid convolution of n_in elements.  in: sdrk::BEAM_IN_* or SDRK_IQ8_*.
int beam_launch(sdrk_plan* p, int in, const void* d_in, size_t n_in, uint32_t freq_word, int decim, uint64_t index0, void* d_out,
                size_t max_blocks, hipStream_t stream) {
    sdrk::BeamArgs a;
    a.d_in = d_in;
    a.n_in = n_in;
    a.channels = p->beam_channels;
    a.taps = p->beam_taps;
    a.decim = decim;
    a.freq_word = freq_word;
    a.index0 = index0;
    a.d_h = p->d_beam_h;
    a.d_twiddle = p->d_twiddle;
    a.d_out = static_cast<float2*>(d_out);
    a.max_blocks = max_blocks;
    a.num_cus = p->num_cus;
    a.stream = stream;
    if (sdrk::beam_launch_outputs(a) == 0) return SDRK_OK;   // nothing kept: a successful no-op
    const hipError_t e = sdrk::launch_beamsum(a, in);
    if (e != hipSuccess) return fail(SDRK_ERR_HIP, "beamformer kernel launch failed: %s", hipGetErrorString(e));
    return SDRK_OK;
}

int exec_device_beam(int in, sdrk_plan* p, const void* d_in, size_t n_in, uint32_t freq_word, int decim, uint64_t index0, void* d_out,
                     void* stream) {
    int st = check_beam_device(p, d_in, n_in, decim, d_out);
    if (st != SDRK_OK) return st;
    HIP_TRY(hipSetDevice(p->device));
    return beam_launch(p, in, d_in, n_in, freq_word, decim, index0, d_out, 0, stream ? static_cast<hipStream_t>(stream) : p->stream);
}

int exec_device_beam_timed(int in, sdrk_plan* p, const void* d_in, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                           void* d_out, int launches, float* each_ms) {
    if (!each_ms || launches < 1 || launches > 4096) return fail(SDRK_ERR_INVALID, "bad launches/each_ms");
    int st = check_beam_device(p, d_in, n_in, decim, d_out);
    if (st != SDRK_OK) return st;
    return timed_each(p, launches, each_ms, [&] { return beam_launch(p, in, d_in, n_in, freq_word, decim, index0, d_out, 0, p->stream); });
}

// The numpy boundary: the down-converter's chunk loop on elements of C samples.
int exec_host_beam(int in, sdrk_plan* p, const void* prefix, const void* iq, size_t n, uint32_t freq_word, int decim, uint64_t sample0,
                   void* out, size_t* n_out) {
    int st = check_beam_call(p, decim);
    if (st != SDRK_OK) return st;
    if (!n_out) return fail(SDRK_ERR_INVALID, "n_out pointer is NULL");
    *n_out = 0;
    if (n == 0) return SDRK_OK;
    if (!iq || !out) return fail(SDRK_ERR_INVALID, "input or output pointer is NULL");
    const size_t in_elem = (size_t)p->beam_channels * sdrk::beam_sample_bytes(in);
    const int pad = in == SDRK_IQ8_UNSIGNED ? 0x80 : 0;   // the byte of a NULL prefix, as for the 8-bit down-converter
    return host_ddc_chunks(in_elem, pad, p->beam_taps, p, prefix, iq, n, 1, decim, sample0, out, 0, n_out,
                           [&](const void* d_in, size_t cn, uint64_t index0, void* d_out, size_t, size_t nb) {
                               return beam_launch(p, in, d_in, cn, freq_word, decim, index0, d_out, nb, p->stream);
                           });
}

}  // namespace

extern "C" {

int sdrk_plan_set_fir(sdrk_plan* p, int ntaps, const void* taps_c64) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (ntaps < 1 || ntaps > sdrk::OLS_MAX_TAPS) return fail(SDRK_ERR_INVALID, "ntaps=%d: must be in [1, %d]", ntaps, sdrk::OLS_MAX_TAPS);
    if (!taps_c64) return fail(SDRK_ERR_INVALID, "taps pointer is NULL");
    constexpr int N = sdrk::OLS_N;
    const std::vector<float2> H = fir_responses(taps_c64, 1, ntaps);
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

size_t sdrk_ddc_outputs(size_t n_in, int taps, int decim, uint64_t index0) {
    if (taps < 1 || decim < 1 || decim > sdrk::DDC_MAX_DECIM) return 0;
    return sdrk::ddc_outputs(n_in, taps, decim, index0);
}

int sdrk_exec_device_ddc(sdrk_plan* p, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                         void* d_out_c64, void* stream) {
    return exec_device_ddc(DDC_IN_C64, false, p, d_in_c64, n_in, 1, &freq_word, decim, index0, d_out_c64, 0, stream);
}

int sdrk_exec_device_ddc_ci16(sdrk_plan* p, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                              void* d_out_c64, void* stream) {
    return exec_device_ddc(DDC_IN_CI16, false, p, d_in_ci16, n_in, 1, &freq_word, decim, index0, d_out_c64, 0, stream);
}

int sdrk_exec_device_ddc_timed_each(sdrk_plan* p, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                                    void* d_out_c64, int launches, float* each_ms) {
    return exec_device_ddc_timed(DDC_IN_C64, false, p, d_in_c64, n_in, 1, &freq_word, decim, index0, d_out_c64, 0, launches, each_ms);
}

int sdrk_exec_host_ddc(sdrk_plan* p, const void* prefix_c64, const void* iq_c64, size_t n, uint32_t freq_word, int decim,
                       uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_ddc(DDC_IN_C64, false, p, prefix_c64, iq_c64, n, 1, &freq_word, decim, sample0, out_c64, 0, n_out);
}

int sdrk_exec_host_ddc_ci16(sdrk_plan* p, const void* prefix_ci16, const void* iq_ci16, size_t n, uint32_t freq_word, int decim,
                            uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_ddc(DDC_IN_CI16, false, p, prefix_ci16, iq_ci16, n, 1, &freq_word, decim, sample0, out_c64, 0, n_out);
}

int sdrk_exec_device_ddcbank(sdrk_plan* p, const void* d_in_c64, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                             uint64_t index0, void* d_out_c64, size_t out_stride, void* stream) {
    return exec_device_ddc(DDC_IN_C64, true, p, d_in_c64, n_in, n_chan, freq_word, decim, index0, d_out_c64, out_stride, stream);
}

int sdrk_exec_device_ddcbank_ci16(sdrk_plan* p, const void* d_in_ci16, size_t n_in, int n_chan, const uint32_t* freq_word, int decim,
                                  uint64_t index0, void* d_out_c64, size_t out_stride, void* stream) {
    return exec_device_ddc(DDC_IN_CI16, true, p, d_in_ci16, n_in, n_chan, freq_word, decim, index0, d_out_c64, out_stride, stream);
}

int sdrk_exec_device_ddcbank_timed_each(sdrk_plan* p, const void* d_in_c64, size_t n_in, int n_chan, const uint32_t* freq_word,
                                        int decim, uint64_t index0, void* d_out_c64, size_t out_stride, int launches, float* each_ms) {
    return exec_device_ddc_timed(DDC_IN_C64, true, p, d_in_c64, n_in, n_chan, freq_word, decim, index0, d_out_c64, out_stride, launches, each_ms);
}

int sdrk_exec_host_ddcbank(sdrk_plan* p, const void* prefix_c64, const void* iq_c64, size_t n, int n_chan, const uint32_t* freq_word,
                           int decim, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out) {
    return exec_host_ddc(DDC_IN_C64, true, p, prefix_c64, iq_c64, n, n_chan, freq_word, decim, sample0, out_c64, out_stride, n_out);
}

int sdrk_exec_host_ddcbank_ci16(sdrk_plan* p, const void* prefix_ci16, const void* iq_ci16, size_t n, int n_chan,
                                const uint32_t* freq_word, int decim, uint64_t sample0, void* out_c64, size_t out_stride, size_t* n_out) {
    return exec_host_ddc(DDC_IN_CI16, true, p, prefix_ci16, iq_ci16, n, n_chan, freq_word, decim, sample0, out_c64, out_stride, n_out);
}

// ---- the down-converter from interleaved 8-bit I,Q (SigMF ci8 / cu8): the entries above with the format behind the samples ----
int sdrk_exec_device_downconv_iq8(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word, int decim,
                                  uint64_t index0, void* d_out_c64, void* stream) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_ddc(iq8_format, false, p, d_in_iq8, n_in, 1, &freq_word, decim, index0, d_out_c64, 0, stream);
}

int sdrk_exec_device_downconv_iq8_timed_each(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word,
                                             int decim, uint64_t index0, void* d_out_c64, int launches, float* each_ms) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_ddc_timed(iq8_format, false, p, d_in_iq8, n_in, 1, &freq_word, decim, index0, d_out_c64, 0, launches, each_ms);
}

int sdrk_exec_host_downconv_iq8(sdrk_plan* p, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n, uint32_t freq_word,
                                int decim, uint64_t sample0, void* out_c64, size_t* n_out) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_ddc(iq8_format, false, p, prefix_iq8, iq_iq8, n, 1, &freq_word, decim, sample0, out_c64, 0, n_out);
}

int sdrk_exec_device_downconvbank_iq8(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, int n_chan,
                                      const uint32_t* freq_word, int decim, uint64_t index0, void* d_out_c64, size_t out_stride,
                                      void* stream) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_ddc(iq8_format, true, p, d_in_iq8, n_in, n_chan, freq_word, decim, index0, d_out_c64, out_stride, stream);
}

int sdrk_exec_device_downconvbank_iq8_timed_each(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, int n_chan,
                                                 const uint32_t* freq_word, int decim, uint64_t index0, void* d_out_c64,
                                                 size_t out_stride, int launches, float* each_ms) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_ddc_timed(iq8_format, true, p, d_in_iq8, n_in, n_chan, freq_word, decim, index0, d_out_c64, out_stride, launches,
                                 each_ms);
}

int sdrk_exec_host_downconvbank_iq8(sdrk_plan* p, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n, int n_chan,
                                    const uint32_t* freq_word, int decim, uint64_t sample0, void* out_c64, size_t out_stride,
                                    size_t* n_out) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_ddc(iq8_format, true, p, prefix_iq8, iq_iq8, n, n_chan, freq_word, decim, sample0, out_c64, out_stride, n_out);
}

// ---- filter-and-sum beamformer ----
int sdrk_plan_set_beam(sdrk_plan* p, int channels, int ntaps, const void* taps_c64) {
    int st = check_fir_plan(p);
    if (st != SDRK_OK) return st;
    if (channels < 1 || channels > sdrk::BEAM_MAX_CHANNELS)
        return fail(SDRK_ERR_INVALID, "channels=%d: must be in [1, %d]", channels, sdrk::BEAM_MAX_CHANNELS);
    if (ntaps < 1 || ntaps > sdrk::OLS_MAX_TAPS) return fail(SDRK_ERR_INVALID, "ntaps=%d: must be in [1, %d]", ntaps, sdrk::OLS_MAX_TAPS);
    if (!taps_c64) return fail(SDRK_ERR_INVALID, "taps pointer is NULL");
    constexpr size_t N = sdrk::OLS_N;
    const std::vector<float2> H = fir_responses(taps_c64, channels, ntaps);   // row c: the bits sdrk_plan_set_fir gives its taps
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));   // as sdrk_plan_set_fir: safe for work on the plan's own stream
    p->beam_channels = 0;
    if (!p->d_beam_h) HIP_TRY(hipMalloc((void**)&p->d_beam_h, sdrk::BEAM_MAX_CHANNELS * N * sizeof(float2)));
    HIP_TRY(hipMemcpy(p->d_beam_h, H.data(), (size_t)channels * N * sizeof(float2), hipMemcpyHostToDevice));
    p->beam_taps = ntaps;
    p->beam_channels = channels;
    return SDRK_OK;
}

int sdrk_plan_beam_channels(const sdrk_plan* p) { return p ? p->beam_channels : fail(SDRK_ERR_INVALID, "plan is NULL"); }
int sdrk_plan_beam_taps(const sdrk_plan* p) {
    if (!p) return fail(SDRK_ERR_INVALID, "plan is NULL");
    return p->beam_channels ? p->beam_taps : 0;
}

int sdrk_exec_device_beam(sdrk_plan* p, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                          void* d_out_c64, void* stream) {
    return exec_device_beam(sdrk::BEAM_IN_C64, p, d_in_c64, n_in, freq_word, decim, index0, d_out_c64, stream);
}

int sdrk_exec_device_beam_ci16(sdrk_plan* p, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                               void* d_out_c64, void* stream) {
    return exec_device_beam(sdrk::BEAM_IN_S16, p, d_in_ci16, n_in, freq_word, decim, index0, d_out_c64, stream);
}

int sdrk_exec_device_beam_iq8(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word, int decim,
                              uint64_t index0, void* d_out_c64, void* stream) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_beam(iq8_format, p, d_in_iq8, n_in, freq_word, decim, index0, d_out_c64, stream);
}

int sdrk_exec_device_beam_timed_each(sdrk_plan* p, const void* d_in_c64, size_t n_in, uint32_t freq_word, int decim, uint64_t index0,
                                     void* d_out_c64, int launches, float* each_ms) {
    return exec_device_beam_timed(sdrk::BEAM_IN_C64, p, d_in_c64, n_in, freq_word, decim, index0, d_out_c64, launches, each_ms);
}

int sdrk_exec_device_beam_ci16_timed_each(sdrk_plan* p, const void* d_in_ci16, size_t n_in, uint32_t freq_word, int decim,
                                          uint64_t index0, void* d_out_c64, int launches, float* each_ms) {
    return exec_device_beam_timed(sdrk::BEAM_IN_S16, p, d_in_ci16, n_in, freq_word, decim, index0, d_out_c64, launches, each_ms);
}

int sdrk_exec_device_beam_iq8_timed_each(sdrk_plan* p, const void* d_in_iq8, int iq8_format, size_t n_in, uint32_t freq_word,
                                         int decim, uint64_t index0, void* d_out_c64, int launches, float* each_ms) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_device_beam_timed(iq8_format, p, d_in_iq8, n_in, freq_word, decim, index0, d_out_c64, launches, each_ms);
}

int sdrk_exec_host_beam(sdrk_plan* p, const void* prefix_c64, const void* iq_c64, size_t n, uint32_t freq_word, int decim,
                        uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_beam(sdrk::BEAM_IN_C64, p, prefix_c64, iq_c64, n, freq_word, decim, sample0, out_c64, n_out);
}

int sdrk_exec_host_beam_ci16(sdrk_plan* p, const void* prefix_ci16, const void* iq_ci16, size_t n, uint32_t freq_word, int decim,
                             uint64_t sample0, void* out_c64, size_t* n_out) {
    return exec_host_beam(sdrk::BEAM_IN_S16, p, prefix_ci16, iq_ci16, n, freq_word, decim, sample0, out_c64, n_out);
}

int sdrk_exec_host_beam_iq8(sdrk_plan* p, const void* prefix_iq8, const void* iq_iq8, int iq8_format, size_t n, uint32_t freq_word,
                            int decim, uint64_t sample0, void* out_c64, size_t* n_out) {
    if (int st = check_iq8_format(p, iq8_format); st != SDRK_OK) return st;
    return exec_host_beam(iq8_format, p, prefix_iq8, iq_iq8, n, freq_word, decim, sample0, out_c64, n_out);
}

}  // extern "C"

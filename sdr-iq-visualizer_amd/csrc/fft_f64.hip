// fft_f64.hip — the double-precision transforms behind sdrk_plan_create_f64 (kernels_f64.h): complex128 frames in, float64
// 20*log10(|X| + eps) or complex128 X out, every power of two 2 ... 2^22.  Plain double2 code (the float32 kernels' packed
// arithmetic of cplx.h has no double form); accuracy first: library hypot / log10 / sincospi, no approximations, and products
// fuse only within one expression (-ffp-contract=on).
//
// Every launch works on tiles of F64_TILE = 4096 complex128 values held in LDS (64 KiB: two workgroups per CU), 256 threads,
// 16 values per thread.  A tile is G "lines" of one sub-transform length n = 2^LN (G * n = 4096), transformed by Stockham
// radix-16 passes (one radix-2/4/8 pass first when LN is not a multiple of four) with one LDS exchange between passes:
//   MODE_FRAME  n = nfft <= 4096: G whole frames per tile (lanes run along a frame: coalesced input and output rows);
//   MODE_COL    nfft = N1 * N2 > 4096, n = N1: G adjacent columns n2 of x[N2 n1 + n2] (lanes run across columns, so a
//               row of the tile is G contiguous samples), window on the load, W_nfft^(n2 k1) on the store into the scratch;
//   MODE_ROW    n = N2: G adjacent rows k1 of the scratch, X[k1 + N1 k2] out (lanes across rows: G contiguous bins).
// The scratch holds each frame as blocks of G_row rows interleaved element by element ([k1 / G_row][n2][k1 % G_row]), the
// order in which the row pass reads it.  LDS addresses are XOR-swizzled within 16-element groups: 16-byte accesses are served
// 16 lanes at a time over 64 banks (cdna_hip_programming.md §2), and the first pass's radix-strided stores would otherwise put
// all 16 lanes of a group on the same banks.
#include <hip/hip_runtime.h>

#include "kernels_f64.h"

namespace sdrk {
namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = F64_TILE / THREADS;   // 16 complex128 values = 64 VGPRs

enum { MODE_FRAME = 0, MODE_COL = 1, MODE_ROW = 2 };

struct Params {
    const double2* in;
    size_t in_stride;        // MODE_FRAME / MODE_COL: samples between frames; MODE_ROW: scratch frame = nfft
    void* out;
    const double* window;    // nullptr = rectangular
    const double2* tw;       // W_4096^m
    size_t n_frames;
    int nfft;
    double eps;
    int shift;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

constexpr int brev(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

// exp(-2 pi i m / 16), m < 8, from the symmetric constants cos(pi/8), sin(pi/8), sqrt(1/2)
constexpr double C8 = 0.92387953251128674, S8 = 0.38268343236508977, R2 = 0.70710678118654752;

// b * exp(-2 pi i m / 16) with m a compile-time constant: multiplications by 1 and -i are moves
template <int M>
__device__ __forceinline__ double2 rot16(double2 b) {
    if constexpr (M == 0) return b;
    else if constexpr (M == 4) return make_double2(b.y, -b.x);
    else {
        constexpr double wr[8] = {1.0, C8, R2, S8, 0.0, -S8, -R2, -C8};
        constexpr double wi[8] = {0.0, -S8, -R2, -C8, -1.0, -C8, -R2, -S8};
        return cmul(b, make_double2(wr[M], wi[M]));
    }
}

// In-register DFT of R = 2, 4, 8, 16 values, natural order in and out (radix-2 decimation in time, fully unrolled).
template <int R, int LEN = 2>
__device__ __forceinline__ void dft_stages(double2* t) {
    if constexpr (LEN <= R) {
#pragma unroll
        for (int i = 0; i < R; i += LEN) {
#pragma unroll
            for (int j = 0; j < LEN / 2; ++j) {
                const double2 a = t[i + j];
                double2 b;
                // the twiddle index j * 16 / LEN is a constant once the loops are unrolled
                switch (j * 16 / LEN) {
                    case 0: b = rot16<0>(t[i + j + LEN / 2]); break;
                    case 1: b = rot16<1>(t[i + j + LEN / 2]); break;
                    case 2: b = rot16<2>(t[i + j + LEN / 2]); break;
                    case 3: b = rot16<3>(t[i + j + LEN / 2]); break;
                    case 4: b = rot16<4>(t[i + j + LEN / 2]); break;
                    case 5: b = rot16<5>(t[i + j + LEN / 2]); break;
                    case 6: b = rot16<6>(t[i + j + LEN / 2]); break;
                    default: b = rot16<7>(t[i + j + LEN / 2]); break;
                }
                t[i + j] = cadd(a, b);
                t[i + j + LEN / 2] = csub(a, b);
            }
        }
        dft_stages<R, LEN * 2>(t);
    }
}

template <int R>
__device__ __forceinline__ void dft(double2* v) {
    double2 t[R];
#pragma unroll
    for (int i = 0; i < R; ++i) t[brev(i, ilog2(R))] = v[i];
    dft_stages<R>(t);
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = t[i];
}

__device__ __forceinline__ int swz(int x) { return x ^ ((x >> 4) & 15); }

template <int LN, int MODE>
struct Tile {
    static constexpr int n = 1 << LN;
    static constexpr int G = F64_TILE / n;
    // LDS index of element i of line g: lines contiguous (MODE_FRAME) or interleaved (lanes across lines)
    __device__ static __forceinline__ int lds(int g, int i) { return swz(MODE == MODE_FRAME ? g * n + i : i * G + g); }
    // butterfly b of a pass with NB butterflies per line -> (line, butterfly within the line)
    template <int NB>
    __device__ static __forceinline__ void map(int b, int& g, int& j) {
        if constexpr (MODE == MODE_FRAME) { g = b / NB; j = b % NB; }
        else { g = b % G; j = b / G; }
    }
};

// Where line g of tile `tile` lives: frame and first column / row (MODE_COL / MODE_ROW) or frame (MODE_FRAME).
template <int LN, int MODE>
struct Where {
    size_t f;
    int c;        // MODE_COL: n2; MODE_ROW: k1
    bool valid;
};

template <int LN, int MODE>
__device__ __forceinline__ Where<LN, MODE> where(const Params& P, int g) {
    using T = Tile<LN, MODE>;
    Where<LN, MODE> w;
    const size_t tile = blockIdx.x;
    if constexpr (MODE == MODE_FRAME) {
        w.f = tile * T::G + g;
        w.c = 0;
        w.valid = w.f < P.n_frames;
    } else {
        const int other = P.nfft >> LN;                 // N2 (columns) for MODE_COL, N1 (rows) for MODE_ROW
        const int tiles_per_frame = other / T::G;
        w.f = tile / tiles_per_frame;
        w.c = (int)(tile % tiles_per_frame) * T::G + g;
        w.valid = true;
    }
    return w;
}

// One radix-R Stockham pass over the tile.  NS_LOG = log2 of the length already transformed.
template <int LN, int MODE, int EPI, int R, int NS_LOG>
__device__ __forceinline__ void pass(const Params& P, double2* sm, double2* v) {
    using T = Tile<LN, MODE>;
    constexpr int n = T::n, NB = n / R, BPT = PER_THREAD / R, NS = 1 << NS_LOG;
    constexpr bool FIRST = NS_LOG == 0, LAST = NS * R == n;
    const int tid = threadIdx.x;
    // ---- gather
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        int g, j;
        T::template map<NB>(tid + q * THREADS, g, j);
        if constexpr (FIRST) {
            const Where<LN, MODE> w = where<LN, MODE>(P, g);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int e = j + r * NB;
                double2 x = make_double2(0.0, 0.0);
                if (w.valid) {
                    if constexpr (MODE == MODE_FRAME) {
                        x = P.in[w.f * P.in_stride + e];
                        if (P.window) { const double wv = P.window[e]; x = make_double2(x.x * wv, x.y * wv); }
                    } else if constexpr (MODE == MODE_COL) {
                        const size_t col = (size_t)w.c + (size_t)e * (size_t)(P.nfft >> LN);
                        x = P.in[w.f * P.in_stride + col];
                        if (P.window) { const double wv = P.window[col]; x = make_double2(x.x * wv, x.y * wv); }
                    } else {
                        // scratch: [k1 / G][n2][k1 % G]; this tile's G rows are one block
                        x = P.in[w.f * P.in_stride + (size_t)(w.c - g) * n + (size_t)e * T::G + g];
                    }
                }
                v[q * R + r] = x;
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) v[q * R + r] = sm[T::lds(g, j + r * NB)];
        }
    }
    // ---- twiddle and butterfly
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        int g, j;
        T::template map<NB>(tid + q * THREADS, g, j);
        (void)g;
        if constexpr (NS > 1) {
            const int k = j & (NS - 1);
            constexpr int stride = F64_TILE / (NS * R);   // W_(NS R)^m = W_4096^(m * stride)
            double2 wp[4];
#pragma unroll
            for (int bit = 0; bit < 4; ++bit)
                if ((1 << bit) < R) wp[bit] = P.tw[(k << bit) * stride];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                double2 wr = make_double2(1.0, 0.0);
                bool have = false;
#pragma unroll
                for (int bit = 0; bit < 4; ++bit)
                    if ((r >> bit) & 1) { wr = have ? cmul(wr, wp[bit]) : wp[bit]; have = true; }
                v[q * R + r] = cmul(v[q * R + r], wr);
            }
        }
        dft<R>(v + q * R);
    }
    // ---- scatter
    if constexpr (!LAST) {
        __syncthreads();                                  // every read of this pass is done
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            int g, j;
            T::template map<NB>(tid + q * THREADS, g, j);
            const int k = j & (NS - 1), base = (j >> NS_LOG) * NS * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) sm[T::lds(g, base + r * NS)] = v[q * R + r];
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            int g, j;
            T::template map<NB>(tid + q * THREADS, g, j);
            const Where<LN, MODE> w = where<LN, MODE>(P, g);
            if (!w.valid) continue;
            const size_t N = (size_t)P.nfft;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int e = j + r * NB;                 // output index of this line's transform
                const double2 X = v[q * R + r];
                if constexpr (MODE == MODE_COL) {
                    // four-step twiddle W_N^(n2 k1), then the scratch block layout of the row pass
                    const int N2 = P.nfft >> LN, G2 = F64_TILE / N2;
                    const unsigned m = ((unsigned)w.c * (unsigned)e) & (unsigned)(P.nfft - 1);
                    double s, c;
                    sincospi(-2.0 * (double)m / (double)P.nfft, &s, &c);
                    static_cast<double2*>(P.out)[w.f * N + (size_t)(e / G2) * G2 * N2 + (size_t)w.c * G2 + (e % G2)] =
                        cmul(X, make_double2(c, s));
                } else {
                    size_t bin = MODE == MODE_FRAME ? (size_t)e : (size_t)w.c + (N >> LN) * (size_t)e;
                    if (P.shift) bin = (bin + N / 2) & (N - 1);
                    if constexpr (EPI == EPI64_DB)
                        static_cast<double*>(P.out)[w.f * N + bin] = 20.0 * log10(hypot(X.x, X.y) + P.eps);
                    else
                        static_cast<double2*>(P.out)[w.f * N + bin] = X;
                }
            }
        }
    }
}

template <int LN, int MODE, int EPI, int DONE>
__device__ __forceinline__ void passes(const Params& P, double2* sm, double2* v) {
    constexpr int LR = (DONE == 0 && (LN % 4) != 0) ? LN % 4 : 4;   // the odd radix first, then radix 16
    pass<LN, MODE, EPI, 1 << LR, DONE>(P, sm, v);
    if constexpr (DONE + LR < LN) passes<LN, MODE, EPI, DONE + LR>(P, sm, v);
}

template <int LN, int MODE, int EPI>
__global__ __launch_bounds__(THREADS) void fft_f64_kernel(Params P) {
    __shared__ double2 sm[F64_TILE];
    double2 v[PER_THREAD];
    passes<LN, MODE, EPI, 0>(P, sm, v);
}

template <int LN, int MODE, int EPI>
hipError_t launch_one(const Params& P, size_t blocks, hipStream_t s) {
    hipLaunchKernelGGL((fft_f64_kernel<LN, MODE, EPI>), dim3((unsigned)blocks), dim3(THREADS), 0, s, P);
    return hipGetLastError();
}

// runtime LN -> template, LN in [LO, HI]
template <int MODE, int EPI, int LO, int HI>
hipError_t dispatch(int ln, const Params& P, size_t blocks, hipStream_t s) {
    if constexpr (LO > HI) {
        (void)ln; (void)P; (void)blocks; (void)s;
        return hipErrorInvalidValue;
    } else {
        if (ln == LO) return launch_one<LO, MODE, EPI>(P, blocks, s);
        return dispatch<MODE, EPI, LO + 1, HI>(ln, P, blocks, s);
    }
}

int log2i(long long v) {
    int l = 0;
    while ((1LL << l) < v) ++l;
    return l;
}

}  // namespace

bool fft_f64_split(int nfft, int* l_col, int* l_row) {
    const int l = log2i(nfft);
    if (nfft < 2 || (1 << l) != nfft || l > 22) return false;
    if (l <= 12) { *l_col = 0; *l_row = l; return true; }
    *l_col = l / 2;            // 6 ... 11
    *l_row = l - l / 2;        // 7 ... 11
    return true;
}

hipError_t launch_fft_f64(const F64Args& a) {
    int lc = 0, lr = 0;
    if (!fft_f64_split(a.nfft, &lc, &lr) || a.n_frames == 0) return hipErrorInvalidValue;
    Params P;
    P.window = a.d_window;
    P.tw = reinterpret_cast<const double2*>(a.d_twiddle);
    P.nfft = a.nfft;
    P.eps = a.eps;
    P.shift = a.shift;
    if (lc == 0) {
        P.in = static_cast<const double2*>(a.d_iq);
        P.in_stride = a.frame_stride;
        P.out = a.d_out;
        P.n_frames = a.n_frames;
        const size_t per = (size_t)(F64_TILE >> lr), blocks = (a.n_frames + per - 1) / per;
        return a.epilogue == EPI64_DB ? dispatch<MODE_FRAME, EPI64_DB, 1, 12>(lr, P, blocks, a.stream)
                                      : dispatch<MODE_FRAME, EPI64_COMPLEX, 1, 12>(lr, P, blocks, a.stream);
    }
    if (!a.d_scratch || a.scratch_frames == 0) return hipErrorInvalidValue;
    const size_t N = (size_t)a.nfft, out_elem = a.epilogue == EPI64_DB ? sizeof(double) : 2 * sizeof(double);
    const size_t col_tiles = (N >> lc) / (size_t)(F64_TILE >> lc), row_tiles = (N >> lr) / (size_t)(F64_TILE >> lr);
    for (size_t f0 = 0; f0 < a.n_frames; f0 += a.scratch_frames) {
        const size_t nf = a.n_frames - f0 < a.scratch_frames ? a.n_frames - f0 : a.scratch_frames;
        Params C = P;
        C.in = static_cast<const double2*>(a.d_iq) + f0 * a.frame_stride;
        C.in_stride = a.frame_stride;
        C.out = a.d_scratch;
        C.n_frames = nf;
        hipError_t e = dispatch<MODE_COL, EPI64_COMPLEX, 6, 11>(lc, C, nf * col_tiles, a.stream);
        if (e != hipSuccess) return e;
        Params Rw = P;
        Rw.in = static_cast<const double2*>(a.d_scratch);
        Rw.in_stride = N;
        Rw.window = nullptr;
        Rw.out = static_cast<char*>(a.d_out) + f0 * N * out_elem;
        Rw.n_frames = nf;
        e = a.epilogue == EPI64_DB ? dispatch<MODE_ROW, EPI64_DB, 7, 11>(lr, Rw, nf * row_tiles, a.stream)
                                   : dispatch<MODE_ROW, EPI64_COMPLEX, 7, 11>(lr, Rw, nf * row_tiles, a.stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sdrk

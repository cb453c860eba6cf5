// The NTT passes and their dispatch, written once against the field traits (GlF: canonical u64 words; BbF: 32-bit Montgomery words).
// Included by kernels_ntt16.hip and kernels_bb16.hip, which define what stays per field - the register DFTs (Dft<F>, below), the
// LDE's contiguous pass (lde_pb_r16) and its strided pass of 2^22 rows - and instantiate the templates declared in kernels.hpp.
// The LDE's strided passes and their dispatcher lde_pa_r16 are in lde_passes.hpp.
//
// Data stays column-major [col][n]; every pass moves tiles HBM -> LDS / registers -> HBM with >= 64-byte contiguous row segments.
//  inverse (values -> coefficients, natural -> natural), n = 2^L:
//     L <= 12:         one LDS tile per column (k_ntt_small)
//     12 < L <= 15:    LDS radix-2 passes, i = a 2^8 + c (LA = L - 8, LC = 8)
//                        P1: DFT over a, twiddle w^-(k_a c)                     tile 2^LA rows x 16 contiguous
//                        P3: DFT over c, * n^-1, transposed write to k = k_a + 2^LA k_c
//     16 <= L <= 22:   radix-16 register passes, i = a 2^(LB+8) + b 2^8 + c (LA = LC = 8, LB = L - 16)
//                        P1 (8 bits strided), P2 (LB bits, none at 2^16 rows), P3 (8 bits, transposed write)
//  LDE (coefficients -> leaf-order evaluations on the 2^r cosets 7 w_N^bitrev(c) H_n):
//     L <= 12:         one LDS tile per (column, coset) (k_lde_pb)
//     12 < L <= 22:    PA (L - 12 bits strided, per-coset loop; lde_passes.hpp), PB (12 bits contiguous, natural -> leaf order; per field)
//  L > 22: one outer radix step (ntt_outer.hpp) around transforms of 2^22 rows and fewer.
#pragma once
#include <algorithm>

#include "kernels.hpp"
#include "ntt_outer.hpp"

namespace gbk {

static constexpr int THREADS = 256;
static constexpr int TILE = 4096;

// Per field (kernels_ntt16.hip, kernels_bb16.hip): the in-register DFTs of the radix-16 passes, natural input order, X[k] in slot
// brev(k) - static members template <bool INV> dft16(T (&)[16]), template <bool INV, int K> dft_small(T (&)[16]) (2^K points, K = 1..3),
// template <bool INV> dft32(T (&)[32]) and template <bool INV, int H, int O> layer64(T*) (one DIF layer of half-size H on
// x[O .. O + 2H), twiddles w_64^(+-j)).
template <class F>
struct Dft;

// ------------------------------------------------------------------ LDS radix-2 passes

__device__ __forceinline__ u32 brev(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }

// Pure size-2^m DFT along bits [p, p+m) of the LDS tile index, natural -> bit-reversed positions,
// all other index bits are batch.  tw = w_4096^(+-j) table (4096 entries).
template <class F>
__device__ __forceinline__ void lds_dft(typename F::T* sh, u32 tile_elems, u32 p, u32 m, const typename F::T* __restrict__ tw) {
    typedef typename F::T T;
    const u32 half = tile_elems >> 1;
    for (u32 l = 0; l < m; l++) {
        const u32 bitpos = p + m - 1 - l;
        const u32 hmask = (1u << (m - 1 - l)) - 1;
        const u32 lowmask = (1u << bitpos) - 1;
        for (u32 q = threadIdx.x; q < half; q += THREADS) {
            u32 e1 = ((q >> bitpos) << (bitpos + 1)) | (q & lowmask);
            u32 e2 = e1 | (1u << bitpos);
            u32 j = (e1 >> p) & hmask;
            T a = sh[e1], b = sh[e2];
            T d = F::sub(a, b);
            if (j) d = F::mul(d, tw[(j << l) << (12 - m)]);
            sh[e1] = F::add(a, b);
            sh[e2] = d;
        }
        __syncthreads();
    }
}

// w_n^(+-e) from the split tables: e = 1024*e_hi + e_lo
template <class F>
__device__ __forceinline__ typename F::T tw_split(const typename F::T* __restrict__ hi, const typename F::T* __restrict__ lo, u32 e) {
    u32 eh = e >> 10, el = e & 1023;
    typename F::T w = lo[el];
    return eh ? F::mul(w, hi[eh]) : w;
}

struct InvGeom {
    u32 L, LA, LC;   // LA = L - 8, LC = 8
};

// P1: grid = ncols * 2^(LC-4); src natural, dst layout [k_a][c]
template <class F>
__global__ __launch_bounds__(THREADS) void k_intt_p1(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, InvGeom g,
                                                     const typename F::T* __restrict__ tw4096, const typename F::T* __restrict__ tw_hi,
                                                     const typename F::T* __restrict__ tw_lo) {
    typedef typename F::T T;
    __shared__ T sh[TILE];
    const u32 tiles_per_col = 1u << (g.LC - 4);
    const size_t col = blockIdx.x / tiles_per_col;
    const u32 tg = blockIdx.x % tiles_per_col;
    const size_t base = (col << g.L) + ((size_t)tg << 4);
    const u32 rows = 1u << g.LA;
    const u32 j = threadIdx.x & 15, r0 = threadIdx.x >> 4;
    for (u32 a = r0; a < rows; a += 16) sh[a * 16 + j] = src[base + ((size_t)a << g.LC) + j];
    __syncthreads();
    lds_dft<F>(sh, rows * 16, 4, g.LA, tw4096);
    const u32 l = (tg << 4) + j;
    for (u32 ka = r0; ka < rows; ka += 16) {
        T v = sh[brev(ka, g.LA) * 16 + j];
        u32 e = ka * l;
        if (e) v = F::mul(v, tw_split<F>(tw_hi, tw_lo, e));
        dst[base + ((size_t)ka << g.LC) + j] = v;
    }
}

// P3: grid = ncols * 2^(LA-4); src layout [k_a][c]; dst natural k = k_a + 2^LA k_c
template <class F>
__global__ __launch_bounds__(THREADS) void k_intt_p3(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, InvGeom g,
                                                     const typename F::T* __restrict__ tw4096, typename F::T n_inv) {
    typedef typename F::T T;
    __shared__ T sh[TILE];
    const u32 n_ga = 1u << (g.LA - 4), nc = 1u << g.LC;
    const size_t col = blockIdx.x / n_ga;
    const u32 ga = blockIdx.x % n_ga;
    const size_t cbase = col << g.L;
    const size_t sbase = cbase + ((size_t)(16 * ga) << g.LC);
    for (u32 t = threadIdx.x; t < 16 * nc; t += THREADS) sh[t] = src[sbase + t];  // 16 rows of 2^LC, contiguous
    __syncthreads();
    lds_dft<F>(sh, 16 * nc, 0, g.LC, tw4096);
    const u32 ia = threadIdx.x & 15, r0 = threadIdx.x >> 4;
    for (u32 kc = r0; kc < nc; kc += 16) {
        T v = F::mul(sh[ia * nc + brev(kc, g.LC)], n_inv);
        dst[cbase + ((size_t)kc << g.LA) + 16 * ga + ia] = v;
    }
}

// single-tile transform for L <= 12: grid = ncols; natural -> natural, scaled by `scale`
template <class F>
__global__ __launch_bounds__(THREADS) void k_ntt_small(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 L,
                                                       const typename F::T* __restrict__ tw4096, typename F::T scale) {
    __shared__ typename F::T sh[TILE];
    const u32 n = 1u << L;
    const size_t base = (size_t)blockIdx.x << L;
    for (u32 t = threadIdx.x; t < n; t += THREADS) sh[t] = src[base + t];
    __syncthreads();
    lds_dft<F>(sh, n, 0, L, tw4096);
    for (u32 k = threadIdx.x; k < n; k += THREADS) dst[base + k] = F::mul(sh[brev(k, L)], scale);
}

// LDE of L <= 12 rows: one tile of 2^LT = n points per (column, coset), coeffs * s^l, forward DIF natural -> bit-reversed.
// grid = ncols * 2^r.
template <class F>
__global__ __launch_bounds__(THREADS) void k_lde_pb(const typename F::T* __restrict__ coeffs, typename F::T* __restrict__ lde, u32 L,
                                                    u32 rate_bits, const typename F::T* __restrict__ tw4096,
                                                    const typename F::T* __restrict__ pow_lo) {
    typedef typename F::T T;
    __shared__ T sh[TILE];
    const u32 LT = L < 12 ? L : 12;
    const u32 te = 1u << LT;
    const size_t tile = blockIdx.x;  // (col, coset) flattened == contiguous tiles of lde
    T* p = lde + (tile << LT);
    const size_t col = tile >> rate_bits;
    const u32 c = (u32)(tile & ((1u << rate_bits) - 1));
    const T* cin = coeffs + (col << L);
    const T* pl = pow_lo + ((size_t)c << LT);
    for (u32 t = threadIdx.x; t < te; t += THREADS) sh[t] = F::mul(cin[t], pl[t]);
    __syncthreads();
    lds_dft<F>(sh, te, 0, LT, tw4096);
    for (u32 t = threadIdx.x; t < te; t += THREADS) p[t] = sh[t];
}

// ------------------------------------------------------------------ radix-16 register passes: shared pieces
// Table products are F::mulc (times a table value in the kernels' form: Goldilocks' Montgomery-form twins, BabyBear's Montgomery
// words), product chains that are only multiplied again F::mul_chain.

__device__ __forceinline__ constexpr u32 brev4(u32 x) { return ((x & 1) << 3) | ((x & 2) << 1) | ((x & 4) >> 1) | ((x & 8) >> 3); }
__device__ __forceinline__ constexpr u32 brevk(u32 x, int k) {
    u32 r = 0;
    for (int i = 0; i < k; i++) r |= ((x >> i) & 1) << (k - 1 - i);
    return r;
}

template <class F>
__device__ __forceinline__ typename F::T tw_split16(const typename F::T* __restrict__ hi, const typename F::T* __restrict__ lo, u32 e) {
    u32 eh = e >> 10, el = e & 1023;
    typename F::T w = lo[el];
    return eh ? F::mul_chain(w, hi[eh]) : w;   // Goldilocks' Montgomery-form tables: (lo R)(hi R) / R = lo hi R, any residue
}

// The 15 inter-stage twiddles w_4096^(k m), k = brev4(slot), as ONE batch of independent loads issued before the
// DFT that precedes their use.  (Loaded one by one behind `if (e)` each of them cost a full memory round trip:
// rocprofv3 showed the waves of these kernels parked in s_waitcnt for 46-66 % of their lifetime.)
template <class F>
__device__ __forceinline__ void load_tw16(typename F::T (&tw)[16], const typename F::T* __restrict__ tw4096, u32 m) {
#pragma unroll
    for (u32 s = 1; s < 16; s++) tw[s] = tw4096[brev4(s) * m];
}

// ------------------------------------------------------------------ inverse NTT, radix-16 passes (LA = 8, LB = 0..6, LC = 8)
struct Inv16Geom {
    u32 L, LB;  // LA = LC = 8, LL = LB + 8
};

// P1: grid = ncols * 2^(LL-4); tile 256 rows (a) x 16 contiguous; rows written in natural k_a order.
// WB (BabyBear only, round 4): the input is CANONICAL - the transform is linear and every twiddle product multiplies by the twiddle's
// value (x (w R) / R), so canonical words go through it unchanged in scale and P3's last factor n^-1 R^2 instead of n^-1 R brings the
// coefficients out in Montgomery form: no conversion pass (k_bb_to_mont: a read and a write of the whole witness).  The columns
// somebody reads as VALUES afterwards - the routed wires, for the permutation argument - are written back in Montgomery form
// here, each element by the one thread that has just read it (col < mont_cols).
template <class F, bool WB>
__global__ __launch_bounds__(THREADS) void k_intt16_p1(const typename F::T* src, typename F::T* __restrict__ dst, Inv16Geom g,
                                                       const typename F::T* __restrict__ tw4096, const typename F::T* __restrict__ tw_hi,
                                                       const typename F::T* __restrict__ tw_lo, typename F::T* src_mont, u32 mont_cols) {
    typedef typename F::T T;
    __shared__ T sh[16 * 272];
    const u32 LL = g.LB + 8;
    const u32 tiles_per_col = 1u << (LL - 4);
    const size_t col = blockIdx.x / tiles_per_col;
    const u32 tg = blockIdx.x % tiles_per_col;
    const size_t base = (col << g.L) + ((size_t)tg << 4);
    const u32 tid = threadIdx.x, hi4 = tid >> 4, j = tid & 15;
    T x[16];
#pragma unroll
    for (u32 a1 = 0; a1 < 16; a1++) x[a1] = src[base + ((size_t)(a1 * 16 + hi4) << LL) + j];
    if (WB && col < mont_cols) {
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) src_mont[base + ((size_t)(a1 * 16 + hi4) << LL) + j] = F::enc(x[a1]);
    }
    T tw[16];
    load_tw16<F>(tw, tw4096, hi4 * 16);
    const u32 l = (tg << 4) + j;
    const u32 ka1 = brev4(hi4);
    // output twiddle w_n^-(k_a l), k_a = k_a1 + 16 k: a geometric progression in k with ratio w_n^-(16 l)
    T f = tw_split16<F>(tw_hi, tw_lo, ka1 * l);
    const T ratio = tw_split16<F>(tw_hi, tw_lo, 16 * l);
    Dft<F>::template dft16<true>(x);
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[s * 272 + tid] = s ? F::mulc(x[s], tw[s]) : x[s];
    __syncthreads();
#pragma unroll
    for (u32 a0 = 0; a0 < 16; a0++) x[a0] = sh[hi4 * 272 + a0 * 16 + j];
    Dft<F>::template dft16<true>(x);
#pragma unroll
    for (u32 k = 0; k < 16; k++) {
        dst[base + ((size_t)(ka1 + 16 * k) << LL) + j] = F::mulc(x[brev4(k)], f);
        if (k < 15) f = F::mul_chain(f, ratio);
    }
}

// P2 (LB = 4): grid = ncols * 16 * 16; tile 16 k_a x 16 b x 16 c; src [k_a][b][c] -> dst [k_b][k_a][c]
template <class F>
__global__ __launch_bounds__(THREADS) void k_intt16_p2(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 L,
                                                       const typename F::T* __restrict__ tw4096) {
    typedef typename F::T T;
    const size_t col = blockIdx.x >> 8;
    const u32 ga = (blockIdx.x >> 4) & 15, gc = blockIdx.x & 15;
    const size_t cbase = col << L;
    const u32 ia = threadIdx.x >> 4, jc = threadIdx.x & 15;
    const u32 ka = 16 * ga + ia, c = 16 * gc + jc;
    T x[16];
#pragma unroll
    for (u32 b = 0; b < 16; b++) x[b] = src[cbase + ((size_t)ka << 12) + ((size_t)b << 8) + c];
    T tw[16];
    load_tw16<F>(tw, tw4096, c);  // w_4096^-(c k_b)
    Dft<F>::template dft16<true>(x);
#pragma unroll
    for (u32 s = 0; s < 16; s++)
        dst[cbase + ((size_t)brev4(s) << 16) + ((size_t)ka << 8) + c] = s ? F::mulc(x[s], tw[s]) : x[s];
}

// P2 for LB = K in 1..3 (L = 16 + K): the same pass with a radix-2^K DFT over b; src [k_a][b][c] -> dst [k_b][k_a][c]
template <class F, int K>
__global__ __launch_bounds__(THREADS) void k_intt16_p2s(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst,
                                                        const typename F::T* __restrict__ tw4096) {
    typedef typename F::T T;
    constexpr u32 L = 16 + K, R = 1u << K;
    const size_t col = blockIdx.x >> 8;
    const u32 ga = (blockIdx.x >> 4) & 15, gc = blockIdx.x & 15;
    const size_t cbase = col << L;
    const u32 ka = 16 * ga + (threadIdx.x >> 4), c = 16 * gc + (threadIdx.x & 15);
    T x[16];
#pragma unroll
    for (u32 b = 0; b < R; b++) x[b] = src[cbase + ((size_t)ka << (8 + K)) + ((size_t)b << 8) + c];
    T tw[R];
#pragma unroll
    for (u32 s = 1; s < R; s++) tw[s] = tw4096[(brevk(s, K) * c) << (4 - K)];  // w_{2^(8+K)}^-(c k_b)
    Dft<F>::template dft_small<true, K>(x);
#pragma unroll
    for (u32 s = 0; s < R; s++)
        dst[cbase + ((size_t)brevk(s, K) << 16) + ((size_t)ka << 8) + c] = s ? F::mulc(x[s], tw[s]) : x[s];
}

// P2 for LB = 5, 6 (2^21 and 2^22 rows, round 6): the middle pass as a radix-32 / radix-64 DFT over b in registers - one or two DIF
// layers with the roots w_64^-j (Goldilocks: powers of two, so the whole DFT is shifts), then 16-point blocks.
// src [k_a][b][c] -> dst [k_b][k_a][c]; tw16k = w_{2^14}^-j, j < 2^14.  X[k_b] ends up in slot brev_LB(k_b).
template <class F, int LB>
__global__ __launch_bounds__(THREADS) void k_intt16_p2w(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst,
                                                        const typename F::T* __restrict__ tw16k) {
    typedef typename F::T T;
    constexpr u32 L = 16 + LB, R = 1u << LB;
    const size_t col = blockIdx.x >> 8;
    const u32 ga = (blockIdx.x >> 4) & 15, gc = blockIdx.x & 15;
    const size_t cbase = col << L;
    const u32 ka = 16 * ga + (threadIdx.x >> 4), c = 16 * gc + (threadIdx.x & 15);
    T x[R];
#pragma unroll
    for (u32 b = 0; b < R; b++) x[b] = src[cbase + ((size_t)ka << (8 + LB)) + ((size_t)b << 8) + c];
    if constexpr (LB == 6) {
        Dft<F>::template layer64<true, 32, 0>(x);
        Dft<F>::template layer64<true, 16, 0>(x);
        Dft<F>::template layer64<true, 16, 32>(x);
    } else {
        Dft<F>::template layer64<true, 16, 0>(x);
    }
#pragma unroll
    for (u32 o = 0; o < R; o += 16) Dft<F>::template dft16<true>(*reinterpret_cast<T(*)[16]>(&x[o]));
#pragma unroll
    for (u32 s = 0; s < R; s++) {
        const u32 kb = brevk(s, LB);
        dst[cbase + ((size_t)kb << 16) + ((size_t)ka << 8) + c] = s ? F::mulc(x[s], tw16k[(kb * c) << (6 - LB)]) : x[s];   // w_{2^(8+LB)}^-(c k_b)
    }
}

// P3: grid = ncols * 2^LB * 16; tile 16 k_a x 256 c (c = 16 c1 + c0); src [k_b][k_a][c];
// dst natural k = k_a + 256 k_b + 2^(8+LB) k_c, scaled by n^-1
template <class F>
__global__ __launch_bounds__(THREADS) void k_intt16_p3(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, Inv16Geom g,
                                                       const typename F::T* __restrict__ tw4096, typename F::T n_inv) {
    typedef typename F::T T;
    __shared__ T sh[16 * 272];
    const u32 nb = 1u << g.LB;
    const size_t col = blockIdx.x / (nb * 16);
    const u32 rem = blockIdx.x % (nb * 16);
    const u32 kb = rem >> 4, ga = rem & 15;
    const size_t cbase = col << g.L;
    const size_t sbase = cbase + ((size_t)kb << 16) + ((size_t)(16 * ga) << 8);
    const u32 tid = threadIdx.x, hi4 = tid >> 4, lo4 = tid & 15;
    T x[16];
    // stage 1 thread = (ia = hi4, c0 = lo4): digit c1
#pragma unroll
    for (u32 c1 = 0; c1 < 16; c1++) x[c1] = src[sbase + hi4 * 256 + c1 * 16 + lo4];
    T tw[16];
    load_tw16<F>(tw, tw4096, lo4 * 16);  // w_256^-(k_c1 c0)
    Dft<F>::template dft16<true>(x);
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[s * 272 + lo4 * 17 + hi4] = s ? F::mulc(x[s], tw[s]) : x[s];  // [k_c1 slot][c0][ia], rows padded to 17
    __syncthreads();
    // stage 2 thread = (k_c1 slot = hi4, ia = lo4): digit c0
#pragma unroll
    for (u32 c0 = 0; c0 < 16; c0++) x[c0] = sh[hi4 * 272 + c0 * 17 + lo4];
    Dft<F>::template dft16<true>(x);
    const u32 kc1 = brev4(hi4);
#pragma unroll
    for (u32 s = 0; s < 16; s++) {
        const u32 kc = kc1 + 16 * brev4(s);
        dst[cbase + ((size_t)kc << (8 + g.LB)) + ((size_t)kb << 8) + 16 * ga + lo4] = F::mulc(x[s], n_inv);
    }
}

// ------------------------------------------------------------------ element-wise kernels

// dst[c] = the canonical value of column c at row `index`, c < width
template <class F>
__global__ void k_gather_row(const typename F::T* __restrict__ cols, size_t col_stride, u32 width, u64 index, typename F::T* dst) {
    u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < width) dst[c] = (typename F::T)F::dec(cols[(size_t)c * col_stride + index]);
}

// canonical src -> dst in device form, dst[col][j] = src[col][bitrev_bits(j)]; total = ncols << bits
template <class F>
__global__ void k_bitrev_copy(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 bits, size_t total) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    size_t col = g >> bits;
    u64 j = g & (((u64)1 << bits) - 1);
    u64 r = bits ? (__brevll(j) >> (64 - bits)) : 0;
    dst[g] = F::enc(src[(col << bits) + r]);
}

// column-major [width][col_stride] -> row-major canonical [rows][width]
template <class F>
__global__ void k_transpose_to_rows(const typename F::T* __restrict__ cols, size_t col_stride, u32 width, u64 rows,
                                    typename F::T* __restrict__ dst) {
    u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= rows * width) return;
    u64 r = g / width;
    u32 c = (u32)(g % width);
    dst[g] = (typename F::T)F::dec(cols[(size_t)c * col_stride + r]);
}

// any word -> its residue below p (F::reduce_word), in place, 16 bytes per thread
template <class F>
__global__ __launch_bounds__(256) void k_reduce_words(typename F::T* __restrict__ p, size_t count) {
    typedef typename F::T T;
    constexpr u32 V = 16 / sizeof(T);
    struct alignas(16) Vec { T v[V]; };
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (i + V - 1 < count) {
        Vec w = *reinterpret_cast<Vec*>(p + i);
#pragma unroll
        for (u32 k = 0; k < V; k++) w.v[k] = F::reduce_word(w.v[k]);
        *reinterpret_cast<Vec*>(p + i) = w;
    } else {
        for (size_t k = i; k < count; k++) p[k] = F::reduce_word(p[k]);
    }
}

// ------------------------------------------------------------------ host launchers

static inline u32 nblk(size_t n, u32 bs) { return (u32)((n + bs - 1) / bs); }

// the LDE's strided pass for 12 < log_n <= 22 (lde_passes.hpp)
template <class F>
void lde_pa_r16(const typename F::T* coeffs, typename F::T* lde, size_t ncols, const NttTables<F>& t, const CosetTables<F>& ct,
                hipStream_t stream);
// per field (kernels_ntt16.hip, kernels_bb16.hip): its contiguous pass over `ntiles` 4096-point tiles of `lde`, in place
void lde_pb_r16(u64* lde, size_t ntiles, const GlNttTables& t, hipStream_t stream);
void lde_pb_r16(u32* lde, size_t ntiles, const BbNttTables& t, hipStream_t stream);

// The tables the radix-16 inverse passes read: Goldilocks' Montgomery-form twins (their products end in gl::mul_mont), BabyBear's
// plain tables (Montgomery words already)
template <class F>
struct Inv16Tables {
    const typename F::T *tw4096, *tw_hi, *tw_lo, *tw16k;
    typename F::T n_inv;
};
inline Inv16Tables<GlF> inv16_tables(const GlNttTables& t) { return {t.tw4096_inv_m, t.tw_hi_inv_m, t.tw_lo_inv_m, t.tw16k_inv_m, t.n_inv_m}; }
inline Inv16Tables<BbF> inv16_tables(const BbNttTables& t) { return {t.tw4096_inv, t.tw_hi_inv, t.tw_lo_inv, t.tw16k_inv, t.n_inv}; }

// The radix-16 inverse passes, 2^16..2^22 rows.  WB: `src` is CANONICAL (BabyBear, k_intt16_p1<BbF, true>) and writable as `src_mont`,
// whose first mont_cols columns are overwritten with their device form; the coefficients come out in device form either way.
template <class F, bool WB>
void intt_columns_r16(const typename F::T* src, typename F::T* coeffs, typename F::T* scratch, size_t ncols, const NttTables<F>& t,
                      hipStream_t stream, typename F::T* src_mont, size_t mont_cols) {
    typedef typename F::T T;
    const Inv16Tables<F> tt = inv16_tables(t);
    const u32 L = t.log_n;
    const Inv16Geom g{L, L - 16};
    const u32 LL = g.LB + 8;
    T* p1_dst = g.LB ? coeffs : scratch;
    const T n_inv = WB ? F::enc(tt.n_inv) : tt.n_inv;   // n^-1 R^2 : n^-1 R
    hipLaunchKernelGGL((k_intt16_p1<F, WB>), dim3((u32)(ncols << (LL - 4))), dim3(THREADS), 0, stream, src, p1_dst, g, tt.tw4096, tt.tw_hi,
                       tt.tw_lo, src_mont, (u32)std::min<size_t>(mont_cols, ncols));
    const dim3 g2((u32)(ncols << 8));
    if (g.LB == 6) hipLaunchKernelGGL((k_intt16_p2w<F, 6>), g2, dim3(THREADS), 0, stream, coeffs, scratch, tt.tw16k);
    else if (g.LB == 5) hipLaunchKernelGGL((k_intt16_p2w<F, 5>), g2, dim3(THREADS), 0, stream, coeffs, scratch, tt.tw16k);
    else if (g.LB == 4) hipLaunchKernelGGL(k_intt16_p2<F>, g2, dim3(THREADS), 0, stream, coeffs, scratch, L, tt.tw4096);
    else if (g.LB == 3) hipLaunchKernelGGL((k_intt16_p2s<F, 3>), g2, dim3(THREADS), 0, stream, coeffs, scratch, tt.tw4096);
    else if (g.LB == 2) hipLaunchKernelGGL((k_intt16_p2s<F, 2>), g2, dim3(THREADS), 0, stream, coeffs, scratch, tt.tw4096);
    else if (g.LB == 1) hipLaunchKernelGGL((k_intt16_p2s<F, 1>), g2, dim3(THREADS), 0, stream, coeffs, scratch, tt.tw4096);
    hipLaunchKernelGGL(k_intt16_p3<F>, dim3((u32)(ncols << (g.LB + 4))), dim3(THREADS), 0, stream, scratch, coeffs, g, tt.tw4096, n_inv);
}

// run(c0, nc) over the column groups of the inverse transform: from 2^18 rows up, groups of INTT_GROUP 8-byte words' worth of columns
// (the same bytes per group from 2^20 rows up)
template <class F, class Run>
void for_intt_groups(u32 log_n, size_t ncols, Run run) {
    const size_t g0 = INTT_GROUP * 8 / sizeof(typename F::T), g = log_n > 20 ? g0 >> (log_n - 20) : g0;
    if (log_n < 18 || ncols <= g) return run(0, ncols);
    for (size_t c0 = 0; c0 < ncols; c0 += g)   // the scratch block of one group is reused by the next: it never leaves the cache
        run(c0, std::min(g, ncols - c0));
}

template <class F>
void intt_group(const typename F::T* src, typename F::T* coeffs, typename F::T* scratch, size_t ncols, const NttTables<F>& t,
                hipStream_t stream) {
    const u32 L = t.log_n;
    if (ncols == 0) return;
    if (L <= 12) {
        hipLaunchKernelGGL(k_ntt_small<F>, dim3((u32)ncols), dim3(THREADS), 0, stream, src, coeffs, L, t.tw4096_inv, t.n_inv);
        return;
    }
    if (L >= 16) return intt_columns_r16<F, false>(src, coeffs, scratch, ncols, t, stream, nullptr, 0);
    const InvGeom g{L, L - 8, 8};
    hipLaunchKernelGGL(k_intt_p1<F>, dim3((u32)(ncols << (g.LC - 4))), dim3(THREADS), 0, stream, src, scratch, g, t.tw4096_inv,
                       t.tw_hi_inv, t.tw_lo_inv);
    hipLaunchKernelGGL(k_intt_p3<F>, dim3((u32)(ncols << (g.LA - 4))), dim3(THREADS), 0, stream, scratch, coeffs, g, t.tw4096_inv,
                       t.n_inv);
}

template <class F>
void intt_columns(const typename F::T* src, typename F::T* coeffs, typename F::T* scratch, size_t ncols, const NttTables<F>& t,
                  hipStream_t stream) {
    typedef typename F::T T;
    if (t.sub) {   // more than 2^22 rows: one outer radix step around the sub-transforms (ntt_outer.hpp)
        outer::intt_columns<F>(src, coeffs, scratch, ncols, t.log_n, t.outer_bits, t.tw_hi_inv, t.tw_lo_inv,
                               [&](const T* s, T* d, T* scr, size_t nc) { intt_columns<F>(s, d, scr, nc, *t.sub, stream); }, stream);
        return;
    }
    const size_t n = (size_t)1 << t.log_n;
    for_intt_groups<F>(t.log_n, ncols, [&](size_t c0, size_t nc) { intt_group<F>(src + c0 * n, coeffs + c0 * n, scratch, nc, t, stream); });
}

template <class F>
void lde_columns(const typename F::T* coeffs, typename F::T* lde, size_t ncols, const NttTables<F>& t, const CosetTables<F>& ct,
                 hipStream_t stream) {
    typedef typename F::T T;
    const u32 L = t.log_n, r = ct.rate_bits;
    if (ncols == 0) return;
    if (t.sub) {
        outer::lde_columns<F>(coeffs, lde, ncols, L, t.outer_bits, r, t.tw_hi_fwd, t.tw_lo_fwd, t.tw_top_fwd, ct.pow_lo, (T*)*ct.work,
                              *ct.work_bytes / sizeof(T),
                              [&](const T* c, T* o, size_t nc) { lde_columns<F>(c, o, nc, *t.sub, *ct.sub, stream); }, stream);
        return;
    }
    if (L <= 12) {
        hipLaunchKernelGGL(k_lde_pb<F>, dim3((u32)(ncols << r)), dim3(THREADS), 0, stream, coeffs, lde, L, r, t.tw4096_fwd, ct.pow_lo);
        return;
    }
    // both passes over all columns per launch: they are bound by VALU issue, not by HBM (column groups sized for the Infinity Cache
    // measured slower in every setting, HISTORY.md round 3)
    lde_pa_r16<F>(coeffs, lde, ncols, t, ct, stream);
    lde_pb_r16(lde, ncols << (r + L - 12), t, stream);
}

template <class F>
void gather_row(const typename F::T* cols, size_t col_stride, u32 width, u64 index, typename F::T* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_gather_row<F>, dim3(nblk(width, 64)), dim3(64), 0, stream, cols, col_stride, width, index, dst);
}
template <class F>
void transpose_to_rows(const typename F::T* cols, size_t col_stride, u32 width, u64 rows, typename F::T* dst, hipStream_t stream) {
    if (rows && width)
        hipLaunchKernelGGL(k_transpose_to_rows<F>, dim3(nblk(rows * width, 256)), dim3(256), 0, stream, cols, col_stride, width, rows, dst);
}
template <class F>
void bitrev_copy(const typename F::T* src, typename F::T* dst, u32 bits, size_t ncols, hipStream_t stream) {
    const size_t total = ncols << bits;
    if (total) hipLaunchKernelGGL(k_bitrev_copy<F>, dim3(nblk(total, 256)), dim3(256), 0, stream, src, dst, bits, total);
}
template <class F>
void reduce_words(typename F::T* p, size_t count, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(k_reduce_words<F>, dim3(nblk(count, 256 * 16 / sizeof(typename F::T))), dim3(256), 0, stream, p, count);
}

// the host templates of kernels.hpp for one field (kernels_ntt16.hip, kernels_bb16.hip)
#define GB_INSTANTIATE_NTT(F)                                                                                                       \
    template void intt_columns<F>(const F::T*, F::T*, F::T*, size_t, const NttTables<F>&, hipStream_t);                              \
    template void lde_columns<F>(const F::T*, F::T*, size_t, const NttTables<F>&, const CosetTables<F>&, hipStream_t);               \
    template void gather_row<F>(const F::T*, size_t, u32, u64, F::T*, hipStream_t);                                                  \
    template void transpose_to_rows<F>(const F::T*, size_t, u32, u64, F::T*, hipStream_t);                                           \
    template void bitrev_copy<F>(const F::T*, F::T*, u32, size_t, hipStream_t);                                                      \
    template void reduce_words<F>(F::T*, size_t, hipStream_t);

}  // namespace gbk

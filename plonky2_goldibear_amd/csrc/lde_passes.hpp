// The LDE's strided passes ("PA": L - 12 bits strided, per-coset loop), written once against the field traits.  Included by
// kernels_ntt16.hip and kernels_bb16.hip after ntt_passes.hpp and their dft_*.hpp.  Both fields run the same tiles, index math and
// memory layouts; what differs is the word, the products (F::mulc times a table value, F::mul_chain for the running twiddles) and
// the tuning collected in LdeTune<F>.  Per field remain the contiguous pass (lde_pb_r16) and the 2^22-row pass (lde_pa_rows22).
//
// Per coset c: scale the coefficients by s_c^(4096 a), DFT over the strided digits a, output twiddle w_n^(k_a l) s_c^l, rows left
// in in-place DIF order.  The coefficients are read once and stay in registers across the coset loop (re-reading them per coset
// measured the same time but 7x the fetch bytes).
#pragma once
#include "field_traits.hpp"
#include "ntt_passes.hpp"

namespace gbk {

// ------------------------------------------------------------------ tuning that differs per field
// WAVES_*: the minimum waves per SIMD of __launch_bounds__, 0 = none stated.
template <class F>
struct LdeTune;

template <>
struct LdeTune<GlF> {
    static constexpr u32 JW = 16;            // columns per tile from 2^20 rows up: 16 x 8 B = a 128-byte row segment
    static constexpr u32 PAD = 16;           // LDS slots [a0][j] padded by 16 words
    static constexpr bool TW_REGS = false;   // inter-stage twiddles read from a table at their use (keeps 30 VGPRs free)
    // pa16xs / pa16x2: 3 waves/SIMD (<= 168 VGPRs): the tile's 16 coefficients per thread stay in registers across the coset loop.
    // pa32: 32 coefficients + 32 working values per thread = two waves per SIMD.
    static constexpr int WAVES_PA16XS = 3, WAVES_PA16X2 = 3, WAVES_PA32 = 2;
    // The products of the 2^20..2^22-row passes keep round 3's five-mad form, mul_mont<true>: measured 3 % faster there than the
    // four-mad form of gl_field.hpp, which wins everywhere else - same box, tools/ab_kernel_times.sh, profiles/r04_ab_kernel_times.txt.
    static __device__ __forceinline__ u64 mulc_big(u64 x, u64 c_form) { return gl::mul_mont<true>(x, c_form); }
    static __device__ __forceinline__ u64 chain_big(u64 acc, u64 f) { return gl::mul_mont_lazy<true>(acc, f); }
};

template <>
struct LdeTune<BbF> {
    static constexpr u32 JW = 32;            // 32 x 4 B: a row segment is a full 128-byte line (16 x 4 B = 64 B segments left the
                                             // stores of v2's first cut at 0.8 TB/s)
    static constexpr u32 PAD = 0;            // 4-byte words, consecutive j -> consecutive banks
    static constexpr bool TW_REGS = true;    // inter-stage twiddles preloaded into registers (load_tw16): the same for every coset
    static constexpr int WAVES_PA16XS = 0, WAVES_PA16X2 = 0, WAVES_PA32 = 4;
    static __device__ __forceinline__ u32 mulc_big(u32 x, u32 c_form) { return bb::mul(x, c_form); }
    static __device__ __forceinline__ u32 chain_big(u32 acc, u32 f) { return bb::mul(acc, f); }
};

// 2^K-point register DFT on x[0 .. 2^K), K = 1..4: natural input order, X[k] in slot brevK(k)
template <class F, int K>
__device__ __forceinline__ void dft_pow2(typename F::T (&x)[16]) {
    if constexpr (K == 4) Dft<F>::template dft16<false>(x);
    else Dft<F>::template dft_small<false, K>(x);
}

// ------------------------------------------------------------------ LA = K in 1..4 (L = 12 + K)
// One radix-2^K stage over the 2^K rows, a thread per column l, no LDS.  grid = ncols * 16, block = 2^K rows x 256 contiguous columns.
template <class F, int K>
__global__ __launch_bounds__(THREADS) void k_lde_pa_small(const typename F::T* __restrict__ coeffs, typename F::T* __restrict__ lde,
                                                          u32 rate_bits, const typename F::T* __restrict__ tw_hi,
                                                          const typename F::T* __restrict__ tw_lo, const typename F::T* __restrict__ pow_lo,
                                                          const typename F::T* __restrict__ pow_hi) {
    typedef typename F::T T;
    constexpr u32 L = 12 + K, R = 1u << K;
    const size_t col = blockIdx.x >> 4;
    const u32 l = ((blockIdx.x & 15) << 8) + threadIdx.x;
    const size_t n = (size_t)1 << L;
    const T* cin = coeffs + col * n + l;
    T orig[R];
#pragma unroll
    for (u32 a = 0; a < R; a++) orig[a] = cin[(size_t)a << 12];
    const u32 ncosets = 1u << rate_bits;
    const T ratio = tw_split16<F>(tw_hi, tw_lo, l);  // w_n^l
    for (u32 c = 0; c < ncosets; c++) {
        const T* ph = pow_hi + ((size_t)c << K);
        T x[16];
#pragma unroll
        for (u32 a = 0; a < R; a++) x[a] = a ? F::mulc(orig[a], ph[a]) : orig[a];  // s_c^(4096 a)
        dft_pow2<F, K>(x);
        T* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        T f = pow_lo[(size_t)c * 4096 + l];  // s^l w_n^(k l), k = 0..R-1
#pragma unroll
        for (u32 k = 0; k < R; k++) {
            out[(size_t)brevk(k, K) << 12] = F::mulc(x[brevk(k, K)], f);
            if (k + 1 < R) f = F::mul_chain(f, ratio);
        }
    }
}

// ------------------------------------------------------------------ LA = 4 + K (L = 16 + K, K = 1..3): a = a1 2^K + a0
// grid = ncols * 2^(4+K); a block holds all 2^LA rows of 2^(8-K) consecutive columns l (row segments of 128 bytes and more):
// stage 1 (thread = (a0, jl), radix 16 over a1), LDS, stage 2 (radix 2^K over a0; a thread takes 2^(4-K) columns so that it still
// moves 16 values).
template <class F, int K>
__global__ __launch_bounds__(THREADS, LdeTune<F>::WAVES_PA16XS) void k_lde_pa16xs(
    const typename F::T* __restrict__ coeffs, typename F::T* __restrict__ lde, u32 rate_bits, const typename F::T* __restrict__ tw4096,
    const typename F::T* __restrict__ tw_hi, const typename F::T* __restrict__ tw_lo, const typename F::T* __restrict__ pow_lo,
    const typename F::T* __restrict__ pow_hi) {
    typedef typename F::T T;
    typedef LdeTune<F> U;
    constexpr u32 L = 16 + K, LA = 4 + K, R = 1u << K, M = 256u >> K, SLOT = 256 + U::PAD;  // M columns per block
    __shared__ T sh[16 * SLOT];                                                                // [k_a1 slot][a0][jl]
    const u32 blocks_per_col = 4096 / M;
    const size_t col = blockIdx.x / blocks_per_col;
    const u32 l0 = (blockIdx.x % blocks_per_col) * M;
    const u32 tid = threadIdx.x, a0 = tid / M, jl = tid % M;   // tid = a0 M + jl
    const size_t n = (size_t)1 << L;
    T orig[16];
    {
        const T* cin = coeffs + col * n + l0 + jl;
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) orig[a1] = cin[(size_t)((a1 << K) + a0) << 12];
    }
    const auto tw_at = [&](u32 s) { return tw4096[((brev4(s) * a0) << (12 - LA)) & 4095]; };  // inter-stage twiddle w_{2^LA}^(k_a1 a0)
    T tw[16];
    if constexpr (U::TW_REGS) {
#pragma unroll
        for (u32 s = 1; s < 16; s++) tw[s] = tw_at(s);
    }
    const u32 s2 = tid >> 4, q = tid & 15;  // stage-2 role: slot s2, columns q + 16 u (u < M / 16)
    const u32 ka1 = brev4(s2);
    const u32 ncosets = 1u << rate_bits;
    for (u32 c = 0; c < ncosets; c++) {
        const T* ph = pow_hi + ((size_t)c << LA) + a0;
        T x[16];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = ph[a1 << K];  // s_c^(4096 a)
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = F::mulc(orig[a1], x[a1]);
        Dft<F>::template dft16<false>(x);
#pragma unroll
        for (u32 s = 0; s < 16; s++) {
            if constexpr (U::TW_REGS) sh[s * SLOT + tid] = s ? F::mulc(x[s], tw[s]) : x[s];
            else sh[s * SLOT + tid] = (s && a0) ? F::mulc(x[s], tw_at(s)) : x[s];
        }
        __syncthreads();
#pragma unroll
        for (u32 u = 0; u < M / 16; u++) {
            const u32 jj = q + 16 * u, l = l0 + jj;
            T y[16];
#pragma unroll
            for (u32 b = 0; b < R; b++) y[b] = sh[s2 * SLOT + b * M + jj];
            Dft<F>::template dft_small<false, K>(y);
            // output twiddle s^l w_n^(k_a l), k_a = k_a1 + 16 k': a geometric progression in k' with ratio w_n^(16 l)
            T f = F::mul_chain(pow_lo[(size_t)c * 4096 + l], tw_split16<F>(tw_hi, tw_lo, ka1 * l));
            const T ratio = tw_split16<F>(tw_hi, tw_lo, 16 * l);
            T* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
#pragma unroll
            for (u32 k = 0; k < R; k++) {  // row position = brev_LA(k_a) = slot * 2^K + brevK(k')
                out[(size_t)(s2 * R + brevk(k, K)) << 12] = F::mulc(y[brevk(k, K)], f);
                if (k + 1 < R) f = F::mul_chain(f, ratio);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ LA = 8 (2^20 rows)
// Tile 256 rows (a = 16 a1 + a0) x JW columns.  grid = ncols * 4096 / JW, 16 * JW threads.  Two radix-16 stages over a.
template <class F>
__global__ __launch_bounds__(16 * LdeTune<F>::JW, LdeTune<F>::WAVES_PA16X2) void k_lde_pa16x2(
    const typename F::T* __restrict__ coeffs, typename F::T* __restrict__ lde, u32 L, u32 rate_bits,
    const typename F::T* __restrict__ tw4096, const typename F::T* __restrict__ tw_hi, const typename F::T* __restrict__ tw_lo,
    const typename F::T* __restrict__ pow_lo, const typename F::T* __restrict__ pow_hi) {
    typedef typename F::T T;
    typedef LdeTune<F> U;
    constexpr u32 JW = U::JW, ROW = 16 * JW + U::PAD, TPC = 4096 / JW;  // ROW: one k_a1 slot [a0][j]; TPC tiles per column
    static_assert(U::TW_REGS || 16 * JW == 256, "tw256 is filled by one store per thread");
    __shared__ T sh[16 * ROW];
    __shared__ T tw256[256];  // w_256^m: the stage-1 twiddles where they are read from LDS at their use (!TW_REGS)
    const size_t col = blockIdx.x / TPC;
    const u32 tg = blockIdx.x % TPC;
    const u32 tid = threadIdx.x, hi4 = tid / JW, j = tid % JW;
    const u32 l = tg * JW + j;
    const size_t n = (size_t)1 << L;
    const T* cin = coeffs + col * n + l;
    if constexpr (!U::TW_REGS) tw256[tid] = tw4096[tid * 16];
    T orig[16];
#pragma unroll
    for (u32 a1 = 0; a1 < 16; a1++) orig[a1] = cin[(size_t)(a1 * 16 + hi4) << 12];  // stage-1 thread = (a0 = hi4, j)
    if constexpr (!U::TW_REGS) __syncthreads();  // tw256 visible
    const T ratio = tw_split16<F>(tw_hi, tw_lo, 16 * l);
    const T f0 = tw_split16<F>(tw_hi, tw_lo, brev4(hi4) * l);  // w_n^(k_a1 l)
    T tw[16];
    if constexpr (U::TW_REGS) load_tw16<F>(tw, tw4096, hi4 * 16);  // w_256^(k_a1 a0): the same for every coset
    for (u32 c = 0; c < (1u << rate_bits); c++) {
        const T* ph = pow_hi + (size_t)c * 256 + hi4;
        T x[16];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = ph[a1 * 16];  // s_c^(4096 a): 16 independent loads (entry 0 is 1)
        const T sl = pow_lo[(size_t)c * 4096 + l];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = U::mulc_big(orig[a1], x[a1]);
        Dft<F>::template dft16<false>(x);
#pragma unroll
        for (u32 s = 0; s < 16; s++) {  // w_256^(k_a1 a0); [k_a1 slot][a0][j]
            if constexpr (U::TW_REGS) sh[s * ROW + tid] = s ? U::mulc_big(x[s], tw[s]) : x[s];
            else sh[s * ROW + tid] = s ? U::mulc_big(x[s], tw256[(brev4(s) * hi4) & 255]) : x[s];
        }
        __syncthreads();
        // stage 2 thread = (k_a1 slot = hi4, j): digit a0
#pragma unroll
        for (u32 a0 = 0; a0 < 16; a0++) x[a0] = sh[hi4 * ROW + a0 * JW + j];
        Dft<F>::template dft16<false>(x);
        T* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        // output twiddle s^l w_n^(k_a l), k_a = k_a1 + 16 k': a geometric progression in k' with ratio w_n^(16 l)
        T f = U::chain_big(sl, f0);
#pragma unroll
        for (u32 k = 0; k < 16; k++) {  // k' = k: slot brev4(k), row position = brev8(k_a)
            out[(size_t)(hi4 * 16 + brev4(k)) << 12] = U::mulc_big(x[brev4(k)], f);
            if (k < 15) f = U::chain_big(f, ratio);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ LA = 8 + K, K = 1, 2 (2^21 and 2^22 rows, round 6)
// (Round 5 ran a de-interleave pass and a combine pass around the 2^20-row kernels.)  The (256 R)-point strided DFT over a' as TWO
// stages with 32 points per thread - 32 x 16 at 2^21 rows (16 a0 x JW columns: radix 32 over a1, then two radix-16 DFTs over a0 per
// thread), 32 x 32 at 2^22 rows.  Goldilocks: every root of unity of order <= 64 is a shift, so the radix-32 DFT costs one butterfly
// layer more and NO general multiplication more: the multiplications per output are those of the 2^20-row pass (scale, inter-stage
// twiddle, output twiddle and its chain); BabyBear adds the fifteen constant twiddles of the extra butterfly layer per 32 points.
// The price is registers - 32 coefficients + 32 working values per thread - and, for Goldilocks, a tile of 64 / 128 KB of LDS:
// 1.20x / 1.39x the 2^20-row pass per element (1.24x / 1.47x before the coset factors s_c^(4096 a') went through LDS one coset
// ahead: the threads of a row share them).
// (The alternative measured on the same box, profiles/r06_large_sizes.txt: 16 points per thread, four waves per SIMD, a radix-R stage
// over the top digit as a butterfly ACROSS LANES - v_permlane16/32_swap - and one general twiddle more per output: 1.27x / 1.58x for
// Goldilocks, its instruction count.  BabyBear's 2^22-row pass is that form, kernels_bb16.hip's k_bb_lde_pa16x2w: its words are half
// as wide, 13.0 against 14.8 ms per 167 columns - the other three (field, size) pairs go the other way.)
// Instantiated for what is launched: K = 1 in both fields, K = 2 for Goldilocks.
template <class F, int K>
__global__ __launch_bounds__((8 << K) * LdeTune<F>::JW, LdeTune<F>::WAVES_PA32) void k_lde_pa32(
    const typename F::T* __restrict__ coeffs, typename F::T* __restrict__ lde, u32 rate_bits, const typename F::T* __restrict__ tw4096,
    const typename F::T* __restrict__ tw_hi, const typename F::T* __restrict__ tw_lo, const typename F::T* __restrict__ pow_lo,
    const typename F::T* __restrict__ pow_hi) {
    typedef typename F::T T;
    typedef LdeTune<F> U;
    constexpr u32 L = 20 + K, A0 = 8u << K /* values of a0: 16 / 32 */, JW = U::JW, NT = A0 * JW, SLOT = NT + U::PAD, ROWS = 256u << K,
                  TPC = 4096 / JW;
    __shared__ T sh[32 * SLOT];      // [k_a1 slot][a0][j]
    __shared__ T twl[ROWS];          // w_ROWS^m: the inter-stage twiddles
    __shared__ T phs[2][ROWS];       // s_c^(4096 a') of this coset and of the next: the JW threads of a row share them, so the
                                     // workgroup loads each once (ROWS / NT per thread, one coset ahead) instead of 32 per thread
    const size_t col = blockIdx.x / TPC;
    const u32 tg = blockIdx.x % TPC;
    const u32 tid = threadIdx.x, hi = tid / JW, j = tid % JW;   // stage 1: a0 = hi; stage 2: slot(s) from hi
    const u32 l = tg * JW + j;
    const size_t n = (size_t)1 << L;
    const T* cin = coeffs + col * n + l;
    for (u32 i = tid; i < ROWS; i += NT) {
        twl[i] = tw4096[i << (4 - K)];
        phs[0][i] = pow_hi[i];
    }
    T orig[32];
#pragma unroll
    for (u32 a1 = 0; a1 < 32; a1++) orig[a1] = cin[(size_t)(a1 * A0 + hi) << 12];
    __syncthreads();  // twl, phs[0] visible
    const T ratio = tw_split16<F>(tw_hi, tw_lo, 32 * l);   // w_n^(32 l)
    const u32 ncosets = 1u << rate_bits;
    T sl_next = pow_lo[l];
    for (u32 c = 0; c < ncosets; c++) {
        const T sl = sl_next;
        T nph[ROWS / NT];                                    // the next coset's factors, in flight across this coset's work
        if (c + 1 < ncosets) {
#pragma unroll
            for (u32 k = 0; k < ROWS / NT; k++) nph[k] = pow_hi[(size_t)(c + 1) * ROWS + tid + k * NT];
            sl_next = pow_lo[(size_t)(c + 1) * 4096 + l];
        }
        const T* ph = phs[c & 1] + hi;
        T x[32];
#pragma unroll
        for (u32 a1 = 0; a1 < 32; a1++) x[a1] = U::mulc_big(orig[a1], ph[a1 * A0]);  // s_c^(4096 a'), a' = a1 A0 + a0
        Dft<F>::template dft32<false>(x);
#pragma unroll
        for (u32 s = 0; s < 32; s++) sh[s * SLOT + tid] = s ? U::mulc_big(x[s], twl[(brevk(s, 5) * hi) & (ROWS - 1)]) : x[s];  // w_ROWS^(k_a1 a0)
        __syncthreads();
        T* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        if constexpr (K == 2) {   // stage 2 thread = (k_a1 slot = hi, j): radix 32 over a0
#pragma unroll
            for (u32 a0 = 0; a0 < 32; a0++) x[a0] = sh[hi * SLOT + a0 * JW + j];
            Dft<F>::template dft32<false>(x);
            T f = U::chain_big(sl, tw_split16<F>(tw_hi, tw_lo, brevk(hi, 5) * l));   // s^l w_n^(k_a1 l)
#pragma unroll
            for (u32 k = 0; k < 32; k++) {  // k_a' = k_a1 + 32 k: row position brev10(k_a') = hi * 32 + brev5(k)
                out[(size_t)(hi * 32 + brevk(k, 5)) << 12] = U::mulc_big(x[brevk(k, 5)], f);
                if (k < 31) f = U::chain_big(f, ratio);
            }
        } else {                  // stage 2 thread = (k_a1 slots hi and hi + 16, j): two radix-16 DFTs over a0
#pragma unroll
            for (u32 u = 0; u < 2; u++) {
                const u32 slot = hi + 16 * u;
                T y[16];
#pragma unroll
                for (u32 a0 = 0; a0 < 16; a0++) y[a0] = sh[slot * SLOT + a0 * JW + j];
                Dft<F>::template dft16<false>(y);
                T f = U::chain_big(sl, tw_split16<F>(tw_hi, tw_lo, brevk(slot, 5) * l));
#pragma unroll
                for (u32 k = 0; k < 16; k++) {  // row position brev9(k_a1 + 32 k) = slot * 16 + brev4(k)
                    out[(size_t)(slot * 16 + brev4(k)) << 12] = U::mulc_big(y[brev4(k)], f);
                    if (k < 15) f = U::chain_big(f, ratio);
                }
            }
        }
        if (c + 1 < ncosets) {
#pragma unroll
            for (u32 k = 0; k < ROWS / NT; k++) phs[(c + 1) & 1][tid + k * NT] = nph[k];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ launcher (called from ntt_passes.hpp's lde_columns<F>)
// The tables the strided passes read: Goldilocks' Montgomery-form twins (all of the passes' general multiplications have a table
// value as one factor, gl::mul_mont), BabyBear's plain tables (Montgomery words already)
template <class F>
struct LdeTables {
    const typename F::T *tw4096, *tw_hi, *tw_lo, *pow_lo, *pow_hi;
};
inline LdeTables<GlF> lde_tables(const GlNttTables& t, const GlCosetTables& ct) {
    return {t.tw4096_fwd_m, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m};
}
inline LdeTables<BbF> lde_tables(const BbNttTables& t, const BbCosetTables& ct) {
    return {t.tw4096_fwd, t.tw_hi_fwd, t.tw_lo_fwd, ct.pow_lo, ct.pow_hi};
}

// per field (kernels_ntt16.hip, kernels_bb16.hip): the strided pass of 2^22 rows - Goldilocks' k_lde_pa32<GlF, 2>, BabyBear's
// cross-lane k_bb_lde_pa16x2w
void lde_pa_rows22(const u64* coeffs, u64* lde, size_t ncols, const GlNttTables& t, const GlCosetTables& ct, hipStream_t stream);
void lde_pa_rows22(const u32* coeffs, u32* lde, size_t ncols, const BbNttTables& t, const BbCosetTables& ct, hipStream_t stream);

template <class F>
void lde_pa_r16(const typename F::T* coeffs, typename F::T* lde, size_t ncols, const NttTables<F>& t, const CosetTables<F>& ct,
                hipStream_t stream) {
    constexpr u32 JW = LdeTune<F>::JW;
    const LdeTables<F> tt = lde_tables(t, ct);
    const u32 r = ct.rate_bits;
    const dim3 tiles((u32)(ncols * (4096 / JW))), tile_threads(16 * JW);   // 2^20 rows and more: tiles of JW columns
#define GB_PA_SMALL(KK)                                                                                                     \
    hipLaunchKernelGGL((k_lde_pa_small<F, KK>), dim3((u32)(ncols << 4)), dim3(THREADS), 0, stream, coeffs, lde, r, tt.tw_hi, \
                       tt.tw_lo, tt.pow_lo, tt.pow_hi)
#define GB_PAS(KK)                                                                                                          \
    hipLaunchKernelGGL((k_lde_pa16xs<F, KK>), dim3((u32)(ncols << (4 + KK))), dim3(THREADS), 0, stream, coeffs, lde, r, tt.tw4096, \
                       tt.tw_hi, tt.tw_lo, tt.pow_lo, tt.pow_hi)
    switch (t.log_n) {
        case 13: GB_PA_SMALL(1); break;
        case 14: GB_PA_SMALL(2); break;
        case 15: GB_PA_SMALL(3); break;
        case 16: GB_PA_SMALL(4); break;
        case 17: GB_PAS(1); break;
        case 18: GB_PAS(2); break;
        case 19: GB_PAS(3); break;
        case 20:
            hipLaunchKernelGGL(k_lde_pa16x2<F>, tiles, tile_threads, 0, stream, coeffs, lde, t.log_n, r, tt.tw4096, tt.tw_hi, tt.tw_lo,
                               tt.pow_lo, tt.pow_hi);
            break;
        case 21:
            hipLaunchKernelGGL((k_lde_pa32<F, 1>), tiles, tile_threads, 0, stream, coeffs, lde, r, tt.tw4096, tt.tw_hi, tt.tw_lo,
                               tt.pow_lo, tt.pow_hi);
            break;
        case 22: lde_pa_rows22(coeffs, lde, ncols, t, ct, stream); break;
    }
#undef GB_PA_SMALL
#undef GB_PAS
}

}  // namespace gbk

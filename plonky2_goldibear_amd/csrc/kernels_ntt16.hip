// Goldilocks NTT passes, v2: radix-16 butterflies held in registers (gfx950).
//
// Why: tools/microbench_valu.hip shows the NTT is bound by integer VALU issue, not by HBM or LDS
// (a 64-bit mod-mul is ~17-26 VALU ops at ~4.2 cycles each).  The reference's generator makes every
// root of unity of order <= 64 a power of two (w_64 = 2^39, w_16 = 2^156 = -2^60, w_4 = 2^48; 2^96 = -1),
// so a 16-point DFT needs no general multiplication: its 17 non-trivial twiddles are shifts + one fold.
// A thread keeps 16 points in registers for four layers; general twiddles (tables) appear only between
// radix-16 stages, and LDS is touched once per stage instead of once per layer.
//
// Pass structure and dispatch: ntt_passes.hpp, shared with BabyBear.  What is Goldilocks' own: the register DFTs (Dft<GlF>, dft_gl.hpp) and
// the LDE's radix-16 passes - PA (1..10 bits strided, per-coset loop), PB (12 bits contiguous, natural -> leaf order).
#include "kernels.hpp"
#include "gl_field.hpp"
#include "ntt_passes.hpp"
#include "dft_gl.hpp"

namespace gbk {

// ------------------------------------------------------------------ LDE pass B: 4096 contiguous points, 3 radix-16 stages
// grid = number of 4096-tiles of `lde` (in place).  natural -> bit-reversed.
// The inter-stage twiddles cost as much as the butterflies here (ablations in DESIGN.md: without their loads and products the pass
// runs 33 % faster, close to a plain copy): the first stage reads them from a copy of the table laid out [slot][tid] (coalesced),
// the second from a 256-entry table in LDS.
__global__ __launch_bounds__(THREADS) void k_gl_lde_pb16(u64* __restrict__ lde, const u64* __restrict__ tw4096) {
    __shared__ u64 sh[16 * 272];
    __shared__ u64 tw2[256];  // the stage-2 twiddles as the threads read them: tw2[s][d0] = w_256^(brev4(s) d0) - consecutive lanes,
                              // consecutive words (indexed by exponent, slots with brev4(s) = 4, 8, 12 were 2- and 4-way bank conflicts)
    u64* p = lde + ((size_t)blockIdx.x << 12);
    const u32 tid = threadIdx.x;
    tw2[tid] = tw4096[((brev4(tid >> 4) * (tid & 15)) & 255) * 16];
    u64 x[16];
    // stage 1: digit d2 (stride 256); this thread is (d1, d0) = tid
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = p[d * 256 + tid];
    u64 tw[16];
#pragma unroll
    for (u32 s = 1; s < 16; s++) tw[s] = tw4096[4096 + s * 256 + tid];  // w_4096^(k2 (16 d1 + d0)), k2 = brev4(s)
    dft16<false>(x);
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[s * 272 + tid] = s ? gl::mul_mont(x[s], tw[s]) : x[s];
    __syncthreads();
    // stage 2: digit d1; this thread is (k2 slot, d0)
    const u32 hi4 = tid >> 4, lo4 = tid & 15;
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = sh[hi4 * 272 + d * 16 + lo4];
    dft16<false>(x);
    __syncthreads();
#pragma unroll
    for (u32 s = 0; s < 16; s++)   // w_256^(k1 d0) from LDS; [k2 slot][d0][k1 slot], rows padded to 17
        sh[hi4 * 272 + lo4 * 17 + s] = s ? gl::mul_mont(x[s], tw2[s * 16 + lo4]) : x[s];
    __syncthreads();
    // stage 3: digit d0; this thread is (k2 slot, k1 slot)
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = sh[hi4 * 272 + d * 17 + lo4];
    dft16<false>(x);
    __syncthreads();
    // x[s] belongs at tile position tid * 16 + s: transpose through LDS for a coalesced store
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[tid * 17 + s] = x[s];
    __syncthreads();
#pragma unroll
    for (u32 it = 0; it < 16; it++) {
        const u32 q = it * 256 + tid;
        p[q] = sh[(q >> 4) * 17 + (q & 15)];
    }
}

// ------------------------------------------------------------------ LDE pass A
// LA = 8: grid = ncols * 256, tile 256 rows (a = 16 a1 + a0) x 16 columns.  Per coset: scale by s^(4096 a),
// two radix-16 stages over a, twiddle w_n^(k_a l) s^l, in-place DIF row order.
// (Its products keep round 3's five-mad form, mul_mont<true>: measured 3 % faster here than the four-mad form of gl_field.hpp, which
// wins everywhere else - same box, tools/ab_kernel_times.sh, profiles/r04_ab_kernel_times.txt.)
// 3 waves/SIMD (<= 168 VGPRs, no spills): the tile's 16 coefficients per thread stay in registers across the coset
// loop, so the coefficients cross HBM once (re-reading them per coset measured the same time but 7x the fetch bytes).
__global__ __launch_bounds__(THREADS, 3) void k_gl_lde_pa16x2(const u64* __restrict__ coeffs, u64* __restrict__ lde, u32 L, u32 rate_bits,
                                                           const u64* __restrict__ tw4096, const u64* __restrict__ tw_hi,
                                                           const u64* __restrict__ tw_lo, const u64* __restrict__ pow_lo,
                                                           const u64* __restrict__ pow_hi) {
    __shared__ u64 sh[16 * 272];
    __shared__ u64 tw256[256];  // w_256^m: the stage-1 twiddles, read from LDS at their use (keeps 30 VGPRs free)
    const size_t col = blockIdx.x >> 8;
    const u32 tg = blockIdx.x & 255;
    const u32 tid = threadIdx.x, hi4 = tid >> 4, j = tid & 15;
    const u32 l = (tg << 4) + j;
    const size_t n = (size_t)1 << L;
    const u64* cin = coeffs + col * n + l;
    tw256[tid] = tw4096[tid * 16];
    u64 orig[16];
#pragma unroll
    for (u32 a1 = 0; a1 < 16; a1++) orig[a1] = cin[(size_t)(a1 * 16 + hi4) << 12];  // stage-1 thread = (a0 = hi4, j)
    __syncthreads();  // tw256 visible
    const u64 ratio = tw_split16<GlF>(tw_hi, tw_lo, 16 * l);
    const u64 f0 = tw_split16<GlF>(tw_hi, tw_lo, brev4(hi4) * l);  // w_n^(k_a1 l)
    for (u32 c = 0; c < (1u << rate_bits); c++) {
        const u64* ph = pow_hi + (size_t)c * 256 + hi4;
        u64 x[16];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = ph[a1 * 16];  // s_c^(4096 a): 16 independent loads (entry 0 is 1)
        const u64 sl = pow_lo[(size_t)c * 4096 + l];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = gl::mul_mont<true>(orig[a1], x[a1]);
        dft16<false>(x);
#pragma unroll
        for (u32 s = 0; s < 16; s++) sh[s * 272 + tid] = s ? gl::mul_mont<true>(x[s], tw256[(brev4(s) * hi4) & 255]) : x[s];  // w_256^(k_a1 a0); [k_a1 slot][a0][j]
        __syncthreads();
        // stage 2 thread = (k_a1 slot = hi4, j): digit a0
#pragma unroll
        for (u32 a0 = 0; a0 < 16; a0++) x[a0] = sh[hi4 * 272 + a0 * 16 + j];
        dft16<false>(x);
        u64* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        // output twiddle s^l w_n^(k_a l), k_a = k_a1 + 16 k': a geometric progression in k' with ratio w_n^(16 l)
        u64 f = gl::mul_mont_lazy<true>(sl, f0);
#pragma unroll
        for (u32 k = 0; k < 16; k++) {  // k' = k: slot brev4(k), row position = brev8(k_a)
            out[(size_t)(hi4 * 16 + brev4(k)) << 12] = gl::mul_mont<true>(x[brev4(k)], f);
            if (k < 15) f = gl::mul_mont_lazy<true>(f, ratio);
        }
        __syncthreads();
    }
}

// LA = 8 + K, K = 1, 2 (2^21 and 2^22 rows, round 6; round 5 ran a de-interleave pass and a combine pass around the 2^20-row kernels):
// the (256 R)-point strided DFT over a' as TWO stages with 32 points per thread - 32 x 16 at 2^21 rows (256 threads: radix 32 over a1,
// then two radix-16 DFTs over a0 per thread), 32 x 32 at 2^22 rows (512 threads).  Every root of unity of order <= 64 is a shift, so
// the radix-32 DFT costs one butterfly layer more and NO general multiplication more: the multiplications per output are those of
// the 2^20-row pass (scale, inter-stage twiddle, output twiddle and its chain).  The price is registers - 32 coefficients + 32
// working values per thread = two waves per SIMD - and a tile of 64 / 128 KB of LDS: 1.20x / 1.39x the 2^20-row pass per element
// (1.24x / 1.47x before the coset factors s_c^(4096 a') went through LDS one coset ahead: the sixteen threads of a row share them).
// (The alternative measured on the same box, profiles/r06_large_sizes.txt: 16 points per thread, four waves per SIMD, a radix-R stage
// over the top digit as a butterfly ACROSS LANES - v_permlane16/32_swap - and one general twiddle more per output: 1.27x / 1.58x,
// its instruction count.  BabyBear's 2^22-row pass is that form, kernels_bb16.hip: its words are half as wide.)
template <int K>
__global__ __launch_bounds__(128 << K, 2) void k_gl_lde_pa32(const u64* __restrict__ coeffs, u64* __restrict__ lde, u32 rate_bits,
                                                             const u64* __restrict__ tw4096, const u64* __restrict__ tw_hi,
                                                             const u64* __restrict__ tw_lo, const u64* __restrict__ pow_lo,
                                                             const u64* __restrict__ pow_hi) {
    constexpr u32 L = 20 + K, A0 = 8u << K /* values of a0: 16 / 32 */, NT = 128u << K, SLOT = NT + 16, ROWS = 256u << K;
    __shared__ u64 sh[32 * SLOT];      // [k_a1 slot][a0][j], slots padded by 16 words
    __shared__ u64 twl[ROWS];          // w_ROWS^m: the inter-stage twiddles
    __shared__ u64 phs[2][ROWS];       // s_c^(4096 a') of this coset and of the next: the 16 threads of a row share them, so the
                                       // workgroup loads each once (two per thread, one coset ahead) instead of 32 per thread
    const size_t col = blockIdx.x >> 8;
    const u32 tg = blockIdx.x & 255;
    const u32 tid = threadIdx.x, hi = tid >> 4, j = tid & 15;   // stage 1: a0 = hi; stage 2: slot(s) from hi
    const u32 l = (tg << 4) + j;
    const size_t n = (size_t)1 << L;
    const u64* cin = coeffs + col * n + l;
    for (u32 i = tid; i < ROWS; i += NT) {
        twl[i] = tw4096[i << (4 - K)];
        phs[0][i] = pow_hi[i];
    }
    u64 orig[32];
#pragma unroll
    for (u32 a1 = 0; a1 < 32; a1++) orig[a1] = cin[(size_t)(a1 * A0 + hi) << 12];
    __syncthreads();  // twl, phs[0] visible
    const u64 ratio = tw_split16<GlF>(tw_hi, tw_lo, 32 * l);   // w_n^(32 l)
    const u32 ncosets = 1u << rate_bits;
    u64 sl_next = pow_lo[l];
    for (u32 c = 0; c < ncosets; c++) {
        const u64 sl = sl_next;
        u64 nph[ROWS / NT];                                  // the next coset's factors, in flight across this coset's work
        if (c + 1 < ncosets) {
#pragma unroll
            for (u32 k = 0; k < ROWS / NT; k++) nph[k] = pow_hi[(size_t)(c + 1) * ROWS + tid + k * NT];
            sl_next = pow_lo[(size_t)(c + 1) * 4096 + l];
        }
        const u64* ph = phs[c & 1] + hi;
        u64 x[32];
#pragma unroll
        for (u32 a1 = 0; a1 < 32; a1++) x[a1] = ph[a1 * A0];  // s_c^(4096 a'), a' = a1 A0 + a0
#pragma unroll
        for (u32 a1 = 0; a1 < 32; a1++) x[a1] = gl::mul_mont<true>(orig[a1], x[a1]);
        dft32<false>(x);
#pragma unroll
        for (u32 s = 0; s < 32; s++) sh[s * SLOT + tid] = s ? gl::mul_mont<true>(x[s], twl[(brevk(s, 5) * hi) & (ROWS - 1)]) : x[s];  // w_ROWS^(k_a1 a0)
        __syncthreads();
        u64* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        if constexpr (K == 2) {   // stage 2 thread = (k_a1 slot = hi, j): radix 32 over a0
#pragma unroll
            for (u32 a0 = 0; a0 < 32; a0++) x[a0] = sh[hi * SLOT + a0 * 16 + j];
            dft32<false>(x);
            u64 f = gl::mul_mont_lazy<true>(sl, tw_split16<GlF>(tw_hi, tw_lo, brevk(hi, 5) * l));   // s^l w_n^(k_a1 l)
#pragma unroll
            for (u32 k = 0; k < 32; k++) {  // k_a' = k_a1 + 32 k: row position brev10(k_a') = hi * 32 + brev5(k)
                out[(size_t)(hi * 32 + brevk(k, 5)) << 12] = gl::mul_mont<true>(x[brevk(k, 5)], f);
                if (k < 31) f = gl::mul_mont_lazy<true>(f, ratio);
            }
        } else {                  // stage 2 thread = (k_a1 slots hi and hi + 16, j): two radix-16 DFTs over a0
#pragma unroll
            for (u32 u = 0; u < 2; u++) {
                const u32 slot = hi + 16 * u;
                u64 y[16];
#pragma unroll
                for (u32 a0 = 0; a0 < 16; a0++) y[a0] = sh[slot * SLOT + a0 * 16 + j];
                dft16<false>(y);
                u64 f = gl::mul_mont_lazy<true>(sl, tw_split16<GlF>(tw_hi, tw_lo, brevk(slot, 5) * l));
#pragma unroll
                for (u32 k = 0; k < 16; k++) {  // row position brev9(k_a1 + 32 k) = slot * 16 + brev4(k)
                    out[(size_t)(slot * 16 + brev4(k)) << 12] = gl::mul_mont<true>(y[brev4(k)], f);
                    if (k < 15) f = gl::mul_mont_lazy<true>(f, ratio);
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

// LA = 4 + K (L = 16 + K, K = 1..3): a = a1 2^K + a0.  grid = ncols * 2^(4+K); a block holds all 2^LA rows of 2^(8-K) consecutive
// columns l: stage 1 (thread = (a0, jl), radix 16 over a1), LDS, stage 2 (radix 2^K over a0; a thread takes 2^(4-K) columns so
// that it still moves 16 values).  Same conventions as k_gl_lde_pa16x2: coefficients read once, kept across the coset loop.
template <int K>
__global__ __launch_bounds__(THREADS, 3) void k_gl_lde_pa16xs(const u64* __restrict__ coeffs, u64* __restrict__ lde, u32 rate_bits,
                                                              const u64* __restrict__ tw4096, const u64* __restrict__ tw_hi,
                                                              const u64* __restrict__ tw_lo, const u64* __restrict__ pow_lo,
                                                              const u64* __restrict__ pow_hi) {
    constexpr u32 L = 16 + K, LA = 4 + K, R = 1u << K, M = 256u >> K;  // M columns per block
    __shared__ u64 sh[16 * (256 + 16)];                                  // [k_a1 slot][a0][jl], slots padded by 16 words
    const u32 blocks_per_col = 4096 / M;
    const size_t col = blockIdx.x / blocks_per_col;
    const u32 l0 = (blockIdx.x % blocks_per_col) * M;
    const u32 tid = threadIdx.x, a0 = tid / M, jl = tid % M;
    const size_t n = (size_t)1 << L;
    u64 orig[16];
    {
        const u64* cin = coeffs + col * n + l0 + jl;
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) orig[a1] = cin[(size_t)((a1 << K) + a0) << 12];
    }
    // stage-2 role: slot s2 = tid >> 4, columns q + 16 u (u < M / 16)
    const u32 s2 = tid >> 4, q = tid & 15;
    const u32 ka1 = brev4(s2);
    const u32 ncosets = 1u << rate_bits;
    for (u32 c = 0; c < ncosets; c++) {
        const u64* ph = pow_hi + ((size_t)c << LA) + a0;
        u64 x[16];
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = ph[a1 << K];  // s_c^(4096 a)
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) x[a1] = gl::mul_mont(orig[a1], x[a1]);
        dft16<false>(x);
#pragma unroll
        for (u32 s = 0; s < 16; s++)  // inter-stage twiddle w_{2^LA}^(k_a1 a0)
            sh[s * 272 + a0 * M + jl] = (s && a0) ? gl::mul_mont(x[s], tw4096[((brev4(s) * a0) << (12 - LA)) & 4095]) : x[s];
        __syncthreads();
#pragma unroll
        for (u32 u = 0; u < M / 16; u++) {
            const u32 jj = q + 16 * u, l = l0 + jj;
            u64 y[16];
#pragma unroll
            for (u32 b = 0; b < R; b++) y[b] = sh[s2 * 272 + b * M + jj];
            dft_small<false, K>(y);
            // output twiddle s^l w_n^(k_a l), k_a = k_a1 + 16 k': a geometric progression in k' with ratio w_n^(16 l)
            u64 f = gl::mul_mont_lazy(pow_lo[(size_t)c * 4096 + l], tw_split16<GlF>(tw_hi, tw_lo, ka1 * l));
            const u64 ratio = tw_split16<GlF>(tw_hi, tw_lo, 16 * l);
            u64* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
#pragma unroll
            for (u32 k = 0; k < R; k++) {  // row position = brev_LA(k_a) = slot * 2^K + brevK(k')
                out[(size_t)(s2 * R + brevk(k, K)) << 12] = gl::mul_mont(y[brevk(k, K)], f);
                if (k + 1 < R) f = gl::mul_mont_lazy(f, ratio);
            }
        }
        __syncthreads();
    }
}

// LA = K in 1..3 (L = 12 + K): one radix-2^K stage over the 2^K rows, a thread per column l, no LDS.  grid = ncols * 16.
template <int K>
__global__ __launch_bounds__(THREADS) void k_gl_lde_pa_small(const u64* __restrict__ coeffs, u64* __restrict__ lde, u32 rate_bits,
                                                             const u64* __restrict__ tw_hi, const u64* __restrict__ tw_lo,
                                                             const u64* __restrict__ pow_lo, const u64* __restrict__ pow_hi) {
    constexpr u32 L = 12 + K, R = 1u << K;
    const size_t col = blockIdx.x >> 4;
    const u32 l = ((blockIdx.x & 15) << 8) + threadIdx.x;
    const size_t n = (size_t)1 << L;
    const u64* cin = coeffs + col * n + l;
    u64 orig[R];
#pragma unroll
    for (u32 a = 0; a < R; a++) orig[a] = cin[(size_t)a << 12];
    const u32 ncosets = 1u << rate_bits;
    const u64 ratio = tw_split16<GlF>(tw_hi, tw_lo, l);  // w_n^l
    for (u32 c = 0; c < ncosets; c++) {
        const u64* ph = pow_hi + ((size_t)c << K);
        u64 x[16];
#pragma unroll
        for (u32 a = 0; a < R; a++) x[a] = a ? gl::mul_mont(orig[a], ph[a]) : orig[a];  // s_c^(4096 a)
        dft_small<false, K>(x);
        u64* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        u64 f = pow_lo[(size_t)c * 4096 + l];  // s^l w_n^(k l), k = 0..R-1
#pragma unroll
        for (u32 k = 0; k < R; k++) {
            out[(size_t)brevk(k, K) << 12] = gl::mul_mont(x[brevk(k, K)], f);
            if (k + 1 < R) f = gl::mul_mont_lazy(f, ratio);
        }
    }
}

// LA = 4 (L = 16): grid = ncols * 16, block = 16 rows x 256 contiguous columns, one radix-16 stage, no LDS.
__global__ __launch_bounds__(THREADS) void k_gl_lde_pa16x1(const u64* __restrict__ coeffs, u64* __restrict__ lde, u32 rate_bits,
                                                           const u64* __restrict__ tw_hi, const u64* __restrict__ tw_lo,
                                                           const u64* __restrict__ pow_lo, const u64* __restrict__ pow_hi) {
    constexpr u32 L = 16;
    const size_t col = blockIdx.x >> 4;
    const u32 l = ((blockIdx.x & 15) << 8) + threadIdx.x;
    const size_t n = (size_t)1 << L;
    const u64* cin = coeffs + col * n + l;
    u64 orig[16];
#pragma unroll
    for (u32 a = 0; a < 16; a++) orig[a] = cin[(size_t)a << 12];
    const u32 ncosets = 1u << rate_bits;
    const u64 ratio = tw_split16<GlF>(tw_hi, tw_lo, l);
    for (u32 c = 0; c < ncosets; c++) {
        const u64* ph = pow_hi + (size_t)c * 16;
        u64 x[16];
#pragma unroll
        for (u32 a = 0; a < 16; a++) x[a] = a ? gl::mul_mont(orig[a], ph[a]) : orig[a];
        dft16<false>(x);
        u64* out = lde + (col << (L + rate_bits)) + (size_t)c * n + l;
        u64 f = pow_lo[(size_t)c * 4096 + l];  // s^l w_n^(k l), k = 0..15
#pragma unroll
        for (u32 k = 0; k < 16; k++) {
            out[(size_t)brev4(k) << 12] = gl::mul_mont(x[brev4(k)], f);
            if (k < 15) f = gl::mul_mont_lazy(f, ratio);
        }
    }
}

// ------------------------------------------------------------------ launchers (called from ntt_passes.hpp's lde_columns<GlF>)
// Every kernel of this file takes the MONTGOMERY-form copies of the tables (GlNttTables::*_m, GlCosetTables::*_m): all of their
// general multiplications have a table value as one factor (gl::mul_mont).

void lde_pa_r16(const u64* coeffs, u64* lde, size_t ncols, const GlNttTables& t, const GlCosetTables& ct, hipStream_t stream) {
    const u32 L = t.log_n;
    if (L == 20) {
        hipLaunchKernelGGL(k_gl_lde_pa16x2, dim3((u32)(ncols << 8)), dim3(THREADS), 0, stream, coeffs, lde, L, ct.rate_bits,
                           t.tw4096_fwd_m, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        return;
    }
    if (L == 21 || L == 22) {
        if (L == 21)
            hipLaunchKernelGGL(k_gl_lde_pa32<1>, dim3((u32)(ncols << 8)), dim3(256), 0, stream, coeffs, lde, ct.rate_bits, t.tw4096_fwd_m,
                               t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        else
            hipLaunchKernelGGL(k_gl_lde_pa32<2>, dim3((u32)(ncols << 8)), dim3(512), 0, stream, coeffs, lde, ct.rate_bits, t.tw4096_fwd_m,
                               t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        return;
    }
#define GB_PAS(KK)                                                                                                        \
    hipLaunchKernelGGL(k_gl_lde_pa16xs<KK>, dim3((u32)(ncols << (4 + KK))), dim3(THREADS), 0, stream, coeffs, lde, ct.rate_bits, \
                       t.tw4096_fwd_m, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m)
    if (L >= 13 && L <= 15) {
        const dim3 grid((u32)(ncols << 4));
        if (L == 13) hipLaunchKernelGGL(k_gl_lde_pa_small<1>, grid, dim3(THREADS), 0, stream, coeffs, lde, ct.rate_bits, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        if (L == 14) hipLaunchKernelGGL(k_gl_lde_pa_small<2>, grid, dim3(THREADS), 0, stream, coeffs, lde, ct.rate_bits, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        if (L == 15) hipLaunchKernelGGL(k_gl_lde_pa_small<3>, grid, dim3(THREADS), 0, stream, coeffs, lde, ct.rate_bits, t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
        return;
    }
    if (L == 17) { GB_PAS(1); return; }
    if (L == 18) { GB_PAS(2); return; }
    if (L == 19) { GB_PAS(3); return; }
#undef GB_PAS
    if (L == 16)
        hipLaunchKernelGGL(k_gl_lde_pa16x1, dim3((u32)(ncols << 4)), dim3(THREADS), 0, stream, coeffs, lde, ct.rate_bits,
                           t.tw_hi_fwd_m, t.tw_lo_fwd_m, ct.pow_lo_m, ct.pow_hi_m);
}

void lde_pb_r16(u64* lde, size_t ntiles, const GlNttTables& t, hipStream_t stream) {
    hipLaunchKernelGGL(k_gl_lde_pb16, dim3((u32)ntiles), dim3(THREADS), 0, stream, lde, t.tw4096_fwd_m);
}

GB_INSTANTIATE_NTT(GlF)

}  // namespace gbk

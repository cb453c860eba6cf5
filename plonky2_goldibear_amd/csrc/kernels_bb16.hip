// BabyBear NTT passes, v2: radix-16 butterflies held in registers (gfx950).
//
// Pass structure and dispatch: ntt_passes.hpp and lde_passes.hpp (the LDE's strided passes), shared with Goldilocks; the contiguous
// LDE pass below follows the same index math as kernels_ntt16.hip's.  What differs is the arithmetic: BabyBear has no power-of-two roots of unity, so the
// 17 non-trivial twiddles inside a 16-point DFT are Montgomery multiplications by compile-time constants w_16^k.  The
// multiplication count per element and layer is therefore the same as radix-2 (1/2); what the register form buys is one LDS round
// trip per four layers instead of one per layer (v1, LDS radix-2 passes: 34.8 ms of LDE per 2^20 proof, ~5x the VALU bound).
#include <algorithm>
#include <cassert>

#include "bb_field.hpp"
#include "kernels.hpp"
#include "ntt_passes.hpp"
#include "dft_bb.hpp"
#include "lde_passes.hpp"

namespace gbk {

// ------------------------------------------------------------------ LDE pass B: 4096 contiguous points, 3 radix-16 stages
// grid = number of 4096-tiles of `lde` (in place).  natural -> bit-reversed.
__global__ __launch_bounds__(THREADS) void k_bb_lde_pb16(u32* __restrict__ lde, const u32* __restrict__ tw4096, u32 ntiles) {
    __shared__ u32 sh[16 * 272];
    const u32 tid = threadIdx.x;
    const u32 hi4 = tid >> 4, lo4 = tid & 15;
    u32 tw1[16], tw2[16];
    load_tw16<BbF>(tw1, tw4096, tid);       // w_4096^(k2 (16 d1 + d0))
    load_tw16<BbF>(tw2, tw4096, lo4 * 16);  // w_256^(k1 d0)
    u32 x[16], nx[16];
    u32 tile = blockIdx.x;
    if (tile < ntiles) {
        const u32* p = lde + ((size_t)tile << 12);
#pragma unroll
        for (u32 d = 0; d < 16; d++) nx[d] = p[d * 256 + tid];
    }
    // persistent workgroups: the next tile's 16 loads are in flight while this tile is transformed
    for (; tile < ntiles; tile += gridDim.x) {
        u32* p = lde + ((size_t)tile << 12);
#pragma unroll
        for (u32 d = 0; d < 16; d++) x[d] = nx[d];
        const u32 next = tile + gridDim.x;
        if (next < ntiles) {
            const u32* q = lde + ((size_t)next << 12);
#pragma unroll
            for (u32 d = 0; d < 16; d++) nx[d] = q[d * 256 + tid];
        }
        // stage 1: digit d2 (stride 256); this thread is (d1, d0) = tid
        dft16<false>(x);
#pragma unroll
        for (u32 s = 0; s < 16; s++) sh[s * 272 + tid] = s ? bb::mul(x[s], tw1[s]) : x[s];
        __syncthreads();
        // stage 2: digit d1; this thread is (k2 slot, d0)
#pragma unroll
        for (u32 d = 0; d < 16; d++) x[d] = sh[hi4 * 272 + d * 16 + lo4];
        dft16<false>(x);
        __syncthreads();
#pragma unroll
        for (u32 s = 0; s < 16; s++) sh[hi4 * 272 + lo4 * 17 + s] = s ? bb::mul(x[s], tw2[s]) : x[s];  // [k2 slot][d0][k1 slot], rows padded to 17
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
        __syncthreads();
    }
}

// ------------------------------------------------------------------ LDE pass A at 2^22 rows (the other sizes: lde_passes.hpp)
// LA = 10 (round 6): the strided pass as a 1024-point DFT over a' = 256 i1 + 16 a1 + a0 in THREE DIF stages - radix 4 over the top
// digit i1, twiddle w_1024^(k1 a), then the two radix-16 stages of k_lde_pa16x2 once per k1.  Output digit k1 is the LEAST
// significant one of k_a' = k1 + 4 k_a, so the rows of (c, k1) land in block brev_2(k1) of coset block c: the 2^(r+2) blocks of 2^20
// leaves ARE the cosets of a rate-2^(r+2) LDE of 2^20 rows, and everything after stage 0 is the 2^20-row pass on that finer coset
// c' = 4 c + brev_2(k1) - output twiddle (s_c w_n^k1)^l w_m^(k_a l) from the tables of m = 2^20 rows and of the rate r + 2.  One
// general multiplication per output more than at 2^20 rows, no extra pass over the data.
// 1024 threads: lanes 0..31 are the 32 columns of a 128-byte row segment, lane bit 5 is digit bit b of i1, the sixteen waves are a0.
// A thread holds i1 = b and b + 2 (32 words), does their butterfly itself and the second one ACROSS the wave's halves
// (v_permlane32_swap hands every lane both operands: no LDS), and goes through the radix-16 stages twice (k1 = 2 b and 2 b + 1).
// Measured against the two-stage form (k_lde_pa32 with K = 2, same box, profiles/r06_large_sizes.txt): 13.0 against 14.8 ms per 167
// columns - the other three (field, size) pairs go the other way.
__device__ __forceinline__ void lane_pair32(u32 x, u32& lower, u32& upper) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);   // upper half of the first operand <-> lower half of the second
    lower = r[0];   // (the builtin, not inline asm: the swap needs wait states after a vector write of its operands, which the compiler's
    upper = r[1];   //  hazard recognizer inserts for its own instructions only - the asm form returned stale halves on the GPU)
}
__global__ __launch_bounds__(1024) void k_bb_lde_pa16x2w(const u32* __restrict__ coeffs, u32* __restrict__ lde, u32 rate_bits,
                                                          const u32* __restrict__ tw4096, const u32* __restrict__ tw_hi,
                                                          const u32* __restrict__ tw_lo, const u32* __restrict__ pow_lo,
                                                          const u32* __restrict__ pow_hi) {
    constexpr u32 L = 22, W = 64, SLOT = 16 * W;   // LDS: [k_a1 slot][a0][b][j]
    __shared__ u32 sh[16 * SLOT];
    __shared__ u32 tw0[1024];   // the stage-0 twiddles w_1024^(k a), [k][a]: in LDS so that they are not 32 more live registers
    const size_t col = blockIdx.x >> 7;
    const u32 tg = blockIdx.x & 127;
    const u32 tid = threadIdx.x, hi4 = tid >> 6, jl = tid & 63, b = jl >> 5, j = jl & 31;
    tw0[tid] = tw4096[((tid >> 8) * (tid & 255)) << 2];
    const u32 l = tg * 32 + j;
    const size_t n = (size_t)1 << L;
    const u32* cin = coeffs + col * n + l;
    u32 orig[2][16];   // digits i1 = b and b + 2
#pragma unroll
    for (u32 h = 0; h < 2; h++)
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) orig[h][a1] = cin[(size_t)((b + 2 * h) * 256 + a1 * 16 + hi4) << 12];
    const u32 ratio = tw_split16<BbF>(tw_hi, tw_lo, 16 * l);          // tables of m = 2^20 rows
    const u32 f0 = tw_split16<BbF>(tw_hi, tw_lo, brev4(hi4) * l);
    u32 tw[16];
    load_tw16<BbF>(tw, tw4096, hi4 * 16);  // w_256^(k_a1 a0)
    // lane mask of the digit bit, opaque to the optimiser: written as selects on a lane-varying bool the butterflies below made the
    // compiler spill registers (it unswitched around them); as bit blends (v_bfi) they cost the same and spill nothing
    u32 m5 = b ? ~0u : 0u;
    asm("" : "+v"(m5));
    __syncthreads();                  // tw0 visible
    for (u32 c = 0; c < (1u << rate_bits); c++) {
        const u32* ph = pow_hi + (size_t)c * 1024 + hi4;
        u32 y[2][16];
#pragma unroll
        for (u32 h = 0; h < 2; h++)
#pragma unroll
            for (u32 a1 = 0; a1 < 16; a1++) y[h][a1] = bb::mul(orig[h][a1], ph[(b + 2 * h) * 256 + a1 * 16]);  // s_c^(4096 a')
#pragma unroll
        for (u32 a1 = 0; a1 < 16; a1++) {
            u32 p, q;
            // (x_b, x_(b+2)) in the thread: sum for the even k1, difference (times w_4 where b = 1) for the odd ones
            const u32 sm = bb::add(y[0][a1], y[1][a1]), d = bb::sub(y[0][a1], y[1][a1]);
            const u32 dw = bb::mul(d, bbc::tw<false, 4>());
            y[0][a1] = sm;
            y[1][a1] = (d & ~m5) | (dw & m5);
            lane_pair32(y[1][a1], p, q);
            const u32 s1 = bb::add(p, q), d1 = bb::sub(p, q);
            y[1][a1] = (s1 & ~m5) | (d1 & m5);          // k1 = 2 b + 1
            lane_pair32(y[0][a1], p, q);
            const u32 s0 = bb::add(p, q), d0 = bb::sub(p, q);
            y[0][a1] = (s0 & ~m5) | (d0 & m5);          // k1 = 2 b
        }
#pragma nounroll
        for (u32 h = 0; h < 2; h++) {   // (a real loop: unrolled, the two passes' addresses and twiddles were live together and spilled)
            const u32 k1 = 2 * b + h;
            const u32 cf = c * 4 + b + 2 * h;   // 4 c + brev_2(k1)
            u32 x[16];
#pragma unroll
            for (u32 a1 = 0; a1 < 16; a1++) x[a1] = bb::mul(y[0][a1], tw0[k1 * 256 + a1 * 16 + hi4]);   // w_1024^(k1 a) (k1 = 0: 1)
#pragma unroll
            for (u32 a1 = 0; a1 < 16; a1++) y[0][a1] = y[1][a1];
            const u32 sl = pow_lo[(size_t)cf * 4096 + l];
            dft16<false>(x);
#pragma unroll
            for (u32 s = 0; s < 16; s++) sh[s * SLOT + tid] = s ? bb::mul(x[s], tw[s]) : x[s];  // [k_a1 slot][a0][b][j]
            __syncthreads();
#pragma unroll
            for (u32 a0 = 0; a0 < 16; a0++) x[a0] = sh[hi4 * SLOT + a0 * W + jl];
            dft16<false>(x);
            u32* out = lde + (col << (L + rate_bits)) + ((size_t)cf << 20) + l;
            u32 f = bb::mul(sl, f0);
#pragma unroll
            for (u32 k = 0; k < 16; k++) {
                out[(size_t)(hi4 * 16 + brev4(k)) << 12] = bb::mul(x[brev4(k)], f);
                if (k < 15) f = bb::mul(f, ratio);
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ launchers (called from lde_columns<BbF> / lde_pa_r16<BbF>)

// The 2^22-row pass reads the twiddles of the 2^20-row transform (t.wide), the cosets of the rate r + 2 (ct.fine) and the
// s_c^(4096 a') of this size: tables_for / cosets_for build both at that size, and no other pass handles it
void lde_pa_rows22(const u32* coeffs, u32* lde, size_t ncols, const BbNttTables& t, const BbCosetTables& ct, hipStream_t stream) {
    assert(t.wide && ct.fine && "the 2^22-row LDE pass needs the 2^20-row twiddles and the rate r + 2 cosets");
    hipLaunchKernelGGL(k_bb_lde_pa16x2w, dim3((u32)(ncols << 7)), dim3(1024), 0, stream, coeffs, lde, ct.rate_bits, t.tw4096_fwd,
                       t.wide->tw_hi_fwd, t.wide->tw_lo_fwd, ct.fine->pow_lo, ct.pow_hi);
}

void lde_pb_r16(u32* lde, size_t ntiles, const BbNttTables& t, hipStream_t stream) {
    const u32 grid = (u32)std::min<size_t>(ntiles, 256 * 7);  // persistent: 7 workgroups per CU (65 VGPRs, 17 KB LDS each)
    hipLaunchKernelGGL(k_bb_lde_pb16, dim3(grid), dim3(THREADS), 0, stream, lde, t.tw4096_fwd, (u32)ntiles);
}

bool bb_intt_columns_canonical(u32* vals, u32* coeffs, u32* scratch, size_t ncols, size_t mont_cols, const BbNttTables& t, hipStream_t stream) {
    if (t.log_n < 16 || t.log_n > NTT_NATIVE_LOG) return false;
    const size_t n = (size_t)1 << t.log_n;
    for_intt_groups<BbF>(t.log_n, ncols, [&](size_t c0, size_t nc) {
        intt_columns_r16<BbF, true>(vals + c0 * n, coeffs + c0 * n, scratch, nc, t, stream, vals + c0 * n, mont_cols > c0 ? mont_cols - c0 : 0);
    });
    return true;
}

GB_INSTANTIATE_NTT(BbF)

}  // namespace gbk

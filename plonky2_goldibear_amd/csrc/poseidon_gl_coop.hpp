// Poseidon width-12 over Goldilocks with ONE STATE PER 16-LANE ROW (lane l < 12 holds word l), for the parts of a proof
// where the number of independent permutations is small: the upper levels of every Merkle tree and all of a
// recursion-sized proof's trees.  The lane-per-state form (poseidon_gl.hpp) runs ~22 k dependent-ish instructions per
// permutation in each lane; a wave with nothing to interleave with takes ~56 us for that, whatever the number of states it
// carries, and a tree below ~2^13 nodes cannot fill the machine.  Here every word has its own lane, so the twelve s-boxes of a
// round cost what one costs, and the fast (w_hat / v / M_init) form of the partial rounds - which saves s-boxes and products
// when one lane carries a whole state - saves nothing: a partial round is written in its DEFINING form, a full round whose
// s-box result is kept in lane 0 only.  Thirty rounds of one shape: constants, s-box, MDS.  Same function as
// hash/poseidon_goldilocks.rs:912-922 (whose fast partial rounds :632-770 are an algebraic rewrite of these), bit-exact;
// tests/test_device_headers_on_host.py checks the 30-round form against the fast form on the host.
//
// Data movement: every round's MDS reads the twelve words through LDS (one b64 write, twelve b64 reads per lane); the next
// round's constant is fetched one round ahead and is the start value of the MDS sums.  Blocks are one wave (64 threads = 4
// states), so __syncthreads() only orders the LDS traffic.
#pragma once
#include "poseidon_gl.hpp"

namespace poseidon_gl_coop {

using gl::u32;
using gl::u64;

// The lazy addition and the DPP all-reduce over a row that the fast-form partial rounds used.  permute() no longer calls them;
// they stay because tests/device/permutation_helpers.hip checks them by name.
// a + b for ANY two u64 residues -> some u64 residue (a carry out of bit 64 is worth EPS; the corrected sum can carry once more)
__device__ __forceinline__ u64 add_lazy(u64 a, u64 b) {
    u64 s, t;
    const bool c1 = __builtin_uaddll_overflow(a, b, &s);
    const bool c2 = __builtin_uaddll_overflow(s, c1 ? gl::EPS : 0, &t);
    return t + (c2 ? gl::EPS : 0);
}
template <int N>
__device__ __forceinline__ u64 row_ror(u64 x) {  // lane i of each 16-lane row receives lane (i - N) mod 16
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(u32)x, 0x120 + N, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(u32)(x >> 32), 0x120 + N, 0xF, 0xF, false);
    return (u64)(u32)lo | ((u64)(u32)hi << 32);
}
// sum of the row's sixteen values, in every lane (as field elements; lanes may hold different representatives)
__device__ __forceinline__ u64 row_sum(u64 x) {
    x = add_lazy(x, row_ror<8>(x));
    x = add_lazy(x, row_ror<4>(x));
    x = add_lazy(x, row_ror<2>(x));
    return add_lazy(x, row_ror<1>(x));
}

// x^7 for a Montgomery-form residue, the function poseidon_gl::sbox computes, written for a wave that has its SIMD to itself:
// nothing else issues into the wait states between a carry's producer and its consumer, so the two independent products x x^2
// and x^2 x^2 are written multiply-add by multiply-add next to each other, and so are their folds (gl::mul_limbs and
// gl::mont_fold_flags, step by step).  The strictly serial parts are x^2 before and x^3 x^4 after.
__device__ __forceinline__ u64 sbox_coop(u64 x) {
    const u64 x2 = gl::mul_mont_lazy(x, x);
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32), y0 = (u32)x2, y1 = (u32)(x2 >> 32);
    // A = x x^2, B = x^2 x^2 as four limbs each
    const u64 a00 = (u64)x0 * y0;
    const u64 b00 = (u64)y0 * y0;
    const u64 a01 = (u64)x0 * y1 + (a00 >> 32);
    const u64 b01 = (u64)y0 * y1 + (b00 >> 32);
    u64 ca, cb;
    const u64 am = gl::mad_carry(x1, y0, a01, ca);
    const u64 bm = gl::mad_carry(y1, y0, b01, cb);
    const u64 a11 = (u64)x1 * y1 + (am >> 32);
    const u64 b11 = (u64)y1 * y1 + (bm >> 32);
    const u32 a3 = gl::addc_carry((u32)(a11 >> 32), ca);
    const u32 b3 = gl::addc_carry((u32)(b11 >> 32), cb);
    // the two Montgomery folds
    u32 ea, eb, wa, wb, ka, kb;
    u64 c0a, c0b, cca, ccb, coa, cob;
    const u32 aa1 = __builtin_addc((u32)am, (u32)a00, 0u, &ea);
    const u32 ba1 = __builtin_addc((u32)bm, (u32)b00, 0u, &eb);
    const u32 ab0 = __builtin_subc((u32)a00, aa1, ea, &wa);
    const u32 bb0 = __builtin_subc((u32)b00, ba1, eb, &wb);
    const u32 ab1 = __builtin_subc(aa1, 0u, wa, &ka);
    const u32 bb1 = __builtin_subc(ba1, 0u, wb, &kb);
    const u32 ar0 = gl::sub_flag((u32)a11, ab0, c0a);
    const u32 br0 = gl::sub_flag((u32)b11, bb0, c0b);
    const u32 ar1 = gl::subb_flag(a3, ab1, c0a, cca);
    const u32 br1 = gl::subb_flag(b3, bb1, c0b, ccb);
    const u32 af0 = gl::addc_flag(ar0, cca, coa);
    const u32 bf0 = gl::addc_flag(br0, ccb, cob);
    const u32 af1 = gl::subb_zero(ar1, cca & ~coa);
    const u32 bf1 = gl::subb_zero(br1, ccb & ~cob);
    const u64 x3 = (u64)af0 | ((u64)af1 << 32), x4 = (u64)bf0 | ((u64)bf1 << 32);
    return gl::mul_mont_lazy(x3, x4);
}

// One permutation per row.  `x`: this lane's word (lanes 12..15: anything; they are kept at zero).  `sh` = this row's 16 u64 of
// LDS.  Returns the lane's output word as a lazy residue (call gl::canon before storing); lanes >= 12 return 0.
// (A permutation that starts from a zero capacity could take lanes 8..11's first s-box from poseidon_gl::ZERO_CAP_SBOX_T, but the
// s-box runs in all lanes anyway: a table load and a select more, no slot less.  Left out.)
__device__ __forceinline__ u64 permute(u64 x, u32 l, u64* __restrict__ sh) {
    const bool live = l < 12;
    const u32 lc = live ? l : 0;       // a valid table index for the idle lanes
    x = poseidon_gl::to_mont(x);       // the s-box and the additive constants work on Montgomery-form residues (poseidon_gl.hpp)
    // res[l] = sum_i v[(l + i) % 12] CIRC[i] + (l == 0) v[0] DIAG[0] + c   (:547-557; c: the constant of the round that follows)
    auto mds = [&](u64 v, u64 c) {
        __syncthreads();               // the previous reads of sh are done
        sh[l] = v;
        __syncthreads();
        u64 sl = (u32)c, shh = c >> 32;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            u32 j = lc + i;
            j = j >= 12 ? j - 12 : j;
            const u64 w = sh[j];
            sl += (u64)(u32)w * poseidon_gl::mds_circ(i);
            shh += (u64)(u32)(w >> 32) * poseidon_gl::mds_circ(i);
        }
        if (l == 0) {
            sl += (u64)(u32)v * poseidon_gl::MDS_DIAG0;
            shh += (u64)(u32)(v >> 32) * poseidon_gl::MDS_DIAG0;
        }
        // sl + 2^32 shh with sl, shh < 2^42: the bits of shh above 32 are worth EPS each (2^64 = EPS)
        const u64 t = sl + (shh >> 32) * gl::EPS;
        u64 r;
        const bool cy = __builtin_uaddll_overflow(t, shh << 32, &r);
        r += cy ? gl::EPS : 0;
        return live ? r : 0;
    };
    // Round r (:889-909 in the defining form): x += RC[r], s-box - in every word of the eight full rounds, in word 0 of the 22
    // partial rounds -, MDS.  The constants of round r + 1 are loaded while round r computes and ride on its MDS sums.
    x = poseidon_gl::add_rc(x, GB_RC[lc]);
#pragma unroll 1
    for (int r = 0; r < 30; r++) {
        const u64 rc = r + 1 < 30 ? GB_RC[12 * (r + 1) + lc] : 0;
        const u64 y = sbox_coop(x);
        const bool full = r < 4 || r >= 26;
        x = mds((full || l == 0) ? y : x, rc);
    }
    return poseidon_gl::mont_fold((u32)x, (u32)(x >> 32), 0u, 0u);   // out of Montgomery form; still a lazy residue
}

}  // namespace poseidon_gl_coop

// gb_constraint_quotient: the alpha-folded constraints of a constraint system (constraint_system.hpp) over any committed oracles,
// divided by Z_H, at every point of the quotient domain - the first 2^rate_bits coset blocks of the oracles' leaf-order LDEs, one
// thread per point with the index math of k_quotient (kernels_prover.hip: j, cidx, il, imod).  The constraints are straight-line
// programs; gates::run_program interprets them as k_gate_programs (kernels_gates.hip) does: the register file is indexed at run
// time, so it lives in LDS - [max_regs][blockDim] words, a register's row lane-consecutive, at most 32 x 256 x 8 bytes = 64 KiB -
// and instruction words, literals, cell words, params and alpha powers are the same for the whole wave and come through the scalar
// unit (const __restrict__, uniform index).  A CELL operand resolves, through its cell word, to an oracle's LDE block, a column and
// a number of rows ahead; the leaf of the rotated row is computed where the cell is read (a per-lane table of rotated leaves would
// be indexed at run time and go to scratch).  X comes from the split power tables, L_first from the L_0 table of k_l0_table and
// L_last = L_0(w X) from the same table at the next row's leaf.  Every constraint is folded into C FoldAcc sums as it is emitted;
// the sums are finished per program (a chain stays within FOLD_ACC_MAX_TERMS), added up, multiplied by 1 / Z_H of the coset and
// stored where intt_columns and quotient_combine expect them.
#include "fold_acc.hpp"
#include "gates.hpp"
#include "kernels.hpp"

namespace gbk {

namespace {
__device__ __forceinline__ u32 brev32c(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }
}  // namespace

static constexpr u32 CONSTRAINT_BLOCK = 256;
template <class F, u32 C>
__global__ __launch_bounds__(CONSTRAINT_BLOCK) void k_constraint_quotient(ConstraintParams<F> p, const typename F::T* __restrict__ apow,
                                                                          const typename F::T* __restrict__ zh_inv,
                                                                          typename F::T* __restrict__ qv) {
    typedef typename F::T T;
    typedef gates::BaseAlg<F> A;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_cons[];
    const gates::LdsRegs<T> regs{reinterpret_cast<T*>(smem_cons) + threadIdx.x, CONSTRAINT_BLOCK};
    const u32 lgn = p.log_n, r = p.rate_bits;
    const size_t n = (size_t)1 << lgn, N = (size_t)1 << p.stride_bits;   // N: column stride of every oracle's LDE
    const size_t j = (size_t)blockIdx.x * CONSTRAINT_BLOCK + threadIdx.x;
    if (j >= (n << r)) return;   // (no barrier below: a lane only ever touches its own LDS words)
    const u32 cidx = (u32)(j >> lgn), jl = (u32)(j & (n - 1));
    const u32 il = brev32c(jl, lgn);
    const u32 imod = brev32c(cidx, r);
    const u64 i = ((u64)il << r) | imod;
    T x;   // g * w_N^i
    {
        const T lo = p.w_N.lo[i & ((1u << p.w_N.lo_bits) - 1)];
        const u64 h = i >> p.w_N.lo_bits;
        x = F::mul(F::generator(), h ? F::mul(lo, p.w_N.hi[h]) : lo);
    }
    const size_t block0 = (size_t)cidx << lgn;
    const u32 row_mask = (u32)(n - 1);
    const u64* __restrict__ cells = p.cells;
    const T* __restrict__ params = p.params;
    const T* __restrict__ l0 = p.l0;
    T acc[C];
#pragma unroll
    for (u32 k = 0; k < C; k++) acc[k] = F::zero();
    u32 idx0 = 0;
    for (u32 g = 0; g < p.num_programs; g++) {
        const constraints::ProgramInfo& pi = p.p[g];
        const u64* __restrict__ pcells = cells + pi.cell_off;
        auto cell = [&](u32 c) {
            const u64 w = pcells[c];
            const T* __restrict__ lde = p.lde[constraints::cell_oracle(w)];
            const size_t leaf = block0 | brev32c((il + constraints::cell_row_offset(w)) & row_mask, lgn);
            return lde[(size_t)constraints::cell_polynomial(w) * N + leaf];
        };
        auto input = [&](u32 k) -> T {
            if (k == constraints::INPUT_X) return x;
            if (k == constraints::INPUT_L_FIRST) return l0[j];
            if (k == constraints::INPUT_L_LAST) return l0[block0 | brev32c((il + 1) & row_mask, lgn)];
            return params[k - constraints::NUM_BUILTIN_INPUTS];
        };
        FoldAcc<F> sum[C];
        u32 idx = idx0;
        auto emit = [&](T c) {
#pragma unroll
            for (u32 k = 0; k < C; k++) sum[k].acc(c, apow[k * p.nterms + idx]);
            idx++;
        };
        gates::run_program<F, A>(p.instrs + pi.instr_off, pi.num_instrs, p.lits + pi.lit_off, regs, cell, input, emit);
#pragma unroll
        for (u32 k = 0; k < C; k++) acc[k] = F::add(acc[k], sum[k].finish());
        idx0 += pi.num_constraints;
    }
    const T zi = zh_inv[imod];
#pragma unroll
    for (u32 k = 0; k < C; k++) qv[(((size_t)k << r) + cidx) * n + il] = F::mul(acc[k], zi);
}

// one launch per slice of challenges (challenge_slices.hpp with the widths 1 .. 4 for either field): a slice [k0, k0 + w) is the
// same kernel on the alpha powers and the qv block of challenge k0
template <class F>
bool constraint_quotient_values(const ConstraintParams<F>& p, u32 num_challenges, const typename F::T* apow, const typename F::T* zh_inv,
                                typename F::T* qv, hipStream_t st) {
    typedef typename F::T T;
    u32 widths[MAX_CHALLENGES];
    const u32 ns = challenge_slices(0, 4, num_challenges, widths);
    if (!ns) return false;
    const size_t points = (size_t)1 << (p.log_n + p.rate_bits);
    const dim3 grid((u32)((points + CONSTRAINT_BLOCK - 1) / CONSTRAINT_BLOCK)), block(CONSTRAINT_BLOCK);
    const size_t smem = (size_t)(p.max_regs ? p.max_regs : 1u) * CONSTRAINT_BLOCK * sizeof(T);
    for (u32 s = 0, k0 = 0; s < ns; k0 += widths[s], s++) {
        const T* a = apow + (size_t)k0 * p.nterms;
        T* q = qv + (((size_t)k0 << p.rate_bits) << p.log_n);
        switch (widths[s]) {
            case 1: hipLaunchKernelGGL((k_constraint_quotient<F, 1>), grid, block, smem, st, p, a, zh_inv, q); break;
            case 2: hipLaunchKernelGGL((k_constraint_quotient<F, 2>), grid, block, smem, st, p, a, zh_inv, q); break;
            case 3: hipLaunchKernelGGL((k_constraint_quotient<F, 3>), grid, block, smem, st, p, a, zh_inv, q); break;
            case 4: hipLaunchKernelGGL((k_constraint_quotient<F, 4>), grid, block, smem, st, p, a, zh_inv, q); break;
            default: return false;
        }
    }
    return true;
}
template bool constraint_quotient_values<GlF>(const ConstraintParams<GlF>&, u32, const u64*, const u64*, u64*, hipStream_t);
template bool constraint_quotient_values<BbF>(const ConstraintParams<BbF>&, u32, const u32*, const u32*, u32*, hipStream_t);

}  // namespace gbk

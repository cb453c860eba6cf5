// FoldAcc: sum_i c_i * a_i of one gate's constraints against the powers of alpha, kept UNREDUCED until the gate is done: a term is a
// product plus carry adds instead of a modular multiplication and a modular addition (Goldilocks 15 instructions against 29,
// BabyBear 3 against 9 - and BabyBear folds against 6..10 challenges).  The accumulators of the gate kernels (kernels_gates.hip:
// k_gate_constraints, k_gate_constraints_tiled, k_gate_programs), in a header of their own so that test programs can call them
// (tests/host_shim/fold_acc.cpp on the CPU through tests/host_shim/shim.h, tests/device/fold_acc.hip on the GPU).
//
// Domain.  acc(c, a) takes c from a gate evaluator's emit() and a from the alpha-power table.
//   c: gates.hpp evaluates over BaseAlg<F>, whose add / sub / mul are F::add / F::sub / F::mul - gl::add / sub / mul and
//      bb::add / sub / mul, each canonical out for canonical in (gl::mul: any u64 in) - on wires, constants and public-input hash
//      words that are canonical in device memory, and on F::enc / F::one literals.  No evaluator uses a lazy form (bb::mul_lazy,
//      bb::reduce_lazy, gl::fold128 without canon); gl's mds_layer_gl_base ends in a canonical reduction.  So every emitted word is
//      canonical, < p, in device form (BabyBear: Montgomery).
//   a: stage_quotient_polys builds the table on the host as x <- F::mul(x, F::enc(alpha)) from F::one(): canonical, device form.
//   Both operands therefore range over [0, p).  A BabyBear word is never lazy here; the tests run exactly [0, p) x [0, p).
// Terms.  One chain is one gate's constraints at one point.  Every gate kind build_gate_set accepts has no more constraints than
//   wires (gates.hpp num_constraints / num_wires, kind by kind), a gate's wires fit the circuit's (build_gate_set), and a circuit has
//   at most 4096 wires (check_circuit_cfg, verifier_create_checked); a constraint program has at most MAX_PROGRAM_CONSTRAINTS = 1024
//   (gate_set.hpp).  So a chain has at most FOLD_ACC_MAX_TERMS = 4096 terms (BaseSumGate with 4095 limbs reaches it).
//   Goldilocks: the sum is < 4096 (p - 1)^2 < 2^140, l4 <= 4095, far inside fold160's r4 <= 2^31 (the bound on the number of terms
//     that keeps l4 there is 2^31: a term adds less than 2^128).
//   BabyBear: the sum is < 4096 (p - 1)^2 < 2^74, hi <= 900.  finish() needs hi R2 < p 2^32 for bb::mul's reduction, which holds for
//     EVERY u32 hi because R2 < p; what the form needs is that hi does not wrap, fewer than 2^32 carries: any count below 2^34 terms.
#pragma once
#include "field_traits.hpp"

namespace gbk {

static constexpr u32 FOLD_ACC_MAX_TERMS = 4096;

template <class F>
struct FoldAcc;
template <>
struct FoldAcc<GlF> {  // 160-bit sum of 128-bit products; fewer than 2^31 terms (gl::fold160)
    u32 l0 = 0, l1 = 0, l2 = 0, l3 = 0, l4 = 0;
    __device__ __forceinline__ void acc(u64 c, u64 a) {
        u32 p0, p1, p2, p3, k0, k1, k2, k3;
        gl::mul_limbs(c, a, p0, p1, p2, p3);
        l0 = __builtin_addc(l0, p0, 0u, &k0);
        l1 = __builtin_addc(l1, p1, k0, &k1);
        l2 = __builtin_addc(l2, p2, k1, &k2);
        l3 = __builtin_addc(l3, p3, k2, &k3);
        l4 += k3;
    }
    __device__ __forceinline__ u64 finish() const { return gl::canon(gl::fold160(l0, l1, l2, l3, l4)); }
};
template <>
struct FoldAcc<BbF> {  // Montgomery words: the sum S of (c R)(a R) is brought back with one reduction, S R^-1 = (sum c a) R
    u64 lo = 0;
    u32 hi = 0;
    __device__ __forceinline__ void acc(u32 c, u32 a) {
        const u64 p = (u64)c * a, s = lo + p;
        hi += s < p;
        lo = s;
    }
    // S = w0 + 2^32 w1 + 2^64 hi:  S 2^-32 = w0 2^-32 + w1 + hi 2^32  (mod p)
    __device__ __forceinline__ u32 finish() const {
        u32 w1 = (u32)(lo >> 32);  // < 2^32 < 3 p
        w1 = w1 >= bb::P ? w1 - bb::P : w1;
        w1 = w1 >= bb::P ? w1 - bb::P : w1;
        return bb::add(bb::add(bb::reduce((u64)(u32)lo), w1), bb::mul(hi, bb::R2));
    }
};

}  // namespace gbk

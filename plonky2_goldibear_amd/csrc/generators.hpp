// Witness generators on the device: generate_partial_witness (iop/generator.rs:25-106) as waves over the schedule of
// generator_schedule.hpp.  One evaluator per generator kind, each the counterpart of its gate's eval_* in gates.hpp and written
// with the same extension algebra (Tup<>), MDS tables and round structure (poseidon_gate_rounds / poseidon2_gate_rounds):
//   ArithmeticBaseGenerator        gates/arithmetic_base.rs:192-240      ArithmeticExtensionGenerator  gates/arithmetic_extension.rs:186-233
//   MulExtensionGenerator          gates/multiplication_extension.rs:160-200   ConstantGenerator / CopyGenerator  iop/generator.rs
//   BaseSplitGenerator             gates/base_sum.rs:178-225             ReducingGenerator             gates/reducing.rs:205-250
//   ReducingExtensionGenerator     gates/reducing_extension.rs:203-245   RandomAccessGenerator         gates/random_access.rs:383-440
//   PoseidonMdsGenerator           gates/poseidon_goldilocks_mds.rs:255-300    InterpolationGenerator  gates/coset_interpolation.rs:451-560
//   ExponentiationGenerator        gates/exponentiation.rs:248-300       PoseidonGenerator             gates/poseidon_goldilocks.rs:436-531
//   Poseidon2BabyBearGenerator     gates/poseidon2_babybear.rs:536-676   AddManyGenerator              gates/add_many.rs:167-215
//   ApplyMat4Generator             gates/apply_mat4.rs:216-270           Poseidon2InternalPermutationGenerator  gates/poseidon2_internal_permutation.rs:225-290
// and the generators of the gadgets, whose operands are arbitrary targets:
//   EqualityGenerator              gadgets/arithmetic.rs:425-452         QuotientOrZeroGenerator       gadgets/arithmetic.rs:487-511
//   NonzeroTestGenerator           iop/generator.rs:400-428              QuotientGeneratorExtension    gadgets/arithmetic_extension.rs:507-532
//   SplitGenerator / WireSplitGenerator  gadgets/split_join.rs:67-161    LowHighGenerator              gadgets/range_check.rs:89-115
//   BaseSumGenerator               gadgets/split_base.rs:84-116
// The values array holds one CANONICAL word per copy class; an evaluator converts to the device form and back (a no-op for
// Goldilocks).  Every class index comes from the schedule, which range-checked it; values that index something - the access index
// of RandomAccessGenerator - are compared with their bound before use.  The reference's assert!s end in the device error word,
// not in a fault.
//
// Depends on the field headers and gates.hpp only (and the plain words of generator_ops.hpp): tests/device/generators.hip and
// tests/host_shim/generators.cpp include it on their own.
#pragma once
#include <type_traits>

#include "gates.hpp"
#include "generator_ops.hpp"

namespace gbk {
namespace gen {

GB_HD void report(u32* err, u32 code, u32 record, u32 cls) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (atomicCAS(err, 0u, code) == 0u) {   // the first report stays
        err[1] = record;
        err[2] = cls;
    }
#else
    if (!err[0]) {
        err[0] = code;
        err[1] = record;
        err[2] = cls;
    }
#endif
}

// an Op's view of the values array.  `values` is written and read again inside one launch of the chain kernel: a plain pointer,
// never const __restrict__ (the scalar-cache path is not coherent with vector stores).
template <class F>
struct Io {
    typedef typename F::T T;
    const Op& op;
    const u32* args;
    T* values;
    u32* err;
    GB_HD T raw(u32 i) const { return values[args[op.in_off + i]]; }   // canonical
    GB_HD T in(u32 i) const { return F::enc(raw(i)); }                  // device form
    GB_HD T operator()(u32 i) const { return in(i); }                   // as a `wire` accessor of Tup<>::load
    GB_HD void put(u32 i, T canonical) const {
        const u32 w = args[op.out_off + i];
        if (w == OUT_SKIP) return;
        const u32 cl = w & ~OUT_CHECK;
        if (w & OUT_CHECK) {
            if (values[cl] != canonical) report(err, ERR_SET_TWICE, op.record, cl);
        } else {
            values[cl] = canonical;
        }
    }
    GB_HD void out(u32 i, T device_form) const { put(i, (T)F::dec(device_form)); }
    template <class X>
    GB_HD void out_ext(u32 i, const X& x) const {
#pragma unroll
        for (u32 k = 0; k < F::D; k++) out(i + k, x.c[k]);
    }
};

template <class F>
GB_HD void gen_arithmetic_extension(const Io<F>& io, bool with_addend) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    constexpr u32 D = F::D;
    X r = (X::load(io, 0) * X::load(io, D)).scalar_c(F::enc(io.op.k[0]));
    if (with_addend) r = r + X::load(io, 2 * D).scalar_c(F::enc(io.op.k[1]));
    io.out_ext(0, r);
}

template <class F>
GB_HD void gen_base_split(const Io<F>& io) {
    const u32 limbs = io.op.p0, base = io.op.p1 < 2 ? 2 : io.op.p1;
    u64 v = (u64)io.raw(0);
    for (u32 i = 0; i < limbs; i++) {
        io.put(i, (typename F::T)(v % base));
        v /= base;
    }
    if (v) report(io.err, ERR_SPLIT_TOO_LARGE, io.op.record, io.args[io.op.in_off]);
}

template <class F>
GB_HD void gen_reducing(const Io<F>& io, bool extension_coeffs) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    constexpr u32 D = F::D;
    const X alpha = X::load(io, 0);
    X acc = X::load(io, D);
    for (u32 i = 0; i < io.op.p0; i++) {
        const X coeff = extension_coeffs ? X::load(io, 2 * D + i * D) : X::from_base(io.in(2 * D + i));
        acc = acc * alpha + coeff;
        io.out_ext(i * D, acc);
    }
}

template <class F>
GB_HD void gen_random_access(const Io<F>& io) {
    const u32 bits = io.op.p0;
    const u64 index = (u64)io.raw(0);
    if (index >> bits) {   // assert!(access_index < vec_size)
        report(io.err, ERR_ACCESS_INDEX, io.op.record, io.args[io.op.in_off]);
        return;
    }
    for (u32 i = 0; i < bits; i++) io.put(i, (typename F::T)((index >> i) & 1));
}

template <class F>
GB_HD void gen_poseidon_mds(const Io<F>& io) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    constexpr u32 D = F::D;
    const gates::PoseidonTab& t = gates::poseidon_tab();
#pragma unroll 1
    for (u32 r = 0; r < 12; r++) {
        X res = X::load(io, r * D).scalar_c(F::enc(t.circ[0] + t.diag[r]));
#pragma unroll 1
        for (u32 i = 1; i < 12; i++) {
            const u32 j = r + i >= 12 ? r + i - 12 : r + i;
            res = res + X::load(io, j * D).scalar_c(F::enc(t.circ[i]));
        }
        io.out_ext(r * D, res);
    }
}

template <class F>
GB_HD void gen_coset_interpolation(const Io<F>& io) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    typedef typename F::T T;
    constexpr u32 D = F::D;
    const u32 bits = io.op.p0, degree = io.op.p1, npts = 1u << bits;
    const u32 nint = degree > 1 ? (npts - 2) / (degree - 1) : 0;
    const T g = F::two_adic_generator(bits), inv_m = F::inv(F::enc(npts));
    const X shifted = X::load(io, 1 + npts * D).scalar_c(F::inv(io.in(0)));
    io.out_ext(0, shifted);
    X ev = X::zero(), prod = X::from_base(F::one());
    T x_i = F::one();
    u32 next = 0;
    auto partial = [&](u32 hi) {   // partial_interpolate (:637-664); the points are visited once, in order
        for (; next < hi; next++) {
            const X val = X::load(io, 1 + next * D).scalar_c(F::mul(x_i, inv_m));   // barycentric weight x_i / 2^bits
            X term = shifted;
            term.c[0] = F::sub(term.c[0], x_i);
            ev = ev * term + val * prod;
            prod = prod * term;
            x_i = F::mul(x_i, g);
        }
    };
    partial(degree < npts ? degree : npts);
    for (u32 i = 0; i < nint; i++) {
        io.out_ext(D + 2 * D * i, ev);
        io.out_ext(2 * D + 2 * D * i, prod);
        const u32 lo = 1 + (degree - 1) * (i + 1), hi = lo + degree - 1 < npts ? lo + degree - 1 : npts;
        partial(hi);
    }
    io.out_ext(D + 2 * D * nint, ev);
}

template <class F>
GB_HD void gen_exponentiation(const Io<F>& io) {
    typedef typename F::T T;
    const u32 n = io.op.p0;
    const T base = io.in(0);
    T cur = F::one();
    for (u32 i = 0; i < n; i++) {
        if (i) cur = F::mul(cur, cur);
        if (io.raw(1 + (n - 1 - i)) != 0) cur = F::mul(cur, base);   // power bits are little-endian, the chain runs big-endian
        io.out(i, cur);
    }
    io.out(n, cur);
}

GB_HD void gen_poseidon(const Io<GlF>& io) {
    typedef gates::BaseAlg<GlF> A;
    const u64 swap = io.raw(12);
    if (swap > 1) {   // assert!(swap_value == F::ZERO || swap_value == F::ONE)
        report(io.err, ERR_SWAP_NOT_BOOLEAN, io.op.record, io.args[io.op.in_off + 12]);
        return;
    }
    u64 s[12];
#pragma unroll
    for (u32 i = 0; i < 4; i++) {
        const u64 lhs = io.raw(i), rhs = io.raw(i + 4), delta = swap ? gl::sub(rhs, lhs) : 0;
        io.put(i, delta);
        s[i] = gl::add(lhs, delta);
        s[i + 4] = gl::sub(rhs, delta);
    }
#pragma unroll
    for (u32 i = 8; i < 12; i++) s[i] = io.raw(i);
    // outputs: wires 25..134 (the deltas and the s-box inputs), then wires 12..23
    gates::poseidon_gate_rounds<A>(s, [&](u32 col, u64 computed) -> u64 {
        io.put(col >= 25 ? col - 25 : 110 + (col - 12), computed);
        return computed;
    });
}

GB_HD void gen_poseidon2_bb(const Io<BbF>& io) {
    typedef gates::BaseAlg<BbF> A;
    const u32 swap = io.raw(16);
    if (swap > 1) {
        report(io.err, ERR_SWAP_NOT_BOOLEAN, io.op.record, io.args[io.op.in_off + 16]);
        return;
    }
    u32 s[16];
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        const u32 lhs = io.in(i), rhs = io.in(i + 8), delta = swap ? bb::sub(rhs, lhs) : 0;
        io.out(i, delta);
        s[i] = bb::add(lhs, delta);
        s[i + 8] = bb::sub(rhs, delta);
    }
    // outputs: the operation's 133 non-routed wires (8 deltas, then the s-box inputs), then its 16 output wires
    gates::poseidon2_gate_rounds<BbF, A>(s, 8, 133, [&](u32 col, u32 computed) -> u32 {
        io.out(col, computed);
        return computed;
    });
}

template <class F>
GB_HD void gen_apply_mat4(const Io<F>& io) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    constexpr u32 D = F::D;
    const X x0 = X::load(io, 0), x1 = X::load(io, D), x2 = X::load(io, 2 * D), x3 = X::load(io, 3 * D);
    const X t01 = x0 + x1, t23 = x2 + x3, t0123 = t01 + t23, t01123 = t0123 + x1, t01233 = t0123 + x3;
    io.out_ext(0, t01123 + t01);
    io.out_ext(D, t01123 + (x2 + x2));
    io.out_ext(2 * D, t01233 + t23);
    io.out_ext(3 * D, t01233 + (x0 + x0));
}

template <class F>
GB_HD void gen_poseidon2_internal(const Io<F>& io) {
    typedef gates::Tup<F, gates::BaseAlg<F>> X;
    constexpr u32 D = F::D;
    constexpr u32 SHIFTS[15] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15};
    const typename F::T k = F::enc(943718400u);
    X part = X::zero();
#pragma unroll 1
    for (u32 i = 1; i < 16; i++) part = part + X::load(io, i * D).scalar_c(k);
    const X s0 = X::load(io, 0).scalar_c(k), full = part + s0;
    io.out_ext(0, part - s0);
#pragma unroll 1
    for (u32 i = 0; i < 15; i++) io.out_ext((1 + i) * D, full + X::load(io, (i + 1) * D).scalar_c(F::mul(k, F::enc((u64)1 << SHIFTS[i]))));
}

// ---- the gadget generators: operands are arbitrary targets, in the order generator_schedule.hpp lists them (dependencies, then
// outputs); the counts are the schedule's, checked against the kind there.
template <class F>
GB_HD void gen_equality(const Io<F>& io) {   // x, y -> equal, inv
    const bool equal = io.raw(0) == io.raw(1);
    io.put(0, (typename F::T)(equal ? 1 : 0));
    if (equal) io.put(1, 0);
    else io.out(1, F::inv(F::sub(io.in(0), io.in(1))));
}

template <class F>
GB_HD void gen_nonzero_test(const Io<F>& io) {   // to_test -> dummy
    if (io.raw(0) == 0) io.put(0, 1);
    else io.out(0, F::inv(io.in(0)));
}

template <class F>
GB_HD void gen_quotient_or_zero(const Io<F>& io) {   // numerator, denominator -> quotient
    if (io.raw(1) == 0) io.put(0, 0);   // compared before the inversion: pow(0, p - 2) is 0 as well, but says nothing
    else io.out(0, F::mul(io.in(0), F::inv(io.in(1))));
}

template <class F>
GB_HD void gen_quotient_extension(const Io<F>& io) {   // numerator[D], denominator[D] -> quotient[D]
    typedef typename F::E E;
    constexpr u32 D = F::D;
    E num = F::ezero(), den = F::ezero();
    bool zero = true;
#pragma unroll
    for (u32 k = 0; k < D; k++) {
        F::set_coord(num, k, io.in(k));
        zero = zero && io.raw(D + k) == 0;
        F::set_coord(den, k, io.in(D + k));
    }
    if (zero) {   // num / dem panics in the reference
        report(io.err, ERR_DIVIDE_BY_ZERO, io.op.record, io.args[io.op.in_off + D]);
        return;
    }
    const E q = F::emul(num, F::einv(den));
#pragma unroll
    for (u32 k = 0; k < D; k++) io.out(k, F::coord(q, k));
}

template <class F>
GB_HD void gen_split(const Io<F>& io) {   // integer -> bits, little-endian
    u64 v = (u64)io.raw(0);
    for (u32 i = 0; i < io.op.num_out; i++) {
        io.put(i, (typename F::T)(v & 1));
        v >>= 1;
    }
    if (v) report(io.err, ERR_SPLIT_TOO_LARGE, io.op.record, io.args[io.op.in_off]);
}

template <class F>
GB_HD void gen_wire_split(const Io<F>& io) {   // integer -> one sum of num_limbs bits per BaseSumGate
    const u32 limbs = io.op.p0;
    u64 v = (u64)io.raw(0);
    for (u32 i = 0; i < io.op.num_out; i++) {
        u64 t = v;
        if (limbs < 64) {   // with 64 limbs or more the first sum takes the whole word; the shift would be undefined
            t = v & (((u64)1 << limbs) - 1);
            v >>= limbs;
        } else {
            v = 0;
        }
        io.put(i, (typename F::T)t);
    }
    if (v) report(io.err, ERR_SPLIT_TOO_LARGE, io.op.record, io.args[io.op.in_off]);
}

template <class F>
GB_HD void gen_low_high(const Io<F>& io) {   // integer -> low, high; n_log <= 63 (the schedule's check)
    const u64 v = (u64)io.raw(0);
    io.put(0, (typename F::T)(v & (((u64)1 << io.op.p0) - 1)));
    io.put(1, (typename F::T)(v >> io.op.p0));
}

template <class F>
GB_HD void gen_base_sum(const Io<F>& io) {   // limbs -> sum, folded from the last limb down in field arithmetic
    typedef typename F::T T;
    const T base = F::enc((u64)io.op.p0 % F::ORDER);
    T acc = F::zero();
    for (u32 i = io.op.num_in; i-- > 0;) {
        const u64 limb = (u64)io.raw(i);
        if (limb > 1) {   // get_bool_target
            report(io.err, ERR_NOT_BOOLEAN, io.op.record, io.args[io.op.in_off + i]);
            return;
        }
        acc = F::add(F::mul(acc, base), limb ? F::one() : F::zero());
    }
    io.out(0, acc);
}

// ---- generator programs (generator_ops.hpp; include/goldibear_gpu.h gives the words)
// sqrt as examples/square_root.rs:185-219 writes it - Euler's criterion, then Tonelli-Shanks with z = two_adic_generator(S),
// S the field's two-adicity - on device-form values.  The root is the one these steps yield; false: x is no residue.  Every loop
// is bounded by S: v falls in every round, and a residue's b reaches one within v squarings.
template <class F>
GB_HD bool field_sqrt(typename F::T x, typename F::T* root) {
    typedef typename F::T T;
    constexpr u32 S = F::TWO_ADICITY;
    constexpr u64 t = (F::ORDER - 1) >> S;
    *root = x;
    if (x == F::zero()) return true;
    if (F::pow(x, (F::ORDER - 1) / 2) != F::one()) return false;
    T z = F::two_adic_generator(S), w = F::pow(x, (t - 1) / 2);
    T r = F::mul(w, x), b = F::mul(r, w);
    u32 v = S;
    for (u32 round = 0; round < S && b != F::one(); round++) {
        u32 k = 0;
        for (T b2k = b; k < v && b2k != F::one(); k++) b2k = F::mul(b2k, b2k);
        if (k >= v) return false;   // (not reached for a residue)
        w = z;
        for (u32 i = 0; i + k + 1 < v; i++) w = F::mul(w, w);
        z = F::mul(w, w);
        b = F::mul(b, z);
        r = F::mul(r, w);
        v = k;
    }
    *root = r;
    return true;
}

// what run_op needs to run a program generator: the tables of DeviceSchedule and this lane's register file (gates::LdsRegs on the
// device, gates::ArrayRegs on the host).  NoPrograms: a schedule without program generators - a GEN_PROGRAM op there is the
// caller's mistake.  Host code reports ERR_NO_PROGRAM_TABLES; the kernels without programs hold no code for it, and
// generator_schedule.hpp device_schedule refuses on the host to hand them a schedule with such an op.
struct NoPrograms {};
template <class R>
struct Programs {
    const ProgramHeader* headers;
    const uint64_t *instrs, *lits, *row_constants;
    R regs;
};

// the integer operations GP_IDIV .. GP_LT on the canonical representatives a, b in [0, p) of two device-form values.  Every
// result is <= a or is 0 or 1, so it is canonical as it stands and F::enc takes it without a reduction.  BabyBear's
// representatives are below 2^31 and stay in 32-bit words; Goldilocks' 64-bit quotient is the compiler's expansion (gfx950 has no
// 64-bit divide), the remainder a - q * b.  false: IDIV or IREM by zero, and nothing was divided.
template <class F>
GB_HD bool gen_integer_op(u32 opcode, typename F::T x, typename F::T y, typename F::T* res) {
    typedef typename std::conditional<sizeof(typename F::T) == 4, u32, u64>::type W;
    const W a = (W)F::dec(x), b = (W)F::dec(y);
    W r;
    switch (opcode) {
        case GP_IDIV:
        case GP_IREM: {
            if (b == 0) return false;
            const W q = a / b;
            r = opcode == GP_IDIV ? q : a - q * b;
            break;
        }
        // a shift by the word's width or more is no C++ shift: a < 2^(8 sizeof(W)), so the result is 0 from there on (for
        // BabyBear from 32 on, which holds the 64 of the definition)
        case GP_SHR: r = b >= 8 * sizeof(W) ? 0 : a >> b; break;
        case GP_AND: r = a & b; break;
        default: r = a < b ? 1 : 0; break;   // GP_LT
    }
    *res = F::enc((u64)r);
    return true;
}

// the interpreter: the operand decode of gates::run_program; space 1 is the dependencies, space 2 the row's constants, OUT ends in
// io.put, so store-or-compare and OUT_SKIP are those of every other generator.  An error ends the program: its outputs stay as
// they are and the error word ends the proof.  (A program's error names no class: OUT_SKIP in the class word.)
template <class F, class R>
GB_HD void gen_program(const Io<F>& io, const Programs<R>& pr) {
    typedef typename F::T T;
    const ProgramHeader& h = pr.headers[io.op.p0];
    const uint64_t* ins = pr.instrs + h.instr_off;
    const uint64_t* lits = pr.lits + h.lit_off;
    const uint64_t* konst = pr.row_constants + io.op.p1;
    auto load = [&](u32 o) -> T {
        const u32 i = gates::prog_index(o);
        switch (gates::prog_space(o)) {
            case gates::PROG_REG: return pr.regs.get(i);
            case gates::PROG_WIRE: return io.in(i);
            case gates::PROG_CONST: return F::enc(konst[i]);
            default: return (T)lits[i];
        }
    };
    u32 next_out = 0;
    for (u32 pc = 0; pc < h.num_instrs; pc++) {
        const u64 w = ins[pc];
        const T a = load(gates::prog_operand(w, 0));
        T res = a;
        const u32 opcode = gen_program_opcode(w);
        switch (opcode) {
            case GP_IDIV:
            case GP_IREM:
            case GP_SHR:
            case GP_AND:
            case GP_LT:
                if (!gen_integer_op<F>(opcode, a, load(gates::prog_operand(w, 1)), &res)) {
                    report(io.err, ERR_INTEGER_DIVIDE_BY_ZERO, io.op.record, OUT_SKIP);
                    return;
                }
                break;
            case GP_ADD: res = F::add(a, load(gates::prog_operand(w, 1))); break;
            case GP_SUB: res = F::sub(a, load(gates::prog_operand(w, 1))); break;
            case GP_MUL: res = F::mul(a, load(gates::prog_operand(w, 1))); break;
            case GP_OUT: io.out(next_out++, a); continue;
            case GP_INV:
                if (a == F::zero()) {
                    report(io.err, ERR_DIVIDE_BY_ZERO, io.op.record, OUT_SKIP);
                    return;
                }
                res = F::inv(a);
                break;
            case GP_INV_OR_ZERO: res = F::inv(a); break;   // pow(0, p - 2) = 0
            case GP_IS_ZERO: res = a == F::zero() ? F::one() : F::zero(); break;
            default:   // GP_SQRT
                if (!field_sqrt<F>(a, &res)) {
                    report(io.err, ERR_NO_SQUARE_ROOT, io.op.record, OUT_SKIP);
                    return;
                }
                break;
        }
        pr.regs.set(gates::prog_dst(w), res);
    }
}

template <class F, class P = NoPrograms>
GB_HD void run_op(const Op& op, const u32* args, typename F::T* values, u32* err, const P& programs = P()) {
    typedef typename F::T T;
    const Io<F> io{op, args, values, err};
    switch (op.kind) {
        case GEN_PROGRAM:
            if constexpr (!std::is_same<P, NoPrograms>::value) gen_program<F>(io, programs);
#if !defined(__HIP_DEVICE_COMPILE__)
            else report(err, ERR_NO_PROGRAM_TABLES, op.record, OUT_SKIP);
#endif
            break;
        case GEN_ARITHMETIC:
            io.out(0, F::add(F::mul(F::mul(io.in(0), io.in(1)), F::enc(op.k[0])), F::mul(io.in(2), F::enc(op.k[1]))));
            break;
        case GEN_ARITHMETIC_EXTENSION: gen_arithmetic_extension<F>(io, true); break;
        case GEN_MUL_EXTENSION: gen_arithmetic_extension<F>(io, false); break;
        case GEN_CONSTANT: io.put(0, (T)op.k[0]); break;
        case GEN_COPY: io.put(0, io.raw(0)); break;
        case GEN_BASE_SPLIT: gen_base_split<F>(io); break;
        case GEN_REDUCING: gen_reducing<F>(io, false); break;
        case GEN_REDUCING_EXTENSION: gen_reducing<F>(io, true); break;
        case GEN_RANDOM_ACCESS: gen_random_access<F>(io); break;
        case GEN_POSEIDON_MDS:
            if constexpr (F::TAG == 0) gen_poseidon_mds<F>(io);
            break;
        case GEN_COSET_INTERPOLATION: gen_coset_interpolation<F>(io); break;
        case GEN_EXPONENTIATION: gen_exponentiation<F>(io); break;
        case GEN_POSEIDON:
            if constexpr (F::TAG == 0) gen_poseidon(io);
            break;
        case GEN_POSEIDON2_BABYBEAR:
            if constexpr (F::TAG == 1) gen_poseidon2_bb(io);
            break;
        case GEN_ADD_MANY: {
            T sum = F::zero();
            for (u32 j = 0; j < op.p0; j++) sum = F::add(sum, io.in(j));
            io.out(0, sum);
            break;
        }
        case GEN_APPLY_MAT4: gen_apply_mat4<F>(io); break;
        case GEN_POSEIDON2_INTERNAL:
            if constexpr (F::TAG == 1) gen_poseidon2_internal<F>(io);
            break;
        case GEN_EQUALITY: gen_equality<F>(io); break;
        case GEN_NONZERO_TEST: gen_nonzero_test<F>(io); break;
        case GEN_QUOTIENT_OR_ZERO: gen_quotient_or_zero<F>(io); break;
        case GEN_QUOTIENT_EXTENSION: gen_quotient_extension<F>(io); break;
        case GEN_SPLIT: gen_split<F>(io); break;
        case GEN_WIRE_SPLIT: gen_wire_split<F>(io); break;
        case GEN_LOW_HIGH: gen_low_high<F>(io); break;
        case GEN_BASE_SUM: gen_base_sum<F>(io); break;
        default: break;
    }
}

#if defined(__HIPCC__)
// The program tables as a kernel argument.  PROGRAMS = false is the kernel of a schedule without program generators: no LDS, and
// no code for GEN_PROGRAM (the host keeps such an op away from it, generator_schedule.hpp device_schedule: a report here costs the
// chain kernels registers, 180 -> 184 and 125 -> 127 VGPRs).  PROGRAMS = true: a program's registers are indexed at run time, so they live in dynamic LDS
// and not in a per-lane array (which would go to scratch), [program_regs][GROUP] words, a register's row lane-consecutive, as in
// k_gate_programs; a lane only ever touches its own words, so the chain kernel's barrier has nothing to do with them.
struct ProgramTables {
    const ProgramHeader* headers = nullptr;
    const uint64_t *instrs = nullptr, *lits = nullptr, *row_constants = nullptr;
};
template <class F, bool PROGRAMS>
__device__ __forceinline__ void run_scheduled_op(const Op& op, const u32* args, typename F::T* values, u32* err, const ProgramTables& pt) {
    if constexpr (PROGRAMS) {
        typedef typename F::T T;
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_generator_regs[];
        const Programs<gates::LdsRegs<T>> pr{pt.headers, pt.instrs, pt.lits, pt.row_constants,
                                             gates::LdsRegs<T>{reinterpret_cast<T*>(smem_generator_regs) + threadIdx.x, GROUP}};
        run_op<F>(op, args, values, err, pr);
    } else {
        run_op<F>(op, args, values, err);
    }
}

// one thread per generator of a level
template <class F, bool PROGRAMS = false>
__global__ __launch_bounds__(GROUP) void k_generate_level(const Op* __restrict__ ops, const u32* __restrict__ args, u32 first, u32 count,
                                                          typename F::T* values, u32* err, ProgramTables pt = ProgramTables()) {
    const u32 i = blockIdx.x * GROUP + threadIdx.x;
    if (i < count) run_scheduled_op<F, PROGRAMS>(ops[first + i], args, values, err, pt);
}

// ONE workgroup walks levels first_level .. first_level + num_levels of level_off, each at most GROUP wide, with a barrier
// between levels: __syncthreads() is a workgroup-scope release, the barrier and a workgroup-scope acquire, which is all a
// hand-off inside one workgroup - one CU, one vector L1 - needs.  Nothing is handed to another workgroup.
template <class F, bool PROGRAMS = false>
__global__ __launch_bounds__(GROUP) void k_generate_chain(const Op* __restrict__ ops, const u32* __restrict__ args,
                                                          const u32* __restrict__ level_off, u32 first_level, u32 num_levels,
                                                          typename F::T* values, u32* err, ProgramTables pt = ProgramTables()) {
    for (u32 l = 0; l < num_levels; l++) {
        const u32 lo = level_off[first_level + l], hi = level_off[first_level + l + 1];
        for (u32 i = lo + threadIdx.x; i < hi; i += GROUP) run_scheduled_op<F, PROGRAMS>(ops[i], args, values, err, pt);
        __syncthreads();
    }
}

// values[cls[i]] = in[i] for the inputs that are the first of their class (the host has compared the others)
template <class F>
__global__ __launch_bounds__(GROUP) void k_scatter_inputs(const u32* __restrict__ cls, const typename F::T* __restrict__ in, u32 count,
                                                          typename F::T* values) {
    const u32 i = blockIdx.x * GROUP + threadIdx.x;
    if (i < count && cls[i] != OUT_SKIP) values[cls[i]] = in[i];
}

// what the host needs before the first challenge, in one block: the public inputs' values, then the error word
template <class F>
__global__ __launch_bounds__(GROUP) void k_gather_public(const u32* __restrict__ pi_cls, u32 count, const typename F::T* values,
                                                         const u32* err, u64* out) {
    const u32 i = blockIdx.x * GROUP + threadIdx.x;
    if (i < count) out[i] = (u64)values[pi_cls[i]];
    if (i < ERROR_WORDS) out[count + i] = err[i];
}

// the launches of one generation pass on `stream`; `values` holds the inputs, everything else zero; err is zero.  A schedule
// without program generators (d.program_regs == 0) launches the kernels without programs and no LDS.
template <class F, bool PROGRAMS>
inline void launch_generators_as(const DeviceSchedule& d, const Launch* launches, size_t num_launches, const u32* level_off_host,
                                 typename F::T* values, u32* err, hipStream_t stream) {
    const size_t lds = PROGRAMS ? (size_t)d.program_regs * GROUP * sizeof(typename F::T) : 0;
    const ProgramTables pt{d.programs, d.program_instrs, d.program_lits, d.row_constants};
    for (size_t k = 0; k < num_launches; k++) {
        const Launch& L = launches[k];
        if (L.chain) {
            hipLaunchKernelGGL((k_generate_chain<F, PROGRAMS>), dim3(1), dim3(GROUP), lds, stream, d.ops, d.args, d.level_off, L.first_level,
                               L.num_levels, values, err, pt);
        } else {
            const u32 first = level_off_host[L.first_level], count = level_off_host[L.first_level + 1] - first;
            hipLaunchKernelGGL((k_generate_level<F, PROGRAMS>), dim3((count + GROUP - 1) / GROUP), dim3(GROUP), lds, stream, d.ops, d.args, first,
                               count, values, err, pt);
        }
    }
}
template <class F>
inline void launch_generators(const DeviceSchedule& d, const Launch* launches, size_t num_launches, const u32* level_off_host,
                              typename F::T* values, u32* err, hipStream_t stream) {
    if (d.program_regs) launch_generators_as<F, true>(d, launches, num_launches, level_off_host, values, err, stream);
    else launch_generators_as<F, false>(d, launches, num_launches, level_off_host, values, err, stream);
}
#endif

}  // namespace gen
}  // namespace gbk

// The checks of one FRI query round (fri/verifier.rs:121-250, hash/merkle_proofs.rs:54-76), written once over the field traits and
// a hasher policy, for the host verifier (verifier_host.inc: HostHash<F>) and the batch verifier's kernels (kernels_verify.hip:
// Sponge<F>) - the way gates.hpp serves the quotient kernel and gb_verify.  Plain integer C++ apart from the qualifiers:
// tests/host_shim/verify_query.cpp compiles it for the CPU.
//
// Words are read where they stand in the proof bytes: canonical, little-endian, at ANY byte offset (a path's length prefix is one
// byte), so every operand is a byte pointer and load_word copies.  The caller has checked that the words are below the order.
//
// A hasher policy H holds one sponge state of F::SPONGE_W words:
//   void set_canonical(int i, T canonical);  void permute();  T out(int i) -> canonical
// The device's permutation is wave-wide, so merkle_path_ok's control flow depends only on (num_words, path_len): lanes of one
// wave must share them.
#pragma once
#include "field_traits.hpp"

namespace gbk {
namespace vq {

// Where a check stands inside its query round: the order fri/verifier.rs reaches them in (verify_fri_parsed).  The batch verifier
// reduces a proof's failures with a minimum over (query round, position).
GB_HD u32 pos_initial_path(u32 oracle) { return oracle; }
GB_HD u32 pos_consistency(u32 num_oracles, u32 layer) { return num_oracles + 2 * layer; }
GB_HD u32 pos_layer_path(u32 num_oracles, u32 layer) { return num_oracles + 2 * layer + 1; }
GB_HD u32 pos_final(u32 num_oracles, u32 num_layers) { return num_oracles + 2 * num_layers; }
static constexpr u32 POS_BITS = 16;
GB_HD u64 fail_key(u32 query_round, u32 pos) { return ((u64)query_round << POS_BITS) | pos; }
static constexpr u64 KEY_NONE = ~(u64)0;

template <class F>
GB_HD typename F::T load_word(const unsigned char* p) {
    typename F::T v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
}
template <class F>
GB_HD typename F::E load_ext(const unsigned char* p) {   // D canonical words -> device form
    typename F::E e = F::ezero();
    for (u32 k = 0; k < F::D; k++) F::set_coord(e, k, F::enc(load_word<F>(p + k * sizeof(typename F::T))));
    return e;
}
template <class F>
GB_HD bool eeq(const typename F::E& a, const typename F::E& b) {
    bool ok = true;
    for (u32 k = 0; k < F::D; k++) ok = ok && F::coord(a, k) == F::coord(b, k);
    return ok;
}
GB_HD u64 rev_bits(u64 x, u32 bits) {
    u64 r = 0;
    for (u32 i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}

// hash_or_noop of a leaf (plonk/config.rs:70-84) into cur[HW]; word(i): the leaf's i-th canonical word
template <class F, class H, class WordAt>
GB_HD void leaf_digest(H& h, u32 num_words, WordAt word, typename F::T* cur) {
    typedef typename F::T T;
    constexpr u32 HW = F::H, W = F::SPONGE_W;
    if (num_words <= HW) {
#pragma unroll
        for (u32 i = 0; i < HW; i++) cur[i] = i < num_words ? word(i) : (T)0;
    } else {   // hash_no_pad: overwrite mode, rate 8
#pragma unroll
        for (u32 i = 0; i < W; i++) h.set_canonical((int)i, (T)0);
        for (u32 k0 = 0; k0 < num_words; k0 += 8) {
#pragma unroll
            for (u32 k = 0; k < 8; k++)
                if (k0 + k < num_words) h.set_canonical((int)k, word(k0 + k));
            h.permute();
        }
#pragma unroll
        for (u32 i = 0; i < HW; i++) cur[i] = h.out((int)i);
    }
}
// two_to_one (hash/hashing.rs:76-96) of cur and its sibling into cur; right: cur is the right child.  sibling(i): canonical word i
template <class F, class H, class SiblingAt>
GB_HD void two_to_one(H& h, typename F::T* cur, SiblingAt sibling, bool right) {
    typedef typename F::T T;
    constexpr u32 HW = F::H, W = F::SPONGE_W;
#pragma unroll
    for (u32 i = 0; i < HW; i++) {
        const T s = sibling(i);
        h.set_canonical((int)i, right ? s : cur[i]);
        h.set_canonical((int)(HW + i), right ? cur[i] : s);
    }
#pragma unroll
    for (u32 i = 2 * HW; i < W; i++) h.set_canonical((int)i, (T)0);
    h.permute();
#pragma unroll
    for (u32 i = 0; i < HW; i++) cur[i] = h.out((int)i);
}

// verify_merkle_proof_to_cap (hash/merkle_proofs.rs:54-76): hash_or_noop of the leaf, two_to_one up `path_len` siblings, then the
// cap entry that is left of the index.
template <class F, class H>
GB_HD bool merkle_path_ok(H& h, const unsigned char* leaf, u32 num_words, u64 index, const unsigned char* siblings, u32 path_len,
                          const typename F::T* cap) {
    typedef typename F::T T;
    constexpr u32 HW = F::H;
    constexpr size_t TS = sizeof(T);
    T cur[HW];
    leaf_digest<F>(h, num_words, [leaf](u32 i) { return load_word<F>(leaf + (size_t)i * TS); }, cur);
    for (u32 l = 0; l < path_len; l++) {
        const unsigned char* sib = siblings + (size_t)l * HW * TS;
        two_to_one<F>(h, cur, [sib](u32 i) { return load_word<F>(sib + i * TS); }, (index & 1) != 0);   // odd: cur is the right child
        index >>= 1;
    }
    bool ok = true;
#pragma unroll
    for (u32 i = 0; i < HW; i++) ok = ok && cur[i] == cap[index * HW + i];
    return ok;
}

// x = g * w_N^rev(x_index) (fri/verifier.rs:177-180), device form
template <class F>
GB_HD typename F::T subgroup_x(u32 lgN, u64 x_index) {
    return F::mul(F::generator(), F::pow(F::two_adic_generator(lgN), rev_bits(x_index, lgN)));
}

// fri_combine_initial (fri/verifier.rs:121-165) with PrecomputedReducedOpenings: per batch b of `sizes[b]` polynomials opened at
// points[b], reduce the opened row values with alpha, subtract red_open[b] = reduce(openings), divide by x - point;
// alpha_shift[b] = alpha^sizes[b].  poly(b, i): the canonical word of batch b's i-th polynomial in the opened rows.
template <class F, class PolyAt>
GB_HD typename F::E combine_initial(u32 num_batches, const u32* sizes, const typename F::E* points, const typename F::E* red_open,
                                    const typename F::E* alpha_shift, typename F::E alpha, typename F::T x, PolyAt poly) {
    typedef typename F::E E;
    E sum = F::ezero();
    for (u32 b = 0; b < num_batches; b++) {
        E acc = F::ezero();   // ReducingFactor::reduce (util/reducing.rs:56-59)
        for (u32 i = sizes[b]; i-- > 0;) acc = F::eadd(F::emul(alpha, acc), F::efrom(F::enc(poly(b, i))));
        const E term = F::emul(F::esub(acc, red_open[b]), F::einv(F::esub(F::efrom(x), points[b])));
        sum = F::eadd(F::emul(alpha_shift[b], sum), term);   // alpha.shift(sum) + numerator / denominator
    }
    return sum;
}

// compute_evaluation (fri/verifier.rs:23-49): the polynomial of degree < arity through the coset's values (eval(k): the k-th
// value as stored, bit-reversed order) at beta.  The coset is c <g>, so its vanishing polynomial is X^arity - c^arity and the
// barycentric weight of x_i is 1 / (arity x_i^(arity-1)) = x_i / (arity c^arity):
//   P(beta) = (beta^arity - c^arity) / (arity c^arity) * sum_i eval(rev i) x_i / (beta - x_i)
// - arity inversions' worth of work instead of the arity^2 products of interpolate(); field arithmetic is exact, so the value
// is the same.  The denominators are inverted G at a time (one inversion and 3 (G - 1) products per group).  beta on the coset
// (no inverse) returns that point's value.
template <class F, class EvalAt>
GB_HD typename F::E compute_evaluation(typename F::T x, u64 within, u32 arity_bits, typename F::E beta, EvalAt eval) {
    typedef typename F::T T;
    typedef typename F::E E;
    // (the quartic extension in groups of four: at eight the unrolled group outgrows the compiler's full-unroll budget, the loops
    // stay rolled and d / pre go to scratch - 272 bytes a lane in every BabyBear queries kernel)
    constexpr u32 G = F::D > 2 ? 4 : 8;
    const u32 arity = 1u << arity_bits;
    const E one = F::efrom(F::one());
    const T g = F::two_adic_generator(arity_bits);
    const T coset_start = F::mul(x, F::pow(g, arity - rev_bits(within, arity_bits)));
    E sum = F::ezero();
    T xp = coset_start;
    for (u32 i0 = 0; i0 < arity; i0 += G) {
        E d[G], pre[G];
        T xs[G];
        E run = one;
#pragma unroll
        for (u32 k = 0; k < G; k++) {
            const bool live = i0 + k < arity;
            xs[k] = xp;
            d[k] = live ? F::esub(beta, F::efrom(xp)) : one;
            if (live && eeq<F>(d[k], F::ezero())) return eval((u32)rev_bits(i0 + k, arity_bits));
            if (live) xp = F::mul(xp, g);
            pre[k] = run;
            run = F::emul(run, d[k]);
        }
        E inv = F::einv(run);
#pragma unroll
        for (u32 kk = G; kk-- > 0;) {
            const E dinv = F::emul(inv, pre[kk]);
            inv = F::emul(inv, d[kk]);
            if (i0 + kk < arity) sum = F::eadd(sum, F::emul(F::escale(eval((u32)rev_bits(i0 + kk, arity_bits)), xs[kk]), dinv));
        }
    }
    T ca = coset_start;   // c^arity
    E ba = beta;          // beta^arity
    for (u32 i = 0; i < arity_bits; i++) { ca = F::mul(ca, ca); ba = F::emul(ba, ba); }
    const T w = F::inv(F::mul(F::enc(arity), ca));
    return F::emul(F::escale(F::esub(ba, F::efrom(ca)), w), sum);
}

// the final polynomial at the folded point (fri/verifier.rs:240-247); coeff(i) in device form
template <class F, class CoeffAt>
GB_HD typename F::E final_eval(u32 len, typename F::T x, CoeffAt coeff) {
    typename F::E acc = F::ezero();
    for (u32 i = len; i-- > 0;) acc = F::eadd(F::escale(acc, x), coeff(i));
    return acc;
}

// The arithmetic of one query round after its initial evaluation: per layer the consistency check (fri/verifier.rs:213-216) and
// the fold, then the final polynomial.  step_row(layer): the layer's opened coset, D << arity_bits canonical words; beta(layer),
// coeff(i) in device form.  Returns the position of the first check that fails, or ~0u.  between(layer, coset_index) runs after a
// layer's consistency check and fold, where the host verifier checks that layer's Merkle path; it returns false to stop there.
template <class F, class StepRow, class BetaAt, class CoeffAt, class Between>
GB_HD u32 fold_checks(u32 num_oracles, u32 num_layers, const u32* arity_bits, u64 x_index, typename F::T x, typename F::E old_eval,
                      u32 final_len, StepRow step_row, BetaAt beta, CoeffAt coeff, Between between) {
    typedef typename F::T T;
    typedef typename F::E E;
    u64 xi = x_index;
    for (u32 li = 0; li < num_layers; li++) {
        const u32 ab = arity_bits[li];
        const u64 coset_index = xi >> ab, within = xi & (((u64)1 << ab) - 1);
        const unsigned char* row = step_row(li);
        auto eval = [row](u32 k) { return load_ext<F>(row + (size_t)k * F::D * sizeof(T)); };
        if (!eeq<F>(eval((u32)within), old_eval)) return pos_consistency(num_oracles, li);
        old_eval = compute_evaluation<F>(x, within, ab, beta(li), eval);
        if (!between(li, coset_index)) return pos_layer_path(num_oracles, li);
        for (u32 i = 0; i < ab; i++) x = F::mul(x, x);
        xi = coset_index;
    }
    const E fin = final_eval<F>(final_len, x, coeff);
    return eeq<F>(fin, old_eval) ? ~0u : pos_final(num_oracles, num_layers);
}

}  // namespace vq
}  // namespace gbk

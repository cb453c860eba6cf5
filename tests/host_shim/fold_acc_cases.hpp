// The chains that tests/host_shim/fold_acc.cpp (CPU) and tests/device/fold_acc.hip (GPU) both run through csrc/fold_acc.hpp's
// FoldAcc<GlF> / FoldAcc<BbF> - one chain = `FoldAcc<F> s; for t < len: s.acc(c[t], a[t]); out = s.finish()` - and the five-limb values
// they feed to gl::fold160 directly.  Everything expected is computed HERE from exact integers: a chain's sum of products in a
// five-limb (160-bit) integer written plainly, then `sum mod p` (Goldilocks) or `sum 2^-32 mod p` (BabyBear), compared as words.
// Nothing comes from the csrc headers.  Operands are words in [0, p): the domain fold_acc.hpp states.
//
// Why chosen sums: on the LDE values the proofs feed them, the unreduced sums are random words, and a running sum that stops on a limb
// boundary, a BabyBear middle word in [p, 2p) or [2p, 2^32) beside a chosen low word, or a fold160 with carry and borrow both set
// are 2^-32 events.  So a "pulled" chain starts from the SUM it must stand at before finish() (or at some point mid-chain) and builds
// terms that reach it: an optional prefix of edge-valued or seeded terms that fit under the target, then terms (p - 1)(p - 1) while
// the rest is at least (p - 1)^2, then fix-up terms c * m against the multipliers m = 2^63, 2^32, 1 (BabyBear 2^30, 1), c =
// min(rest / m, p - 1): at most 3 + 1 + 1 (BabyBear 3 + 1) of them.  reach() then requires the exact sum of the chain's terms to BE
// the target and every word to be < p; a failure ends the program with status 3.
// A chain has at most MAX_TERMS = 4096 terms (fold_acc.hpp: FOLD_ACC_MAX_TERMS).  The largest sum that allows is 4096 (p - 1)^2:
// top limb 4095 (Goldilocks l4; low limbs 0xffffe000'00001000'00000000'00000000) and 900 (BabyBear hi, low words 0) - reached by
// the all-(p - 1)^2 chain of the edge family only.  A chosen pattern of low limbs takes the largest top limb at which reach() still
// fits 4096 terms ("top": the fix-ups cost up to five terms, so at most eight below the cap - the generator checks); gl::fold160 gets
// every pattern with r4 = 4095 and 2^31 directly.
//
// fold160's branches, from gl_field.hpp (r0 r1 hl hh r4 = l0..l4):  cs = carry of hl + hh;  c1 = carry of r1 + hl (one 2^64 = +EPS);
// bw = r0 < lo32(hl + hh);  B = borrow of (r1 + hl) - (cs + r4) - bw (one -2^64 = -EPS).  (c1 - B) EPS enters as (cl, ch):
//   c1 only: cl = 0xffffffff, the final d0 + cl carries unless d0 = 0;    B only: mC - mB borrows ("cl borrowing"), cl = 1,
//   ch = 0xffffffff, d0 + cl carries only for d0 = 0xffffffff;            both or neither: cl = ch = 0.
// c1 needs l1 + l2 >= 2^32; B needs l1 + l2 (mod 2^32) below cs + l4 + bw - small words after a wrap, or any l4 above them; "both"
// needs a wrap of l1 + l2 that lands below cs + l4 + bw, e.g. l1 = l2 = 0x80000000 with l4 >= 1.  The limb set of the targets,
// {0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff}^4, holds every one; the census counts them and the runners fail on a zero.
#pragma once
#include <map>

#include "register_dft_cases.hpp"

namespace fold_acc_cases {
namespace rc = register_dft_cases;
typedef rc::u64 u64;
typedef rc::u32 u32;
typedef rc::u128 u128;
using rc::generator_failed;

static constexpr u32 MAX_TERMS = 4096;

// a 160-bit unsigned integer as five 32-bit limbs, schoolbook
struct U160 {
    u32 l[5] = {0, 0, 0, 0, 0};
    static U160 limbs(u32 a0, u32 a1, u32 a2, u32 a3, u32 a4) {
        U160 r;
        r.l[0] = a0; r.l[1] = a1; r.l[2] = a2; r.l[3] = a3; r.l[4] = a4;
        return r;
    }
    static U160 of(u128 x) { return limbs((u32)x, (u32)(x >> 32), (u32)(x >> 64), (u32)(x >> 96), 0); }
    void add(const U160& b) {
        u64 carry = 0;
        for (int i = 0; i < 5; i++) {
            const u64 t = (u64)l[i] + b.l[i] + carry;
            l[i] = (u32)t;
            carry = t >> 32;
        }
        if (carry) generator_failed("U160 overflow");
    }
    void sub(const U160& b) {   // needs *this >= b
        u64 borrow = 0;
        for (int i = 0; i < 5; i++) {
            const u64 t = (u64)l[i] - b.l[i] - borrow;
            l[i] = (u32)t;
            borrow = (t >> 32) & 1;
        }
        if (borrow) generator_failed("U160 underflow");
    }
    int cmp(const U160& b) const {
        for (int i = 4; i >= 0; i--)
            if (l[i] != b.l[i]) return l[i] < b.l[i] ? -1 : 1;
        return 0;
    }
    u128 low128() const { return (u128)l[0] | (u128)l[1] << 32 | (u128)l[2] << 64 | (u128)l[3] << 96; }
    u64 mod(u64 p) const {
        u64 r = 0;
        for (int i = 4; i >= 0; i--) r = (u64)((((u128)r << 32) | l[i]) % p);
        return r;
    }
    U160 times(u32 k) const {
        U160 r;
        u64 carry = 0;
        for (int i = 0; i < 5; i++) {
            const u64 t = (u64)l[i] * k + carry;
            r.l[i] = (u32)t;
            carry = t >> 32;
        }
        if (carry) generator_failed("U160 overflow");
        return r;
    }
};

struct GlAcc : rc::Gl {
    static const char* name() { return "gl_fold_acc"; }
    static std::vector<int> multiplier_bits() { return {63, 32, 0}; }
    static u64 expected(const U160& sum) { return sum.mod(P); }
    static std::vector<u64> operand_words() { return edges(); }   // canonical value = word
};
struct BbAcc : rc::Bb {
    static const char* name() { return "bb_fold_acc"; }
    static std::vector<int> multiplier_bits() { return {30, 0}; }
    static u64 expected(const U160& sum) {   // sum 2^-32 mod p
        static const u64 rinv = rc::powmod((1ULL << 32) % P, P - 2, P);
        return rc::mulmod(sum.mod(P), rinv, P);
    }
    static std::vector<u64> operand_words() {   // the Montgomery words of the carry-edge values
        std::vector<u64> w;
        for (u64 e : edges()) rc::push_unique(w, (u64)word(e), P);
        return w;
    }
};

enum Kind { PULLED = 0, EDGE = 1, RANDOM = 2 };

// chain i: terms [off[i], off[i + 1]) of c / a; `expect[i]` the word finish() must return
template <class F>
struct Chains {
    typedef typename F::W W;
    std::vector<u32> off{0};
    std::vector<W> c, a, expect;
    std::vector<unsigned char> kind;
    std::vector<std::pair<std::string, size_t>> census;   // class -> chains, in the order the classes were declared
    std::vector<U160> final_sum;                          // of every chain (the Goldilocks ones go to fold160 as well)
    size_t by_kind[3] = {0, 0, 0};
    size_t count() const { return expect.size(); }
    void declare(const std::string& cls) {
        for (auto& e : census)
            if (e.first == cls) return;
        census.emplace_back(cls, 0);
    }
    void tally(const std::string& cls) {
        declare(cls);
        for (auto& e : census)
            if (e.first == cls) e.second++;
    }
};

// what gl::fold160 does with a five-limb value, step by step as gl_field.hpp writes it: for the census only
struct Fold160Flags {
    bool cs, c1, bw, B, k1, k2;
    explicit Fold160Flags(const U160& s) {
        const u32 r0 = s.l[0], r1 = s.l[1], hl = s.l[2], hh = s.l[3], r4 = s.l[4];
        const u64 sh = (u64)hl + hh;
        const u32 s0 = (u32)sh;
        cs = sh >> 32;
        const u32 s1 = (u32)cs + r4;
        const u64 ah = (u64)r1 + hl;
        const u32 a1 = (u32)ah;
        c1 = ah >> 32;
        bw = r0 < s0;
        const u32 d0 = r0 - s0;
        B = (u64)a1 < (u64)s1 + (bw ? 1 : 0);
        const u32 mC = c1 ? 0xffffffffu : 0u, mB = B ? 0xffffffffu : 0u;
        k1 = mC < mB;
        const u32 cl = mC - mB;
        k2 = ((u64)d0 + cl) >> 32;
    }
    const char* branch() const {
        if (c1 && B) return "fold160_c1_and_B";
        if (c1) return k2 ? "fold160_c1_only_final_carry" : "fold160_c1_only_no_final_carry";
        if (B) return k2 ? "fold160_B_only_cl_borrows_final_carry" : "fold160_B_only_cl_borrows_no_final_carry";
        return "fold160_neither";
    }
};
inline void declare_fold160(std::vector<std::pair<std::string, size_t>>& census) {
    for (const char* cls : {"fold160_neither", "fold160_c1_only_final_carry", "fold160_c1_only_no_final_carry",
                            "fold160_B_only_cl_borrows_final_carry", "fold160_B_only_cl_borrows_no_final_carry", "fold160_c1_and_B",
                            "fold160_cs", "fold160_bw"})
        census.emplace_back(cls, 0);
}
inline void tally_fold160(std::vector<std::pair<std::string, size_t>>& census, const U160& s) {
    const Fold160Flags f(s);
    for (auto& e : census)
        if (e.first == f.branch() || (f.cs && e.first == "fold160_cs") || (f.bw && e.first == "fold160_bw")) e.second++;
}

template <class F>
struct Builder {
    typedef typename F::W W;
    Chains<F>& ch;
    U160 sum;
    const U160 max_product = U160::of((u128)(F::P - 1) * (F::P - 1));
    bool fired[4] = {false, false, false, false};   // the carry out of limb i of a running sum, on some term of this chain
    std::vector<std::string> classes;
    explicit Builder(Chains<F>& c) : ch(c) {}
    size_t terms() const { return ch.c.size() - ch.off.back(); }
    void term(u64 c, u64 a) {
        if (c >= F::P || a >= F::P) generator_failed(std::string(F::name()) + ": operand word outside [0, p)");
        ch.c.push_back((W)c);
        ch.a.push_back((W)a);
        const U160 p = U160::of((u128)c * a);
        u64 carry = 0;
        for (int i = 0; i < 4; i++) {
            carry = ((u64)sum.l[i] + p.l[i] + carry) >> 32;
            if (carry) fired[i] = true;
        }
        sum.add(p);
    }
    void cls(const std::string& c) { classes.push_back(c); }
    void end(Kind kind) {
        if (terms() > MAX_TERMS) generator_failed(std::string(F::name()) + ": a chain of more than MAX_TERMS terms");
        ch.off.push_back((u32)ch.c.size());
        ch.expect.push_back((W)F::expected(sum));
        ch.kind.push_back((unsigned char)kind);
        ch.by_kind[kind]++;
        ch.final_sum.push_back(sum);
        for (auto& c : classes) ch.tally(c);
        if (F::P >> 32) {   // Goldilocks: the carries of acc(), the branch of fold160 in finish()
            for (int i = 0; i < 4; i++)
                if (fired[i]) ch.tally("acc_carry_k" + std::to_string(i));
            tally_fold160(ch.census, sum);
        } else {            // BabyBear: the carry into hi, the range of the middle word in finish()
            if (fired[1]) ch.tally("acc_carry_into_hi");
            const char* mid = sum.l[1] < F::P ? "finish_mid_below_p" : sum.l[1] < 2 * F::P ? "finish_mid_in_p_2p" : "finish_mid_from_2p";
            ch.tally(mid);
            // finish() adds x = w0 2^-32, y = w1 mod p, z = hi 2^32: which of its two bb::add wrap
            const u64 x = F::expected(U160::limbs(sum.l[0], 0, 0, 0, 0)), y = sum.l[1] % F::P, z = rc::mulmod(sum.l[2], 1ULL << 32, F::P);
            const bool first = x + y >= F::P, second = (x + y) % F::P + z >= F::P;
            ch.tally(std::string(mid) + (first ? second ? "_both_adds_wrap" : "_first_add_wraps" : second ? "_second_add_wraps" : "_no_add_wraps"));
        }
        sum = U160();
        for (bool& f : fired) f = false;
        classes.clear();
    }
    // terms that bring the running sum to exactly `target` (>= the running sum): (p - 1)(p - 1) while the rest allows, then fix-ups
    void reach(const U160& target) {
        if (sum.cmp(target) > 0) generator_failed(std::string(F::name()) + ": target below the running sum");
        U160 rest = target;
        rest.sub(sum);
        while (rest.cmp(max_product) >= 0) {
            term(F::P - 1, F::P - 1);
            rest.sub(max_product);
            if (terms() > MAX_TERMS) generator_failed(std::string(F::name()) + ": target out of reach of MAX_TERMS terms");
        }
        u128 r = rest.low128();
        for (int bits : F::multiplier_bits()) {
            while (bits ? (r >> bits) != 0 : true) {
                const u128 q = r >> bits;
                const u64 c = q > F::P - 1 ? F::P - 1 : (u64)q;
                term(c, 1ULL << bits);
                r -= (u128)c << bits;
                if (!bits) break;   // the last fix-up is written even when it is zero
            }
        }
        if (r != 0 || sum.cmp(target) != 0) generator_failed(std::string(F::name()) + ": the chain does not sum to its target");
    }
    // up to n edge-valued (style 1) or seeded (style 2) terms that fit under `target`
    template <class Rng>
    void prefix(const U160& target, int style, int n, Rng& rng, const std::vector<u64>& E) {
        for (int i = 0; style && i < n; i++) {
            const u64 c = style == 1 ? E[rng() % E.size()] : rc::uniform(rng, F::P);
            const u64 a = style == 1 ? E[rng() % E.size()] : rc::uniform(rng, F::P);
            U160 next = sum;
            next.add(U160::of((u128)c * a));
            if (next.cmp(target) <= 0) term(c, a);
        }
    }
    // how many terms reach() would write from a zero sum
    size_t terms_to_reach(const U160& target) const {
        U160 rest = target;
        size_t n = 0;
        // rest / max_product by the top limbs first, so that this stays cheap: subtract 2^k multiples
        for (int k = 12; k >= 0; k--) {
            const U160 m = max_product.times(1u << k);
            while (rest.cmp(m) >= 0) { rest.sub(m); n += (size_t)1 << k; }
        }
        u128 r = rest.low128();
        for (int bits : F::multiplier_bits()) {
            while (bits ? (r >> bits) != 0 : true) {
                const u128 q = r >> bits;
                const u64 c = q > F::P - 1 ? F::P - 1 : (u64)q;
                n++;
                r -= (u128)c << bits;
                if (!bits) break;
            }
        }
        return n;
    }
};

// the largest value of limb `top` (<= cap) at which `low` + top 2^(32 top_limb) is within reach of MAX_TERMS terms
template <class F>
inline U160 with_top(Builder<F>& b, U160 low, int top_limb, u32 cap) {
    for (u32 v = cap;; v--) {
        low.l[top_limb] = v;
        if (b.terms_to_reach(low) <= MAX_TERMS) return low;
        if (v == 0) generator_failed(std::string(F::name()) + ": no top limb within reach");
    }
}

// A target stood at before finish(): no prefix, an edge-valued prefix, a seeded prefix (styles 0, 1, 2)
template <class F, class Rng>
inline void pulled_to(Builder<F>& b, const U160& target, const std::string& cls, int styles, Rng& rng, const std::vector<u64>& E) {
    for (int style = 0; style < styles; style++) {
        b.prefix(target, style, 4, rng, E);
        b.reach(target);
        b.cls(cls);
        b.end(PULLED);
    }
}

// edge-valued and random chains of every listed length; `share`: chains per length for the short ones
template <class F, class Rng>
inline void edge_and_random_chains(Builder<F>& b, Rng& rng, const std::vector<u64>& E) {
    const u64 p = F::P;
    const u32 lengths[] = {1, 2, 3, 4, 5, 16, 17, 123, MAX_TERMS};
    for (u32 len : lengths) {
        const std::string L = "length_" + std::to_string(len);
        // all (p - 1)(p - 1); all zeros; zero words against p - 1; largest and smallest products alternating (both phases)
        for (int pat = 0; pat < 6; pat++) {
            for (u32 t = 0; t < len; t++) {
                const bool big = pat == 4 ? t % 2 == 0 : t % 2 == 1;
                if (pat == 0) b.term(p - 1, p - 1);
                else if (pat == 1) b.term(0, 0);
                else if (pat == 2) b.term(0, p - 1);
                else if (pat == 3) b.term(p - 1, 0);
                else b.term(big ? p - 1 : t % 4 < 2 ? 0 : 1, big ? p - 1 : 1);
            }
            b.cls(L);
            b.cls(pat == 0 ? "edge_all_largest_products" : pat < 4 ? "edge_all_zero_products" : "edge_alternating_products");
            b.end(EDGE);
        }
        // 2^14 of each kind over the lengths: 2048 each for the seven short ones, 1984 of 123 terms, 64 of MAX_TERMS
        const size_t n = len == MAX_TERMS ? 64 : len == 123 ? 1984 : 2048;
        for (size_t i = 0; i < n; i++) {
            for (u32 t = 0; t < len; t++) b.term(E[rng() % E.size()], E[rng() % E.size()]);
            b.cls(L);
            b.end(EDGE);
        }
        for (size_t i = 0; i < n; i++) {
            for (u32 t = 0; t < len; t++) b.term(rc::uniform(rng, p), rc::uniform(rng, p));
            b.cls(L);
            b.end(RANDOM);
        }
    }
}

// the running sum stopped on a limb boundary MID-chain: limbs i..j all ones (fire = true) or limb i one short of it (fire = false),
// the limbs around them seeded, then the term 2^(32 i) - the carry out of limb i fires and runs through limb j, or fails to by one -
// then up to three seeded terms
template <class F, class Rng>
inline void mid_chain_boundaries(Builder<F>& b, int limbs, u32 top_cap, Rng& rng, const std::vector<u64>& E) {
    const u64 unit[4][2] = {{1, 1}, {1ULL << 32, 1}, {1ULL << 32, 1ULL << 32}, {1ULL << 63, 1ULL << 33}};   // c a = 2^(32 i)
    const u64 bb_unit[2][2] = {{1, 1}, {1ULL << 30, 4}};
    for (int i = 0; i < limbs; i++)
        for (int j = i; j < limbs; j++)
            for (int fire = 0; fire < 2; fire++)
                for (int rep = 0; rep < 64; rep++) {
                    U160 stop;
                    for (int k = 0; k < limbs; k++) stop.l[k] = (u32)rng();
                    stop.l[limbs] = (u32)(rng() % (top_cap + 1));
                    for (int k = i; k <= j; k++) stop.l[k] = 0xffffffffu;
                    if (!fire) stop.l[i] = 0xfffffffeu;
                    if (rep % 4 == 0)
                        for (int k = 0; k < i; k++) stop.l[k] = 0;
                    b.prefix(stop, rep % 3, 3, rng, E);
                    b.reach(stop);
                    if (limbs == 4) b.term(unit[i][0], unit[i][1]);
                    else b.term(bb_unit[i][0], bb_unit[i][1]);
                    U160 want = stop, one;
                    one.l[i] = 1;
                    want.add(one);
                    if (b.sum.cmp(want) != 0) generator_failed(std::string(F::name()) + ": mid-chain step");
                    for (int t = rep % 4; t > 0; t--) b.term(rc::uniform(rng, F::P), rc::uniform(rng, F::P));
                    b.cls(fire ? "mid_chain_carry_fires" : "mid_chain_carry_one_short");
                    b.cls(std::string(fire ? "mid_chain_fires_limbs_" : "mid_chain_short_limbs_") + std::to_string(i) + "_" + std::to_string(j));
                    b.end(PULLED);
                }
}

inline Chains<GlAcc> gl_chains() {
    typedef GlAcc F;
    const u64 p = F::P;
    Chains<F> ch;
    Builder<F> b(ch);
    std::mt19937_64 rng(rc::seed_of(F::name()));
    const std::vector<u64> E = F::operand_words();
    for (const char* cls : {"target_limbs_l4_0", "target_limbs_l4_1", "target_limbs_l4_2", "target_limbs_l4_top", "target_0_mod_p",
                            "target_1_mod_p", "target_p_minus_1_mod_p", "target_listed_sum", "mid_chain_carry_fires",
                            "mid_chain_carry_one_short", "acc_carry_k0", "acc_carry_k1", "acc_carry_k2", "acc_carry_k3",
                            "edge_all_largest_products", "edge_all_zero_products", "edge_alternating_products"})
        ch.declare(cls);
    for (int i = 0; i < 4; i++)
        for (int j = i; j < 4; j++)
            for (const char* f : {"mid_chain_fires_limbs_", "mid_chain_short_limbs_"}) ch.declare(f + std::to_string(i) + "_" + std::to_string(j));
    for (u32 len : {1u, 2u, 3u, 4u, 5u, 16u, 17u, 123u, MAX_TERMS}) ch.declare("length_" + std::to_string(len));
    declare_fold160(ch.census);
    // every combination of the limb values, l4 = 0, 1, 2 (three styles each) and the top value (one chain of ~4096 terms)
    const u32 V[6] = {0, 1, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (int i0 = 0; i0 < 6; i0++)
        for (int i1 = 0; i1 < 6; i1++)
            for (int i2 = 0; i2 < 6; i2++)
                for (int i3 = 0; i3 < 6; i3++) {
                    for (u32 l4 = 0; l4 < 3; l4++)
                        pulled_to(b, U160::limbs(V[i0], V[i1], V[i2], V[i3], l4), "target_limbs_l4_" + std::to_string(l4), 3, rng, E);
                    const U160 top = with_top(b, U160::limbs(V[i0], V[i1], V[i2], V[i3], 0), 4, MAX_TERMS - 1);
                    if (top.l[4] < MAX_TERMS - 8) generator_failed("gl: top l4");
                    pulled_to(b, top, "target_limbs_l4_top", 1, rng, E);
                }
    // k p + r with a seeded k of 40..75 bits: the limbs are not small
    const u64 residues[3] = {0, 1, p - 1};
    const char* residue_cls[3] = {"target_0_mod_p", "target_1_mod_p", "target_p_minus_1_mod_p"};
    for (int r = 0; r < 3; r++)
        for (int i = 0; i < 256; i++) {
            const int bits = 40 + i % 36;
            const u128 k = (((u128)rng() << 64) | rng()) >> (128 - bits);
            U160 t;   // k p, schoolbook: p = 2^64 - 2^32 + 1
            t.add(U160::of(k));
            U160 k64 = U160::limbs(0, 0, (u32)k, (u32)(k >> 32), (u32)(k >> 64));
            if (k >> 96) generator_failed("gl: k");
            t.add(k64);
            t.sub(U160::limbs(0, (u32)k, (u32)(k >> 32), (u32)(k >> 64), 0));
            t.add(U160::of(residues[r]));
            if (t.mod(p) != residues[r]) generator_failed("gl: residue target");
            pulled_to(b, t, residue_cls[r], 3, rng, E);
        }
    const U160 listed[] = {U160::of(p), U160::of((u128)p * 2), U160::of((u128)1 << 64), U160::of((u128)1 << 96), U160::of(~(u128)0),
                           U160::limbs(0, 0, 0, 0, 1), U160::limbs(0, 1, 0, 0, 1)};
    for (const U160& t : listed) pulled_to(b, t, "target_listed_sum", 3, rng, E);
    mid_chain_boundaries(b, 4, 2, rng, E);
    edge_and_random_chains(b, rng, E);
    return ch;
}

inline Chains<BbAcc> bb_chains() {
    typedef BbAcc F;
    const u32 p = (u32)F::P;
    Chains<F> ch;
    Builder<F> b(ch);
    std::mt19937_64 rng(rc::seed_of(F::name()));
    const std::vector<u64> E = F::operand_words();
    for (const char* cls : {"target_words_hi_0", "target_words_hi_1", "target_words_hi_2", "target_words_hi_top", "target_0_mod_p",
                            "target_p_minus_1_mod_p", "mid_chain_carry_fires", "mid_chain_carry_one_short", "acc_carry_into_hi",
                            "finish_mid_below_p", "finish_mid_in_p_2p", "finish_mid_from_2p", "edge_all_largest_products",
                            "edge_all_zero_products", "edge_alternating_products", "target_finish_sums"})
        ch.declare(cls);
    for (const char* mid : {"finish_mid_below_p", "finish_mid_in_p_2p", "finish_mid_from_2p"})
        for (const char* adds : {"_no_add_wraps", "_first_add_wraps", "_second_add_wraps", "_both_adds_wrap"}) ch.declare(std::string(mid) + adds);
    for (int i = 0; i < 2; i++)
        for (int j = i; j < 2; j++)
            for (const char* f : {"mid_chain_fires_limbs_", "mid_chain_short_limbs_"}) ch.declare(f + std::to_string(i) + "_" + std::to_string(j));
    for (u32 len : {1u, 2u, 3u, 4u, 5u, 16u, 17u, 123u, MAX_TERMS}) ch.declare("length_" + std::to_string(len));
    const u32 LOW[5] = {0, 1, p - 1, p, 0xffffffffu};
    const u32 MID[8] = {0, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 0xffffffffu};
    const u32 hi_cap = (u32)(((u128)MAX_TERMS * (p - 1) * (p - 1)) >> 64);   // 900
    for (u32 w0 : LOW)
        for (u32 w1 : MID) {
            for (u32 hi = 0; hi < 3; hi++) pulled_to(b, U160::limbs(w0, w1, hi, 0, 0), "target_words_hi_" + std::to_string(hi), 3, rng, E);
            const U160 top = with_top(b, U160::limbs(w0, w1, 0, 0, 0), 2, hi_cap);
            if (top.l[2] < hi_cap - 8) generator_failed("bb: top hi");
            pulled_to(b, top, "target_words_hi_top", 1, rng, E);
        }
    // The listed words alone leave finish()'s own sums untested: it adds x = w0 2^-32, y = w1 less 0, p or 2p, and z = hi 2^32 (mod p)
    // with two bb::add, and a word y left in [p, 2p) is absorbed by the first of them unless BOTH have to wrap (x + y + z >= 2p; y
    // < 2^32 - 2p there, so x and z must both be near p).  So: x and z chosen (w0 = x 2^32 mod p, or that plus p where it fits a
    // word; hi = 7, 15, 30 give z = 0.93 p, p - 32, p - 64), y on either side of p - x and of 2p - x - z, in each of the three ranges.
    const u64 r1 = (1ULL << 32) % p, half = (p - 1) / 2;
    for (u64 x : {(u64)0, (u64)1, (u64)31, (u64)32, half, half + 1, (u64)p - 2, (u64)p - 1})
        for (u32 hi : {0u, 1u, 2u, 7u, 8u, 15u, 16u, 30u}) {
            const u64 z = rc::mulmod(hi, r1, p);
            for (u32 k = 0; k < 3; k++) {   // w1 = y + k p
                const u64 y_max = k < 2 ? (u64)p - 1 : 0xffffffffULL - 2 * (u64)p;
                std::vector<u64> ys = {0, 1, y_max - 1, y_max};
                for (u64 edge : {(u64)p - x, 2 * (u64)p - x - z, (u64)p - z})   // x + y = p, x + y + z = 2p, y + z = p
                    for (int d = -1; d <= 1; d++)
                        if (edge + d <= y_max && (edge || d >= 0)) rc::push_unique(ys, edge + d, p);
                for (u64 y : ys)
                    for (int alt = 0; alt < 2; alt++) {
                        const u64 w0 = rc::mulmod(x, r1, p) + (alt ? p : 0);
                        if (w0 >> 32) continue;
                        const U160 t = U160::limbs((u32)w0, (u32)(y + (u64)k * p), hi, 0, 0);
                        if (F::expected(U160::limbs(t.l[0], 0, 0, 0, 0)) != x) generator_failed("bb: low word of a finish() target");
                        pulled_to(b, t, "target_finish_sums", 1 + (alt == 0), rng, E);
                    }
            }
        }
    const u64 residues[2] = {0, (u64)p - 1};
    const char* residue_cls[2] = {"target_0_mod_p", "target_p_minus_1_mod_p"};
    for (int r = 0; r < 2; r++)
        for (int i = 0; i < 256; i++) {
            const int bits = 8 + i % 35;   // k p up to 2^73, under 900 2^64
            const u64 k = rng() >> (64 - bits);
            U160 t = U160::of((u128)k * p);
            t.add(U160::of(residues[r]));
            if (t.mod(p) != residues[r]) generator_failed("bb: residue target");
            pulled_to(b, t, residue_cls[r], 3, rng, E);
        }
    mid_chain_boundaries(b, 2, 2, rng, E);
    edge_and_random_chains(b, rng, E);
    return ch;
}

// gl::fold160 on its own: the limb patterns with every listed l4 and with the two values no chain reaches (4095 beside any low
// limbs; 2^31, the bound fold160 states), then the final sum of every Goldilocks chain.  expect = the value mod p: the runners
// canonicalise fold160's word, as FoldAcc<GlF>::finish does.
struct Fold160Cases {
    std::vector<U160> in;
    std::vector<u64> expect;
    std::vector<std::pair<std::string, size_t>> census;
    size_t patterns = 0;
    size_t count() const { return in.size(); }
};
inline Fold160Cases fold160_cases(const Chains<GlAcc>& gl) {
    Fold160Cases f;
    declare_fold160(f.census);
    const u32 V[6] = {0, 1, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    const u32 R4[] = {0, 1, 2, MAX_TERMS - 6, MAX_TERMS - 5, MAX_TERMS - 1, 0x7fffffffu, 0x80000000u};
    for (u32 a0 : V)
        for (u32 a1 : V)
            for (u32 a2 : V)
                for (u32 a3 : V)
                    for (u32 r4 : R4) f.in.push_back(U160::limbs(a0, a1, a2, a3, r4));
    f.patterns = f.in.size();
    f.in.insert(f.in.end(), gl.final_sum.begin(), gl.final_sum.end());
    for (const U160& s : f.in) {
        f.expect.push_back(s.mod(GlAcc::P));
        tally_fold160(f.census, s);
    }
    return f;
}

// prints the census lines "census <name> <class>=<chains>"; false when a class is empty
inline bool print_census(const char* name, const std::vector<std::pair<std::string, size_t>>& census) {
    bool ok = true;
    for (auto& e : census) {
        printf("census %s %s=%zu\n", name, e.first.c_str(), e.second);
        if (!e.second) ok = false;
    }
    if (!ok) printf("census %s: a class is EMPTY\n", name);
    return ok;
}

// out[i]: what the code under test returned for chain i.  Prints the first five mismatching chains and the line
// "name cases=N mismatches=M (pulled=a edge=b random=c)"; returns M.
template <class F>
inline size_t report(const Chains<F>& ch, const std::vector<typename F::W>& out) {
    size_t bad = 0, by_kind[3] = {0, 0, 0};
    static const char* kinds[3] = {"pulled", "edge", "random"};
    for (size_t i = 0; i < ch.count(); i++) {
        if (out[i] == ch.expect[i]) continue;
        by_kind[ch.kind[i]]++;
        if (bad++ < 5) {
            const U160& s = ch.final_sum[i];
            printf("  %s chain %zu (%s, %u terms): got %llx, expected %llx; exact sum %08x %08x %08x %08x %08x (high limb first)\n", F::name(), i,
                   kinds[ch.kind[i]], ch.off[i + 1] - ch.off[i], (u64)out[i], (u64)ch.expect[i], s.l[4], s.l[3], s.l[2], s.l[1], s.l[0]);
        }
    }
    printf("%s cases=%zu mismatches=%zu (pulled=%zu edge=%zu random=%zu)\n", F::name(), ch.count(), bad, by_kind[0], by_kind[1], by_kind[2]);
    printf("%s chains: pulled=%zu edge=%zu random=%zu terms=%zu\n", F::name(), ch.by_kind[0], ch.by_kind[1], ch.by_kind[2], ch.c.size());
    return bad;
}
inline size_t report(const Fold160Cases& f, const std::vector<u64>& out) {
    size_t bad = 0, bad_patterns = 0;
    for (size_t i = 0; i < f.count(); i++) {
        if (out[i] == f.expect[i]) continue;
        if (i < f.patterns) bad_patterns++;
        if (bad++ < 5) {
            const U160& s = f.in[i];
            printf("  gl_fold160 case %zu: got %llx, expected %llx; limbs %08x %08x %08x %08x %08x (high limb first)\n", i, out[i], f.expect[i],
                   s.l[4], s.l[3], s.l[2], s.l[1], s.l[0]);
        }
    }
    printf("gl_fold160 cases=%zu mismatches=%zu (patterns=%zu chain_sums=%zu)\n", f.count(), bad, bad_patterns, bad - bad_patterns);
    return bad;
}

}  // namespace fold_acc_cases

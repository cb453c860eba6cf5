// gl::mul_mont_lazy (csrc/gl_field.hpp: the product whose fold takes its final "- borrow * EPS" as an add-with-carry and a
// subtract-with-borrow on the flag itself, mont_fold_flags) against mont_fold(mul_limbs(a, b)), the form it replaces: the same
// u64 WORD for every pair of operands, not merely a congruent one, for both FIVE forms.  The host overloads of the flag helpers
// model the device instructions limb by limb with the flags as bits, so the sequence checked here is the one the device runs.
//
// Pairs for which (m2.hi, 0) - b does not borrow have probability ~2^-32 on random operands; the edge set holds operands that
// reach them (products whose low 64 bits vanish, and pairs built for m2.hi >= b > 0), and the run reports how many pairs did.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gl_field.hpp"
#include "mul_mont_cases.hpp"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;

static u64 old_form_four(u64 a, u64 b) {
    u32 r0, r1, hl, hh;
    gl::mul_limbs<false>(a, b, r0, r1, hl, hh);
    return gl::mont_fold(r0, r1, hl, hh);
}
static u64 old_form_five(u64 a, u64 b) {
    u32 r0, r1, hl, hh;
    gl::mul_limbs<true>(a, b, r0, r1, hl, hh);
    return gl::mont_fold(r0, r1, hl, hh);
}
// a b / 2^64 mod p from the definition, for the congruence check (independent of the limb code)
static u64 mont_reference(u64 a, u64 b) {
    const u128 t = (u128)a * b;
    const u64 lo = (u64)t, hi = (u64)(t >> 64);
    const u64 m = lo + (lo << 32);                       // lo / p mod 2^64 = lo (1 + 2^32)
    const u128 mp = (u128)m * gl::P;                     // lo - m p = 0 (mod 2^64): (1 + 2^32) p = 2^96 + 1
    const u64 bh = (u64)(mp >> 64);                      // (t - m p) / 2^64 = hi - bh
    const u128 pp = gl::P;
    return (u64)(((u128)hi + pp - bh % pp) % pp);
}
int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000000;
    const u64 P = gl::P;
    const std::vector<u64> edge = mul_mont_cases::edge_values();
    std::mt19937_64 rng(20261016);
    const std::vector<std::pair<u64, u64>> constructed = mul_mont_cases::no_borrow_pairs(rng);
    long bad = 0, word_bad = 0, by0 = 0, by0_nonzero_low = 0, pairs = 0;
    auto check = [&](u64 a, u64 b) {
        pairs++;
        const u64 n4 = gl::mul_mont_lazy<false>(a, b), n5 = gl::mul_mont_lazy<true>(a, b);
        const u64 o4 = old_form_four(a, b), o5 = old_form_five(a, b);
        if (n4 != o4 || n5 != o5 || o4 != o5) {
            if (++word_bad < 5) printf("word mismatch: a=%016llx b=%016llx new4=%016llx old4=%016llx new5=%016llx old5=%016llx\n", a, b, n4, o4, n5, o5);
        }
        if (n4 % P != mont_reference(a, b)) {
            if (++bad < 5) printf("residue mismatch: a=%016llx b=%016llx new4=%016llx want=%016llx\n", a, b, n4, mont_reference(a, b));
        }
        if (a < P && b < P && (gl::mul_mont<false>(a, b) >= P || gl::mul_mont<true>(a, b) >= P)) {
            if (++bad < 5) printf("not canonical: a=%016llx b=%016llx\n", a, b);
        }
        if (mul_mont_cases::no_borrow(a, b)) {
            by0++;
            if ((u64)((u128)a * b) != 0) by0_nonzero_low++;
        }
    };
    for (u64 a : edge)
        for (u64 b : edge) check(a, b);
    for (auto& pr : constructed) {
        check(pr.first, pr.second);
        check(pr.second, pr.first);
    }
    for (long t = 0; t < n; t++) {
        u64 a = rng(), b = rng();
        if (t % 4 == 1) { a %= P; b %= P; }                         // canonical operands: the contract of mul_mont
        if (t % 16 == 2) a = edge[(size_t)(rng() % edge.size())];   // one edge operand against a random one
        if (t % 16 == 3) b = edge[(size_t)(rng() % edge.size())];
        check(a, b);
    }
    printf("pairs=%ld by0=%ld by0_nonzero_low=%ld constructed=%zu mismatches=%ld\n", pairs, by0, by0_nonzero_low, constructed.size(), bad + word_bad);
    return (bad + word_bad) != 0;
}

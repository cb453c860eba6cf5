// The inputs and expected outputs that tests/host_shim/register_dfts.cpp (CPU) and tests/device/register_dfts.hip (GPU) both run through
// the register DFTs of csrc/dft_gl.hpp and csrc/dft_bb.hpp (mul_pow2, dft16, dft32, dft_small, layer64) and csrc/ntt_outer.hpp's dft_r.
// Everything expected is computed HERE, in 128-bit integer arithmetic mod p from the fields' defining constants; nothing comes from the
// csrc headers.  An R-point DFT is the plain sum X[k] = sum_i x[i] w^(ik).
//
// Why chosen inputs: the limb code's rare branches (a sum landing in [p, 2^64), a borrow, |a - b| near p - 1 in front of the signed
// Montgomery product) fire with probability ~2^-32 on random words, and edge words placed in a transform's INPUT reach its first
// butterfly layer only.  So for every butterfly layer L of a function and every ordered pair (u, v) of edge values, one case puts u on
// the a side and v on the b side of every layer-L butterfly, by applying the exact inverse of layers 1..L-1 to that state ("pulled
// back").  The generator then runs its own layers 1..L-1 forward and requires the state back: a failure there, or a non-canonical input
// word, ends the program with status 3 - no case is ever left out.  Beside those: 2^14 vectors with every slot drawn from the edge
// set ("mixed") and 2^14 vectors of seeded uniform canonical words ("random").
// BabyBear values are canonical here and cross to the functions as Montgomery words (c 2^32 mod p): outputs are compared AS WORDS, so a
// result that is right mod p but not canonical is a mismatch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

namespace register_dft_cases {
typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;

[[noreturn]] inline void generator_failed(const std::string& what) {
    printf("case generator failed: %s\n", what.c_str());
    fflush(stdout);
    exit(3);
}

inline u64 mulmod(u64 a, u64 b, u64 p) { return (u64)((u128)a * b % p); }
inline u64 addmod(u64 a, u64 b, u64 p) { return (u64)(((u128)a + b) % p); }
inline u64 submod(u64 a, u64 b, u64 p) { return (u64)(((u128)a + p - b) % p); }
inline u64 powmod(u64 b, u64 e, u64 p) {
    u64 r = 1;
    for (b %= p; e; e >>= 1, b = mulmod(b, b, p))
        if (e & 1) r = mulmod(r, b, p);
    return r;
}
inline u32 brev(u32 x, int bits) {
    u32 r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}
inline void push_unique(std::vector<u64>& v, u64 x, u64 p) {
    if (x < p && std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);   // canonical values only
}

struct Gl {
    typedef u64 W;
    static constexpr u64 P = 0xFFFFFFFF00000001ULL;
    static const char* tag() { return "gl"; }
    static W word(u64 canonical) { return canonical; }
    // F::two_adic_generator(bits): the generator of order 2^32 squared down
    static u64 two_adic(int bits) {
        u64 g = 1753635133440165772ULL;
        for (int i = bits; i < 32; i++) g = mulmod(g, g, P);
        return g;
    }
    // the primitive 2^log_r-th root of the register DFTs: w_64 = 2^39, so w_16 = 2^156 (log_r <= 6)
    static u64 root(int log_r) { return powmod(2, 39ULL * (64u >> log_r), P); }
    static std::vector<u64> edges() {
        std::vector<u64> e;
        for (u64 x : {(u64)0, (u64)1, (u64)2, P - 1, P - 2}) push_unique(e, x, P);
        for (int d = -2; d <= 2; d++) push_unique(e, (1ULL << 32) + d, P);
        for (int d = -2; d <= 2; d++) push_unique(e, P - (1ULL << 32) + d, P);
        for (int d = -1; d <= 1; d++) push_unique(e, (1ULL << 63) + d, P);
        push_unique(e, 0xFFFFFFFEFFFFFFFFULL, P);
        push_unique(e, 0x7FFFFFFF00000000ULL, P);
        for (int k = 0; k < 64; k++) {
            push_unique(e, 1ULL << k, P);
            push_unique(e, (1ULL << k) - 1, P);
            push_unique(e, P - (1ULL << k), P);
        }
        return e;
    }
};

struct Bb {
    typedef u32 W;
    static constexpr u64 P = 2013265921ULL;   // 2^31 - 2^27 + 1
    static const char* tag() { return "bb"; }
    static W word(u64 canonical) { return (W)mulmod(canonical, (1ULL << 32) % P, P); }   // Montgomery: c 2^32 mod p
    static u64 two_adic(int bits) {
        u64 g = 0x1a427a41ULL;   // order 2^27
        for (int i = bits; i < 27; i++) g = mulmod(g, g, P);
        return g;
    }
    static u64 root(int log_r) { return two_adic(log_r); }
    static std::vector<u64> edges() {
        std::vector<u64> e;
        for (u64 x : {(u64)0, (u64)1, (u64)2, P - 1, P - 2, (P - 1) / 2, (P + 1) / 2, (u64)1 << 27, ((u64)1 << 27) - 1, ((u64)1 << 27) + 1,
                      P - ((u64)1 << 27)})
            push_unique(e, x, P);
        // the canonical values whose Montgomery WORD is 0, 1, p - 1, (p -+ 1) / 2: the kernels subtract words, so the word is what
        // reaches the signed product
        const u64 rinv = powmod((1ULL << 32) % P, P - 2, P);
        for (u64 w : {(u64)0, (u64)1, P - 1, (P - 1) / 2, (P + 1) / 2}) {
            const u64 c = mulmod(w, rinv, P);
            if (word(c) != w) generator_failed("BabyBear word edge does not convert back");
            push_unique(e, c, P);
        }
        return e;
    }
};

// w must be a primitive 2^log_r-th root of unity
inline void require_order(u64 w, int log_r, u64 p, const std::string& name) {
    if (powmod(w, 1ULL << log_r, p) != 1 || (log_r > 0 && powmod(w, 1ULL << (log_r - 1), p) != p - 1))
        generator_failed(name + ": root of the wrong order");
}

inline unsigned workers() { return std::min(8u, std::max(1u, std::thread::hardware_concurrency())); }
template <class Fn>
inline void parallel_for(size_t n, Fn fn) {
    const unsigned nw = workers();
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nw; t++)
        pool.emplace_back([=] {
            for (size_t i = n * t / nw; i < n * (t + 1) / nw; i++) fn(i);
        });
    for (auto& th : pool) th.join();
}

inline u64 seed_of(const std::string& name) {   // FNV-1a: the same cases on every machine
    u64 h = 1469598103934665603ULL;
    for (unsigned char c : name) h = (h ^ c) * 1099511628211ULL;
    return h;
}
template <class Rng>
inline u64 uniform(Rng& rng, u64 p) {
    for (;;) {
        const u64 x = p >> 32 ? rng() : rng() >> 33;   // 64 bits for Goldilocks, 31 for BabyBear: rejection keeps it uniform
        if (x < p) return x;
    }
}

static constexpr size_t MIXED = 1u << 14, RANDOM = 1u << 14;

// `width` words per case, pulled-back cases first, then mixed, then random
template <class F>
struct Cases {
    std::string name;
    int width = 0;
    size_t pulled = 0, mixed = 0, random = 0;
    std::vector<u64> canonical;                     // inputs as field elements
    std::vector<typename F::W> in, expect;          // as the words the functions see
    typename F::W wr = 0;                           // dft_r: the root it is given
    size_t count() const { return pulled + mixed + random; }
    const char* kind(size_t i) const { return i < pulled ? "pulled" : i < pulled + mixed ? "mixed" : "random"; }
};

template <class F>
inline void add_mixed_and_random(Cases<F>& c) {
    const std::vector<u64> E = F::edges();
    std::mt19937_64 rng(seed_of(c.name));
    for (size_t i = 0; i < MIXED * c.width; i++) c.canonical.push_back(E[rng() % E.size()]);
    for (size_t i = 0; i < RANDOM * c.width; i++) c.canonical.push_back(uniform(rng, F::P));
    c.mixed = MIXED;
    c.random = RANDOM;
}
// expected[i] = ref(canonical inputs of case i) (canonical), both then converted to words
template <class F, class Ref>
inline void finish(Cases<F>& c, Ref ref) {
    const size_t n = c.count(), w = (size_t)c.width;
    if (c.canonical.size() != n * w) generator_failed(c.name + ": case count");
    for (u64 x : c.canonical)
        if (x >= F::P) generator_failed(c.name + ": non-canonical input word");
    c.in.resize(n * w);
    c.expect.resize(n * w);
    parallel_for(n, [&c, w, ref](size_t i) {
        std::vector<u64> out(w);
        ref(&c.canonical[i * w], out.data());
        for (size_t s = 0; s < w; s++) {
            c.in[i * w + s] = F::word(c.canonical[i * w + s]);
            c.expect[i * w + s] = F::word(out[s]);
        }
    });
}

// One DIF layer of half-size h on t[0 .. r), forward (in place): (a, b) -> (a + b, (a - b) w_{2h}^j), w_{2h}^j = wp[j r / (2 h)]
inline void dif_layer(u64* t, u32 r, u32 h, const std::vector<u64>& wp, u64 p) {
    for (u32 o = 0; o < r; o += 2 * h)
        for (u32 j = 0; j < h; j++) {
            const u64 a = t[o + j], b = t[o + j + h];
            t[o + j] = addmod(a, b, p);
            t[o + j + h] = mulmod(submod(a, b, p), wp[j * (r / (2 * h))], p);
        }
}
// its exact inverse: a = (s + d / w) / 2, b = (s - d / w) / 2
inline void dif_layer_inverse(u64* t, u32 r, u32 h, const std::vector<u64>& wp, u64 p) {
    const u64 half = (p + 1) / 2;
    for (u32 o = 0; o < r; o += 2 * h)
        for (u32 j = 0; j < h; j++) {
            const u64 s = t[o + j], dw = mulmod(t[o + j + h], wp[(r - j * (r / (2 * h))) % r], p);
            t[o + j] = mulmod(addmod(s, dw, p), half, p);
            t[o + j + h] = mulmod(submod(s, dw, p), half, p);
        }
}

// dft16 (log_r = 4), dft32 (5), dft_small<K> (K): natural input order, X[k] in slot brev(k); log_r butterfly layers of half-sizes
// r/2, r/4, .., 1.  Pulled-back cases: layers x |E|^2.
template <class F>
inline Cases<F> dft_cases(const std::string& name, int log_r, bool inv) {
    const u64 p = F::P;
    const u32 r = 1u << log_r;
    u64 w = F::root(log_r);
    require_order(w, log_r, p, name);
    if (inv) w = powmod(w, r - 1, p);
    require_order(w, log_r, p, name);
    std::vector<u64> wp(r);
    for (u32 e = 0; e < r; e++) wp[e] = powmod(w, e, p);
    const std::vector<u64> E = F::edges();
    Cases<F> c;
    c.name = name;
    c.width = (int)r;
    std::vector<u64> t(r), back(r);
    for (int L = 1; L <= log_r; L++) {
        const u32 hl = r >> L;
        for (u64 u : E)
            for (u64 v : E) {
                for (u32 i = 0; i < r; i++) t[i] = (i & hl) ? v : u;   // the state in front of layer L
                back = t;
                for (int l = L - 1; l >= 1; l--) dif_layer_inverse(back.data(), r, r >> l, wp, p);
                std::vector<u64> again = back;
                for (int l = 1; l < L; l++) dif_layer(again.data(), r, r >> l, wp, p);
                if (again != t) generator_failed(name + ": pulled-back input does not reach its target state");
                c.canonical.insert(c.canonical.end(), back.begin(), back.end());
                c.pulled++;
            }
    }
    add_mixed_and_random(c);
    finish(c, [=](const u64* x, u64* out) {
        for (u32 k = 0; k < r; k++) {
            u128 acc = 0;   // r <= 64 terms below 2^64 each
            for (u32 i = 0; i < r; i++) acc += mulmod(x[i], wp[(i * k) % r], p);
            out[brev(k, log_r)] = (u64)(acc % p);
        }
    });
    return c;
}

// layer64<INV, H, O>: one DIF layer of half-size H on 2 H words, twiddles w_{2H}^j
template <class F>
inline Cases<F> layer_cases(const std::string& name, int log_h, bool inv) {
    const u64 p = F::P;
    const u32 h = 1u << log_h, r = 2 * h;
    u64 w = F::root(log_h + 1);
    if (inv) w = powmod(w, r - 1, p);
    require_order(w, log_h + 1, p, name);
    std::vector<u64> wp(r);
    for (u32 e = 0; e < r; e++) wp[e] = powmod(w, e, p);
    const std::vector<u64> E = F::edges();
    Cases<F> c;
    c.name = name;
    c.width = (int)r;
    for (u64 u : E)
        for (u64 v : E) {
            for (u32 i = 0; i < r; i++) c.canonical.push_back(i < h ? u : v);
            c.pulled++;
        }
    add_mixed_and_random(c);
    finish(c, [=](const u64* x, u64* out) {
        for (u32 j = 0; j < h; j++) {
            out[j] = addmod(x[j], x[j + h], p);
            out[j + h] = mulmod(submod(x[j], x[j + h], p), wp[j], p);
        }
    });
    return c;
}

// dft_r<F, K>: 2^K points, natural order in and out, the root handed in by the caller - two_adic_generator(K) or its inverse
// (K = 1: unused, the callers pass the fourth root).  No layer structure for K >= 3: E^2 on (z[0], z[1..]).
template <class F>
inline Cases<F> dft_r_cases(const std::string& name, int K, bool inv) {
    const u64 p = F::P;
    const u32 r = 1u << K;
    const int bits = K < 2 ? 2 : K;
    u64 given = F::two_adic(bits);
    if (inv) given = powmod(given, (1ULL << bits) - 1, p);
    require_order(given, bits, p, name);
    const u64 w = K == 1 ? p - 1 : given;
    require_order(w, K, p, name);
    std::vector<u64> wp(r);
    for (u32 e = 0; e < r; e++) wp[e] = powmod(w, e, p);
    const std::vector<u64> E = F::edges();
    Cases<F> c;
    c.name = name;
    c.width = (int)r;
    c.wr = F::word(given);
    for (u64 u : E)
        for (u64 v : E) {
            for (u32 i = 0; i < r; i++) c.canonical.push_back(i ? v : u);
            c.pulled++;
        }
    add_mixed_and_random(c);
    finish(c, [=](const u64* x, u64* out) {
        for (u32 k = 0; k < r; k++) {
            u128 acc = 0;
            for (u32 i = 0; i < r; i++) acc += mulmod(x[i], wp[(i * k) % r], p);
            out[k] = (u64)(acc % p);
        }
    });
    return c;
}

// Goldilocks mul_pow2<K>: every edge value ("pulled" in the counts) and 2^12 random canonical words
inline Cases<Gl> mul_pow2_cases(const std::string& name, int K) {
    Cases<Gl> c;
    c.name = name;
    c.width = 1;
    c.canonical = Gl::edges();
    c.pulled = c.canonical.size();
    std::mt19937_64 rng(seed_of(name));
    c.random = 1u << 12;
    for (size_t i = 0; i < c.random; i++) c.canonical.push_back(uniform(rng, Gl::P));
    const u64 f = powmod(2, (u64)K, Gl::P);
    finish(c, [=](const u64* x, u64* out) { out[0] = mulmod(x[0], f, Gl::P); });
    return c;
}

// What the Goldilocks sources say about their roots, checked once: the 64th root the reference's generator gives is 2^39
inline void check_constants() {
    if (Gl::two_adic(6) != (1ULL << 39) || Gl::root(4) != powmod(2, 156, Gl::P) || Gl::root(6) != (1ULL << 39))
        generator_failed("Goldilocks: the 64th root of unity is not 2^39");
    if (powmod(2, 96, Gl::P) != Gl::P - 1) generator_failed("Goldilocks: 2^96 is not -1");
    for (int b = 1; b <= 6; b++) {
        require_order(Gl::two_adic(b), b, Gl::P, "gl two_adic");
        require_order(Bb::two_adic(b), b, Bb::P, "bb two_adic");
    }
}

// out: what the function under test left in the case's words.  Prints the first five mismatching cases with their inputs and the line
// "name cases=N mismatches=M (pulled=a mixed=b random=c)"; returns M.
template <class F>
inline size_t report(const Cases<F>& c, const std::vector<typename F::W>& out) {
    size_t bad = 0, by_kind[3] = {0, 0, 0};
    const size_t w = (size_t)c.width;
    for (size_t i = 0; i < c.count(); i++) {
        size_t s = 0;
        while (s < w && out[i * w + s] == c.expect[i * w + s]) s++;
        if (s == w) continue;
        by_kind[i < c.pulled ? 0 : i < c.pulled + c.mixed ? 1 : 2]++;
        if (bad++ < 5) {
            printf("  %s case %zu (%s) slot %zu: got %llx, expected %llx; input words:", c.name.c_str(), i, c.kind(i), s,
                   (u64)out[i * w + s], (u64)c.expect[i * w + s]);
            for (size_t k = 0; k < w; k++) printf(" %llx", (u64)c.in[i * w + k]);
            printf("\n");
        }
    }
    printf("%s cases=%zu mismatches=%zu (pulled=%zu mixed=%zu random=%zu)\n", c.name.c_str(), c.count(), bad, by_kind[0], by_kind[1], by_kind[2]);
    return bad;
}

}  // namespace register_dft_cases

// The permutation headers' own helpers on the GPU, one kernel per function, against 128-bit integer arithmetic mod p written HERE
// (nothing expected comes from the headers; the round constants and the MDS entries are read from poseidon_constants.h, the BabyBear
// scale sequence is restated): edge operands squared plus 2^16 seeded operands per scalar function, each drawn inside the function's
// stated domain ("any u64 in" gets any u64), and for the functions on whole states the edge states plus 2^14 .. 2^16 seeded ones.
//   csrc/poseidon_gl.hpp:          to_mont, from_mont, add_rc, mul_lazy, mul_add_lazy, reduce128_lazy, sbox, fold_halves, mds_layer_mfma<0 / 8>
//   csrc/poseidon_gl_grouped.hpp:  sub_lazy, fold_rows_rare_carry<12>, partial_group<4> / <2> at the product's start rounds
//   csrc/poseidon_gl_coop.hpp:     add_lazy (second carry included), row_sum
//   csrc/poseidon2_bb.hpp:         sbox7, external_layer<false / true>, internal_round, renorm, renorm_lazy, canonical_out
//   csrc/poseidon2_bb_coop.hpp:    sbox7, external_layer
// Results that are "some residue" are compared mod p; where the header states a range for the result it is asserted: from_mont
// canonical, sbox7 in (0, 2p), lazy words below LAZY_MAX, renorm_lazy in [0, 2p), word 0 after internal_round in (-p, p) as a signed
// word, external_layer<true> within +-1.03 p.  MFMA, DPP and the wave-uniform carry branch are wave-wide: in those kernels the lanes
// past the end work on a clamped index and skip the store.  One hipDeviceSynchronize, comparison on the host; prints
// "cases=N mismatches=M", exit status 1 on a mismatch, 2 on a HIP error.  Built and run by tests/test_device_permutation_helpers.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "poseidon_gl_grouped.hpp"
#include "poseidon_gl_coop.hpp"
#include "poseidon2_bb.hpp"
#include "poseidon2_bb_coop.hpp"
#include "../host_shim/mul_mont_cases.hpp"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;
typedef __int128 i128;

// ---------------------------------------------------------------- kernels
#define IDX const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return
// wave-wide code: every lane runs, on a clamped index (n >= 1)
#define CLAMPED const u32 i0 = blockIdx.x * blockDim.x + threadIdx.x; const bool live = i0 < n; const u32 i = live ? i0 : n - 1
__global__ void k_to_mont(const u64* a, u64* o, u32 n) { IDX; o[i] = poseidon_gl::to_mont(a[i]); }
__global__ void k_from_mont(const u64* a, u64* o, u32 n) { IDX; o[i] = poseidon_gl::from_mont(a[i]); }
__global__ void k_add_rc(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = poseidon_gl::add_rc(a[i], b[i]); }
__global__ void k_mul_lazy(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = poseidon_gl::mul_lazy(a[i], b[i]); }
__global__ void k_mul_add_lazy(const u64* a, const u64* b, const u64* c, u64* o, u32 n) { IDX; o[i] = poseidon_gl::mul_add_lazy(a[i], b[i], c[i]); }
__global__ void k_reduce128_lazy(const u64* lo, const u64* hi, u64* o, u32 n) { IDX; o[i] = poseidon_gl::reduce128_lazy(lo[i], hi[i]); }
__global__ void k_sbox(const u64* a, u64* o, u32 n) { IDX; o[i] = poseidon_gl::sbox(a[i]); }
__global__ void k_fold_halves(const u64* sl, const u64* sh, u64* o, u32 n) { IDX; o[i] = poseidon_gl::fold_halves(sl[i], sh[i]); }
__global__ void k_sub_lazy(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = poseidon_gl::sub_lazy(a[i], b[i]); }
__global__ void k_coop_add_lazy(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = poseidon_gl_coop::add_lazy(a[i], b[i]); }
// n a multiple of 64: one word per lane, every 16-lane row sums its own words
__global__ void k_row_sum(const u64* x, u64* o, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = poseidon_gl_coop::row_sum(x[i]);
}
__global__ void k_fold_rows(const u64* lo, const u64* hi, u64* o, u32 n) {   // [n][12] each
    CLAMPED;
    long long l[12], h[12];
    u64 s[12];
#pragma unroll
    for (int q = 0; q < 12; q++) { l[q] = (long long)lo[12 * i + q]; h[q] = (long long)hi[12 * i + q]; }
    poseidon_gl::fold_rows_rare_carry<12>(s, l, h);
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 12; q++) o[12 * i + q] = s[q];
}
template <int Q0>
__global__ __launch_bounds__(256) void k_mds_mfma(const u64* in, u64* o, int rnext, u32 n) {
    CLAMPED;
    const poseidon_gl::MdsOperand amat = poseidon_gl::mds_mfma_matrix();
    u64 s[12];
#pragma unroll
    for (int q = 0; q < 12; q++) s[q] = in[12 * i + q];
    poseidon_gl::mds_layer_mfma<Q0>(s, amat, rnext);
    if (!live) return;
#pragma unroll
    for (int q = Q0; q < 12; q++) o[12 * i + q] = s[q];
}
template <int G>
__global__ __launch_bounds__(256) void k_partial_group(const u64* in, u64* o, int r0, u32 n) {
    CLAMPED;
    const poseidon_gl::MdsOperand amat = poseidon_gl::mds_mfma_matrix();
    __shared__ poseidon_gl::v4i gops_lds[poseidon_gl::GROUP_LDS_V4];
    poseidon_gl::group_ops_init(gops_lds);
    const poseidon_gl::v4i* gops = gops_lds + (threadIdx.x & 63) + (G == poseidon_gl::GROUP_G ? 0 : poseidon_gl::GROUP_OPS_MAIN * 64);
    u64 s[12];
#pragma unroll
    for (int q = 0; q < 12; q++) s[q] = in[12 * i + q];
    poseidon_gl::partial_group<G>(s, amat, gops, r0);
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 12; q++) o[12 * i + q] = s[q];
}
__global__ void k_bb_sbox7(const u32* a, u32* o, u32 n) { IDX; o[i] = poseidon2_bb::sbox7(a[i]); }
template <bool SIGNED>
__global__ void k_bb_external(const u32* in, const u32* c, u32* o, u32 n) {   // [n][16] each
    IDX;
    u32 s[16];
#pragma unroll
    for (int q = 0; q < 16; q++) s[q] = in[16 * i + q];
    poseidon2_bb::external_layer<SIGNED>(s, c + 16 * i);
#pragma unroll
    for (int q = 0; q < 16; q++) o[16 * i + q] = s[q];
}
__global__ void k_bb_internal(const u32* in, const u32* rc_next, const u32* sumc, u32* o, u32 n) {
    IDX;
    u32 s[16];
#pragma unroll
    for (int q = 0; q < 16; q++) s[q] = in[16 * i + q];
    poseidon2_bb::internal_round(s, rc_next[i], sumc[i]);
#pragma unroll
    for (int q = 0; q < 16; q++) o[16 * i + q] = s[q];
}
__global__ void k_bb_renorm(const u32* a, u32* o, u32 n) { IDX; o[i] = poseidon2_bb::renorm(a[i]); }
__global__ void k_bb_renorm_lazy(const u32* a, u32* o, u32 n) { IDX; o[i] = poseidon2_bb::renorm_lazy(a[i]); }
__global__ void k_bb_canonical_out(const u32* a, u32* o, u32 n) { IDX; o[i] = poseidon2_bb::canonical_out(a[i]); }
__global__ void k_bbc_sbox7(const u32* a, u32* o, u32 n) { IDX; o[i] = poseidon2_bb_coop::sbox7(a[i]); }
// n a multiple of 64: one word per lane, one state per 16-lane row
__global__ void k_bbc_external(const u32* x, u32* o, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    o[i] = poseidon2_bb_coop::external_layer(x[i]);
}

// ---------------------------------------------------------------- the host's own arithmetic
static const u64 GP = 0xFFFFFFFF00000001ULL;
static const u64 GR = 0xFFFFFFFFULL;   // 2^64 mod p
static const u64 BP = 2013265921ULL;   // 2^31 - 2^27 + 1
static u64 mulmod(u64 a, u64 b, u64 p) { return (u64)((u128)a * b % p); }
static u64 addmod(u64 a, u64 b, u64 p) { return (u64)(((u128)a + b) % p); }
static u64 submod(u64 a, u64 b, u64 p) { return (u64)(((u128)a + p - b % p) % p); }
static u64 powmod(u64 b, u64 e, u64 p) {
    u64 r = 1;
    for (b %= p; e; e >>= 1, b = mulmod(b, b, p))
        if (e & 1) r = mulmod(r, b, p);
    return r;
}
static u64 smod(i128 x, u64 p) { const i128 r = x % (i128)p; return (u64)(r < 0 ? r + (i128)p : r); }
static const u64 G_RINV = powmod(GR, GP - 2, GP);
static u64 g_sbox_mont(u64 w) {   // x R -> x^7 R
    const u64 x = mulmod(w % GP, G_RINV, GP);
    return mulmod(powmod(x, 7, GP), GR, GP);
}
static const u64 G_CIRC[12] = {GL_POSEIDON_MDS_CIRC_LIST};
static const u64 G_DIAG[12] = {GL_POSEIDON_MDS_DIAG_LIST};
static const u64 G_RC[360] = {GL_POSEIDON_ALL_ROUND_CONSTANTS_LIST};
// res[q] = sum_i s[(i + q) % 12] CIRC[i] + s[q] DIAG[q] on residues, then + (round `rnext`'s constants) R when rnext < 30
static void g_mds(const u64* v, u64* out, int rnext) {
    for (int q = 0; q < 12; q++) {
        u128 acc = (u128)(v[q] % GP) * G_DIAG[q];   // entries < 2^6: twelve terms fit 128 bits with room
        for (int i = 0; i < 12; i++) acc += (u128)(v[(i + q) % 12] % GP) * G_CIRC[i];
        u64 r = (u64)(acc % GP);
        if (rnext < 30) r = addmod(r, mulmod(G_RC[12 * rnext + q] % GP, GR, GP), GP);
        out[q] = r;
    }
}
static const u64 B_R = (1ULL << 32) % BP;
static const u64 B_RINV = powmod(B_R, BP - 2, BP);
// the scale sequence of csrc/poseidon2_bb.hpp restated: a word holds kappa 2^32 x; a layer divides kappa by 2^32, an s-box takes kappa^7
static u64 b_kappa(int external_rounds_done) {
    u64 k = B_RINV;   // Montgomery input through the initial layer
    for (int r = 0; r < external_rounds_done; r++) k = mulmod(powmod(k, 7, BP), B_RINV, BP);
    return k;
}
static const u64 B_K_INT = b_kappa(4), B_K_FINAL = b_kappa(8);
static const u64 B_FIX6 = powmod(powmod(B_K_INT, 6, BP), BP - 2, BP);   // kappa^-6 of the internal rounds
static const int B_SH[15] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15};
static const u64 B_HALF_P = (BP + 1) / 2, B_LAZY_MAX = 2 * BP + (1ULL << 15) + 1;
static const long long SLIM = 2073663898LL;   // floor(1.03 p)
static void b_external(const u64* x, u64* out) {   // M_E on residues
    u64 nn[16];
    for (int b = 0; b < 16; b += 4) {
        const u64 x0 = x[b] % BP, x1 = x[b + 1] % BP, x2 = x[b + 2] % BP, x3 = x[b + 3] % BP;
        nn[b] = (2 * x0 + 3 * x1 + x2 + x3) % BP;
        nn[b + 1] = (x0 + 2 * x1 + 3 * x2 + x3) % BP;
        nn[b + 2] = (x0 + x1 + 2 * x2 + 3 * x3) % BP;
        nn[b + 3] = (3 * x0 + x1 + x2 + 2 * x3) % BP;
    }
    for (int i = 0; i < 16; i++) out[i] = (nn[i] + nn[i & 3] + nn[4 + (i & 3)] + nn[8 + (i & 3)] + nn[12 + (i & 3)]) % BP;
}

// ---------------------------------------------------------------- plumbing
static int hip_failed = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        hipError_t e_ = (x);                                              \
        if (e_ != hipSuccess) {                                           \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                \
            hip_failed = 1;                                               \
        }                                                                 \
    } while (0)
static std::vector<void*> allocations;
template <class T>
static T* up(const std::vector<T>& v) {
    T* d = nullptr;
    if (hip_failed) return d;
    CHECK(hipMalloc(&d, v.size() * sizeof(T) + 16));
    if (!hip_failed) { allocations.push_back(d); CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); }
    return d;
}
template <class T>
struct Out {
    T* d = nullptr;
    std::vector<T> h;
    explicit Out(size_t n) : h(n) {
        if (hip_failed) return;
        CHECK(hipMalloc(&d, n * sizeof(T) + 16));
        if (!hip_failed) { allocations.push_back(d); CHECK(hipMemset(d, 0xA5, n * sizeof(T))); }
    }
    void fetch() { if (!hip_failed) CHECK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost)); }
};
#define LAUNCH_B(kernel, bs, n, ...)                                                            \
    do {                                                                                        \
        if (!hip_failed) {                                                                      \
            kernel<<<((n) + (bs) - 1) / (bs), (bs)>>>(__VA_ARGS__, (u32)(n));                   \
            CHECK(hipGetLastError());                                                           \
        }                                                                                       \
    } while (0)
#define LAUNCH(kernel, n, ...) LAUNCH_B(kernel, 256, n, __VA_ARGS__)

static long cases = 0, bad = 0;
static void report(bool ok, const char* what, size_t i, const std::string& detail) {
    cases++;
    if (ok) return;
    if (++bad <= 16) printf("mismatch %s[%zu]: %s\n", what, i, detail.c_str());
}
static std::string hx(std::initializer_list<u64> v) {
    std::string s;
    char buf[32];
    for (u64 x : v) { snprintf(buf, sizeof buf, "%016llx ", x); s += buf; }
    return s;
}

int main() {
    std::mt19937_64 rng(20261019);
    const int NR = 1 << 16;
    // ---------------- Goldilocks operand sets
    std::vector<u64> any = mul_mont_cases::edge_values();
    for (u64 v : {2ULL, 0xFFFFFFFEULL, 1ULL << 63, GP - (1ULL << 32), (GP - 1) / 2, (GP + 1) / 2, GP - 2, 0x8080808080808080ULL, 0x7F7F7F7F7F7F7F7FULL,
                  0x00FF00FF00FF00FFULL, 0xFF00FF00FF00FF00ULL, 0x80007FFF0100FF80ULL, 0xFFFFFFFF00000002ULL, 0xFFFFFFFFFFFF0000ULL})
        any.push_back(v);
    std::vector<u64> can;
    for (u64 v : any) can.push_back(v >= GP ? v - GP : v);
    std::vector<u64> ua, ub, uc, rcb;              // any-u64 pairs (and a third any-u64 operand); a canonical partner for add_rc
    for (size_t x = 0; x < any.size(); x++)
        for (size_t y = 0; y < any.size(); y++) { ua.push_back(any[x]); ub.push_back(any[y]); uc.push_back(any[(x + 2 * y + 1) % any.size()]); rcb.push_back(can[y]); }
    // sums that wrap twice (poseidon_gl_coop::add_lazy's second carry): a + b - 2^64 in [2^64 - 2^32 + 1, 2^64 - 2]
    for (u64 i = 0; i < 32; i++)
        for (u64 j = 0; j < 32; j++) { ua.push_back(~0ULL - i * 0x08000000ULL); ub.push_back(~0ULL - j * 0x07FFFFFFULL); uc.push_back(~0ULL - i); rcb.push_back(GP - 1 - j); }
    for (int t = 0; t < NR; t++) {
        u64 p = rng(), q = rng();
        if (t % 8 == 1) q = (u64)(0 - p) + (t % 5) - 2;                 // sums next to 2^64
        if (t % 8 == 2) q = p + (t % 3) - 1;                            // differences next to 0
        if (t % 8 == 3) { p |= 0xFFFFFFFF00000000ULL; q |= 0xFFFFFFFF00000000ULL; }   // both within 2^32 of 2^64: the double carry
        if (t % 8 == 4) q = any[rng() % any.size()];
        if (t % 8 == 5) p = GP + (rng() & 0xFFFFFFFFULL) - 1;           // the representatives above p
        ua.push_back(p); ub.push_back(q); uc.push_back(t % 4 ? rng() : ~0ULL - (rng() & 0xFFFF)); rcb.push_back(t % 16 ? rng() % GP : GP - 1 - (rng() & 0xFF));
    }
    const size_t nu = ua.size();
    // fold_halves: sl, sh < 2^63 (sh >> 32 < 2^31)
    const std::vector<u64> half = {0, 1, 0xFFFFFFFFULL, 1ULL << 32, (1ULL << 32) + 1, 0x7FFFFFFFFFFFFFFFULL, 0x7FFFFFFF00000000ULL, 0x7FFFFFFEFFFFFFFFULL,
                                   0x00000001FFFFFFFFULL, 0x7FFFFFFF00000001ULL, 0x00000000FFFFFFFEULL, 0x7FFFFFFFFFFFFFFEULL, 1ULL << 62, 0x000003FFFFFFFFFFULL,
                                   0x3FFFFFFFFFFFFFFFULL, 0x0000100000000000ULL};
    std::vector<u64> hl, hh;
    for (u64 x : half) for (u64 y : half) { hl.push_back(x); hh.push_back(y); }
    for (int t = 0; t < NR; t++) {
        u64 x = rng() >> 1, y = rng() >> 1;
        if (t % 4 == 1) y |= 0xFFFFFF00ULL;                              // the low word of sh next to 2^32: the carry
        if (t % 4 == 2) { x = rng() >> 23; y = rng() >> 23; }            // the sizes an MDS row sum has
        if (t % 8 == 3) { x |= 0x7FFFFFFF00000000ULL; y |= 0xFFFFFFFFULL; }
        hl.push_back(x); hh.push_back(y);
    }
    // row_sum: rows of 16 words, each near 2^64; then random rows
    std::vector<u64> rows;
    for (int r = 0; r < 64; r++)
        for (int l = 0; l < 16; l++)
            rows.push_back(r == 0 ? ~0ULL : r == 1 ? GP - 1 : r == 2 ? (l & 1 ? ~0ULL : 0) : r == 3 ? ~0ULL - (u64)l : r < 32 ? ~0ULL - (rng() & 0xFFFFFFFFULL) : r < 48 ? rng() | 0xFFFFFFFF00000000ULL : any[rng() % any.size()]);
    for (int t = 0; t < NR; t++) rows.push_back(t % 3 ? rng() : ~0ULL - (rng() >> 33));
    // fold_rows_rare_carry<12>: accumulators as the matrix pipe leaves them, non-negative and below 2^45.  Wave by wave: no lane
    // carries; one lane carries (in one word); every lane carries (in every word); then random waves
    const u32 NF = 64 * 48 + 37;
    std::vector<u64> flo(12 * NF), fhi(12 * NF);
    for (u32 i = 0; i < NF; i++) {
        const u32 wave = i / 64, lane = i % 64, kind = wave < 36 ? wave % 3 : 3;
        for (int q = 0; q < 12; q++) {
            u64 lo = rng() >> 19, hi = rng() >> 19;                       // < 2^45
            if (kind != 3) hi &= ~0x80000000ULL;                          // low word of hi below 2^31: no carry (t >> 32 < 2^14)
            const bool carry = kind == 2 || (kind == 1 && lane == (wave * 7) % 64 && q == (int)(wave % 12));
            if (carry) { hi |= 0xFFFFFFFFULL; hi -= rng() & 0xFF; lo |= 0x100ULL << 32; }   // (u32)hi within 2^8 of 2^32, t >> 32 >= 2^8
            if (kind == 3 && q == 5 && lane % 16 == 3) hi |= 0xFFFFF000ULL;
            flo[12 * i + q] = lo; fhi[12 * i + q] = hi;
        }
    }
    // states of arbitrary u64 words for mds_layer_mfma and partial_group
    const u32 N_EDGE_STATES = 200, NS = N_EDGE_STATES + (1 << 14);
    std::vector<u64> st(12 * NS);
    for (u32 i = 0; i < NS; i++)
        for (int q = 0; q < 12; q++) {
            u64 v = rng();
            if (i == 0) v = ~0ULL;
            else if (i == 1) v = 0x8080808080808080ULL;
            else if (i == 2) v = 0;
            else if (i == 3) v = GP - 1;
            else if (i == 4) v = 0x7F7F7F7F7F7F7F7FULL;
            else if (i < 5 + any.size()) v = any[(i - 5 + (size_t)q * (i % 3)) % any.size()];
            else if (i < 100) { v = rng() & 0xFFFFFFFEULL; if ((q + i) & 1) v += GP; }       // canonical words and their + p representatives, mixed
            else if (i < 150) v = (q + i) % 3 ? (rng() | 0xFFFFFFFF00000000ULL) : (rng() & 0xFFFFFFFFULL);
            else if (i < N_EDGE_STATES) v = any[rng() % any.size()];
            st[12 * i + q] = v;
        }
    const int MDS_RNEXT[5] = {1, 4, 26, 29, poseidon_gl::MFMA_NO_RC}, GROUP4_R0[5] = {4, 8, 12, 16, 20}, GROUP2_R0 = 24;

    // ---------------- BabyBear operand sets
    std::vector<u32> sx;                             // sbox7: signed words within +-1.03 p
    for (long long v : {0LL, 1LL, 2LL, 1LL << 27, (1LL << 27) - 1, (long long)(BP - 1) / 2, (long long)(BP + 1) / 2, (long long)BP - 1, (long long)BP, (long long)BP + 1,
                        SLIM - 1, SLIM, 0x7F7F7F7FLL % (long long)BP, (1LL << 31) % (long long)BP}) {
        sx.push_back((u32)(int)v);
        if (v) sx.push_back((u32)(int)-v);
    }
    for (int t = 0; t < NR; t++) sx.push_back((u32)(int)(t % 16 ? (long long)(rng() % (2 * SLIM + 1)) - SLIM : (t % 32 ? SLIM : -SLIM) - (long long)(rng() % 4096) * (t % 32 ? 1 : -1)));
    std::vector<u32> cw = {0, 1, 2, (u32)BP - 1, (u32)BP - 2, (u32)((BP - 1) / 2), (u32)((BP + 1) / 2), 1u << 27, (1u << 27) - 1, (u32)((1ULL << 31) % BP), (u32)B_R,
                           (u32)(BP - B_R)};   // canonical words (for renorm / canonical_out / the cooperative s-box)
    for (int t = 0; t < NR; t++) cw.push_back((u32)(rng() % BP));
    std::vector<u32> lw = cw;                        // renorm_lazy: and the words up to 2p
    for (int t = 0; t < 4096; t++) lw.push_back((u32)(BP + rng() % BP));
    lw.push_back(2 * (u32)BP - 1);
    const u32 NB = 64 + (1 << 13);                   // states for external_layer: lazy words in [0, 2p), constants canonical
    std::vector<u32> es(16 * NB), ec(16 * NB);
    for (u32 i = 0; i < NB; i++)
        for (int q = 0; q < 16; q++) {
            u32 v = (u32)(rng() % (2 * BP)), c = (u32)(rng() % BP);
            if (i == 0) { v = 2 * (u32)BP - 1; c = (u32)BP - 1; }
            else if (i == 1) { v = 2 * (u32)BP - 1; c = 0; }
            else if (i == 2) { v = 0; c = 0; }
            else if (i == 3) { v = (u32)BP - 1; c = (u32)BP - 1; }
            else if (i == 4) v = (q & 1) ? 2 * (u32)BP - 1 : 0;
            else if (i < 64) v = (q == (int)(i % 16)) ? 2 * (u32)BP - 1 - (i / 16) : (i & 32 ? 0 : v);
            es[16 * i + q] = v; ec[16 * i + q] = c;
        }
    const u32 NI = 64 + (1 << 13);                   // internal_round: word 0 signed within +-p, words 1..15 below LAZY_MAX
    std::vector<u32> is(16 * NI), irc(NI), isum(NI);
    for (u32 i = 0; i < NI; i++) {
        const long long w0s[6] = {(long long)BP - 1, -((long long)BP - 1), 0, 1, -1, (long long)(BP + 1) / 2};
        is[16 * i] = i < 48 ? (u32)(int)w0s[i % 6] : (u32)(int)((long long)(rng() % (2 * BP - 1)) - (long long)(BP - 1));
        for (int q = 1; q < 16; q++) {
            u32 v = (u32)(rng() % B_LAZY_MAX);
            if (i < 48) v = (i / 6) % 4 == 0 ? 0 : (i / 6) % 4 == 1 ? (u32)B_LAZY_MAX - 1 : (i / 6) % 4 == 2 ? ((q & 1) ? (u32)B_LAZY_MAX - 1 : 0) : v;
            is[16 * i + q] = v;
        }
        irc[i] = i < 64 ? (i & 1 ? (u32)BP - 1 : 0) : (u32)(rng() % BP);
        isum[i] = i < 64 ? (i & 2 ? (u32)BP - 1 : 0) : (u32)(rng() % BP);
    }
    std::vector<u32> crow;                           // the cooperative external layer: canonical rows of 16
    for (int r = 0; r < 16 + (1 << 12); r++)
        for (int l = 0; l < 16; l++) crow.push_back(r == 0 ? (u32)BP - 1 : r == 1 ? 0 : r == 2 ? (l & 1 ? (u32)BP - 1 : 0) : r < 16 ? (l == r ? (u32)BP - 1 : 1) : (u32)(rng() % BP));

    // ---------------- upload, launch everything, synchronize once
    u64 *d_ua = up(ua), *d_ub = up(ub), *d_uc = up(uc), *d_rcb = up(rcb), *d_hl = up(hl), *d_hh = up(hh), *d_rows = up(rows), *d_flo = up(flo), *d_fhi = up(fhi),
        *d_st = up(st);
    u32 *d_sx = up(sx), *d_cw = up(cw), *d_lw = up(lw), *d_es = up(es), *d_ec = up(ec), *d_is = up(is), *d_irc = up(irc), *d_isum = up(isum), *d_crow = up(crow);
    Out<u64> o_tm(nu), o_fm(nu), o_arc(nu), o_ml(nu), o_mal(nu), o_r128(nu), o_sb(nu), o_fh(hl.size()), o_sl(nu), o_al(nu), o_rs(rows.size()), o_fr(12 * NF);
    std::vector<Out<u64>> o_mds, o_mds8, o_g4;
    for (int k = 0; k < 5; k++) { o_mds.emplace_back(12 * NS); o_mds8.emplace_back(12 * NS); o_g4.emplace_back(12 * NS); }
    Out<u64> o_g2(12 * NS);
    Out<u32> o_s7(sx.size()), o_ef(16 * NB), o_et(16 * NB), o_ir(16 * NI), o_rn(cw.size()), o_rl(lw.size()), o_co(cw.size()), o_cs7(cw.size()), o_ce(crow.size());
    LAUNCH(k_to_mont, nu, d_ua, o_tm.d);
    LAUNCH(k_from_mont, nu, d_ua, o_fm.d);
    LAUNCH(k_add_rc, nu, d_ua, d_rcb, o_arc.d);
    LAUNCH(k_mul_lazy, nu, d_ua, d_ub, o_ml.d);
    LAUNCH(k_mul_add_lazy, nu, d_ua, d_ub, d_uc, o_mal.d);
    LAUNCH(k_reduce128_lazy, nu, d_ua, d_ub, o_r128.d);
    LAUNCH(k_sbox, nu, d_ua, o_sb.d);
    LAUNCH(k_fold_halves, hl.size(), d_hl, d_hh, o_fh.d);
    LAUNCH(k_sub_lazy, nu, d_ua, d_ub, o_sl.d);
    LAUNCH(k_coop_add_lazy, nu, d_ua, d_ub, o_al.d);
    static_assert(((64 * 16 + (1 << 16)) % 64) == 0, "row_sum runs whole waves");
    LAUNCH_B(k_row_sum, 64, rows.size(), d_rows, o_rs.d);
    LAUNCH(k_fold_rows, NF, d_flo, d_fhi, o_fr.d);
    for (int k = 0; k < 5; k++) {
        LAUNCH(k_mds_mfma<0>, NS, d_st, o_mds[k].d, MDS_RNEXT[k]);
        LAUNCH(k_mds_mfma<8>, NS, d_st, o_mds8[k].d, MDS_RNEXT[k]);
        LAUNCH(k_partial_group<4>, NS, d_st, o_g4[k].d, GROUP4_R0[k]);
    }
    LAUNCH(k_partial_group<2>, NS, d_st, o_g2.d, GROUP2_R0);
    LAUNCH(k_bb_sbox7, sx.size(), d_sx, o_s7.d);
    LAUNCH(k_bb_external<false>, NB, d_es, d_ec, o_ef.d);
    LAUNCH(k_bb_external<true>, NB, d_es, d_ec, o_et.d);
    LAUNCH(k_bb_internal, NI, d_is, d_irc, d_isum, o_ir.d);
    LAUNCH(k_bb_renorm, cw.size(), d_cw, o_rn.d);
    LAUNCH(k_bb_renorm_lazy, lw.size(), d_lw, o_rl.d);
    LAUNCH(k_bb_canonical_out, cw.size(), d_cw, o_co.d);
    LAUNCH(k_bbc_sbox7, cw.size(), d_cw, o_cs7.d);
    static_assert(((16 * (16 + (1 << 12))) % 64) == 0, "the cooperative layer runs whole waves");
    LAUNCH_B(k_bbc_external, 64, crow.size(), d_crow, o_ce.d);
    if (rows.size() % 64 || crow.size() % 64) { printf("row sets must fill whole waves\n"); hip_failed = 1; }
    if (!hip_failed) CHECK(hipDeviceSynchronize());
    o_tm.fetch(); o_fm.fetch(); o_arc.fetch(); o_ml.fetch(); o_mal.fetch(); o_r128.fetch(); o_sb.fetch(); o_fh.fetch(); o_sl.fetch(); o_al.fetch(); o_rs.fetch(); o_fr.fetch();
    for (int k = 0; k < 5; k++) { o_mds[k].fetch(); o_mds8[k].fetch(); o_g4[k].fetch(); }
    o_g2.fetch(); o_s7.fetch(); o_ef.fetch(); o_et.fetch(); o_ir.fetch(); o_rn.fetch(); o_rl.fetch(); o_co.fetch(); o_cs7.fetch(); o_ce.fetch();
    for (void* p : allocations) (void)hipFree(p);
    if (hip_failed) return 2;

    // ---------------- compare: Goldilocks
    for (size_t i = 0; i < nu; i++) {
        const u64 a = ua[i], b = ub[i], c = uc[i], am = a % GP, bm = b % GP;
        report(o_tm.h[i] % GP == mulmod(am, GR, GP), "to_mont", i, hx({a, o_tm.h[i]}));
        report(o_fm.h[i] == mulmod(am, G_RINV, GP), "from_mont", i, hx({a, o_fm.h[i]}));                       // canonical: equality, not congruence
        report(o_arc.h[i] % GP == addmod(am, rcb[i], GP), "add_rc", i, hx({a, rcb[i], o_arc.h[i]}));
        report(o_ml.h[i] % GP == mulmod(am, bm, GP), "mul_lazy", i, hx({a, b, o_ml.h[i]}));
        report(o_mal.h[i] % GP == addmod(mulmod(am, bm, GP), c % GP, GP), "mul_add_lazy", i, hx({a, b, c, o_mal.h[i]}));
        report(o_r128.h[i] % GP == addmod(am, mulmod(bm, GR, GP), GP), "reduce128_lazy", i, hx({a, b, o_r128.h[i]}));
        report(o_sb.h[i] % GP == g_sbox_mont(a), "poseidon_gl::sbox", i, hx({a, o_sb.h[i]}));
        report(o_sl.h[i] % GP == submod(am, bm, GP), "sub_lazy", i, hx({a, b, o_sl.h[i]}));
        report(o_al.h[i] % GP == addmod(am, bm, GP), "poseidon_gl_coop::add_lazy", i, hx({a, b, o_al.h[i]}));
    }
    for (size_t i = 0; i < hl.size(); i++)
        report(o_fh.h[i] % GP == (u64)(((u128)hl[i] + ((u128)hh[i] << 32)) % GP), "fold_halves", i, hx({hl[i], hh[i], o_fh.h[i]}));
    for (size_t r = 0; r < rows.size() / 16; r++) {
        u64 want = 0;
        for (int l = 0; l < 16; l++) want = addmod(want, rows[16 * r + l] % GP, GP);
        for (int l = 0; l < 16; l++) report(o_rs.h[16 * r + l] % GP == want, "row_sum", 16 * r + l, hx({rows[16 * r + l], o_rs.h[16 * r + l], want}));
    }
    for (size_t i = 0; i < (size_t)12 * NF; i++)
        report(o_fr.h[i] % GP == (u64)(((u128)flo[i] + ((u128)fhi[i] << 32)) % GP), "fold_rows_rare_carry", i, hx({flo[i], fhi[i], o_fr.h[i]}));
    for (u32 i = 0; i < NS; i++) {
        u64 want[12];
        for (int k = 0; k < 5; k++) {
            g_mds(&st[12 * i], want, MDS_RNEXT[k]);
            for (int q = 0; q < 12; q++) {
                report(o_mds[k].h[12 * i + q] % GP == want[q], "mds_layer_mfma<0>", 12 * (size_t)i + q, hx({(u64)MDS_RNEXT[k], st[12 * i + q], o_mds[k].h[12 * i + q], want[q]}));
                if (q >= 8) report(o_mds8[k].h[12 * i + q] % GP == want[q], "mds_layer_mfma<8>", 12 * (size_t)i + q, hx({(u64)MDS_RNEXT[k], o_mds8[k].h[12 * i + q], want[q]}));
            }
        }
        for (int k = 0; k < 6; k++) {   // G rounds from r0: s-box on word 0 (Montgomery form), MDS, the next round's constants
            const int G = k < 5 ? 4 : 2, r0 = k < 5 ? GROUP4_R0[k] : GROUP2_R0;
            u64 v[12];
            for (int q = 0; q < 12; q++) v[q] = st[12 * i + q] % GP;
            for (int j = 0; j < G; j++) {
                v[0] = g_sbox_mont(v[0]);
                g_mds(v, want, r0 + j + 1);
                for (int q = 0; q < 12; q++) v[q] = want[q];
            }
            const std::vector<u64>& got = k < 5 ? o_g4[k].h : o_g2.h;
            for (int q = 0; q < 12; q++)
                report(got[12 * i + q] % GP == v[q], G == 4 ? "partial_group<4>" : "partial_group<2>", 12 * (size_t)i + q, hx({(u64)r0, st[12 * i + q], got[12 * i + q], v[q]}));
        }
    }
    // ---------------- compare: BabyBear
    const u64 rinv6 = powmod(B_RINV, 6, BP);
    for (size_t i = 0; i < sx.size(); i++) {
        const u64 want = mulmod(powmod(smod((int)sx[i], BP), 7, BP), rinv6, BP);   // (x R)^7 / R^6
        report(o_s7.h[i] > 0 && o_s7.h[i] < 2 * BP && o_s7.h[i] % BP == want, "poseidon2_bb::sbox7", i, hx({sx[i], o_s7.h[i], want}));
    }
    for (u32 i = 0; i < NB; i++) {
        u64 x[16], m[16];
        for (int q = 0; q < 16; q++) x[q] = es[16 * i + q];
        b_external(x, m);
        for (int q = 0; q < 16; q++) {
            const u64 want = mulmod(addmod(m[q], ec[16 * i + q], BP), B_RINV, BP);
            const long long sg = (int)o_et.h[16 * i + q];
            report(o_ef.h[16 * i + q] == want, "external_layer<false>", 16 * (size_t)i + q, hx({es[16 * i + q], ec[16 * i + q], o_ef.h[16 * i + q], want}));
            report(smod(sg, BP) == want && sg <= SLIM && sg >= -SLIM, "external_layer<true>", 16 * (size_t)i + q, hx({es[16 * i + q], ec[16 * i + q], o_et.h[16 * i + q], want}));
        }
    }
    for (u32 i = 0; i < NI; i++) {
        const u32* s = &is[16 * i];
        u64 sum = isum[i];
        for (int q = 1; q < 16; q++) sum += s[q];
        const u64 part = mulmod(sum % BP, B_RINV, BP);
        const u64 x0 = smod((int)s[0], BP);
        const u64 y0 = mulmod(mulmod(mulmod(powmod(x0, 7, BP), rinv6, BP), B_FIX6, BP), B_RINV, BP);   // the s-box's output times kappa^-6 / R
        const u64 full = addmod(part, y0, BP);
        const long long n0 = (int)o_ir.h[16 * i];
        report(smod(n0, BP) == submod(addmod(part, irc[i], BP), y0, BP) && n0 > -(long long)BP && n0 < (long long)BP, "internal_round word 0", i,
               hx({s[0], irc[i], isum[i], o_ir.h[16 * i]}));
        for (int q = 0; q < 15; q++) {
            const u64 want = addmod(addmod(full, B_HALF_P, BP), mulmod(mulmod(s[q + 1] % BP, (1ULL << B_SH[q]) % BP, BP), B_RINV, BP), BP);
            const u64 got = o_ir.h[16 * i + q + 1];
            report(got < B_LAZY_MAX && got % BP == want, "internal_round lazy word", 16 * (size_t)i + q + 1, hx({s[q + 1], got, want}));
        }
    }
    const u64 kf_inv = powmod(B_K_FINAL, BP - 2, BP);
    for (size_t i = 0; i < cw.size(); i++) {
        report(o_rn.h[i] == mulmod(cw[i], kf_inv, BP), "renorm", i, hx({cw[i], o_rn.h[i]}));
        report(o_co.h[i] == mulmod(mulmod(cw[i], kf_inv, BP), B_RINV, BP), "canonical_out", i, hx({cw[i], o_co.h[i]}));
        report(o_cs7.h[i] == mulmod(powmod(cw[i], 7, BP), rinv6, BP), "poseidon2_bb_coop::sbox7", i, hx({cw[i], o_cs7.h[i]}));
    }
    for (size_t i = 0; i < lw.size(); i++)
        report(o_rl.h[i] < 2 * BP && o_rl.h[i] % BP == mulmod(lw[i] % BP, kf_inv, BP), "renorm_lazy", i, hx({lw[i], o_rl.h[i]}));
    for (size_t r = 0; r < crow.size() / 16; r++) {
        u64 x[16], m[16];
        for (int q = 0; q < 16; q++) x[q] = crow[16 * r + q];
        b_external(x, m);
        for (int q = 0; q < 16; q++) report(o_ce.h[16 * r + q] == m[q], "poseidon2_bb_coop::external_layer", 16 * r + q, hx({crow[16 * r + q], o_ce.h[16 * r + q], m[q]}));
    }
    printf("cases=%ld mismatches=%ld\n", cases, bad);
    return bad != 0;
}

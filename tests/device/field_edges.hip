// The device arithmetic of csrc/gl_field.hpp, csrc/bb_field.hpp and csrc/field_traits.hpp on the GPU, one kernel per function, against
// 128-bit integer arithmetic mod p written HERE (nothing expected comes from the headers): the carry edges squared plus 2^16 seeded
// random operands per function, each drawn inside the function's stated domain.  Values only.  One launch per kernel (two of the accumulator's, whose constants are
// kernel arguments), one hipDeviceSynchronize, comparison on the host; prints "cases=N mismatches=M", exit status 1 on a mismatch, 2 on a HIP error.
// Built and run by tests/test_device_field_edges.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "field_traits.hpp"
#include "../host_shim/mul_mont_cases.hpp"

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;
typedef __int128 i128;
using gbk::BbF;
using gbk::GlF;

// ---------------------------------------------------------------- kernels: out[i] = f(in[i]...)
#define IDX const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return
__global__ void k_gl_add(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = gl::add(a[i], b[i]); }
__global__ void k_gl_sub(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = gl::sub(a[i], b[i]); }
__global__ void k_gl_mul(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = gl::mul(a[i], b[i]); }
__global__ void k_gl_mul_lazy(const u64* a, const u64* b, u64* o, u32 n) { IDX; o[i] = GlF::mul_lazy(a[i], b[i]); }
__global__ void k_gl_fold160(const u64* lo, const u64* hi, const u32* r4, u64* o, u32 n) {
    IDX;
    o[i] = gl::fold160((u32)lo[i], (u32)(lo[i] >> 32), (u32)hi[i], (u32)(hi[i] >> 32), r4[i]);
}
__global__ void k_gl_mulc(const u64* x, const u64* c_form, u64* o, u32 n) { IDX; o[i] = GlF::mulc(x[i], c_form[i]); }
__global__ void k_gl_emul(const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* o0, u64* o1, u32 n) {
    IDX;
    const gl::ext2 r = GlF::emul(gl::e2(a0[i], a1[i]), gl::e2(b0[i], b1[i]));
    o0[i] = r.c0; o1[i] = r.c1;
}
__global__ void k_gl_einv(const u64* a0, const u64* a1, u64* o0, u64* o1, u32 n) {
    IDX;
    const gl::ext2 r = GlF::einv(gl::e2(a0[i], a1[i]));
    o0[i] = r.c0; o1[i] = r.c1;
}
__global__ void k_bb_add(const u32* a, const u32* b, u32* o, u32 n) { IDX; o[i] = bb::add(a[i], b[i]); }
__global__ void k_bb_sub(const u32* a, const u32* b, u32* o, u32 n) { IDX; o[i] = bb::sub(a[i], b[i]); }
__global__ void k_bb_mul(const u32* a, const u32* b, u32* o, u32 n) { IDX; o[i] = bb::mul(a[i], b[i]); }
__global__ void k_bb_reduce(const u64* t, u32* o, u32 n) { IDX; o[i] = bb::reduce(t[i]); }
__global__ void k_bb_reduce_lazy(const u64* t, u32* o, u32 n) { IDX; o[i] = bb::reduce_lazy(t[i]); }
__global__ void k_bb_mul_lazy(const u32* a, const u32* b, u32* o, u32 n) { IDX; o[i] = bb::mul_lazy(a[i], b[i]); }
__global__ void k_bb_mul_signed(const u32* a, const u32* b, u32* o, u32* o_bias, u32 n) {
    IDX;
    o[i] = (u32)bb::mul_signed((int)a[i], (int)b[i]);
    o_bias[i] = (u32)bb::mul_signed((int)a[i], (int)b[i], bb::P);
}
__global__ void k_bb_reduce_signed(const u64* t, u32* o, u32 n) { IDX; o[i] = (u32)bb::reduce_signed(t[i]); }
__global__ void k_bb_add_lazy_mul(const u32* a, const u32* b, const u32* c, u32* o, u32 n) { IDX; o[i] = bb::mul(BbF::add_lazy(a[i], b[i]), c[i]); }
// chain i: two sums started from x0[i], x1[i], then len[i] terms terms[i * stride + t], each times the wave-uniform c0 / c1
__global__ void k_bb_acc(const u32* x0, const u32* x1, const u32* len, const u32* terms, u32 stride, u32 c0, u32 c1, u32* o0, u32* o1, u32 n) {
    IDX;
    BbF::Acc a0 = BbF::acc_from(x0[i]), a1 = BbF::acc_from(x1[i]);
    const u32* t = terms + (size_t)i * stride;
    for (u32 k = 0; k < len[i]; k++) BbF::acc_mac2(a0, a1, t[k], c0, c1);
    o0[i] = BbF::acc_finish(a0);
    o1[i] = BbF::acc_finish(a1);
}
__global__ void k_bb_emul(const u32* a, const u32* b, u32* o, u32 n) {   // [n][4] each
    IDX;
    const BbF::E r = BbF::emul(BbF::E{{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}}, BbF::E{{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]}});
    for (int k = 0; k < 4; k++) o[4 * i + k] = r.c[k];
}
__global__ void k_bb_einv(const u32* a, u32* o, u32 n) {
    IDX;
    const BbF::E r = BbF::einv(BbF::E{{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}});
    for (int k = 0; k < 4; k++) o[4 * i + k] = r.c[k];
}

// ---------------------------------------------------------------- the host's own arithmetic
static const u64 GP = 0xFFFFFFFF00000001ULL;
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
static const u64 B_RINV = powmod(1ULL << 32, BP - 2, BP);             // 2^-32 mod p: Montgomery word -> canonical
static u64 b_canon(u64 word) { return mulmod(word % BP, B_RINV, BP); }
static u32 b_word(u64 canonical) { return (u32)mulmod(canonical, (1ULL << 32) % BP, BP); }
// binomial extensions F[x]/(x^D - W) on canonical coordinates
template <int D>
static void emul_ref(const u64* a, const u64* b, u64* r, u64 W, u64 p) {
    u64 t[2 * D - 1] = {};
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) t[i + j] = addmod(t[i + j], mulmod(a[i], b[j], p), p);
    for (int k = 0; k < D; k++) r[k] = k + D < 2 * D - 1 ? addmod(t[k], mulmod(W, t[k + D], p), p) : t[k];
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
#define LAUNCH(kernel, n, ...)                                                                  \
    do {                                                                                        \
        if (!hip_failed) {                                                                      \
            kernel<<<((n) + 255) / 256, 256>>>(__VA_ARGS__, (u32)(n));                          \
            CHECK(hipGetLastError());                                                           \
        }                                                                                       \
    } while (0)

static long cases = 0, bad = 0;
static void report(bool ok, const char* what, size_t i, const std::string& detail) {
    cases++;
    if (ok) return;
    if (++bad <= 12) printf("mismatch %s[%zu]: %s\n", what, i, detail.c_str());
}
static std::string hx(std::initializer_list<u64> v) {
    std::string s;
    char buf[32];
    for (u64 x : v) { snprintf(buf, sizeof buf, "%016llx ", x); s += buf; }
    return s;
}

int main() {
    std::mt19937_64 rng(20261018);
    const int NR = 1 << 16;
    // ---- operand sets
    std::vector<u64> gl_any = mul_mont_cases::edge_values();
    for (u64 v : {2ULL, 0xFFFFFFFEULL, 1ULL << 48, 1ULL << 63, GP - (1ULL << 32), GP - (1ULL << 32) + 1, (GP - 1) / 2, (GP + 1) / 2, GP - 2}) gl_any.push_back(v);
    std::vector<u64> gl_can;                       // canonical: the same set, what is not below p taken down by p
    for (u64 v : gl_any) gl_can.push_back(v >= GP ? v - GP : v);
    const std::vector<u64> gl_small = {0, 1, 2, 0xFFFFFFFEULL, 0xFFFFFFFFULL, 1ULL << 32, (1ULL << 32) + 1, 1ULL << 48, 1ULL << 63, GP - (1ULL << 32),
                                       GP - (1ULL << 32) + 1, (GP - 1) / 2, (GP + 1) / 2, GP - 2, GP - 1};   // for the extension: its 4th power
    std::vector<u32> bb_w = {0, 1, 2, 1u << 27, (1u << 27) + 1, (u32)((BP - 1) / 2), (u32)((BP + 1) / 2), (u32)BP - 2, (u32)BP - 1};
    for (size_t k = 1, n0 = bb_w.size(); k < n0; k++) bb_w.push_back(b_word(bb_w[k]));   // and the words of those canonical values
    auto gcan = [&] { return rng() % GP; };
    auto bcan = [&] { return (u32)(rng() % BP); };

    // pairs: edges squared + random, per domain
    std::vector<u64> ca, cb, ua, ub;               // canonical pairs, any-u64 pairs
    for (u64 x : gl_can) for (u64 y : gl_can) { ca.push_back(x); cb.push_back(y); }
    for (u64 x : gl_any) for (u64 y : gl_any) { ua.push_back(x); ub.push_back(y); }
    for (int t = 0; t < NR; t++) {
        u64 x = gcan(), y = gcan();
        if (t % 8 == 1) y = GP - x + (t % 3) - 1;                      // sums next to p
        if (t % 8 == 2) y = x + (t % 3) - 1;                           // differences next to 0
        if (t % 8 == 3) y = (u64)(0 - x) + (t % 5) - 2;                // sums next to 2^64
        if (t % 8 == 4) x = gl_can[rng() % gl_can.size()];
        ca.push_back(x % GP); cb.push_back(y % GP);
        u64 p = rng(), q = rng();
        if (t % 8 == 5) p |= 0xFFFFFFFF00000000ULL;
        if (t % 8 == 6) q = gl_any[rng() % gl_any.size()];
        ua.push_back(p); ub.push_back(q);
    }
    // fold160: any four limbs, r4 <= 2^31
    std::vector<u64> f_lo = ua, f_hi = ub;
    std::vector<u32> f_r4;
    { const u32 r4s[] = {0, 1, 2, 255, 0x7FFFFFFFu, 0x80000000u};
      for (size_t i = 0; i < f_lo.size(); i++) f_r4.push_back(i % 7 == 6 ? (u32)(rng() % 0x80000001ULL) : r4s[i % 7 % 6]); }
    // mulc: canonical x, constant c in constant form c 2^64 mod p
    std::vector<u64> mc_form;
    for (u64 c : cb) mc_form.push_back(mulmod(c, 0xFFFFFFFFULL, GP));
    // Goldilocks extension
    std::vector<u64> ea0, ea1, eb0, eb1, ia0, ia1;
    for (u64 p : gl_small) for (u64 q : gl_small) {
        if (p | q) { ia0.push_back(p); ia1.push_back(q); }
        for (u64 r : gl_small) for (u64 s : gl_small) { ea0.push_back(p); ea1.push_back(q); eb0.push_back(r); eb1.push_back(s); }
    }
    for (int t = 0; t < NR; t++) {
        ea0.push_back(gcan()); ea1.push_back(gcan()); eb0.push_back(gcan()); eb1.push_back(gcan());
        ia0.push_back(gcan() | 1); ia1.push_back(t % 16 ? gcan() : 0);
        if (ia0.back() >= GP) ia0.back() -= GP;
    }
    // BabyBear words
    std::vector<u32> ba, bbv, bl_a, bl_b, bc;       // canonical pairs; (canonical, lazy < 2p) pairs; a third canonical word
    for (u32 x : bb_w) for (u32 y : bb_w) {
        ba.push_back(x); bbv.push_back(y);
        bl_a.push_back(x); bl_b.push_back(y);
        bl_a.push_back(x); bl_b.push_back(y + (u32)BP);
    }
    bl_a.push_back((u32)BP - 1); bl_b.push_back(2 * (u32)BP - 1);
    for (int t = 0; t < NR; t++) {
        u32 x = bcan(), y = bcan();
        if (t % 8 == 1) y = (u32)((BP - x + (t % 3) + BP - 1) % BP);
        if (t % 8 == 2) y = (u32)((x + (t % 3) + BP - 1) % BP);
        ba.push_back(x); bbv.push_back(y);
        bl_a.push_back(bcan()); bl_b.push_back((u32)(rng() % (2 * BP)));
    }
    for (size_t i = 0; i < ba.size(); i++) bc.push_back(i < bb_w.size() * bb_w.size() ? bb_w[(i * 7 + 3) % bb_w.size()] : bcan());
    // reduce / reduce_lazy: t < p 2^32
    std::vector<u64> rt = {0, 1, (BP << 32) - 1, (BP << 32) - 2, BP, BP - 1, 1ULL << 32, (1ULL << 32) - 1, 0x80000000ULL, (BP - 1) * (BP - 1), (BP - 1) << 32};
    for (size_t i = 0; i < bl_a.size(); i++) rt.push_back((u64)bl_a[i] * bl_b[i]);
    for (int t = 0; t < NR; t++) rt.push_back(t % 4 ? rng() % (BP << 32) : ((rng() % BP) << 32) | (t % 8 ? 0x80000000u : 0xFFFFFFFFu));
    // signed products: |a|, |b| <= 1.03 p
    const long long SLIM = 2073663898LL;           // floor(1.03 p)
    std::vector<long long> sedge;
    for (long long v : {0LL, 1LL, 2LL, 1LL << 27, (long long)(BP - 1) / 2, (long long)(BP + 1) / 2, (long long)BP - 1, (long long)BP, (long long)BP + 1, SLIM - 1, SLIM}) {
        sedge.push_back(v);
        if (v) sedge.push_back(-v);
    }
    std::vector<u32> sa, sb;
    for (long long x : sedge) for (long long y : sedge) { sa.push_back((u32)(int)x); sb.push_back((u32)(int)y); }
    for (int t = 0; t < NR; t++) {
        const long long x = (long long)(rng() % (2 * SLIM + 1)) - SLIM, y = t % 4 ? (long long)(rng() % (2 * SLIM + 1)) - SLIM : (t % 8 ? SLIM : -SLIM) - (long long)(rng() % 1024) * (t % 8 ? 1 : -1);
        sa.push_back((u32)(int)x); sb.push_back((u32)(int)y);
    }
    std::vector<u64> st = {0, 1, (1ULL << 38) - 1, 0x80000000ULL, (63ULL << 32) | 0x80000000ULL, 0xFFFFFFFFULL, 1ULL << 32, 71 * BP};   // reduce_signed: t < 2^38
    for (int t = 0; t < NR; t++) st.push_back(t % 16 ? rng() >> 26 : ((rng() >> 58) << 32) | 0x80000000ULL);
    // acc chains: 1, 2, 255 and 600 terms, every term equal to p - 1; then chains of random terms and lengths.  Two launches over the
    // same chains: both constants p - 1 (both sums and both carry registers at the largest product per term), then two other constants
    const u32 STRIDE = 600, ACC_C[2][2] = {{(u32)BP - 1, (u32)BP - 1}, {0x3C6EF372u % (u32)BP, b_word(BP - 1)}};
    std::vector<u32> ax0, ax1, alen, aterms;
    auto chain = [&](u32 len, u32 x0, u32 x1, int kind) {
        ax0.push_back(x0); ax1.push_back(x1); alen.push_back(len);
        for (u32 k = 0; k < STRIDE; k++) aterms.push_back(kind == 0 ? (u32)BP - 1 : kind == 1 ? bb_w[rng() % bb_w.size()] : bcan());
    };
    for (u32 len : {1u, 2u, 255u, 600u}) { chain(len, 0, 0, 0); chain(len, (u32)BP - 1, (u32)BP - 1, 0); }
    chain(0, 5, (u32)BP - 1, 0);
    for (int t = 0; t < 503; t++) chain(t % 4 == 0 ? 600 : (u32)(rng() % 601), bcan(), bcan(), 1 + t % 2);
    // BabyBear extension: [n][4] Montgomery words
    std::vector<u32> xa, xb, xi;
    { const u32 few[] = {0, 1, (u32)BP - 1, b_word(1), b_word(BP - 1), (u32)((BP + 1) / 2)};
      for (int m = 0; m < 6 * 6 * 6 * 6; m++) {
          const u32 e[4] = {few[m % 6], few[m / 6 % 6], few[m / 36 % 6], few[m / 216]};
          for (int k = 0; k < 4; k++) { xa.push_back(e[k]); xb.push_back(few[(m * 5 + k * 3 + 1) % 6]); }
          if (m) for (int k = 0; k < 4; k++) xi.push_back(e[k]);
      } }
    for (int t = 0; t < NR; t++)
        for (int k = 0; k < 4; k++) {
            xa.push_back(bcan()); xb.push_back(bcan());
            xi.push_back(t % 8 == 0 && k != t / 8 % 4 ? 0 : (u32)(1 + rng() % (BP - 1)));
        }

    // ---- upload, launch everything, synchronize once
    u64 *d_ca = up(ca), *d_cb = up(cb), *d_ua = up(ua), *d_ub = up(ub), *d_flo = up(f_lo), *d_fhi = up(f_hi), *d_mcf = up(mc_form);
    u32* d_fr4 = up(f_r4);
    u64 *d_ea0 = up(ea0), *d_ea1 = up(ea1), *d_eb0 = up(eb0), *d_eb1 = up(eb1), *d_ia0 = up(ia0), *d_ia1 = up(ia1);
    u32 *d_ba = up(ba), *d_bb = up(bbv), *d_bc = up(bc), *d_bla = up(bl_a), *d_blb = up(bl_b), *d_sa = up(sa), *d_sb = up(sb);
    u64 *d_rt = up(rt), *d_st = up(st);
    u32 *d_ax0 = up(ax0), *d_ax1 = up(ax1), *d_alen = up(alen), *d_aterms = up(aterms), *d_xa = up(xa), *d_xb = up(xb), *d_xi = up(xi);
    const size_t nc = ca.size(), nu = ua.size(), ne = ea0.size(), ni = ia0.size(), nb = ba.size(), nl = bl_a.size(), ns = sa.size();
    const size_t nchains = alen.size(), nx = xa.size() / 4, nxi = xi.size() / 4;
    Out<u64> o_add(nc), o_sub(nc), o_mul(nu), o_lazy(nu), o_f160(nu), o_mulc(nc), o_em0(ne), o_em1(ne), o_ei0(ni), o_ei1(ni);
    Out<u32> o_badd(nb), o_bsub(nb), o_bmul(nb), o_red(rt.size()), o_redl(rt.size()), o_bml(nl), o_sg(ns), o_sgb(ns), o_rs(st.size()), o_alm(nb);
    Out<u32> o_acc0(nchains), o_acc1(nchains), o_acc2(nchains), o_acc3(nchains), o_xm(4 * nx), o_xi(4 * nxi);
    LAUNCH(k_gl_add, nc, d_ca, d_cb, o_add.d);
    LAUNCH(k_gl_sub, nc, d_ca, d_cb, o_sub.d);
    LAUNCH(k_gl_mul, nu, d_ua, d_ub, o_mul.d);
    LAUNCH(k_gl_mul_lazy, nu, d_ua, d_ub, o_lazy.d);
    LAUNCH(k_gl_fold160, nu, d_flo, d_fhi, d_fr4, o_f160.d);
    LAUNCH(k_gl_mulc, nc, d_ca, d_mcf, o_mulc.d);
    LAUNCH(k_gl_emul, ne, d_ea0, d_ea1, d_eb0, d_eb1, o_em0.d, o_em1.d);
    LAUNCH(k_gl_einv, ni, d_ia0, d_ia1, o_ei0.d, o_ei1.d);
    LAUNCH(k_bb_add, nb, d_ba, d_bb, o_badd.d);
    LAUNCH(k_bb_sub, nb, d_ba, d_bb, o_bsub.d);
    LAUNCH(k_bb_mul, nb, d_ba, d_bb, o_bmul.d);
    LAUNCH(k_bb_reduce, rt.size(), d_rt, o_red.d);
    LAUNCH(k_bb_reduce_lazy, rt.size(), d_rt, o_redl.d);
    LAUNCH(k_bb_mul_lazy, nl, d_bla, d_blb, o_bml.d);
    LAUNCH(k_bb_mul_signed, ns, d_sa, d_sb, o_sg.d, o_sgb.d);
    LAUNCH(k_bb_reduce_signed, st.size(), d_st, o_rs.d);
    LAUNCH(k_bb_add_lazy_mul, nb, d_ba, d_bb, d_bc, o_alm.d);
    LAUNCH(k_bb_acc, nchains, d_ax0, d_ax1, d_alen, d_aterms, STRIDE, ACC_C[0][0], ACC_C[0][1], o_acc0.d, o_acc1.d);
    LAUNCH(k_bb_acc, nchains, d_ax0, d_ax1, d_alen, d_aterms, STRIDE, ACC_C[1][0], ACC_C[1][1], o_acc2.d, o_acc3.d);
    LAUNCH(k_bb_emul, nx, d_xa, d_xb, o_xm.d);
    LAUNCH(k_bb_einv, nxi, d_xi, o_xi.d);
    if (!hip_failed) CHECK(hipDeviceSynchronize());
    o_add.fetch(); o_sub.fetch(); o_mul.fetch(); o_lazy.fetch(); o_f160.fetch(); o_mulc.fetch(); o_em0.fetch(); o_em1.fetch(); o_ei0.fetch(); o_ei1.fetch();
    o_badd.fetch(); o_bsub.fetch(); o_bmul.fetch(); o_red.fetch(); o_redl.fetch(); o_bml.fetch(); o_sg.fetch(); o_sgb.fetch(); o_rs.fetch(); o_alm.fetch();
    o_acc0.fetch(); o_acc1.fetch(); o_acc2.fetch(); o_acc3.fetch(); o_xm.fetch(); o_xi.fetch();
    for (void* p : allocations) (void)hipFree(p);
    if (hip_failed) return 2;

    // ---- compare
    for (size_t i = 0; i < nc; i++) {
        report(o_add.h[i] == addmod(ca[i], cb[i], GP), "gl::add", i, hx({ca[i], cb[i], o_add.h[i]}));
        report(o_sub.h[i] == submod(ca[i], cb[i], GP), "gl::sub", i, hx({ca[i], cb[i], o_sub.h[i]}));
        report(o_mulc.h[i] == mulmod(ca[i], cb[i], GP), "GlF::mulc", i, hx({ca[i], cb[i], mc_form[i], o_mulc.h[i]}));
    }
    for (size_t i = 0; i < nu; i++) {
        const u64 want = mulmod(ua[i] % GP, ub[i] % GP, GP);
        report(o_mul.h[i] == want, "gl::mul", i, hx({ua[i], ub[i], o_mul.h[i]}));
        report(o_lazy.h[i] % GP == want, "GlF::mul_lazy", i, hx({ua[i], ub[i], o_lazy.h[i]}));
        // lo + 2^64 hi + 2^128 r4 with 2^64 = 2^32 - 1 and 2^128 = -2^32 (mod p)
        const u64 f = submod(addmod(f_lo[i] % GP, mulmod(f_hi[i] % GP, 0xFFFFFFFFULL, GP), GP), mulmod(f_r4[i], 1ULL << 32, GP), GP);
        report(o_f160.h[i] % GP == f, "gl::fold160", i, hx({f_lo[i], f_hi[i], f_r4[i], o_f160.h[i]}));
    }
    for (size_t i = 0; i < ne; i++) {
        const u64 a[2] = {ea0[i], ea1[i]}, b[2] = {eb0[i], eb1[i]};
        u64 r[2];
        emul_ref<2>(a, b, r, 7, GP);
        report(o_em0.h[i] == r[0] && o_em1.h[i] == r[1], "GlF::emul", i, hx({a[0], a[1], b[0], b[1], o_em0.h[i], o_em1.h[i]}));
    }
    for (size_t i = 0; i < ni; i++) {
        const u64 a[2] = {ia0[i], ia1[i]}, g[2] = {o_ei0.h[i], o_ei1.h[i]};
        u64 r[2];
        emul_ref<2>(a, g, r, 7, GP);
        report(g[0] < GP && g[1] < GP && r[0] == 1 && r[1] == 0, "GlF::einv", i, hx({a[0], a[1], g[0], g[1]}));
    }
    for (size_t i = 0; i < nb; i++) {
        const u64 a = ba[i], b = bbv[i];
        report(o_badd.h[i] == (a + b) % BP, "bb::add", i, hx({a, b, o_badd.h[i]}));
        report(o_bsub.h[i] == (a + BP - b) % BP, "bb::sub", i, hx({a, b, o_bsub.h[i]}));
        report(o_bmul.h[i] == mulmod(mulmod(a, b, BP), B_RINV, BP), "bb::mul", i, hx({a, b, o_bmul.h[i]}));
        report(o_alm.h[i] == mulmod(mulmod(a + b, bc[i], BP), B_RINV, BP), "BbF::add_lazy then bb::mul", i, hx({a, b, bc[i], o_alm.h[i]}));
    }
    for (size_t i = 0; i < rt.size(); i++) {
        const u64 want = mulmod(rt[i] % BP, B_RINV, BP);
        report(o_red.h[i] == want, "bb::reduce", i, hx({rt[i], o_red.h[i]}));
        report(o_redl.h[i] < 2 * BP && o_redl.h[i] % BP == want, "bb::reduce_lazy", i, hx({rt[i], o_redl.h[i]}));
    }
    for (size_t i = 0; i < nl; i++)
        report(o_bml.h[i] < 2 * BP && o_bml.h[i] % BP == mulmod(mulmod(bl_a[i], bl_b[i], BP), B_RINV, BP), "bb::mul_lazy", i, hx({bl_a[i], bl_b[i], o_bml.h[i]}));
    for (size_t i = 0; i < ns; i++) {
        const long long a = (int)sa[i], b = (int)sb[i], r = (int)o_sg.h[i], t = a * b;
        const u64 want = mulmod(smod(t, BP), B_RINV, BP);
        // r 2^32 = a b - m p with a signed 32-bit m: |r| 2^32 <= |a b| + 2^31 p, which for |a|, |b| <= 1.03 p is < 0.9973 p 2^32
        const i128 mag = (i128)(r < 0 ? -r : r) << 32, lim = (i128)(t < 0 ? -t : t) + ((i128)BP << 31);
        const bool ok = smod(r, BP) == want && mag <= lim && (r < 0 ? -r : r) * 10000 < 9973 * (long long)BP + 10000;
        report(ok, "bb::mul_signed", i, hx({sa[i], sb[i], o_sg.h[i]}));
        report(o_sgb.h[i] > 0 && o_sgb.h[i] < 2 * BP && o_sgb.h[i] % BP == want && o_sgb.h[i] == (u32)(o_sg.h[i] + (u32)BP), "bb::mul_signed + p", i,
               hx({sa[i], sb[i], o_sgb.h[i]}));
    }
    for (size_t i = 0; i < st.size(); i++) {
        const long long r = (int)o_rs.h[i];
        // r 2^32 = t - m p, m in [-2^31, 2^31): t / 2^32 - p / 2 < r <= t / 2^32 + p / 2, within +-1.03 p for t < 2^38
        const i128 diff = ((i128)r << 32) - (i128)st[i];
        const bool ok = smod(r, BP) == mulmod(st[i] % BP, B_RINV, BP) && diff <= ((i128)BP << 31) && diff > -((i128)BP << 31) && (r < 0 ? -r : r) <= SLIM;
        report(ok, "bb::reduce_signed", i, hx({st[i], o_rs.h[i]}));
    }
    for (int l = 0; l < 2; l++)
        for (size_t i = 0; i < nchains; i++) {
            const u32 c0 = ACC_C[l][0], c1 = ACC_C[l][1], g0 = (l ? o_acc2 : o_acc0).h[i], g1 = (l ? o_acc3 : o_acc1).h[i];
            u128 s0 = (u128)ax0[i] << 32, s1 = (u128)ax1[i] << 32;       // the exact integer sums
            for (u32 k = 0; k < alen[i]; k++) { s0 += (u128)aterms[i * STRIDE + k] * c0; s1 += (u128)aterms[i * STRIDE + k] * c1; }
            const u64 w0 = mulmod((u64)(s0 % BP), B_RINV, BP), w1 = mulmod((u64)(s1 % BP), B_RINV, BP);
            report(g0 == w0 && g1 == w1, "BbF::acc_mac2 / acc_finish", i, hx({alen[i], ax0[i], ax1[i], c0, c1, g0, g1, w0, w1}));
        }
    for (size_t i = 0; i < nx; i++) {
        u64 a[4], b[4], r[4];
        for (int k = 0; k < 4; k++) { a[k] = b_canon(xa[4 * i + k]); b[k] = b_canon(xb[4 * i + k]); }
        emul_ref<4>(a, b, r, 11, BP);
        bool ok = true;
        for (int k = 0; k < 4; k++) ok = ok && o_xm.h[4 * i + k] == b_word(r[k]);
        report(ok, "BbF::emul", i, hx({xa[4 * i], xa[4 * i + 1], xa[4 * i + 2], xa[4 * i + 3], xb[4 * i], xb[4 * i + 1], xb[4 * i + 2], xb[4 * i + 3]}));
    }
    for (size_t i = 0; i < nxi; i++) {
        u64 a[4], g[4], r[4];
        bool ok = true;
        for (int k = 0; k < 4; k++) { a[k] = b_canon(xi[4 * i + k]); g[k] = b_canon(o_xi.h[4 * i + k]); ok = ok && o_xi.h[4 * i + k] < BP; }
        emul_ref<4>(a, g, r, 11, BP);
        report(ok && r[0] == 1 && r[1] == 0 && r[2] == 0 && r[3] == 0, "BbF::einv", i, hx({xi[4 * i], xi[4 * i + 1], xi[4 * i + 2], xi[4 * i + 3]}));
    }
    printf("cases=%ld mismatches=%ld\n", cases, bad);
    return bad != 0;
}

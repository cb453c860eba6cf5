// Goldilocks register DFTs (Dft<GlF>): the 2- to 64-point butterflies that kernels_ntt16.hip's and ntt_passes.hpp's radix-16 passes keep
// in registers.  The reference's generator makes every root of unity of order <= 64 a power of two (w_64 = 2^39, w_16 = 2^156 = -2^60,
// w_4 = 2^48; 2^96 = -1), so none of them needs a general multiplication: the twiddles are shifts + one fold.
// A header of their own so that a test program can call them one at a time (tests/host_shim/register_dfts.cpp on the CPU,
// tests/device/register_dfts.hip on the GPU).
#pragma once
#include "field_traits.hpp"
#include "gl_field.hpp"

namespace gbk {

template <class F>
struct Dft;   // ntt_passes.hpp

// x * 2^K mod p, canonical in, canonical out, 0 <= K < 96.  With f = 2^32 (f^2 = f - 1, f^3 = -1 mod p) and
// y = x 2^(K mod 32) = y0 + y1 f + y2 f^2 (y2 < 2^(K mod 32)), multiplying on by f^(K / 32) only shuffles limbs:
//   K <  32:  y0 + y1 f + y2 (f - 1)            = lo64 + y2 EPS             one conditional subtraction of p
//   K <  64:  (y0 + y1) f - (y1 + y2)           = (u0 + cu) f - (y1 + y2 + cu),  u = y0 + y1 = u0 + cu f
//   K <  96:  (y0 - y2) f - (y0 + y1)
// In the last two the minuend is a multiple of f below p and the subtrahend is small, so one "+ p on borrow" leaves the
// canonical value: 10-12 VALU ops where shift + generic fold + canonicalisation took 17 and the K >= 64 cases a full
// multiplication by a 64-bit constant (four of the seventeen twiddles of a 16-point DFT).
template <int K>
__device__ __forceinline__ u64 mul_pow2(u64 x) {
    static_assert(K >= 0 && K < 96, "shift range");
    if constexpr (K == 0) return x;
    constexpr int k = K % 32, j = K / 32;
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32);
    const u32 y0 = k ? x0 << k : x0;
    const u32 y1 = k ? (x1 << k) | (x0 >> ((32 - k) & 31)) : x1;
    const u32 y2 = k ? x1 >> ((32 - k) & 31) : 0u;
    if constexpr (j == 0) {
        const u64 lo = (u64)y0 | ((u64)y1 << 32), he = ((u64)y2 << 32) - y2;  // y2 EPS < 2^63
        u64 t, t2;
        const bool c = __builtin_uaddll_overflow(lo, he, &t);
        const bool d = __builtin_uaddll_overflow(t, gl::EPS, &t2);            // t - p
        return (c | d) ? t2 : t;
    } else {
        u32 cu, cw, b0, B1, B2, kk;
        u32 hi, s0;   // minuend hi f, subtrahend s0 + cw f (cw: carry flag)
        if constexpr (j == 1) {
            const u32 u0 = __builtin_addc(y0, y1, 0u, &cu);
            hi = u0 + cu;                                   // no overflow: cu = 1 leaves u0 <= 2^32 - 2
            s0 = __builtin_addc(y1, y2, cu, &cw);
        } else {
            hi = y0;
            s0 = __builtin_addc(y0, y1, 0u, &cw);
            cw += y2;                                       // high word of the subtrahend: y2 + carry (< 2^31 + 1)
        }
        const u32 d0 = __builtin_subc(0u, s0, 0u, &b0);
        const u32 d1 = __builtin_subc(hi, cw, b0, &B1);
        (void)B2;
        const u32 m = 0u - B1;                              // borrowed: + p, i.e. - EPS (mod 2^64)
        const u32 e0 = __builtin_subc(d0, m, 0u, &kk);
        const u32 e1 = d1 - kk;
        return (u64)e0 | ((u64)e1 << 32);
    }
}

// (a - b) * w_16^(+-M): every such root is +-2^K (forward w_16 = 2^156; inverse w_16^-1 = 2^36)
template <bool INV, int M>
__device__ __forceinline__ u64 sub_twiddle(u64 a, u64 b) {
    constexpr int e = (INV ? 36 * M : 156 * M) % 192;
    if constexpr (e == 0) return gl::sub(a, b);
    else if constexpr (e < 96) return mul_pow2<e>(gl::sub(a, b));
    else return mul_pow2<e - 96>(gl::sub(b, a));  // 2^96 = -1
}

template <bool INV, int H, int J>
__device__ __forceinline__ void bfly(u64& a, u64& b) {  // DIF butterfly of half-size H at offset J: twiddle w_{2H}^J = w_16^(J * 8 / H)
    u64 s = gl::add(a, b);
    b = sub_twiddle<INV, J*(8 / H)>(a, b);
    a = s;
}

// 16-point DFT in registers, natural input order, output X[k] in slot brev4(k) (in-place DIF)
template <bool INV>
__device__ __forceinline__ void dft16(u64 (&x)[16]) {
#define B8(J) bfly<INV, 8, J>(x[J], x[J + 8]);
    B8(0) B8(1) B8(2) B8(3) B8(4) B8(5) B8(6) B8(7)
#undef B8
#define B4(O, J) bfly<INV, 4, J>(x[O + J], x[O + J + 4]);
    B4(0, 0) B4(0, 1) B4(0, 2) B4(0, 3) B4(8, 0) B4(8, 1) B4(8, 2) B4(8, 3)
#undef B4
#define B2(O, J) bfly<INV, 2, J>(x[O + J], x[O + J + 2]);
    B2(0, 0) B2(0, 1) B2(4, 0) B2(4, 1) B2(8, 0) B2(8, 1) B2(12, 0) B2(12, 1)
#undef B2
#define B1(O) bfly<INV, 1, 0>(x[O], x[O + 1]);
    B1(0) B1(2) B1(4) B1(6) B1(8) B1(10) B1(12) B1(14)
#undef B1
}

// 2-, 4- and 8-point DFTs of the same family (the tail stages of dft16 on the first 2^K registers): natural input order,
// output X[k] in slot brevK(k).  They carry the sizes between the multiples of four bits (2^17..2^19 rows).
template <bool INV, int K>
__device__ __forceinline__ void dft_small(u64 (&x)[16]) {
    static_assert(K >= 1 && K <= 3, "radix 2, 4 or 8");
    if constexpr (K == 3) {
        bfly<INV, 4, 0>(x[0], x[4]); bfly<INV, 4, 1>(x[1], x[5]); bfly<INV, 4, 2>(x[2], x[6]); bfly<INV, 4, 3>(x[3], x[7]);
    }
    if constexpr (K >= 2) {
#pragma unroll
        for (int o = 0; o < (1 << K); o += 4) {
            bfly<INV, 2, 0>(x[o], x[o + 2]);
            bfly<INV, 2, 1>(x[o + 1], x[o + 3]);
        }
    }
#pragma unroll
    for (int o = 0; o < (1 << K); o += 2) bfly<INV, 1, 0>(x[o], x[o + 1]);
}

// (a - b) * w_64^(+-M): w_64 = 2^39 (w_64^4 = w_16 = 2^156), w_64^-1 = 2^153 - shifts like the roots of the 16-point DFT
template <bool INV, int M>
__device__ __forceinline__ u64 sub_twiddle64(u64 a, u64 b) {
    constexpr int e = (INV ? 153 * M : 39 * M) % 192;
    if constexpr (e == 0) return gl::sub(a, b);
    else if constexpr (e < 96) return mul_pow2<e>(gl::sub(a, b));
    else return mul_pow2<e - 96>(gl::sub(b, a));  // 2^96 = -1
}
// one DIF layer of half-size H (32 or 16) on x[O .. O + 2H): twiddle w_{2H}^J = w_64^(J * 32 / H)
template <bool INV, int H, int O, int J = 0>
__device__ __forceinline__ void layer64(u64* x) {
    if constexpr (J < H) {
        const u64 s = gl::add(x[O + J], x[O + J + H]);
        x[O + J + H] = sub_twiddle64<INV, J*(32 / H)>(x[O + J], x[O + J + H]);
        x[O + J] = s;
        layer64<INV, H, O, J + 1>(x);
    }
}

// 32-point DFT in registers, natural input order, output X[k] in slot brev5(k): one DIF layer, then two 16-point blocks
template <bool INV>
__device__ __forceinline__ void dft32(u64 (&x)[32]) {
    layer64<INV, 16, 0>(x);
    dft16<INV>(*reinterpret_cast<u64(*)[16]>(&x[0]));
    dft16<INV>(*reinterpret_cast<u64(*)[16]>(&x[16]));
}

template <>
struct Dft<GlF> {
    template <bool INV>
    static __device__ __forceinline__ void dft16(u64 (&x)[16]) { gbk::dft16<INV>(x); }
    template <bool INV, int K>
    static __device__ __forceinline__ void dft_small(u64 (&x)[16]) { gbk::dft_small<INV, K>(x); }
    template <bool INV, int H, int O>
    static __device__ __forceinline__ void layer64(u64* x) { gbk::layer64<INV, H, O>(x); }
    template <bool INV>
    static __device__ __forceinline__ void dft32(u64 (&x)[32]) { gbk::dft32<INV>(x); }
};

}  // namespace gbk

// BabyBear register DFTs (Dft<BbF>): the 2- to 64-point butterflies that kernels_bb16.hip's and ntt_passes.hpp's radix-16 passes keep in
// registers.  BabyBear has no power-of-two roots of unity, so the twiddles inside them are Montgomery multiplications by
// compile-time constants w_16^k / w_64^k, taken as signed words (bb::mul_signed).
// A header of their own so that a test program can call them one at a time (tests/host_shim/register_dfts.cpp on the CPU,
// tests/device/register_dfts.hip on the GPU).
#pragma once
#include "bb_field.hpp"
#include "field_traits.hpp"

namespace gbk {

template <class F>
struct Dft;   // ntt_passes.hpp

namespace bbc {  // compile-time twiddles (canonical arithmetic, stored in Montgomery form)
constexpr u32 cmul(u32 a, u32 b) { return (u32)((u64)a * b % bb::P); }
constexpr u32 cpow(u32 b, u64 e) {
    u32 r = 1;
    while (e) {
        if (e & 1) r = cmul(r, b);
        b = cmul(b, b);
        e >>= 1;
    }
    return r;
}
constexpr u32 W16 = cpow(bb::TWO_ADIC_GEN_27, 1u << 23);  // primitive 16th root of unity (two_adic_generator(4))
constexpr u32 W16_INV = cpow(W16, 15);
constexpr u32 mont(u32 x) { return (u32)(((u64)x << 32) % bb::P); }
template <bool INV, int M>
constexpr u32 tw() { return mont(cpow(INV ? W16_INV : W16, M)); }
// the same twiddle as a signed word of magnitude <= p/2, for the signed Montgomery product (bb::mul_signed)
template <bool INV, int M>
constexpr int tw_centred() { return tw<INV, M>() > bb::P / 2 ? (int)tw<INV, M>() - (int)bb::P : (int)tw<INV, M>(); }
static_assert(cpow(W16, 16) == 1 && cpow(W16, 8) == bb::P - 1, "W16 must be a primitive 16th root of unity");
}  // namespace bbc

// (a - b) * w_16^(+-M)
template <bool INV, int M>
__device__ __forceinline__ u32 sub_twiddle(u32 a, u32 b) {
    if constexpr (M == 0) return bb::sub(a, b);
    else {   // a - b as a signed word in (-p, p) times a twiddle within +-p/2: the signed product lands within +-0.74 p and one
             // selection makes it canonical - six instructions where a - b + p and the unsigned product took seven
        const int r = bb::mul_signed((int)(a - b), bbc::tw_centred<INV, M>());
        const u32 e = (u32)r + bb::P;
        return e < (u32)r ? e : (u32)r;
    }
}

template <bool INV, int H, int J>
__device__ __forceinline__ void bfly(u32& a, u32& b) {  // DIF butterfly of half-size H at offset J: twiddle w_{2H}^J = w_16^(J * 8 / H)
    u32 s = bb::add(a, b);
    b = sub_twiddle<INV, J*(8 / H)>(a, b);
    a = s;
}

// 16-point DFT in registers, natural input order, output X[k] in slot brev4(k) (in-place DIF)
template <bool INV>
__device__ __forceinline__ void dft16(u32 (&x)[16]) {
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
// output X[k] in slot brevK(k) - for the sizes between the multiples of four bits (2^17..2^19 rows)
template <bool INV, int K>
__device__ __forceinline__ void dft_small(u32 (&x)[16]) {
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

namespace bbc {
constexpr u32 W64 = cpow(bb::TWO_ADIC_GEN_27, 1u << 21), W64_INV = cpow(W64, 63);
static_assert(cpow(W64, 4) == W16 && cpow(W64, 32) == bb::P - 1, "W64 must be the 64th root above W16");
template <bool INV, int M>
constexpr int tw64_centred() {
    const u32 t = mont(cpow(INV ? W64_INV : W64, M));
    return t > bb::P / 2 ? (int)t - (int)bb::P : (int)t;
}
}  // namespace bbc
template <bool INV, int H, int O, int J = 0>
__device__ __forceinline__ void layer64(u32* x) {   // one DIF layer of half-size H (32 or 16) on x[O .. O + 2H): twiddle w_64^(J * 32 / H)
    if constexpr (J < H) {
        const u32 a = x[O + J], b = x[O + J + H];
        x[O + J] = bb::add(a, b);
        if constexpr (J == 0) x[O + J + H] = bb::sub(a, b);
        else {
            const int r = bb::mul_signed((int)(a - b), bbc::tw64_centred<INV, J*(32 / H)>());
            const u32 e = (u32)r + bb::P;
            x[O + J + H] = e < (u32)r ? e : (u32)r;
        }
        layer64<INV, H, O, J + 1>(x);
    }
}
// 32-point DFT in registers, natural input order, output X[k] in slot brev5(k): one DIF layer, then two 16-point blocks
template <bool INV>
__device__ __forceinline__ void dft32(u32 (&x)[32]) {
    layer64<INV, 16, 0>(x);
    dft16<INV>(*reinterpret_cast<u32(*)[16]>(&x[0]));
    dft16<INV>(*reinterpret_cast<u32(*)[16]>(&x[16]));
}

template <>
struct Dft<BbF> {
    template <bool INV>
    static __device__ __forceinline__ void dft16(u32 (&x)[16]) { gbk::dft16<INV>(x); }
    template <bool INV, int K>
    static __device__ __forceinline__ void dft_small(u32 (&x)[16]) { gbk::dft_small<INV, K>(x); }
    template <bool INV, int H, int O>
    static __device__ __forceinline__ void layer64(u32* x) { gbk::layer64<INV, H, O>(x); }
    template <bool INV>
    static __device__ __forceinline__ void dft32(u32 (&x)[32]) { gbk::dft32<INV>(x); }
};

}  // namespace gbk

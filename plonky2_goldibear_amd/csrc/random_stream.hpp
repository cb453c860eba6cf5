// The keyed element stream behind gb_random_elements and GB_SALTS_FROM_SEED (kernels_random.hip, the provers' seeded salts, the
// builder mirror's blinding values).  A stream is (seed[32], nonce[3]); element e of it, for e >> 2 < 2^32, is
//   block   the ChaCha20 block function of RFC 8439 2.3 (20 rounds, the "expand 32-byte k" constants): words 4-11 the seed as
//           eight little-endian words, word 12 the block counter e >> 2, words 13-15 nonce[0..2];
//   x       bytes 16 (e & 3) .. 16 (e & 3) + 15 of the block's 64 serialized bytes as a little-endian 128-bit integer -
//           i.e. output words 4 (e & 3) .. 4 (e & 3) + 3, lowest first;
//   value   x mod p, canonical.
// Every block is used in full - four elements per block in both fields - and nothing is rejected, so position e depends on no
// other position and any range can be produced by any number of lanes.  The price is a bias: x is uniform on [0, 2^128), so a
// residue is hit floor(2^128 / p) or one more time, and the distance of x mod p from uniform is below p / 2^128 - under 2^-64 for
// Goldilocks, under 2^-97 for BabyBear.
// Plain integer C++; the same text runs on the host (the ABI's host destination, tests/host_shim/random_stream.cpp).
#pragma once
#include <stdint.h>

#include "field_traits.hpp"

namespace gbk {
namespace rnd {

// the `nonce[0]` values the library itself uses (goldibear_gpu.h: GB_STREAM_*)
constexpr u32 STREAM_SALTS = 1, STREAM_BLINDING = 2;

struct Key {
    u32 seed[8];    // the 32 seed bytes as little-endian words
    u32 nonce[3];
};
GB_HD Key make_key(const uint8_t* seed, const u32* nonce) {
    Key k;
    for (int i = 0; i < 8; i++)
        k.seed[i] = (u32)seed[4 * i] | ((u32)seed[4 * i + 1] << 8) | ((u32)seed[4 * i + 2] << 16) | ((u32)seed[4 * i + 3] << 24);
    for (int i = 0; i < 3; i++) k.nonce[i] = nonce[i];
    return k;
}

#define GB_CHACHA_QR(a, b, c, d)                               \
    a += b; d ^= a; d = __builtin_rotateleft32(d, 16);         \
    c += d; b ^= c; b = __builtin_rotateleft32(b, 12);         \
    a += b; d ^= a; d = __builtin_rotateleft32(d, 8);          \
    c += d; b ^= c; b = __builtin_rotateleft32(b, 7);

// out[16]: the block's words; its serialized bytes are these words little-endian, in order
GB_HD void chacha20_block(const Key& k, u32 counter, u32* out) {
    const u32 i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;
    u32 x0 = i0, x1 = i1, x2 = i2, x3 = i3;
    u32 x4 = k.seed[0], x5 = k.seed[1], x6 = k.seed[2], x7 = k.seed[3];
    u32 x8 = k.seed[4], x9 = k.seed[5], x10 = k.seed[6], x11 = k.seed[7];
    u32 x12 = counter, x13 = k.nonce[0], x14 = k.nonce[1], x15 = k.nonce[2];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        GB_CHACHA_QR(x0, x4, x8, x12)
        GB_CHACHA_QR(x1, x5, x9, x13)
        GB_CHACHA_QR(x2, x6, x10, x14)
        GB_CHACHA_QR(x3, x7, x11, x15)
        GB_CHACHA_QR(x0, x5, x10, x15)
        GB_CHACHA_QR(x1, x6, x11, x12)
        GB_CHACHA_QR(x2, x7, x8, x13)
        GB_CHACHA_QR(x3, x4, x9, x14)
    }
    out[0] = x0 + i0; out[1] = x1 + i1; out[2] = x2 + i2; out[3] = x3 + i3;
    out[4] = x4 + k.seed[0]; out[5] = x5 + k.seed[1]; out[6] = x6 + k.seed[2]; out[7] = x7 + k.seed[3];
    out[8] = x8 + k.seed[4]; out[9] = x9 + k.seed[5]; out[10] = x10 + k.seed[6]; out[11] = x11 + k.seed[7];
    out[12] = x12 + counter; out[13] = x13 + k.nonce[0]; out[14] = x14 + k.nonce[1]; out[15] = x15 + k.nonce[2];
}
#undef GB_CHACHA_QR

// (w[0] + 2^32 w[1] + 2^64 w[2] + 2^96 w[3]) mod p, canonical
// Goldilocks: gl::reduce128 on the two halves (2^64 = 2^32 - 1, 2^96 = -1)
GB_HD u64 reduce_u128_gl(const u32* w) { return gl::reduce128((u64)w[0] | ((u64)w[1] << 32), (u64)w[2] | ((u64)w[3] << 32)); }
// BabyBear: bb::reduce(t) = t 2^-32 mod p for t < 2^32 p, so word k is multiplied by 2^(32 (k + 1)) mod p; two words share one
// reduction because the two constants of each pair add up to less than p (the sum of the two products stays below 2^32 p)
constexpr u32 BB_R3 = 0x12f37bfbu, BB_R4 = 0x27922ab6u;   // 2^96 mod p, 2^128 mod p
static_assert((u64)bb::R1 + bb::R2 < bb::P && (u64)BB_R3 + BB_R4 < bb::P, "a pair of words shares one Montgomery reduction");
static_assert(((u64)bb::R2 * bb::R1) % bb::P == BB_R3 && ((u64)BB_R3 * bb::R1) % bb::P == BB_R4, "powers of 2^32 mod p");
GB_HD u32 reduce_u128_bb(const u32* w) {
    const u32 lo = bb::reduce((u64)w[0] * bb::R1 + (u64)w[1] * bb::R2);
    const u32 hi = bb::reduce((u64)w[2] * BB_R3 + (u64)w[3] * BB_R4);
    return bb::add(lo, hi);
}
template <class F>
GB_HD typename F::T reduce_u128(const u32* w);
template <>
GB_HD u64 reduce_u128<GlF>(const u32* w) { return reduce_u128_gl(w); }
template <>
GB_HD u32 reduce_u128<BbF>(const u32* w) { return reduce_u128_bb(w); }

// the four canonical elements 4 b .. 4 b + 3 of the stream
template <class F>
GB_HD void block_elements(const Key& k, u32 block, typename F::T* out4) {
    u32 w[16];
    chacha20_block(k, block, w);
    for (int i = 0; i < 4; i++) out4[i] = reduce_u128<F>(w + 4 * i);
}
// element e alone (e >> 2 < 2^32)
template <class F>
GB_HD typename F::T element(const Key& k, u64 e) {
    typename F::T v[4];
    block_elements<F>(k, (u32)(e >> 2), v);
    return v[e & 3];
}
// a range is valid when its last block index fits 32 bits
GB_HD bool range_ok(u64 first, u64 count) {
    const u64 limit = (u64)1 << 34;
    return first <= limit && count <= limit - first;
}
// elements first .. first + count - 1 on the calling thread (the host destination of gb_random_elements)
template <class F>
inline void fill_range(const Key& k, u64 first, u64 count, typename F::T* out) {
    typename F::T v[4];
    for (u64 e = first, end = first + count; e < end;) {
        block_elements<F>(k, (u32)(e >> 2), v);
        for (u32 i = (u32)(e & 3); i < 4 && e < end; i++, e++) out[e - first] = v[i];
    }
}

}  // namespace rnd
}  // namespace gbk

// The operand pairs that tests/host_shim/mul_mont_forms.cpp (CPU) and tests/device/mul_mont_edges.hip (GPU) both run through
// gl::mul_mont_lazy: the carry edges of the 32-bit limb code, and pairs built so that (m2.hi, 0) - b does not borrow (m2 the
// middle partial sum, b the Montgomery fold's subtrahend; probability ~2^-32 on random operands).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace mul_mont_cases {
typedef unsigned long long u64;

inline std::vector<u64> edge_values() {
    const u64 P = 0xFFFFFFFF00000001ULL;
    return {0, 1, 0xFFFFFFFFULL, 1ULL << 32, (1ULL << 32) + 1, P - 1, P, P + 1, ~0ULL, 0xFFFFFFFF00000000ULL, 7ULL << 61,
            // x0 = 0 (low limbs that vanish in the product)
            2ULL << 32, 0x80000000ULL << 32, 0x12345678ULL << 32, 0x10000ULL, 0x80000000ULL, 0xFFFF0000ULL << 32,
            // m2 carries (large cross products)
            0xFFFFFFFFFFFFFFFEULL, 0xFFFFFFFEFFFFFFFFULL, 0xFFFFFFFF7FFFFFFFULL, 0x8000000080000000ULL, 0xFFFFFFFF80000000ULL,
            0xFFFFFFFE00000001ULL, 0x7FFFFFFFFFFFFFFFULL, 0x00000001FFFFFFFFULL, 0xAAAAAAAAAAAAAAAAULL, 0x5555555555555555ULL};
}
// m2.hi >= b with a product whose low half does not vanish: b = m - (m >> 32) - e is small only when the middle limb of
// m = lo (1 + 2^32) is zero, that is lo = (x0, 2^32 - x0), and then b = x0 - 1.  For an odd a, t = lo / a mod 2^64 gives that lo.
template <class Rng>
inline std::vector<std::pair<u64, u64>> no_borrow_pairs(Rng& rng) {
    std::vector<std::pair<u64, u64>> v;
    for (int i = 0; i < 64; i++) {
        const u64 a = rng() | 1, x0 = 1 + (i < 8 ? (u64)i : (rng() & 0xFFFF));
        u64 inv = a;                                                  // Newton: five doublings of 3 correct bits cover 64
        for (int k = 0; k < 5; k++) inv *= 2 - a * inv;
        const u64 lo = x0 | ((0x100000000ULL - x0) << 32);
        v.push_back({a, lo * inv});
    }
    return v;
}
// does (m2.hi, 0) - b borrow?  m2 and b recomputed from 128-bit arithmetic, not from the limb code under test
inline bool no_borrow(u64 a, u64 b) {
    typedef unsigned __int128 u128;
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const u64 p00 = (u64)a0 * b0;
    const u64 p01 = (u64)a0 * b1 + (p00 >> 32);
    const u64 m2 = (u64)((u128)a1 * b0 + p01);
    const u64 lo = (u64)((u128)a * b);
    const u64 m = lo + (lo << 32);
    const u64 bb = m - (m >> 32) - ((u64)(uint32_t)lo + (lo >> 32) > 0xFFFFFFFFULL ? 1 : 0);   // mont_fold's b = a - (a >> 32) - e
    return (m2 >> 32) >= bb;
}
}  // namespace mul_mont_cases

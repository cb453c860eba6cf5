// Reading the copy permutation back out of the sigma columns (gb_circuit_decode_sigmas; kernels_sigma.hip, sigma_host.inc).
// A sigma value is s = k_is[col'] w^row' (plonk/permutation_argument.rs), w the generator of the subgroup H of order n = 2^lg:
//   the coset   s^n = k_is[col']^n, and the k_i^n are distinct exactly when the k_i name distinct cosets of H: lg squarings and
//               a scan of the num_routed_wires values k_i^n
//   the row     the discrete logarithm of x = s / k_is[col'] in H, two levels: lg = a + b, a = ceil(lg / 2), e = lo + 2^a hi.
//               x^(2^b) = (w^(2^b))^lo lies in the subgroup of order 2^a: a sorted table of that subgroup gives lo;
//               x w^-lo = (w^(2^a))^hi lies in the subgroup of order 2^b <= 2^a, which is part of the same table: entry e2 of it,
//               hi = e2 >> (a - b).  b squarings, two binary searches of a steps and one product.
// Exact for every lg up to the two-adicity: nothing is approximated, a value that is in no routed coset is reported as NO_CELL.
// All values are in the field's device form (field_traits.hpp: canonical u64 / Montgomery u32) - F::mul's results are unique
// words there, so equality of elements is equality of words.  The same text runs on the host (tests/host_shim/sigma_decode.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "field_traits.hpp"

namespace gbk {
namespace sigma {

constexpr u32 NO_CELL = 0xFFFFFFFFu;

// the tables of one (field, lg): sorted[i] ascending as words, the elements (w^(2^b))^j of the subgroup of order 2^a;
// exps[i] = that j (a <= 16); inv_lo[j] = w^-j, j < 2^a
template <class F>
struct DlogTables {
    u32 lg, a, b;
    const typename F::T* sorted;
    const uint16_t* exps;
    const typename F::T* inv_lo;
};
GB_HD u32 dlog_low_bits(u32 lg) { return (lg + 1) / 2; }
template <class F>
GB_HD size_t dlog_table_bytes(u32 lg) {
    return ((size_t)1 << dlog_low_bits(lg)) * (2 * sizeof(typename F::T) + sizeof(uint16_t));
}

template <class F>
GB_HD typename F::T square_times(typename F::T x, u32 k) {
    for (u32 i = 0; i < k; i++) x = F::mul(x, x);
    return x;
}

// the index of v in sorted[0 .. 2^bits), or NO_CELL
template <class T>
GB_HD u32 find_sorted(const T* sorted, u32 bits, T v) {
    u32 pos = 0;
    for (u32 step = bits ? 1u << (bits - 1) : 0; step; step >>= 1)
        if (sorted[pos + step] <= v) pos += step;
    return sorted[pos] == v ? pos : NO_CELL;
}

// *e < 2^lg with w^e = x; false where x is not in H
template <class F>
GB_HD bool dlog(const DlogTables<F>& t, typename F::T x, u32* e) {
    typedef typename F::T T;
    const u32 i = find_sorted<T>(t.sorted, t.a, square_times<F>(x, t.b));
    if (i == NO_CELL) return false;
    const u32 lo = t.exps[i];
    const u32 j = find_sorted<T>(t.sorted, t.a, F::mul(x, t.inv_lo[lo]));
    if (j == NO_CELL) return false;
    const u32 e2 = t.exps[j], spare = t.a - t.b;
    if (e2 & ((1u << spare) - 1)) return false;
    *e = lo | ((e2 >> spare) << t.a);
    return true;
}

// the col' < num_routed with k_pow_n[col'] = s^n, or NO_CELL
template <class F>
GB_HD u32 match_coset(const typename F::T* k_pow_n, u32 num_routed, typename F::T s_pow_n) {
    for (u32 j = 0; j < num_routed; j++)
        if (k_pow_n[j] == s_pow_n) return j;
    return NO_CELL;
}

// s -> (col', row'); false where s names no routed cell: 0, a value of another coset
template <class F>
GB_HD bool decode_value(const DlogTables<F>& t, const typename F::T* k_pow_n, const typename F::T* k_inv, u32 num_routed, typename F::T s,
                        u32* col, u32* row) {
    *col = match_coset<F>(k_pow_n, num_routed, square_times<F>(s, t.lg));
    if (*col == NO_CELL) return false;
    return dlog<F>(t, F::mul(s, k_inv[*col]), row);
}

// ---------------------------------------------------------------- host: the tables
template <class F>
struct DlogTablesHost {
    u32 lg = 0;
    std::vector<typename F::T> sorted, inv_lo;
    std::vector<uint16_t> exps;
    DlogTables<F> view() const { return DlogTables<F>{lg, dlog_low_bits(lg), lg - dlog_low_bits(lg), sorted.data(), exps.data(), inv_lo.data()}; }
};
template <class F>
inline DlogTablesHost<F> build_dlog_tables(u32 lg) {
    typedef typename F::T T;
    DlogTablesHost<F> h;
    h.lg = lg;
    const u32 a = dlog_low_bits(lg), b = lg - a;
    const size_t m = (size_t)1 << a;
    const T w = F::two_adic_generator(lg), w_inv = F::inv(w), wa = square_times<F>(w, b);
    std::vector<std::pair<T, uint16_t>> order(m);
    h.inv_lo.resize(m);
    T x = F::one(), y = F::one();
    for (size_t j = 0; j < m; j++) {
        order[j] = std::make_pair(x, (uint16_t)j);
        h.inv_lo[j] = y;
        x = F::mul(x, wa);
        y = F::mul(y, w_inv);
    }
    std::sort(order.begin(), order.end());
    h.sorted.resize(m);
    h.exps.resize(m);
    for (size_t j = 0; j < m; j++) {
        h.sorted[j] = order[j].first;
        h.exps[j] = order[j].second;
    }
    return h;
}
// k_is (device form) -> k_i^n and 1 / k_i; false where two k_i^n coincide (the same coset twice) or a k_i is zero
template <class F>
inline bool build_coset_tables(const typename F::T* k_is, u32 num_routed, u32 lg, std::vector<typename F::T>* k_pow_n,
                               std::vector<typename F::T>* k_inv) {
    k_pow_n->resize(num_routed);
    k_inv->resize(num_routed);
    for (u32 j = 0; j < num_routed; j++) {
        if (k_is[j] == F::zero()) return false;
        (*k_pow_n)[j] = square_times<F>(k_is[j], lg);
        (*k_inv)[j] = F::inv(k_is[j]);
    }
    std::vector<typename F::T> seen(*k_pow_n);
    std::sort(seen.begin(), seen.end());
    return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

}  // namespace sigma
}  // namespace gbk

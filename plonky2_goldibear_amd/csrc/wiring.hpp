// Copy constraints -> sigma columns and representative map (gb_wiring_sigmas; kernels_wiring.hip, wiring_host.inc): what one
// thread does to one pair, one key or one cell.  The same text runs on the host (tests/host_shim/wiring.cpp), where the passes
// are emulated one element after the other.
//   targets   Target::index: wire (row, column) is row * num_wires + column - a "cell" -, virtual target i is
//             degree * num_wires + i.  All of them are below 2^32 here.
//   classes   a forest parent[t] <= t over the targets.  A pair is united by hooking the HIGHER of its two roots under the
//             lower one with a compare-and-swap on the higher root's own entry, and trying again from there when another
//             thread got to that root first.  Pointers only ever fall, so there are no cycles, and a tree's root is the lowest
//             index of its class whatever the schedule was.  find_root shortens the path it walks (path splitting: every node
//             on it is pointed at its grandparent, with an atomic minimum - any ancestor is a valid parent).
//   order     the routed cells of classes that hold two of them or more, as (label, cell) in ascending cell order, sorted by
//             label with a stable least-significant-digit radix sort of RADIX_BITS-bit digits; a class is then a run, its cells
//             ascending, and a cell's successor is the next entry of its run, the last one's the run's first
//   sigmas    sigma[col][row] = k_is[col'] w^row' for the successor (row', col'), the cell itself where it has none;
//             w^e = hi[e >> 10] lo[e & 1023], the split root tables of the transforms
#pragma once
#include <stdint.h>

#include "field_traits.hpp"

namespace gbk {
namespace wiring {

constexpr u32 NONE = 0xFFFFFFFFu;
constexpr u32 BLOCK = 256;                         // threads of every workgroup here
constexpr u32 SORT_TILE = 1024;                    // keys of one workgroup in the compaction and in a sort pass
constexpr u32 CHUNK = 64;                          // consecutive keys one wave ranks with ballots
constexpr u32 TILE_CHUNKS = SORT_TILE / CHUNK;
constexpr u32 RADIX_BITS = 8, RADIX = 1u << RADIX_BITS;
constexpr u32 PAIR_OK = 0, PAIR_OUT_OF_RANGE = 1, PAIR_NOT_ROUTABLE = 2;

// ---- the forest.  On the device the entries are read and written by many threads at once: relaxed atomics at device scope.
GB_HD u32 load_parent(const u32* parent, u32 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return parent[x];
#endif
}
// parent[x] = min(parent[x], v)
GB_HD void lower_parent(u32* parent, u32 x, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_min(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (v < parent[x]) parent[x] = v;
#endif
}
// parent[x] = desired if it holds `expected`; what it held
GB_HD u32 swap_parent(u32* parent, u32 x, u32 expected, u32 desired) {
#if defined(__HIP_DEVICE_COMPILE__)
    u32 seen = expected;
    (void)__hip_atomic_compare_exchange_strong(parent + x, &seen, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return seen;
#else
    const u32 seen = parent[x];
    if (seen == expected) parent[x] = desired;
    return seen;
#endif
}

// the root of x's tree; the nodes passed on the way are pointed at their grandparents
GB_HD u32 find_root(u32* parent, u32 x) {
    u32 p = load_parent(parent, x);
    while (p != x) {
        const u32 g = load_parent(parent, p);
        if (g == p) return p;
        lower_parent(parent, x, g);
        x = p;
        p = g;
    }
    return x;
}
// the hook rule: which of two distinct roots goes under which
GB_HD void hook_order(u32 a, u32 b, u32* child, u32* under) {
    *child = a > b ? a : b;
    *under = a > b ? b : a;
}
// the classes of a and b become one
GB_HD void unite(u32* parent, u32 a, u32 b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        u32 child, under;
        hook_order(a, b, &child, &under);
        if (swap_parent(parent, child, child, under) == child) return;
        a = child;   // no root any more: somebody else hooked it - on from where it hangs now
        b = under;
    }
}
// one pointer-jumping step of a compression pass: up to JUMPS ancestors above x's parent.  true: parent[x] fell
constexpr u32 JUMPS = 4;
GB_HD bool jump(u32* parent, u32 x) {
    const u32 p = load_parent(parent, x);
    u32 r = p;
    for (u32 s = 0; s < JUMPS; s++) {
        const u32 g = load_parent(parent, r);
        if (g == r) break;
        r = g;
    }
    if (r == p) return false;
    lower_parent(parent, x, r);
    return true;
}

// a pair as the caller wrote it: both entries name targets, and a wire cell among them is in a routed column
// (circuit_builder.rs:543-551).  cells = degree * num_wires
GB_HD u32 check_pair(u64 a, u64 b, u64 num_targets, u64 cells, u32 num_wires, u32 num_routed) {
    if (a >= num_targets || b >= num_targets) return PAIR_OUT_OF_RANGE;
    if ((a < cells && (u32)(a % num_wires) >= num_routed) || (b < cells && (u32)(b % num_wires) >= num_routed)) return PAIR_NOT_ROUTABLE;
    return PAIR_OK;
}

// ---- numberings.  sigma's own: i = col * n + row, the order the values lie in; the routed cells in ascending cell order:
// j = row * num_routed + col
GB_HD u32 cell_of_index(u32 i, u32 lg, u32 num_wires) { return (i & (u32)(((u64)1 << lg) - 1)) * num_wires + (u32)((u64)i >> lg); }
GB_HD u32 index_of_cell(u32 cell, u32 lg, u32 num_wires) { return (u32)(((u64)(cell % num_wires) << lg) + cell / num_wires); }
GB_HD u32 routed_cell(u32 j, u32 num_routed, u32 num_wires) { return (j / num_routed) * num_wires + j % num_routed; }

// ---- the sort's digits.  Labels are cells: below `limit` = degree * num_wires, which the host knows - the digits above its
// highest set bit are zero for every key and their passes are not run
GB_HD u32 key_bits(u64 limit) {   // the bits of the largest key, limit - 1 (0: every key is 0)
    u32 bits = 0;
    for (u64 top = limit ? limit - 1 : 0; top; top >>= 1) bits++;
    return bits;
}
GB_HD u32 digit_passes(u64 limit) { return (key_bits(limit) + RADIX_BITS - 1) / RADIX_BITS; }
GB_HD u32 digit_of(u32 key, u32 pass) { return (key >> (pass * RADIX_BITS)) & (RADIX - 1); }

// ---- the successor of entry i of the m sorted entries: the next one where that has the same label, else the first of i's
// run, which is run_length entries long (the label's count)
GB_HD u32 successor_index(u32 i, u32 m, bool next_has_same_label, u32 run_length) {
    if (i + 1 < m && next_has_same_label) return i + 1;
    return run_length <= i + 1 ? i + 1 - run_length : i;   // (a count that does not fit the list: the cell keeps itself)
}

// ---- k_is[col'] w^row' of a target cell, canonical.  lo, hi, k_is in the field's device form
template <class F>
GB_HD typename F::T sigma_value(const typename F::T* lo, const typename F::T* hi, const typename F::T* k_is, u32 cell, u32 num_wires) {
    const u32 row = cell / num_wires, col = cell % num_wires;
    return (typename F::T)F::dec(F::mul(F::mul(hi[row >> 10], lo[row & 1023]), k_is[col]));
}

}  // namespace wiring
}  // namespace gbk

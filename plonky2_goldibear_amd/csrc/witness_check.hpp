// Row logic of the witness check (kernels_check.hip, check_host.inc): which gate a row runs, and which of its constraints fails
// first.  The quotient stage evaluates filter * constraint on the LDE coset g H, where nothing has to vanish; the check evaluates
// the same evaluators (gates.hpp) on H itself, where a satisfied witness makes every active gate's constraints zero
// (plonk/vanishing_poly.rs: the vanishing polynomial is divisible by Z_H iff it is zero on H).
//   active gate   compute_filter (gates/gate.rs:391-404) is non-zero exactly for the gate whose index the selector column holds;
//                 the field has no zero divisors, so "filter * constraint != 0" is "that gate's constraint != 0"
//   selector      a value that is neither an index of the column's group nor UNUSED_SELECTOR makes EVERY filter of the group
//                 non-zero: the circuit data is broken, no gate is evaluated for that column on that row.  With one selector column
//                 the filter has no UNUSED factor (gate.rs:400-402) and UNUSED_SELECTOR is such a value too.
// Everything here is GB_HD: the host re-runs a reported row through the same source (tests/sanitize/witness_check.cpp).
#pragma once
#include <vector>

#include "gates.hpp"

namespace gbk {
namespace check {

constexpr u32 NO_GATE = 0xFFFFFFFFu;        // the selector column holds UNUSED_SELECTOR on this row
constexpr u32 BAD_SELECTOR = 0xFFFFFFFEu;   // ... or a value that names no gate of its group
constexpr u32 NO_FAILURE = 0xFFFFFFFFu;     // FirstFail::index of a row whose constraints all vanish
constexpr u32 MAX_LISTS = gates::MAX_GATES + 1;   // a row list per gate, and one of the rows with a selector violation

template <class F>
GB_HD u64 unused_selector() {   // UNUSED_SELECTOR as a field element, canonical (filter() reduces it the same way)
    return (u64)gates::UNUSED_SELECTOR % F::ORDER;
}

// [start, end): the gate indices that share selector column `col`; false: no gate uses the column
GB_HD bool column_group(const gates::GateSet& gs, u32 col, u32* start, u32* end) {
    for (u32 g = 0; g < gs.num_gates; g++)
        if (gs.g[g].selector_index == col) {
            *start = gs.g[g].group_start;
            *end = gs.g[g].group_end;
            return true;
        }
    return false;
}

// the gate that selector column `col` activates on a row where it holds the canonical value `s`: a gate index, NO_GATE or BAD_SELECTOR
template <class F>
GB_HD u32 active_gate(const gates::GateSet& gs, u32 col, u64 s) {
    u32 start = 0, end = 0;
    if (column_group(gs, col, &start, &end) && s >= start && s < end && gs.g[(u32)s].selector_index == col) return (u32)s;
    if (gs.num_selectors > 1 && s == unused_selector<F>()) return NO_GATE;
    return BAD_SELECTOR;
}

// is row `r` on list `l`?  l < num_gates: gate l is active there; l == num_gates: one of its selector columns is violated.
// `sel(col)` gives the canonical value of selector column col on the row.
template <class F, class Sel>
GB_HD bool row_on_list(const gates::GateSet& gs, u32 l, Sel&& sel) {
    if (l < gs.num_gates) {
        const u32 col = gs.g[l].selector_index;
        return active_gate<F>(gs, col, sel(col)) == l;
    }
    for (u32 col = 0; col < gs.num_selectors; col++)
        if (active_gate<F>(gs, col, sel(col)) == BAD_SELECTOR) return true;
    return false;
}

// the `emit` of a checked row: index and value (device form) of the first constraint that is not zero, in eval_unfiltered order
template <class F>
struct FirstFail {
    typedef typename F::T T;
    u32 index = NO_FAILURE, seen = 0;
    T value = F::zero();
    GB_HD void operator()(T c) {
        if (index == NO_FAILURE && c != F::zero()) {
            index = seen;
            value = c;
        }
        seen++;
    }
    GB_HD bool failed() const { return index != NO_FAILURE; }
};

// one row of a built-in gate through the evaluators of gates.hpp (either subset); wire / konst give device-form values
template <class F, class W, class K>
GB_HD FirstFail<F> check_row(const gates::GateSet& gs, const gb_gate& g, W&& wire, K&& konst, const typename F::T* pi_hash) {
    FirstFail<F> ff;
    if (gates::is_heavy(g)) gates::eval_gate<F, gates::BaseAlg<F>, gates::HEAVY_GATES>(gs, g, wire, konst, pi_hash, ff);
    else gates::eval_gate<F, gates::BaseAlg<F>, gates::LIGHT_GATES>(gs, g, wire, konst, pi_hash, ff);
    return ff;
}

// The row lists as the device builds them (k_check_count, k_check_scan, k_check_fill), on the host: per list a count, the
// exclusive scan of the counts, and the rows of every list in ascending order.  sel[col * n + row]: canonical selector values.
struct RowLists {
    std::vector<u32> counts, offsets, rows;   // [num_gates + 1], [num_gates + 2] (the last entry is the total), [total]
};
template <class F>
inline RowLists row_lists_host(const gates::GateSet& gs, const u64* sel, size_t n) {
    RowLists out;
    const u32 nl = gs.num_gates + 1;
    out.counts.assign(nl, 0);
    for (u32 l = 0; l < nl; l++)
        for (size_t r = 0; r < n; r++)
            out.counts[l] += row_on_list<F>(gs, l, [&](u32 col) { return sel[(size_t)col * n + r]; });
    out.offsets.assign(nl + 1, 0);
    for (u32 l = 0; l < nl; l++) out.offsets[l + 1] = out.offsets[l] + out.counts[l];
    out.rows.assign(out.offsets[nl], 0);
    for (u32 l = 0; l < nl; l++) {
        u32 at = out.offsets[l];
        for (size_t r = 0; r < n; r++)
            if (row_on_list<F>(gs, l, [&](u32 col) { return sel[(size_t)col * n + r]; })) out.rows[at++] = (u32)r;
    }
    return out;
}

}  // namespace check
}  // namespace gbk

// What a COMPRESSED proof's query rounds share (hash/path_compression.rs:12-117, fri/proof.rs:137-232), written once for the batch
// verifier's host stage (verify_batch_host.inc), its kernels (kernels_verify.hip) and the CPU build of tests/host_shim - beside
// verify_query.hpp, whose hashing and query arithmetic it uses.  Plain integer C++ apart from the qualifiers.
//
// Merkle paths.  The paths of one tree are stored together: per level (leaves first) and per query k in order, the sibling of
// k's node is stored in k's own path iff no query's node at that level IS the sibling and k is the first query with that node
// (decompress_merkle_proofs, restated in compress_host.inc: decompress_paths).  So the queries climb a tree level by level
// together, and at each level a query's sibling is either the node another query just computed or the next stored sibling of
// the first query that holds its node.
//
// Evaluations.  Per FRI layer a coset's stored row lacks the element at the position of the FIRST query round that lands in the
// coset (fri/proof.rs:178-180); that query's running evaluation goes there.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "verify_query.hpp"

namespace gbk {
namespace vc {

static constexpr u32 NO_QUERY = ~0u;

// Where query k's sibling comes from at one level.  node(j): query j's node at this level, any numbering in which siblings differ
// in bit 0 alone.
//   sibling != NO_QUERY   the node query `sibling` holds (the first such query; they all hold the same one)
//   otherwise             the next stored sibling of query `first`, the first query with k's node - k itself iff first == k
struct Source {
    u32 sibling, first;
};
template <class NodeAt>
GB_HD Source sibling_source(u32 num_queries, u32 k, NodeAt node) {
    const u64 mine = node(k);
    Source s{NO_QUERY, NO_QUERY};
    for (u32 j = 0; j < num_queries; j++) {
        const u64 nj = node(j);
        if (nj == (mine ^ 1) && s.sibling == NO_QUERY) s.sibling = j;
        if (nj == mine && s.first == NO_QUERY) s.first = j;
    }
    return s;
}
// the first query with query k's value (its coset index, its leaf): where the stored entry of a repeated value belongs
template <class ValueAt>
GB_HD u32 first_with(u32 k, ValueAt value) {
    const u64 mine = value(k);
    u32 j = 0;
    while (value(j) != mine) j++;   // (ends at k at the latest)
    return j;
}

// One level of one tree for every query at once, in the two phases the kernel separates with barriers: every query reads its
// sibling (digest(j): query j's node, HW canonical words; stored(j, i): word i of query j's next stored sibling), then every query
// hashes, replaces its node and - if it took a stored sibling of its own - moves on in its path.  The sequential form of
// k_vc_paths' level loop, for the host.
template <class F, class H>
void climb_level(H& h, u32 num_queries, const u64* nodes, typename F::T* digests /* [num_queries][F::H] */,
                 const typename F::T* const* paths, u32* taken) {
    typedef typename F::T T;
    constexpr u32 HW = F::H;
    std::vector<T> next((size_t)num_queries * HW);
    std::vector<u32> took(num_queries, 0);
    for (u32 k = 0; k < num_queries; k++) {
        const Source s = sibling_source(num_queries, k, [&](u32 j) { return nodes[j]; });
        const T* sib = s.sibling != NO_QUERY ? digests + (size_t)s.sibling * HW : paths[s.first] + (size_t)taken[s.first] * HW;
        took[k] = s.sibling == NO_QUERY && s.first == k;
        T cur[HW];
        for (u32 i = 0; i < HW; i++) cur[i] = digests[(size_t)k * HW + i];
        vq::two_to_one<F>(h, cur, [&](u32 i) { return sib[i]; }, (nodes[k] & 1) != 0);
        for (u32 i = 0; i < HW; i++) next[(size_t)k * HW + i] = cur[i];
    }
    for (u32 k = 0; k < num_queries; k++) taken[k] += took[k];
    std::copy(next.begin(), next.end(), digests);
}

// How many siblings each query's own path must hold for a tree of `path_len` levels below its cap: counts[k], zero for a query
// that is not the first with its leaf.  Follows from the indices alone.  O(path_len * queries) after one sort.
inline void sibling_counts(const u64* indices, u32 num_queries, u32 path_len, u32* counts) {
    std::vector<std::pair<u64, u32>> nodes(num_queries);   // (node, the first query below it), sorted by node
    for (u32 k = 0; k < num_queries; k++) { nodes[k] = std::make_pair(indices[k], k); counts[k] = 0; }
    std::sort(nodes.begin(), nodes.end());
    size_t n = 0;
    for (size_t i = 0; i < nodes.size(); i++) {   // (sorted by query within a node, so the first stays)
        if (n && nodes[n - 1].first == nodes[i].first) continue;
        nodes[n++] = nodes[i];
    }
    for (u32 level = 0; level < path_len; level++) {
        for (size_t i = 0; i < n; i++) {
            const u64 sib = nodes[i].first ^ 1;
            const bool held = (i > 0 && nodes[i - 1].first == sib) || (i + 1 < n && nodes[i + 1].first == sib);
            if (!held) counts[nodes[i].second]++;
        }
        size_t m = 0;
        for (size_t i = 0; i < n; i++) {
            const std::pair<u64, u32> up(nodes[i].first >> 1, nodes[i].second);
            if (m && nodes[m - 1].first == up.first) nodes[m - 1].second = std::min(nodes[m - 1].second, up.second);
            else nodes[m++] = up;
        }
        n = m;
    }
}

// A re-inflated coset: `stored` holds its evaluations but the one at position `at`, D canonical words each.
template <class F>
GB_HD typename F::E inflated_eval(const unsigned char* stored, u32 at, typename F::E inferred, u32 k) {
    if (k == at) return inferred;
    return vq::load_ext<F>(stored + (size_t)(k - (k > at ? 1u : 0u)) * F::D * sizeof(typename F::T));
}
// word i of the same row as the layer tree's leaf; inferred: D canonical words
template <class F>
GB_HD typename F::T inflated_word(const unsigned char* stored, u32 at, const typename F::T* inferred, u32 i) {
    const u32 k = i / F::D;
    if (k == at) return inferred[i % F::D];
    return vq::load_word<F>(stored + (size_t)(i - (k > at ? F::D : 0u)) * sizeof(typename F::T));
}

// One layer of one query round whose coset was first opened by query round `first` (itself included): the consistency check
// against the re-inflated row and the fold.  Returns the new evaluation; *consistent says whether the check held.
template <class F>
GB_HD typename F::E fold_layer(typename F::T x, u64 within, u32 arity_bits, typename F::E beta, const unsigned char* stored, u32 at,
                               typename F::E inferred, typename F::E old_eval, bool* consistent) {
    auto eval = [stored, at, inferred](u32 k) { return inflated_eval<F>(stored, at, inferred, k); };
    *consistent = vq::eeq<F>(eval((u32)within), old_eval);
    return vq::compute_evaluation<F>(x, within, arity_bits, beta, eval);
}

}  // namespace vc
}  // namespace gbk

// gb_verify_batch's device stage (verify_batch_host.inc): the query rounds of many proofs of one circuit, the checks of
// verify_query.hpp run lane-per-item - what verify_fri_parsed (verifier_host.inc) walks in sequence on the host.
//   k_verify_paths    one lane per (tree, proof, query round): hash_or_noop of the opened row, two_to_one up to the cap
//                     (verify_merkle_proof_to_cap, hash/merkle_proofs.rs:54-76) - the four oracles, then the FRI layers
//   k_verify_queries  one lane per (proof, query round): fri_combine_initial, per layer the consistency check and
//                     compute_evaluation, the final polynomial (fri/verifier.rs:121-250)
// Every check runs whether or not an earlier one of its proof failed; the proof's result is the minimum of the failing checks'
// keys (query round, position in the round), which is the check the host verifier reaches first, whatever the schedule.
// All offsets come from the circuit's shape (VerifyLayout, kernels.hpp); the proofs' bytes are only ever read as field words.
//
// gb_fri_verify_batch's device stage: the same two kernels over any FriInstanceInfo (k_fri_verify_paths, k_fri_verify_queries) - the
// shape's tables live in device memory (FriVerifyLayout, kernels.hpp) instead of the launch argument, every cap in the item's record.
//
// gb_verify_compressed_batch's device stage: the same checks where the query rounds of a proof are no longer independent
// (verify_compressed.hpp), so one workgroup holds all query rounds of a proof, a lane each, and they advance together through LDS.
//   k_vc_queries      one workgroup per proof: fri_combine_initial, then layer by layer - the lanes publish their running
//                     evaluation, every lane finds the first lane of its coset, re-inflates the stored row with that lane's
//                     evaluation, checks consistency and folds; the final polynomial.  Leaves the inserted elements for:
//   k_vc_paths        one workgroup per (proof, tree): the leaves' digests, then level by level up to the cap - a lane's sibling
//                     is the node another lane just computed or the next stored sibling of the first lane with its node
// The keys are the ones above: "path k leads to the cap" on the decompressed proof is "lane k's node is its cap entry" here.
#include "kernels.hpp"
#include "sponge.hpp"
#include "verify_compressed.hpp"
#include "verify_query.hpp"

namespace gbk {

namespace {

template <class F>
struct RecordView {   // one proof's record (kernels.hpp)
    typedef typename F::T T;
    typedef typename F::E E;
    const unsigned char* p;
    const VerifyLayout& L;
    __device__ __forceinline__ const E* ext() const { return reinterpret_cast<const E*>(p); }
    __device__ __forceinline__ E fri_alpha() const { return ext()[0]; }
    __device__ __forceinline__ const E* red_open() const { return ext() + 1; }
    __device__ __forceinline__ const E* alpha_shift() const { return ext() + 3; }
    __device__ __forceinline__ const E* points() const { return ext() + 5; }
    __device__ __forceinline__ const E* betas() const { return ext() + 7; }
    __device__ __forceinline__ const E* final_poly() const { return ext() + 7 + L.num_layers; }
    __device__ __forceinline__ u64 x_index(u32 qr) const { return reinterpret_cast<const u64*>(p + L.rec_x_off)[qr]; }
    __device__ __forceinline__ const T* caps() const { return reinterpret_cast<const T*>(p + L.rec_caps_off); }
};

// blockIdx.y = tree, so that a wave's lanes share a row width and a path length (the Goldilocks permutation is wave-wide: lanes
// past the end clamp their index instead of returning, as k_fri_leaves does)
template <class F>
__global__ __launch_bounds__(256) void k_verify_paths(VerifyLayout L, const unsigned char* __restrict__ rounds,
                                                      const unsigned char* __restrict__ records,
                                                      const typename F::T* __restrict__ circuit_cap, u64* __restrict__ keys) {
    const VerifyTree tr = L.trees[blockIdx.y];
    const u32 total = L.num_proofs * L.nqr;
    const u32 g0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = g0 < total;
    const u32 g = live ? g0 : total - 1;
    const u32 proof = g / L.nqr, qr = g % L.nqr;
    const RecordView<F> rec{records + (size_t)proof * L.rec_bytes, L};
    const unsigned char* round = rounds + ((size_t)proof * L.nqr + qr) * L.round_bytes;
    const typename F::T* cap = tr.cap_word == ~0u ? circuit_cap : rec.caps() + tr.cap_word;
    __shared__ poseidon_gl::v4i sponge_lds[Sponge<F>::LDS_V4];
    Sponge<F> sp;
    sp.init(sponge_lds);
    const bool ok = vq::merkle_path_ok<F>(sp, round + tr.row_off, tr.num_words, rec.x_index(qr) >> tr.shift, round + tr.path_off,
                                          tr.path_len, cap);
    const u32 pos = blockIdx.y < VERIFY_ORACLES ? vq::pos_initial_path(blockIdx.y) : vq::pos_layer_path(VERIFY_ORACLES, blockIdx.y - VERIFY_ORACLES);
    if (live && !ok) atomicMin(reinterpret_cast<unsigned long long*>(keys + proof), (unsigned long long)vq::fail_key(qr, pos));
}

template <class F>
__global__ __launch_bounds__(64) void k_verify_queries(VerifyLayout L, const unsigned char* __restrict__ rounds,
                                                       const unsigned char* __restrict__ records, u64* __restrict__ keys) {
    typedef typename F::T T;
    typedef typename F::E E;
    const u32 g = blockIdx.x * 64 + threadIdx.x;
    if (g >= L.num_proofs * L.nqr) return;
    const u32 proof = g / L.nqr, qr = g % L.nqr;
    const RecordView<F> rec{records + (size_t)proof * L.rec_bytes, L};
    const unsigned char* round = rounds + ((size_t)proof * L.nqr + qr) * L.round_bytes;
    const u64 x_index = rec.x_index(qr);
    const T x = vq::subgroup_x<F>(L.lgN, x_index);
    // batch 0 runs over the four oracles' polynomials in order, batch 1 over the first polynomials of the Zs oracle
    // (get_fri_instance, plonk/circuit_data.rs:438-520)
    auto poly = [&](u32 b, u32 i) {
        u32 o = 2;
        if (b == 0) {
            o = 0;
            while (i >= L.widths[o]) { i -= L.widths[o]; o++; }
        }
        return vq::load_word<F>(round + L.trees[o].row_off + (size_t)i * sizeof(T));
    };
    const E old_eval = vq::combine_initial<F>(2, L.batch_sizes, rec.points(), rec.red_open(), rec.alpha_shift(), rec.fri_alpha(), x, poly);
    const E* betas = rec.betas();
    const E* fin = rec.final_poly();
    const u32 pos = vq::fold_checks<F>(
        VERIFY_ORACLES, L.num_layers, L.arity_bits, x_index, x, old_eval, L.final_len,
        [&](u32 li) { return round + L.trees[VERIFY_ORACLES + li].row_off; }, [&](u32 li) { return betas[li]; },
        [&](u32 i) { return fin[i]; }, [](u32, u64) { return true; });   // (the layers' paths: k_verify_paths)
    if (pos != ~0u) atomicMin(reinterpret_cast<unsigned long long*>(keys + proof), (unsigned long long)vq::fail_key(qr, pos));
}

// gb_fri_verify_batch: the two kernels above over a FriVerifyLayout (kernels.hpp) - any number of oracles and batches, the shape's
// tables in device memory.  An item's record, as RecordView reads the PLONK one:
template <class F>
struct FriRecordView {
    typedef typename F::T T;
    typedef typename F::E E;
    const unsigned char* p;
    const FriVerifyLayout& L;
    __device__ __forceinline__ const E* ext() const { return reinterpret_cast<const E*>(p); }
    __device__ __forceinline__ E fri_alpha() const { return ext()[0]; }
    __device__ __forceinline__ const E* red_open() const { return ext() + 1; }
    __device__ __forceinline__ const E* alpha_shift() const { return ext() + 1 + L.num_batches; }
    __device__ __forceinline__ const E* points() const { return ext() + 1 + 2 * L.num_batches; }
    __device__ __forceinline__ const E* betas() const { return ext() + 1 + 3 * L.num_batches; }
    __device__ __forceinline__ const E* final_poly() const { return betas() + L.num_layers; }
    __device__ __forceinline__ u64 x_index(u32 qr) const { return reinterpret_cast<const u64*>(p + L.rec_x_off)[qr]; }
    __device__ __forceinline__ const T* caps() const { return reinterpret_cast<const T*>(p + L.rec_caps_off); }
};

// blockIdx.y = tree, as k_verify_paths: the lanes of a wave share (num_words, path_len), lanes past the end clamp their index.
// Every tree's cap - the initial ones too - comes from the item's record.
template <class F>
__global__ __launch_bounds__(256) void k_fri_verify_paths(FriVerifyLayout L, const unsigned char* __restrict__ rounds,
                                                          const unsigned char* __restrict__ records, u64* __restrict__ keys) {
    const VerifyTree tr = L.trees[blockIdx.y];
    const u32 total = L.num_proofs * L.nqr;
    const u32 g0 = blockIdx.x * 256 + threadIdx.x;
    const bool live = g0 < total;
    const u32 g = live ? g0 : total - 1;
    const u32 item = g / L.nqr, qr = g % L.nqr;
    const FriRecordView<F> rec{records + (size_t)item * L.rec_bytes, L};
    const unsigned char* round = rounds + ((size_t)item * L.nqr + qr) * L.round_bytes;
    __shared__ poseidon_gl::v4i sponge_lds[Sponge<F>::LDS_V4];
    Sponge<F> sp;
    sp.init(sponge_lds);
    const bool ok = vq::merkle_path_ok<F>(sp, round + tr.row_off, tr.num_words, rec.x_index(qr) >> tr.shift, round + tr.path_off,
                                          tr.path_len, rec.caps() + tr.cap_word);
    const u32 pos = blockIdx.y < L.num_oracles ? vq::pos_initial_path(blockIdx.y) : vq::pos_layer_path(L.num_oracles, blockIdx.y - L.num_oracles);
    if (live && !ok) atomicMin(reinterpret_cast<unsigned long long*>(keys + item), (unsigned long long)vq::fail_key(qr, pos));
}

// one lane per (item, query round).  poly(b, i) reads the word at the tabled offset: the index batch_base[b] + i is the same in
// every lane, so the table is read through the scalar unit and only the word itself is a per-lane load.
template <class F>
__global__ __launch_bounds__(64) void k_fri_verify_queries(FriVerifyLayout L, const unsigned char* __restrict__ rounds,
                                                           const unsigned char* __restrict__ records, u64* __restrict__ keys) {
    typedef typename F::T T;
    typedef typename F::E E;
    const u32 g = blockIdx.x * 64 + threadIdx.x;
    if (g >= L.num_proofs * L.nqr) return;
    const u32 item = g / L.nqr, qr = g % L.nqr;
    const FriRecordView<F> rec{records + (size_t)item * L.rec_bytes, L};
    const unsigned char* round = rounds + ((size_t)item * L.nqr + qr) * L.round_bytes;
    const u64 x_index = rec.x_index(qr);
    const T x = vq::subgroup_x<F>(L.lgN, x_index);
    const u32* __restrict__ poly_off = L.poly_off;
    const u32* __restrict__ batch_base = L.batch_base;
    auto poly = [&](u32 b, u32 i) { return vq::load_word<F>(round + poly_off[batch_base[b] + i]); };
    const E old_eval = vq::combine_initial<F>(L.num_batches, L.batch_sizes, rec.points(), rec.red_open(), rec.alpha_shift(), rec.fri_alpha(), x, poly);
    const E* betas = rec.betas();
    const E* fin = rec.final_poly();
    const VerifyTree* layer_trees = L.trees + L.num_oracles;
    const u32 pos = vq::fold_checks<F>(
        L.num_oracles, L.num_layers, L.arity_bits, x_index, x, old_eval, L.final_len,
        [&](u32 li) { return round + layer_trees[li].row_off; }, [&](u32 li) { return betas[li]; },
        [&](u32 i) { return fin[i]; }, [](u32, u64) { return true; });   // (the layers' paths: k_fri_verify_paths)
    if (pos != ~0u) atomicMin(reinterpret_cast<unsigned long long*>(keys + item), (unsigned long long)vq::fail_key(qr, pos));
}

template <class F>
__global__ __launch_bounds__(VERIFY_COMPRESSED_MAX_QUERIES) void k_vc_queries(VerifyCompressedLayout C, const unsigned char* __restrict__ rounds,
                                                                              const unsigned char* __restrict__ records,
                                                                              typename F::T* __restrict__ inferred, u64* __restrict__ keys) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 D = F::D;
    const VerifyLayout& L = C.L;
    __shared__ u64 s_x[VERIFY_COMPRESSED_MAX_QUERIES];
    __shared__ E s_eval[VERIFY_COMPRESSED_MAX_QUERIES];
    const u32 proof = blockIdx.x, nqr = L.nqr;
    const bool live = threadIdx.x < nqr;   // lanes past the end follow the last query round: the barriers below need every lane
    const u32 k = live ? threadIdx.x : nqr - 1;
    const RecordView<F> rec{records + (size_t)proof * L.rec_bytes, L};
    const unsigned char* section = rounds + (size_t)proof * C.proof_stride;
    const u32* dir = reinterpret_cast<const u32*>(rec.p + C.rec_dir_off);
    const u64 x_index = rec.x_index(k);
    if (live) s_x[k] = x_index;
    T x = vq::subgroup_x<F>(L.lgN, x_index);
    auto poly = [&](u32 b, u32 i) {
        u32 o = 2;
        if (b == 0) {
            o = 0;
            while (i >= L.widths[o]) { i -= L.widths[o]; o++; }
        }
        return vq::load_word<F>(section + dir[o * nqr + k] + (size_t)i * sizeof(T));
    };
    E old_eval = vq::combine_initial<F>(2, L.batch_sizes, rec.points(), rec.red_open(), rec.alpha_shift(), rec.fri_alpha(), x, poly);
    const E* betas = rec.betas();
    u32 fail = ~0u, shift = 0;
    u64 xi = x_index;
    for (u32 li = 0; li < L.num_layers; li++) {
        const u32 ab = L.arity_bits[li];
        const u64 mask = ((u64)1 << ab) - 1, within = xi & mask, coset = xi >> ab;
        if (live) s_eval[k] = old_eval;
        __syncthreads();
        const u32 first = vc::first_with(k, [&](u32 j) { return s_x[j] >> (shift + ab); });
        const u32 at = (u32)((s_x[first] >> shift) & mask);
        const E ins = s_eval[first];
        bool consistent;
        const E next = vc::fold_layer<F>(x, within, ab, betas[li], section + dir[(VERIFY_ORACLES + li) * nqr + k], at, ins, old_eval, &consistent);
        if (!consistent && fail == ~0u) fail = vq::pos_consistency(VERIFY_ORACLES, li);
        if (live) {
            T* out = inferred + (((size_t)proof * L.num_layers + li) * nqr + k) * D;
            for (u32 d = 0; d < D; d++) out[d] = (T)F::dec(F::coord(ins, d));
        }
        __syncthreads();   // every lane has read s_eval before the next layer overwrites it
        old_eval = next;
        for (u32 i = 0; i < ab; i++) x = F::mul(x, x);
        xi = coset;
        shift += ab;
    }
    const E* fin = rec.final_poly();
    const E end = vq::final_eval<F>(L.final_len, x, [&](u32 i) { return fin[i]; });
    if (!vq::eeq<F>(end, old_eval) && fail == ~0u) fail = vq::pos_final(VERIFY_ORACLES, L.num_layers);
    if (live && fail != ~0u) atomicMin(reinterpret_cast<unsigned long long*>(keys + proof), (unsigned long long)vq::fail_key(k, fail));
}

// blockIdx.y = tree: the lanes of a workgroup share a leaf width and a path length (Sponge<GlF> is wave-wide)
template <class F>
__global__ __launch_bounds__(VERIFY_COMPRESSED_MAX_QUERIES) void k_vc_paths(VerifyCompressedLayout C, const unsigned char* __restrict__ rounds,
                                                                            const unsigned char* __restrict__ records,
                                                                            const typename F::T* __restrict__ circuit_cap,
                                                                            const typename F::T* __restrict__ inferred, u64* __restrict__ keys) {
    typedef typename F::T T;
    constexpr u32 D = F::D, HW = F::H;
    constexpr size_t TS = sizeof(T);
    const VerifyLayout& L = C.L;
    __shared__ poseidon_gl::v4i sponge_lds[Sponge<F>::LDS_V4];
    __shared__ u64 s_leaf[VERIFY_COMPRESSED_MAX_QUERIES];
    __shared__ u32 s_taken[VERIFY_COMPRESSED_MAX_QUERIES];
    __shared__ T s_node[VERIFY_COMPRESSED_MAX_QUERIES * HW];
    const u32 t = blockIdx.y, proof = blockIdx.x, nqr = L.nqr;
    const VerifyTree tr = L.trees[t];
    const bool live = threadIdx.x < nqr;
    const u32 k = live ? threadIdx.x : nqr - 1;
    const RecordView<F> rec{records + (size_t)proof * L.rec_bytes, L};
    const unsigned char* section = rounds + (size_t)proof * C.proof_stride;
    const u32* dir = reinterpret_cast<const u32*>(rec.p + C.rec_dir_off) + t * nqr;
    const T* cap = tr.cap_word == ~0u ? circuit_cap : rec.caps() + tr.cap_word;
    const u64 leaf = rec.x_index(k) >> tr.shift;
    if (live) { s_leaf[k] = leaf; s_taken[k] = 0; }
    Sponge<F> sp;
    sp.init(sponge_lds);
    __syncthreads();
    const unsigned char* entry = section + dir[k];
    const u32 stored_words = t < VERIFY_ORACLES ? tr.num_words : tr.num_words - D;   // a layer's coset lacks one element
    T cur[HW];
    if (t < VERIFY_ORACLES) {
        vq::leaf_digest<F>(sp, tr.num_words, [entry](u32 i) { return vq::load_word<F>(entry + (size_t)i * TS); }, cur);
    } else {
        const u32 li = t - VERIFY_ORACLES, ab = L.arity_bits[li];
        const u32 first = vc::first_with(k, [&](u32 j) { return s_leaf[j]; });
        const u32 at = (u32)((rec.x_index(first) >> (tr.shift - ab)) & (((u64)1 << ab) - 1));
        const T* ins = inferred + (((size_t)proof * L.num_layers + li) * nqr + k) * D;
        vq::leaf_digest<F>(sp, tr.num_words, [entry, at, ins](u32 i) { return vc::inflated_word<F>(entry, at, ins, i); }, cur);
    }
    const size_t path_at = (size_t)stored_words * TS + 1;   // behind the row and the length byte
    for (u32 level = 0; level < tr.path_len; level++) {
#pragma unroll
        for (u32 i = 0; i < HW; i++)
            if (live) s_node[k * HW + i] = cur[i];
        __syncthreads();
        const vc::Source src = vc::sibling_source(nqr, k, [&](u32 j) { return s_leaf[j] >> level; });
        T sib[HW];
        if (src.sibling != vc::NO_QUERY) {
#pragma unroll
            for (u32 i = 0; i < HW; i++) sib[i] = s_node[src.sibling * HW + i];
        } else {
            const u32 nth = min(s_taken[src.first], tr.path_len - 1);   // (the host checked the counts; this keeps the read in the slot)
            const unsigned char* stored = section + dir[src.first] + path_at + (size_t)nth * HW * TS;
#pragma unroll
            for (u32 i = 0; i < HW; i++) sib[i] = vq::load_word<F>(stored + i * TS);
        }
        const bool took = src.sibling == vc::NO_QUERY && src.first == k;
        __syncthreads();   // every lane has read the nodes and the counters of this level
        vq::two_to_one<F>(sp, cur, [&sib](u32 i) { return sib[i]; }, ((leaf >> level) & 1) != 0);
        if (live && took) s_taken[k]++;
    }
    const u64 cap_index = leaf >> tr.path_len;
    bool ok = true;
#pragma unroll
    for (u32 i = 0; i < HW; i++) ok = ok && cur[i] == cap[cap_index * HW + i];
    const u32 pos = t < VERIFY_ORACLES ? vq::pos_initial_path(t) : vq::pos_layer_path(VERIFY_ORACLES, t - VERIFY_ORACLES);
    if (live && !ok) atomicMin(reinterpret_cast<unsigned long long*>(keys + proof), (unsigned long long)vq::fail_key(k, pos));
}

inline u32 nblk(u64 n, u32 b) { return (u32)((n + b - 1) / b); }

}  // namespace

template <class F>
void verify_paths(const VerifyLayout& L, const unsigned char* rounds, const unsigned char* records, const typename F::T* circuit_cap,
                  u64* keys, hipStream_t st) {
    const u64 total = (u64)L.num_proofs * L.nqr;
    if (!total) return;
    hipLaunchKernelGGL(k_verify_paths<F>, dim3(nblk(total, 256), VERIFY_ORACLES + L.num_layers), dim3(256), 0, st, L, rounds, records,
                       circuit_cap, keys);
}
template <class F>
void verify_queries(const VerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st) {
    const u64 total = (u64)L.num_proofs * L.nqr;
    if (!total) return;
    hipLaunchKernelGGL(k_verify_queries<F>, dim3(nblk(total, 64)), dim3(64), 0, st, L, rounds, records, keys);
}

template <class F>
void fri_verify_paths(const FriVerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st) {
    const u64 total = (u64)L.num_proofs * L.nqr;
    if (!total) return;
    hipLaunchKernelGGL(k_fri_verify_paths<F>, dim3(nblk(total, 256), L.num_oracles + L.num_layers), dim3(256), 0, st, L, rounds, records, keys);
}
template <class F>
void fri_verify_queries(const FriVerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st) {
    const u64 total = (u64)L.num_proofs * L.nqr;
    if (!total) return;
    hipLaunchKernelGGL(k_fri_verify_queries<F>, dim3(nblk(total, 64)), dim3(64), 0, st, L, rounds, records, keys);
}

template <class F>
void verify_compressed_queries(const VerifyCompressedLayout& C, const unsigned char* rounds, const unsigned char* records,
                               typename F::T* inferred, u64* keys, hipStream_t st) {
    if (!C.L.num_proofs || !C.L.nqr) return;
    hipLaunchKernelGGL(k_vc_queries<F>, dim3(C.L.num_proofs), dim3(64 * nblk(C.L.nqr, 64)), 0, st, C, rounds, records, inferred, keys);
}
template <class F>
void verify_compressed_paths(const VerifyCompressedLayout& C, const unsigned char* rounds, const unsigned char* records,
                             const typename F::T* circuit_cap, const typename F::T* inferred, u64* keys, hipStream_t st) {
    if (!C.L.num_proofs || !C.L.nqr) return;
    hipLaunchKernelGGL(k_vc_paths<F>, dim3(C.L.num_proofs, VERIFY_ORACLES + C.L.num_layers), dim3(64 * nblk(C.L.nqr, 64)), 0, st, C, rounds,
                       records, circuit_cap, inferred, keys);
}

template void verify_compressed_queries<GlF>(const VerifyCompressedLayout&, const unsigned char*, const unsigned char*, u64*, u64*, hipStream_t);
template void verify_compressed_queries<BbF>(const VerifyCompressedLayout&, const unsigned char*, const unsigned char*, u32*, u64*, hipStream_t);
template void verify_compressed_paths<GlF>(const VerifyCompressedLayout&, const unsigned char*, const unsigned char*, const u64*, const u64*, u64*, hipStream_t);
template void verify_compressed_paths<BbF>(const VerifyCompressedLayout&, const unsigned char*, const unsigned char*, const u32*, const u32*, u64*, hipStream_t);
template void verify_paths<GlF>(const VerifyLayout&, const unsigned char*, const unsigned char*, const u64*, u64*, hipStream_t);
template void verify_paths<BbF>(const VerifyLayout&, const unsigned char*, const unsigned char*, const u32*, u64*, hipStream_t);
template void verify_queries<GlF>(const VerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void verify_queries<BbF>(const VerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void fri_verify_paths<GlF>(const FriVerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void fri_verify_paths<BbF>(const FriVerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void fri_verify_queries<GlF>(const FriVerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void fri_verify_queries<BbF>(const FriVerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);

}  // namespace gbk

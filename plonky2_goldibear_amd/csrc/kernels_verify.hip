// gb_verify_batch's device stage (verify_batch_host.inc): the query rounds of many proofs of one circuit, the checks of
// verify_query.hpp run lane-per-item - what verify_fri_parsed (verifier_host.inc) walks in sequence on the host.
//   k_verify_paths    one lane per (tree, proof, query round): hash_or_noop of the opened row, two_to_one up to the cap
//                     (verify_merkle_proof_to_cap, hash/merkle_proofs.rs:54-76) - the four oracles, then the FRI layers
//   k_verify_queries  one lane per (proof, query round): fri_combine_initial, per layer the consistency check and
//                     compute_evaluation, the final polynomial (fri/verifier.rs:121-250)
// Every check runs whether or not an earlier one of its proof failed; the proof's result is the minimum of the failing checks'
// keys (query round, position in the round), which is the check the host verifier reaches first, whatever the schedule.
// All offsets come from the circuit's shape (VerifyLayout, kernels.hpp); the proofs' bytes are only ever read as field words.
#include "kernels.hpp"
#include "sponge.hpp"
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

template void verify_paths<GlF>(const VerifyLayout&, const unsigned char*, const unsigned char*, const u64*, u64*, hipStream_t);
template void verify_paths<BbF>(const VerifyLayout&, const unsigned char*, const unsigned char*, const u32*, u64*, hipStream_t);
template void verify_queries<GlF>(const VerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);
template void verify_queries<BbF>(const VerifyLayout&, const unsigned char*, const unsigned char*, u64*, hipStream_t);

}  // namespace gbk

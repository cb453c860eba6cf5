// The lane-per-item sponge of the FRI kernels (k_fri_leaves, k_pow_grind in kernels_prover.hip) and of the batch verifier
// (kernels_verify.hip): device code only.
#pragma once
#include "field_traits.hpp"
#include "poseidon2_bb.hpp"
#include "poseidon_gl_grouped.hpp"

namespace gbk {

// Sponge over the field's permutation, rate 8, fed with DEVICE-form elements; out() gives canonical words.
template <class F>
struct Sponge;
// The Goldilocks sponge runs the permutation with its MDS layers on the matrix pipe and its partial rounds in groups
// (poseidon_gl_grouped.hpp), like the tree kernels: init() and permute() must be reached by all 64 lanes of a wave, so the kernels below clamp the index of lanes past
// the end instead of returning early.
template <>
struct Sponge<GlF> {
    static constexpr int LDS_V4 = poseidon_gl::GROUP_LDS_V4;   // the workgroup's operand table of the grouped partial rounds
    u64 s[12];
    poseidon_gl::MdsOperand amat;
    const poseidon_gl::v4i* gops;
    __device__ __forceinline__ void init(poseidon_gl::v4i* lds) {   // all threads of the workgroup (fills the table, one barrier)
        amat = poseidon_gl::mds_mfma_matrix();
        poseidon_gl::group_ops_init(lds);
        gops = lds + (threadIdx.x & 63);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = 0;
    }
    __device__ __forceinline__ void permute() {   // plain lazy residues in and out, as poseidon_gl::permute_lazy
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = poseidon_gl::to_mont(s[i]);
        poseidon_gl::permute_mont_mfma_grouped(s, amat, gops);
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = poseidon_gl::mont_fold((u32)s[i], (u32)(s[i] >> 32), 0u, 0u);
    }
    __device__ __forceinline__ u64 out(int i) { return poseidon_gl::to_canonical(s[i]); }
    __device__ __forceinline__ void set_canonical(int i, u64 v) { s[i] = v; }
};
template <>
struct Sponge<BbF> {
    static constexpr int LDS_V4 = 1;   // none needed
    u32 s[16];
    __device__ __forceinline__ void init(poseidon_gl::v4i*) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = 0;
    }
    __device__ __forceinline__ void permute() { poseidon2_bb::permute(s); }
    __device__ __forceinline__ u32 out(int i) { return bb::from_mont(s[i]); }
    __device__ __forceinline__ void set_canonical(int i, u32 v) { s[i] = bb::to_mont(v); }
};

}  // namespace gbk

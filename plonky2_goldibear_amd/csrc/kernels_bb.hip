// BabyBear kernels for gfx950: the Poseidon2-16 Merkle tree (H = 8) and the Montgomery-form conversions (the transforms are
// ntt_passes.hpp / kernels_bb16.hip).
//
// Replaces, for F = BabyBear, the same reference code as the Goldilocks kernels:
// hash/merkle_tree.rs:86-181 with Poseidon2BabyBearHash (hash/poseidon2_babybear.rs:163-176).
// Device-resident element data is in Montgomery form; digests are canonical.
#include "kernels.hpp"
#include "poseidon2_bb.hpp"
#include "poseidon2_bb_coop.hpp"

namespace gbk {

// ------------------------------------------------------------------ Merkle (Poseidon2, rate 8, digest 8 x u32 canonical)

__global__ __launch_bounds__(256) void k_bb_merkle_leaves(const u32* __restrict__ cols, size_t col_stride, u32 width, u64 num_leaves,
                                                          u32* __restrict__ out) {
    u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    u32 s[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = 0;
    uint4* o = reinterpret_cast<uint4*>(out + 8 * j);
    if (width <= 8) {  // hash_or_noop (plonk/config.rs:70-84), NUM_HASH_OUT_ELTS = 8
        for (u32 c = 0; c < width; c++) s[c] = bb::from_mont(cols[(size_t)c * col_stride + j]);
        o[0] = make_uint4(s[0], s[1], s[2], s[3]);
        o[1] = make_uint4(s[4], s[5], s[6], s[7]);
        return;
    }
    for (u32 c0 = 0; c0 < width; c0 += 8) {  // one loop, one inlined copy of the permutation
        if (c0) {  // the capacity words go on at scale 1; the rate words are overwritten (partially in the last absorption)
#pragma unroll
            for (int i = 8; i < 16; i++) s[i] = poseidon2_bb::renorm_lazy(s[i]);
            if (c0 + 8 > width) {
#pragma unroll
                for (int i = 0; i < 8; i++) s[i] = poseidon2_bb::renorm_lazy(s[i]);
            }
        }
        if (c0 + 8 <= width) {
#pragma unroll
            for (int i = 0; i < 8; i++) s[i] = cols[(size_t)(c0 + i) * col_stride + j];
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (c0 + i < width) s[i] = cols[(size_t)(c0 + i) * col_stride + j];
        }
        poseidon2_bb::permute_scaled(s);
    }
    using poseidon2_bb::canonical_out;
    o[0] = make_uint4(canonical_out(s[0]), canonical_out(s[1]), canonical_out(s[2]), canonical_out(s[3]));
    o[1] = make_uint4(canonical_out(s[4]), canonical_out(s[5]), canonical_out(s[6]), canonical_out(s[7]));
}
// The leaf sponge in column SEGMENTS [c_begin, c_end) (see k_gl_merkle_leaves_seg): between segments the capacity words 8..15 - as
// the permutation left them: the next absorption's renorm brings them back to scale 1 - and, in front of a ragged last
// absorption, the rate words it leaves alone (`keep_from`..7) wait in `state` [8 + 8 - keep_from][num_leaves].
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256, 7) void k_bb_merkle_leaves_seg(const u32* __restrict__ cols, size_t col_stride, u32 c_begin, u32 c_end,
                                                                 u64 num_leaves, u32* __restrict__ state, u32 keep_from,
                                                                 u32* __restrict__ out) {
    u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= num_leaves) return;
    u32 s[16];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = 0;
    // `state` holds only the rows that are used: [0, 8) the capacity words 8..15, then rate word i >= keep_from at row 8 + i - keep_from
#pragma unroll
    for (int i = 8; i < 16; i++) s[i] = FIRST ? 0 : state[(size_t)(i - 8) * num_leaves + j];
    if (LAST && !FIRST && c_end - c_begin < 8) {
        const u32 kf = c_end - c_begin;   // = the keep_from the segment before was given
#pragma unroll
        for (int i = 1; i < 8; i++)
            if ((u32)i >= kf) s[i] = state[(size_t)(8 + i - kf) * num_leaves + j];
    }
    for (u32 c0 = c_begin; c0 < c_end; c0 += 8) {
        if (c0) {  // the capacity words go on at scale 1; the rate words are overwritten (partially in the last absorption)
#pragma unroll
            for (int i = 8; i < 16; i++) s[i] = poseidon2_bb::renorm_lazy(s[i]);
            if (LAST && c0 + 8 > c_end) {
#pragma unroll
                for (int i = 0; i < 8; i++) s[i] = poseidon2_bb::renorm_lazy(s[i]);
            }
        }
        if (!LAST || c0 + 8 <= c_end) {
#pragma unroll
            for (int i = 0; i < 8; i++) s[i] = cols[(size_t)(c0 + i) * col_stride + j];
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (c0 + i < c_end) s[i] = cols[(size_t)(c0 + i) * col_stride + j];
        }
        poseidon2_bb::permute_scaled(s);
    }
    if (!LAST) {
#pragma unroll
        for (int i = 8; i < 16; i++) state[(size_t)(i - 8) * num_leaves + j] = s[i];
        if (keep_from < 8) {
#pragma unroll
            for (int i = 1; i < 8; i++)
                if ((u32)i >= keep_from) state[(size_t)(8 + i - keep_from) * num_leaves + j] = s[i];
        }
        return;
    }
    uint4* o = reinterpret_cast<uint4*>(out + 8 * j);
    using poseidon2_bb::canonical_out;
    o[0] = make_uint4(canonical_out(s[0]), canonical_out(s[1]), canonical_out(s[2]), canonical_out(s[3]));
    o[1] = make_uint4(canonical_out(s[4]), canonical_out(s[5]), canonical_out(s[6]), canonical_out(s[7]));
}
__global__ __launch_bounds__(256) void k_bb_merkle_level(const u32* __restrict__ in, u32* __restrict__ out, u64 num_out) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_out) return;
    const uint4* p = reinterpret_cast<const uint4*>(in + 16 * i);
    uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    u32 s[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < 16; k++) s[k] = bb::to_mont(s[k]);
    poseidon2_bb::permute_scaled(s);
    using poseidon2_bb::canonical_out;
    uint4* o = reinterpret_cast<uint4*>(out + 8 * i);
    o[0] = make_uint4(canonical_out(s[0]), canonical_out(s[1]), canonical_out(s[2]), canonical_out(s[3]));
    o[1] = make_uint4(canonical_out(s[4]), canonical_out(s[5]), canonical_out(s[6]), canonical_out(s[7]));
}
// The same two kernels (and the FRI layer leaves) with one state per 16-lane row (poseidon2_bb_coop.hpp) for small trees.
__global__ __launch_bounds__(64) void k_bb_merkle_level_coop(const u32* __restrict__ in, u32* __restrict__ out, u64 num_out) {
    const u32 l = threadIdx.x & 15;
    const u64 node = (u64)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = node < num_out;
    u32 x = bb::to_mont(in[16 * (valid ? node : 0) + l]);
    x = poseidon2_bb_coop::permute(x, l);
    if (valid && l < 8) out[8 * node + l] = bb::from_mont(x);
}
// width > 8 (narrower leaves are not hashed, plonk/config.rs:70-84); cols in Montgomery form
__global__ __launch_bounds__(64) void k_bb_merkle_leaves_coop(const u32* __restrict__ cols, size_t col_stride, u32 width,
                                                              u64 num_leaves, u32* __restrict__ out) {
    const u32 l = threadIdx.x & 15;
    const u64 leaf = (u64)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = leaf < num_leaves;
    const u64 j = valid ? leaf : 0;
    u32 x = 0;
    for (u32 c0 = 0; c0 < width; c0 += 8) {
        if (l < 8 && c0 + l < width) x = cols[(size_t)(c0 + l) * col_stride + j];  // overwrite-mode absorption
        x = poseidon2_bb_coop::permute(x, l);
    }
    if (valid && l < 8) out[8 * leaf + l] = bb::from_mont(x);
}
// FRI layer leaves (fri/prover.rs:101-107), D = 4: vals = [4][len] coordinate columns (Montgomery), 4 * arity > 8 only
__global__ __launch_bounds__(64) void k_bb_fri_leaves_coop(const u32* __restrict__ vals, size_t len, u32 arity_bits, u64 num_leaves,
                                                           u32* __restrict__ out) {
    const u32 l = threadIdx.x & 15;
    const u64 leaf = (u64)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = leaf < num_leaves;
    const u32* a = vals + ((valid ? leaf : 0) << arity_bits);
    const u32 arity = 1u << arity_bits;
    u32 x = 0;
    for (u32 k0 = 0; k0 < arity; k0 += 2) {   // two extension elements = eight base elements per absorption
        const u32 k = k0 + (l >> 2);
        if (l < 8 && k < arity) x = a[(size_t)(l & 3) * len + k];
        x = poseidon2_bb_coop::permute(x, l);
    }
    if (valid && l < 8) out[8 * leaf + l] = bb::from_mont(x);
}

__global__ __launch_bounds__(256) void k_bb_permute(const u32* __restrict__ in, u32* __restrict__ out, u64 count) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    u32 s[16];
#pragma unroll
    for (int e = 0; e < 16; e++) s[e] = bb::to_mont(in[16 * i + e]);
    poseidon2_bb::permute(s);
#pragma unroll
    for (int e = 0; e < 16; e++) out[16 * i + e] = bb::from_mont(s[e]);
}

// ------------------------------------------------------------------ Montgomery form <-> canonical
__global__ void k_bb_to_mont(const u32* __restrict__ src, u32* __restrict__ dst, size_t n) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) dst[g] = bb::to_mont(src[g]);
}
__global__ void k_bb_from_mont(const u32* __restrict__ src, u32* __restrict__ dst, size_t n) {
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) dst[g] = bb::from_mont(src[g]);
}

// ------------------------------------------------------------------ launchers
static inline u32 nblk(size_t n, u32 bs) { return (u32)((n + bs - 1) / bs); }

// as for Goldilocks (kernels_merkle.hip): below this many states the lane-per-state kernels are latency-bound
static constexpr u64 BB_COOP_MAX_STATES = 16384;

void bb_merkle_leaves(const u32* cols, size_t col_stride, u32 width, u64 num_leaves, u32* out, hipStream_t stream) {
    if (width > 8 && num_leaves <= BB_COOP_MAX_STATES) {
        hipLaunchKernelGGL(k_bb_merkle_leaves_coop, dim3(nblk(num_leaves, 4)), dim3(64), 0, stream, cols, col_stride, width, num_leaves, out);
        return;
    }
    hipLaunchKernelGGL(k_bb_merkle_leaves, dim3(nblk(num_leaves, 256)), dim3(256), 0, stream, cols, col_stride, width, num_leaves, out);
}
void bb_merkle_leaves_segment(const u32* cols, size_t col_stride, u32 c_begin, u32 c_end, u64 num_leaves, u32* state, bool last,
                              u32 next_cols, u32* out, hipStream_t stream) {
    const dim3 grid(nblk(num_leaves, 256)), block(256);
    const u32 keep_from = next_cols < 8u ? next_cols : 8u;
    if (c_begin == 0 && !last)
        hipLaunchKernelGGL((k_bb_merkle_leaves_seg<true, false>), grid, block, 0, stream, cols, col_stride, c_begin, c_end, num_leaves, state, keep_from, out);
    else if (!last)
        hipLaunchKernelGGL((k_bb_merkle_leaves_seg<false, false>), grid, block, 0, stream, cols, col_stride, c_begin, c_end, num_leaves, state, keep_from, out);
    else
        hipLaunchKernelGGL((k_bb_merkle_leaves_seg<false, true>), grid, block, 0, stream, cols, col_stride, c_begin, c_end, num_leaves, state, keep_from, out);
}
bool bb_fri_leaves_coop(const u32* vals, size_t len, u32 arity_bits, u64 num_leaves, u32* out, hipStream_t stream) {
    if (num_leaves > BB_COOP_MAX_STATES || (4u << arity_bits) <= 8) return false;
    hipLaunchKernelGGL(k_bb_fri_leaves_coop, dim3(nblk(num_leaves, 4)), dim3(64), 0, stream, vals, len, arity_bits, num_leaves, out);
    return true;
}
void bb_merkle_level(const u32* in, u32* out, u64 num_out, hipStream_t stream) {
    if (num_out <= BB_COOP_MAX_STATES) {
        hipLaunchKernelGGL(k_bb_merkle_level_coop, dim3(nblk(num_out, 4)), dim3(64), 0, stream, in, out, num_out);
        return;
    }
    hipLaunchKernelGGL(k_bb_merkle_level, dim3(nblk(num_out, 256)), dim3(256), 0, stream, in, out, num_out);
}
void bb_poseidon2_permute(const u32* in, u32* out, u64 count, hipStream_t stream) {
    hipLaunchKernelGGL(k_bb_permute, dim3(nblk(count, 256)), dim3(256), 0, stream, in, out, count);
}
void bb_to_mont(const u32* src, u32* dst, size_t n, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_bb_to_mont, dim3(nblk(n, 256)), dim3(256), 0, stream, src, dst, n);
}
void bb_from_mont(const u32* src, u32* dst, size_t n, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_bb_from_mont, dim3(nblk(n, 256)), dim3(256), 0, stream, src, dst, n);
}

}  // namespace gbk

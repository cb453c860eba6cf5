// The passes around the transforms and the Merkle kernels that the stand-alone entry points need (gb_fft / gb_ifft / gb_lde,
// gb_merkle_tree_create): natural-order output, extension elements as interleaved words, per-power scaling, row-major leaves.
// Field-generic over the traits (GlF: canonical u64 words; BbF: 32-bit Montgomery words).
//
// The transform passes move CANONICAL words and convert nothing, for BabyBear too: the transforms are linear and every product in
// them is data times a table value, which the tables hold in Montgomery form (w R) - so a Montgomery product x (w R) / R = x w takes
// canonical words to canonical words, through the inverse passes, the LDE passes and the scaling here alike.  (Seen the other way: a
// canonical word x is the Montgomery word of x / R, and T(x / R) = T(x) / R has the Montgomery word T(x).)  Only the leaves of a
// Merkle tree are converted: the hash is not linear.
//
// An extension column [len][D] is D coordinate columns at word stride D: the transforms are F-linear with base-field twiddles and
// a base-field shift, so they run on the coordinate columns [D][len] like on any other column.
#include "kernels.hpp"

namespace gbk {

namespace {

constexpr int PT = 256;           // threads of every kernel here
constexpr u32 TB = 6, TS = 64;    // the permutation's tile: 64 x 64 elements (32 KiB of u64)

__device__ __forceinline__ u32 brev_bits(u32 x, u32 bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }

// LDS tile [row][col] with the columns of row r rotated by r (4-byte words) or r / 2 (8-byte words): a wave that reads one column
// of 64 rows - or of the 32 even / 32 odd rows a 64-bit read is served in - then touches every bank once, and a wave that writes
// one row still does
template <class T>
__device__ __forceinline__ u32 tile_at(u32 r, u32 c) { return r * TS + ((c + (sizeof(T) == 8 ? r >> 1 : r)) & (TS - 1)); }

// extension elements [ncols][len][D] -> coordinate columns [ncols * D][len]; total = ncols * len elements
template <class F>
__global__ __launch_bounds__(PT) void k_ext_load(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 log_len,
                                                 size_t total) {
    constexpr u32 D = F::D;
    const size_t e = (size_t)blockIdx.x * PT + threadIdx.x;
    if (e >= total) return;
    const size_t col = e >> log_len, i = e & (((size_t)1 << log_len) - 1);
#pragma unroll
    for (u32 k = 0; k < D; k++) dst[((col * D + k) << log_len) + i] = src[e * D + k];
}

// coordinate columns [ncols * D][len], natural order -> [ncols][len] (ext: [ncols][len][D]), element i times
// lo[i % 4096] hi[i / 4096] where SCALE (the powers of coset_ifft's shift^-1, plain device form; len <= 4096: hi is [1] = one).
// total = ncols * D * len words.  In place (dst == src) unless EXT.
template <class F, bool EXT, bool SCALE>
__global__ __launch_bounds__(PT) void k_poly_store(const typename F::T* src, typename F::T* dst, u32 log_len, size_t total,
                                                   const typename F::T* __restrict__ lo, const typename F::T* __restrict__ hi) {
    typedef typename F::T T;
    constexpr u32 D = EXT ? F::D : 1;
    const size_t e = (size_t)blockIdx.x * PT + threadIdx.x;
    if (e >= total) return;
    const size_t cc = e >> log_len, i = e & (((size_t)1 << log_len) - 1);
    T x = src[e];
    if (SCALE) {
        x = F::mul(x, lo[i & 4095]);
        if (i >> 12) x = F::mul(x, hi[i >> 12]);
    }
    dst[EXT ? (((cc / D) << log_len) + i) * D + cc % D : e] = x;
}

// leaf order -> natural order, up to one tile (log_len <= 12): one workgroup per column, the column through LDS.
// src: coordinate columns [ncols * D][len], src[j] = the value at point bitrev(j); dst natural order, interleaved if EXT
template <class F, bool EXT>
__global__ __launch_bounds__(PT) void k_bitrev_small(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 log_len) {
    typedef typename F::T T;
    constexpr u32 D = EXT ? F::D : 1;
    __shared__ T sh[4096];
    const u32 len = 1u << log_len;
    const size_t cc = blockIdx.x;
    const T* in = src + (cc << log_len);
    for (u32 t = threadIdx.x; t < len; t += PT) sh[t] = in[t];
    __syncthreads();
    T* out = dst + (((cc / D) << log_len) * D + cc % D);
    for (u32 i = threadIdx.x; i < len; i += PT) out[(size_t)i * D] = sh[brev_bits(i, log_len)];
}

// leaf order -> natural order above one tile (log_len = L > 12).  i = A 2^(L-6) + M 2^6 + C has bitrev(i) = rev(C) 2^(L-6) +
// rev(M) 2^6 + rev(A): for one M, the 64 x 64 elements (A, C) are 64 runs of 64 consecutive words on either side - rows rev(C) of
// the source, rows A of the destination - and the tile between them is transposed with both indices bit-reversed.
// grid = (ncols * D) << (L - 12); EXT: the D coordinate tiles of an element land in the same 64-element runs of the output.
template <class F, bool EXT>
__global__ __launch_bounds__(PT) void k_bitrev_tiles(const typename F::T* __restrict__ src, typename F::T* __restrict__ dst, u32 L) {
    typedef typename F::T T;
    constexpr u32 D = EXT ? F::D : 1;
    __shared__ T sh[TS * TS];
    const u32 mbits = L - 2 * TB;
    const size_t cc = (size_t)blockIdx.x >> mbits;
    const u32 M = blockIdx.x & ((1u << mbits) - 1);
    const u32 tx = threadIdx.x & (TS - 1), ty = threadIdx.x >> TB;
    const T* in = src + (cc << L) + ((size_t)brev_bits(M, mbits) << TB);
    for (u32 r = ty; r < TS; r += PT / TS) sh[tile_at<T>(r, tx)] = in[((size_t)r << (L - TB)) + tx];
    __syncthreads();
    T* out = dst + (((cc / D) << L) * D + cc % D);
    const u32 rc = brev_bits(tx, TB);
    for (u32 a = ty; a < TS; a += PT / TS) {
        const size_t i = ((size_t)a << (L - TB)) + ((size_t)M << TB) + tx;
        out[i * D] = sh[tile_at<T>(rc, brev_bits(a, TB))];
    }
}

// row-major canonical leaves [num_rows][width] -> column-major device form [width][num_rows] (what the leaf kernels read), a
// 64 x 64 tile per workgroup through LDS: 64-word runs on both sides.  grid = (ceil(num_rows / 64), ceil(width / 64))
template <class F>
__global__ __launch_bounds__(PT) void k_rows_to_columns(const typename F::T* __restrict__ rows, typename F::T* __restrict__ cols,
                                                        u64 num_rows, u32 width) {
    typedef typename F::T T;
    __shared__ T sh[TS * TS];
    const u64 r0 = (u64)blockIdx.x * TS;
    const u32 c0 = blockIdx.y * TS;
    const u32 tx = threadIdx.x & (TS - 1), ty = threadIdx.x >> TB;
    for (u32 r = ty; r < TS; r += PT / TS)
        if (r0 + r < num_rows && c0 + tx < width) sh[tile_at<T>(r, tx)] = rows[(r0 + r) * width + c0 + tx];
    __syncthreads();
    for (u32 c = ty; c < TS; c += PT / TS)
        if (r0 + tx < num_rows && c0 + c < width) cols[(u64)(c0 + c) * num_rows + r0 + tx] = F::enc(sh[tile_at<T>(tx, c)]);
}

inline u32 blocks(size_t n) { return (u32)((n + PT - 1) / PT); }

}  // namespace

template <class F>
void ext_load(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, hipStream_t stream) {
    const size_t total = ncols << log_len;
    if (total) hipLaunchKernelGGL(k_ext_load<F>, dim3(blocks(total)), dim3(PT), 0, stream, src, dst, log_len, total);
}

template <class F>
void poly_store(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, bool ext, const typename F::T* pow_lo,
                const typename F::T* pow_hi, hipStream_t stream) {
    const size_t total = (ncols * (ext ? F::D : 1)) << log_len;
    if (!total) return;
    const dim3 g(blocks(total)), b(PT);
    if (ext && pow_lo) hipLaunchKernelGGL((k_poly_store<F, true, true>), g, b, 0, stream, src, dst, log_len, total, pow_lo, pow_hi);
    else if (ext) hipLaunchKernelGGL((k_poly_store<F, true, false>), g, b, 0, stream, src, dst, log_len, total, pow_lo, pow_hi);
    else if (pow_lo) hipLaunchKernelGGL((k_poly_store<F, false, true>), g, b, 0, stream, src, dst, log_len, total, pow_lo, pow_hi);
    // (neither: the words are where they belong already)
}

template <class F>
void poly_bitrev_store(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, bool ext, hipStream_t stream) {
    const size_t cc = ncols * (ext ? F::D : 1);
    if (!cc) return;
    if (log_len <= POLY_SMALL_LOG) {
        if (ext) hipLaunchKernelGGL((k_bitrev_small<F, true>), dim3((u32)cc), dim3(PT), 0, stream, src, dst, log_len);
        else hipLaunchKernelGGL((k_bitrev_small<F, false>), dim3((u32)cc), dim3(PT), 0, stream, src, dst, log_len);
        return;
    }
    const dim3 g((u32)(cc << (log_len - 2 * TB)));
    if (ext) hipLaunchKernelGGL((k_bitrev_tiles<F, true>), g, dim3(PT), 0, stream, src, dst, log_len);
    else hipLaunchKernelGGL((k_bitrev_tiles<F, false>), g, dim3(PT), 0, stream, src, dst, log_len);
}

template <class F>
void rows_to_columns(const typename F::T* rows, typename F::T* cols, u64 num_rows, u32 width, hipStream_t stream) {
    if (!num_rows || !width) return;
    hipLaunchKernelGGL(k_rows_to_columns<F>, dim3((u32)((num_rows + TS - 1) / TS), (width + TS - 1) / TS), dim3(PT), 0, stream, rows,
                       cols, num_rows, width);
}

#define GB_INSTANTIATE_POLY(F)                                                                              \
    template void ext_load<F>(const F::T*, F::T*, size_t, u32, hipStream_t);                                \
    template void poly_store<F>(const F::T*, F::T*, size_t, u32, bool, const F::T*, const F::T*, hipStream_t); \
    template void poly_bitrev_store<F>(const F::T*, F::T*, size_t, u32, bool, hipStream_t);                 \
    template void rows_to_columns<F>(const F::T*, F::T*, u64, u32, hipStream_t);
GB_INSTANTIATE_POLY(GlF)
GB_INSTANTIATE_POLY(BbF)

}  // namespace gbk

// k_random_elements (random_stream.hpp): gb_random_elements on the device and the seeded salt columns of the provers.
// One lane computes one ChaCha20 block - the 16 working words in registers beside the initial state, which is the same for the
// whole launch but for the counter and therefore lives in scalar registers - reduces its four 128-bit pieces and stores the
// four elements as one contiguous 32-byte (Goldilocks) or 16-byte (BabyBear) piece: consecutive lanes write consecutive pieces.
// A range that starts or ends inside a block costs its first and last lane one bounds-checked path; every other lane stores
// without looking at the range.  The whole-piece stores need `first` to be a multiple of four elements (the destination is
// 16-byte aligned at `first`, so only then is every block's piece aligned); other ranges store element by element - a choice
// made once per launch, the same in every lane.
#include "kernels.hpp"
#include "random_stream.hpp"

namespace gbk {

constexpr u32 RANDOM_BLOCK = 256;

template <class T>
__device__ __forceinline__ void store_piece(T* dst, const T* v);
template <>
__device__ __forceinline__ void store_piece<u64>(u64* dst, const u64* v) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4((u32)v[0], (u32)(v[0] >> 32), (u32)v[1], (u32)(v[1] >> 32));
    d[1] = make_uint4((u32)v[2], (u32)(v[2] >> 32), (u32)v[3], (u32)(v[3] >> 32));
}
template <>
__device__ __forceinline__ void store_piece<u32>(u32* dst, const u32* v) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
}

// blocks block0 .. block0 + num_blocks - 1 of the streams (key.seed, (nonce[0], nonce[1], nonce[2] + blockIdx.y)); element e of
// stream y goes to out[y * stream_stride + e - first] for first <= e < first + count
template <class F, bool ALIGNED>
__global__ __launch_bounds__(RANDOM_BLOCK) void k_random_elements(rnd::Key key, u32 block0, u32 num_blocks, u64 first, u64 count,
                                                                  typename F::T* __restrict__ out, u64 stream_stride) {
    typedef typename F::T T;
    const u32 g = blockIdx.x * RANDOM_BLOCK + threadIdx.x;
    if (g >= num_blocks) return;
    const u32 block = block0 + g;
    key.nonce[2] += blockIdx.y;
    out += (u64)blockIdx.y * stream_stride;
    T v[4];
    rnd::block_elements<F>(key, block, v);
    const u64 e0 = (u64)block << 2;
    if (e0 >= first && e0 + 4 <= first + count) {
        T* dst = out + (e0 - first);
        if (ALIGNED) {
            store_piece<T>(dst, v);
        } else {
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
    } else {   // the first or the last block of a ragged range
        for (u32 i = 0; i < 4; i++) {
            const u64 e = e0 + i;
            if (e >= first && e - first < count) out[e - first] = v[i];
        }
    }
}

template <class F>
bool random_elements(const rnd::Key& key, u64 first, u64 count, u32 num_streams, typename F::T* out, u64 stream_stride, hipStream_t stream) {
    if (!count || !num_streams) return true;
    const u64 b0 = first >> 2, b1 = (first + count - 1) >> 2;
    // whole-piece stores: every stream's destination must be 16-byte aligned at a block boundary
    const bool aligned = (first & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                         (num_streams == 1 || (stream_stride * sizeof(typename F::T)) % 16 == 0);
    constexpr u64 PER_LAUNCH = (u64)1 << 30;   // lanes per launch: the grid's size stays below 2^32 threads
    for (u64 b = b0; b <= b1; b += PER_LAUNCH) {
        const u32 nb = (u32)std::min<u64>(PER_LAUNCH, b1 - b + 1);
        const dim3 grid((nb + RANDOM_BLOCK - 1) / RANDOM_BLOCK, num_streams);
        if (aligned)
            hipLaunchKernelGGL((k_random_elements<F, true>), grid, dim3(RANDOM_BLOCK), 0, stream, key, (u32)b, nb, first, count, out, stream_stride);
        else
            hipLaunchKernelGGL((k_random_elements<F, false>), grid, dim3(RANDOM_BLOCK), 0, stream, key, (u32)b, nb, first, count, out, stream_stride);
        if (hipGetLastError() != hipSuccess) return false;
    }
    return true;
}
template bool random_elements<GlF>(const rnd::Key&, u64, u64, u32, u64*, u64, hipStream_t);
template bool random_elements<BbF>(const rnd::Key&, u64, u64, u32, u32*, u64, hipStream_t);

}  // namespace gbk

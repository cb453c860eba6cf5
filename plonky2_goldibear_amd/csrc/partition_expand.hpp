// PartitionWitness::full_witness (iop/witness.rs:359-371) on the device: out[col][row] = staged[slots[row][col]] - a gather fused
// with a transpose.  `slots` is the row-major [n][num_wires] map of partition_map.hpp, `staged` the compacted class values (one
// per slot, in ascending target index - so a cell that is its own representative reads staged[] at an index that grows with
// row * num_wires + col), `out` the column-major [num_wires][n] matrix MatrixWitness.wire_values is.  Words are copied, never
// interpreted: canonical words in, canonical words out.
//
// A workgroup owns a tile of TILE_ROWS x TILE_COLS cells and takes it through LDS:
//   read phase   lanes run along the columns of a row: 32 consecutive u32 slots (128 B) per half wave, then the values they
//                name, which for untouched cells are 32 consecutive elements too; all of a thread's slot loads are issued before
//                its first value load;
//   LDS          tile[col][row] with a row stride of TILE_ROWS + 1 elements: 8-byte elements land 2 dwords apart per column
//                (32 lanes cover 16 even banks twice: the two-cycle minimum of a 64-bit write), 4-byte elements 1 bank apart;
//   write phase  lanes run along the rows of a column and each stores 16 bytes (2 Goldilocks / 4 BabyBear rows): a column of the
//                tile is one contiguous 512 B / 256 B run of `out`.
// n = 2^log_n with log_n >= 2 (the prover's range), so a row that is inside the matrix has its whole 16-byte group inside; n below
// TILE_ROWS and num_wires that is no multiple of TILE_COLS are masked.
//
// Depends on nothing but the field traits' element type F::T: tests/device/partition_expand.hip includes it on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace gbk {
namespace partition {

constexpr unsigned TILE_ROWS = 64, TILE_COLS = 32, EXPAND_THREADS = 256;

template <class F>
__global__ __launch_bounds__(EXPAND_THREADS) void k_expand_partition(const uint32_t* __restrict__ slots,
                                                                     const typename F::T* __restrict__ staged,
                                                                     typename F::T* __restrict__ out, unsigned log_n,
                                                                     unsigned num_wires) {
    typedef typename F::T T;
    constexpr unsigned VEC = 16 / sizeof(T);                        // rows per 16-byte store
    constexpr unsigned STRIDE = TILE_ROWS + 1;
    constexpr unsigned ROWS_PER_PASS = EXPAND_THREADS / TILE_COLS;  // 8
    constexpr unsigned READS = TILE_ROWS / ROWS_PER_PASS;           // 8 cells per thread
    constexpr unsigned LANES_PER_COL = TILE_ROWS / VEC;
    constexpr unsigned COLS_PER_PASS = EXPAND_THREADS / LANES_PER_COL;
    static_assert(TILE_ROWS % ROWS_PER_PASS == 0 && TILE_COLS % COLS_PER_PASS == 0, "tile shape");
    __shared__ T tile[TILE_COLS * STRIDE];
    const size_t n = (size_t)1 << log_n;
    const size_t row0 = (size_t)blockIdx.x * TILE_ROWS;
    const unsigned col0 = blockIdx.y * TILE_COLS, t = threadIdx.x;
    {
        const unsigned c = t % TILE_COLS, r0 = t / TILE_COLS, col = col0 + c;
        uint32_t slot[READS];
        bool inside[READS];
#pragma unroll
        for (unsigned i = 0; i < READS; i++) {
            const size_t row = row0 + r0 + i * ROWS_PER_PASS;
            inside[i] = col < num_wires && row < n;
            slot[i] = inside[i] ? slots[row * num_wires + col] : 0;
        }
#pragma unroll
        for (unsigned i = 0; i < READS; i++)
            if (inside[i]) tile[c * STRIDE + r0 + i * ROWS_PER_PASS] = staged[slot[i]];
    }
    __syncthreads();
    {
        const unsigned rv = (t % LANES_PER_COL) * VEC;
        const size_t row = row0 + rv;
#pragma unroll
        for (unsigned cc = t / LANES_PER_COL; cc < TILE_COLS; cc += COLS_PER_PASS) {
            const unsigned col = col0 + cc;
            if (col >= num_wires || row >= n) continue;
            alignas(16) T v[VEC];
#pragma unroll
            for (unsigned k = 0; k < VEC; k++) v[k] = tile[cc * STRIDE + rv + k];
            *reinterpret_cast<uint4*>(out + (size_t)col * n + row) = *reinterpret_cast<const uint4*>(v);
        }
    }
}

// slots [2^log_n][num_wires] (every entry below the length of `staged`), out [num_wires][2^log_n] 16-byte aligned; log_n >= 2
template <class F>
inline void launch_expand_partition(const uint32_t* slots, const typename F::T* staged, typename F::T* out, unsigned log_n,
                                    unsigned num_wires, hipStream_t stream) {
    if (!num_wires) return;
    const size_t n = (size_t)1 << log_n;
    const dim3 grid((unsigned)((n + TILE_ROWS - 1) / TILE_ROWS), (num_wires + TILE_COLS - 1) / TILE_COLS);
    hipLaunchKernelGGL(k_expand_partition<F>, grid, dim3(EXPAND_THREADS), 0, stream, slots, staged, out, log_n, num_wires);
}

}  // namespace partition
}  // namespace gbk

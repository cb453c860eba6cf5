// gb_wiring_sigmas: copy constraints -> sigma columns and representative map.  What a thread does to one pair, key or cell is
// wiring.hpp's (GB_HD, shared with the host); the passes:
//   classes   k_wiring_init (parent[t] = t), k_wiring_union: one thread per pair of a slice, grid-stride - the range and
//             routability checks first (the lowest offending pair of each kind by a 64-bit atomic minimum, and such a pair is
//             never used as an address), then the lock-free hook.  k_wiring_jump: one compression pass, every target jumps up
//             to JUMPS ancestors; a wave that moved a pointer sets the pass's flag, and the host stops after a pass that moved none.
//   order     k_wiring_count: routed cells per label (a wave whose cells all have one label adds them in one atomic).
//             k_wiring_keep_count / k_wiring_compact: the routed cells whose label counts two or more, in ascending cell order -
//             kept cells per tile, an exclusive scan of the tiles, and the position from the scan plus the wave's ballot.
//             k_sort_hist / k_sort_scatter: one stable pass of the radix sort - a digit histogram per workgroup (LDS atomics),
//             written [digit][tile] with no global atomic at all, an exclusive scan over it, and a scatter whose rank inside the
//             workgroup is a ballot match per 64-key chunk plus a running sum over the chunks in LDS: nothing depends on the order
//             in which threads run.  k_wiring_successors: a cell's successor from the sorted runs, and the class statistics.
//   scan      k_scan_reduce / k_scan_spine / k_scan_apply: exclusive scan of u32 words in place, tiles of SCAN_TILE words
//   sigmas    k_wiring_sigmas: one thread per routed cell in sigma's numbering col * n + row, grid-stride, coalesced along rows
//   map       k_wiring_widen (u32 -> u64), k_wiring_merged (targets that are not their own representative)
#include "kernels.hpp"
#include "wiring.hpp"

namespace gbk {

namespace {
using namespace wiring;
constexpr u32 MAX_BLOCKS = 4096, SCAN_ITEMS = 8, SCAN_TILE = BLOCK * SCAN_ITEMS, TILE_ITEMS = SORT_TILE / BLOCK, WAVES = BLOCK / 64;
static_assert(RADIX == BLOCK, "one thread per digit in the sort kernels");

static inline dim3 blocks_for(u64 count) { return dim3((u32)std::max<u64>(1, (count + BLOCK - 1) / BLOCK)); }
static inline dim3 stride_blocks(u64 count) { return dim3(std::min<u32>(blocks_for(count).x, MAX_BLOCKS)); }
static inline u32 tiles_of(u64 count, u32 tile) { return (u32)std::max<u64>(1, (count + tile - 1) / tile); }

__device__ __forceinline__ u64 lanes_below() { return ((u64)1 << (threadIdx.x & 63)) - 1; }

// the workgroup's sum of v in every thread
__device__ __forceinline__ u64 block_sum(u64 v) {
    __shared__ u64 wave_sum[WAVES];
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();   // (the array may still be read from a call before)
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
    for (u32 w = 0; w < WAVES; w++) t += wave_sum[w];
    return t;
}
}  // namespace

__global__ __launch_bounds__(BLOCK) void k_wiring_init(u32* __restrict__ parent, u32 num_targets) {
    const u32 stride = gridDim.x * BLOCK;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < num_targets; t += stride) parent[t] = (u32)t;
}

// pairs: [count][2] target indices as the caller wrote them, the slice that starts at pair `first`; err = {lowest pair out of
// range, lowest pair that names a wire that is not routable}, all ones to start with
__global__ __launch_bounds__(BLOCK) void k_wiring_union(const u64* __restrict__ pairs, u32 count, u64 first, u32* parent, u64 num_targets,
                                                      u64 cells, u32 num_wires, u32 num_routed, u64* __restrict__ err) {
    const u32 stride = gridDim.x * BLOCK;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < count; i += stride) {
        const u64 a = pairs[2 * i], b = pairs[2 * i + 1];
        const u32 bad = check_pair(a, b, num_targets, cells, num_wires, num_routed);
        if (bad != PAIR_OK) {
            atomicMin(&err[bad == PAIR_OUT_OF_RANGE ? 0 : 1], first + i);
            continue;
        }
        if (a != b) unite(parent, (u32)a, (u32)b);
    }
}

__global__ __launch_bounds__(BLOCK) void k_wiring_jump(u32* parent, u32 num_targets, u32* __restrict__ changed) {
    const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const bool moved = t < num_targets && jump(parent, (u32)t);
    if (__ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1;
}

// count[label]++ for every routed cell; j = row * num_routed + col walks them in ascending cell order
__global__ __launch_bounds__(BLOCK) void k_wiring_count(const u32* __restrict__ parent, u32 routed, u32 num_routed, u32 num_wires,
                                                      u32* __restrict__ count) {
    const u32 stride = gridDim.x * BLOCK;
    for (u64 j0 = (u64)blockIdx.x * BLOCK; j0 < routed; j0 += stride) {   // (workgroup-uniform bounds: the ballots see whole waves)
        const u64 j = j0 + threadIdx.x;
        const bool valid = j < routed;
        const u32 label = valid ? parent[routed_cell((u32)j, num_routed, num_wires)] : NONE;
        const u32 first = __shfl(label, 0);
        const u64 live = __ballot(valid), same = __ballot(valid && label == first);
        if (same == live) {
            if ((threadIdx.x & 63) == 0 && valid) atomicAdd(&count[first], (u32)__popcll(live));
        } else if (valid) {
            atomicAdd(&count[label], 1u);
        }
    }
}

// tile_count[tile] = the routed cells of the tile whose label counts two or more
__global__ __launch_bounds__(BLOCK) void k_wiring_keep_count(const u32* __restrict__ parent, const u32* __restrict__ count, u32 routed,
                                                           u32 num_routed, u32 num_wires, u32* __restrict__ tile_count) {
    u32 kept = 0;
    for (u32 k = 0; k < TILE_ITEMS; k++) {
        const u64 j = (u64)blockIdx.x * SORT_TILE + k * BLOCK + threadIdx.x;
        if (j < routed && count[parent[routed_cell((u32)j, num_routed, num_wires)]] >= 2) kept++;
    }
    const u64 total = block_sum(kept);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = (u32)total;
}
// ... and those cells as keys[pos] = label, cells[pos] = cell, pos ascending with the cell; tile_start: the scanned counts
__global__ __launch_bounds__(BLOCK) void k_wiring_compact(const u32* __restrict__ parent, const u32* __restrict__ count, u32 routed,
                                                        u32 num_routed, u32 num_wires, const u32* __restrict__ tile_start, u32 m,
                                                        u32* __restrict__ keys, u32* __restrict__ cells) {
    __shared__ u32 chunk_count[TILE_CHUNKS];
    u32 label[TILE_ITEMS], cell[TILE_ITEMS], rank[TILE_ITEMS];
    bool keep[TILE_ITEMS];
    for (u32 k = 0; k < TILE_ITEMS; k++) {   // element k * BLOCK + threadIdx.x of the tile lies in chunk k * WAVES + wave
        const u64 j = (u64)blockIdx.x * SORT_TILE + k * BLOCK + threadIdx.x;
        keep[k] = false;
        if (j < routed) {
            cell[k] = routed_cell((u32)j, num_routed, num_wires);
            label[k] = parent[cell[k]];
            keep[k] = count[label[k]] >= 2;
        }
        const u64 kept = __ballot(keep[k]);
        rank[k] = (u32)__popcll(kept & lanes_below());
        if ((threadIdx.x & 63) == 0) chunk_count[k * WAVES + (threadIdx.x >> 6)] = (u32)__popcll(kept);
    }
    __syncthreads();
    const u32 start = tile_start[blockIdx.x];
    for (u32 k = 0; k < TILE_ITEMS; k++) {
        if (!keep[k]) continue;
        u32 pos = start + rank[k];
        for (u32 c = 0; c < k * WAVES + (threadIdx.x >> 6); c++) pos += chunk_count[c];
        if (pos < m) {
            keys[pos] = label[k];
            cells[pos] = cell[k];
        }
    }
}

// ---- exclusive scan of `count` words in place: sums[tile], then the scan of the sums by one workgroup, then the tiles
__global__ __launch_bounds__(BLOCK) void k_scan_reduce(const u32* __restrict__ data, u32 count, u32* __restrict__ sums) {
    u32 s = 0;
    for (u32 q = 0; q < SCAN_ITEMS; q++) {
        const u64 i = (u64)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + q;
        if (i < count) s += data[i];
    }
    const u64 total = block_sum(s);
    if (threadIdx.x == 0) sums[blockIdx.x] = (u32)total;
}
// the exclusive prefix of v over the workgroup's threads; *total = the workgroup's sum
__device__ __forceinline__ u32 block_exclusive(u32 v, u32* total) {
    __shared__ u32 wave_total[WAVES];
    u32 incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 up = __shfl_up(incl, d);
        if ((int)(threadIdx.x & 63) >= d) incl += up;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) wave_total[threadIdx.x >> 6] = incl;
    __syncthreads();
    u32 before = 0, all = 0;
    for (u32 w = 0; w < WAVES; w++) {
        if (w < (threadIdx.x >> 6)) before += wave_total[w];
        all += wave_total[w];
    }
    *total = all;
    return before + incl - v;
}
__global__ __launch_bounds__(BLOCK) void k_scan_spine(u32* __restrict__ sums, u32 tiles) {
    u32 carry = 0;
    for (u32 base = 0; base < tiles; base += BLOCK) {   // (workgroup-uniform bounds)
        const u32 i = base + threadIdx.x;
        const u32 v = i < tiles ? sums[i] : 0;
        u32 total;
        const u32 ex = block_exclusive(v, &total);
        if (i < tiles) sums[i] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(BLOCK) void k_scan_apply(u32* __restrict__ data, u32 count, const u32* __restrict__ sums) {
    u32 v[SCAN_ITEMS], s = 0;
    for (u32 q = 0; q < SCAN_ITEMS; q++) {
        const u64 i = (u64)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + q;
        v[q] = i < count ? data[i] : 0;
        s += v[q];
    }
    u32 total;
    u32 run = sums[blockIdx.x] + block_exclusive(s, &total);
    for (u32 q = 0; q < SCAN_ITEMS; q++) {
        const u64 i = (u64)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS + q;
        if (i < count) data[i] = run;
        run += v[q];
    }
}

// ---- one pass of the radix sort over m (key, cell) entries, tiles of SORT_TILE.  hist: [RADIX][tiles]
__global__ __launch_bounds__(BLOCK) void k_sort_hist(const u32* __restrict__ keys, u32 m, u32 pass, u32 tiles, u32* __restrict__ hist) {
    __shared__ u32 h[RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 k = 0; k < TILE_ITEMS; k++) {
        const u64 i = (u64)blockIdx.x * SORT_TILE + k * BLOCK + threadIdx.x;
        if (i < m) atomicAdd(&h[digit_of(keys[i], pass)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}
// start: the scanned histogram - where the tile's first key of each digit goes.  Inside the tile a key goes behind the keys of
// its digit in the chunks before its own (a running sum per digit over the chunk counts) and behind those in lower lanes of
// its own chunk (the ballot match): the order of equal digits is the order of the input
__global__ __launch_bounds__(BLOCK) void k_sort_scatter(const u32* __restrict__ keys, const u32* __restrict__ cells, u32 m, u32 pass,
                                                      u32 tiles, const u32* __restrict__ start, u32* __restrict__ keys_out,
                                                      u32* __restrict__ cells_out) {
    __shared__ u32 chunk_hist[TILE_CHUNKS][RADIX];
    for (u32 c = 0; c < TILE_CHUNKS; c++) chunk_hist[c][threadIdx.x] = 0;
    __syncthreads();
    u32 key[TILE_ITEMS], cell[TILE_ITEMS], rank[TILE_ITEMS];
    for (u32 k = 0; k < TILE_ITEMS; k++) {
        const u64 i = (u64)blockIdx.x * SORT_TILE + k * BLOCK + threadIdx.x;
        const bool valid = i < m;
        key[k] = valid ? keys[i] : 0;
        cell[k] = valid ? cells[i] : 0;
        const u32 digit = digit_of(key[k], pass);
        u64 match = __ballot(valid);
        for (u32 b = 0; b < RADIX_BITS; b++) {
            const bool bit = (digit >> b) & 1;
            const u64 with_bit = __ballot(valid && bit);
            match &= bit ? with_bit : ~with_bit;
        }
        rank[k] = (u32)__popcll(match & lanes_below());
        if (valid && rank[k] == 0) chunk_hist[k * WAVES + (threadIdx.x >> 6)][digit] = (u32)__popcll(match);   // one writer per entry
    }
    __syncthreads();
    u32 run = start[(size_t)threadIdx.x * tiles + blockIdx.x];   // thread d: digit d
    for (u32 c = 0; c < TILE_CHUNKS; c++) {
        const u32 here = chunk_hist[c][threadIdx.x];
        chunk_hist[c][threadIdx.x] = run;
        run += here;
    }
    __syncthreads();
    for (u32 k = 0; k < TILE_ITEMS; k++) {
        const u64 i = (u64)blockIdx.x * SORT_TILE + k * BLOCK + threadIdx.x;
        if (i >= m) continue;
        const u32 pos = chunk_hist[k * WAVES + (threadIdx.x >> 6)][digit_of(key[k], pass)] + rank[k];
        if (pos < m) {
            keys_out[pos] = key[k];
            cells_out[pos] = cell[k];
        }
    }
}

// succ[index of the cell in sigma's numbering] = its successor's cell; stats = {classes, the largest class}
__global__ __launch_bounds__(BLOCK) void k_wiring_successors(const u32* __restrict__ keys, const u32* __restrict__ cells, u32 m,
                                                           const u32* __restrict__ count, u32 lg, u32 num_wires, u32 routed,
                                                           u32* __restrict__ succ, u64* __restrict__ stats) {
    u32 classes = 0, largest = 0;
    const u32 stride = gridDim.x * BLOCK;
    for (u64 at = (u64)blockIdx.x * BLOCK + threadIdx.x; at < m; at += stride) {
        const u32 i = (u32)at, key = keys[i], run = count[key];
        const u32 s = successor_index(i, m, i + 1 < m && keys[i + 1] == key, run);
        const u32 index = index_of_cell(cells[i], lg, num_wires);
        if (index < routed) succ[index] = cells[s];
        if (i == 0 || keys[i - 1] != key) {
            classes++;
            largest = run > largest ? run : largest;
        }
    }
    const u64 total = block_sum(classes);
    __shared__ u32 wave_largest[WAVES];
    for (int d = 32; d; d >>= 1) {
        const u32 other = __shfl_xor(largest, d);
        largest = other > largest ? other : largest;
    }
    if ((threadIdx.x & 63) == 0) wave_largest[threadIdx.x >> 6] = largest;
    __syncthreads();
    if (threadIdx.x == 0 && total) {
        for (u32 w = 1; w < WAVES; w++) largest = wave_largest[w] > largest ? wave_largest[w] : largest;
        atomicAdd(&stats[0], total);
        atomicMax(&stats[1], (u64)largest);
    }
}

template <class F>
__global__ __launch_bounds__(BLOCK) void k_wiring_sigmas(const typename F::T* __restrict__ lo, const typename F::T* __restrict__ hi,
                                                       const typename F::T* __restrict__ k_is, const u32* __restrict__ succ, u32 routed,
                                                       u32 lg, u32 num_wires, typename F::T* __restrict__ out) {
    const u32 stride = gridDim.x * BLOCK;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < routed; i += stride) {
        const u32 s = succ[i];
        out[i] = sigma_value<F>(lo, hi, k_is, s == NONE ? cell_of_index((u32)i, lg, num_wires) : s, num_wires);
    }
}

__global__ __launch_bounds__(BLOCK) void k_wiring_widen(const u32* __restrict__ parent, u32 num_targets, u64* __restrict__ out) {
    const u32 stride = gridDim.x * BLOCK;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < num_targets; t += stride) out[t] = parent[t];
}
__global__ __launch_bounds__(BLOCK) void k_wiring_merged(const u32* __restrict__ parent, u32 num_targets, u64* __restrict__ merged) {
    u32 mine = 0;
    const u32 stride = gridDim.x * BLOCK;
    for (u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x; t < num_targets; t += stride) mine += parent[t] != (u32)t;
    const u64 total = block_sum(mine);
    if (threadIdx.x == 0 && total) atomicAdd(merged, total);
}

// ---------------------------------------------------------------- launchers (kernels.hpp)
void wiring_init(u32* parent, u32 num_targets, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_init, stride_blocks(num_targets), dim3(BLOCK), 0, st, parent, num_targets);
}
void wiring_union(const u64* pairs, u32 count, u64 first, u32* parent, u64 num_targets, u64 cells, u32 num_wires, u32 num_routed, u64* err,
                  hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_union, stride_blocks(count), dim3(BLOCK), 0, st, pairs, count, first, parent, num_targets, cells, num_wires,
                       num_routed, err);
}
void wiring_jump(u32* parent, u32 num_targets, u32* changed, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_jump, blocks_for(num_targets), dim3(BLOCK), 0, st, parent, num_targets, changed);
}
void wiring_count(const u32* parent, u32 routed, u32 num_routed, u32 num_wires, u32* count, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_count, stride_blocks(routed), dim3(BLOCK), 0, st, parent, routed, num_routed, num_wires, count);
}
u32 wiring_scan_tiles(u32 count) { return tiles_of(count, SCAN_TILE); }
void wiring_scan(u32* data, u32 count, u32* sums, hipStream_t st) {
    const u32 tiles = tiles_of(count, SCAN_TILE);
    hipLaunchKernelGGL(k_scan_reduce, dim3(tiles), dim3(BLOCK), 0, st, data, count, sums);
    hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(BLOCK), 0, st, sums, tiles);
    hipLaunchKernelGGL(k_scan_apply, dim3(tiles), dim3(BLOCK), 0, st, data, count, sums);
}
u32 wiring_sort_tiles(u32 count) { return tiles_of(count, SORT_TILE); }
void wiring_keep_count(const u32* parent, const u32* count, u32 routed, u32 num_routed, u32 num_wires, u32* tile_count, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_keep_count, dim3(tiles_of(routed, SORT_TILE)), dim3(BLOCK), 0, st, parent, count, routed, num_routed,
                       num_wires, tile_count);
}
void wiring_compact(const u32* parent, const u32* count, u32 routed, u32 num_routed, u32 num_wires, const u32* tile_start, u32 m, u32* keys,
                    u32* cells, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_compact, dim3(tiles_of(routed, SORT_TILE)), dim3(BLOCK), 0, st, parent, count, routed, num_routed, num_wires,
                       tile_start, m, keys, cells);
}
void wiring_sort_pass(const u32* keys, const u32* cells, u32 m, u32 pass, u32* hist, u32* sums, u32* keys_out, u32* cells_out,
                      hipStream_t st) {
    const u32 tiles = tiles_of(m, SORT_TILE);
    hipLaunchKernelGGL(k_sort_hist, dim3(tiles), dim3(BLOCK), 0, st, keys, m, pass, tiles, hist);
    wiring_scan(hist, RADIX * tiles, sums, st);
    hipLaunchKernelGGL(k_sort_scatter, dim3(tiles), dim3(BLOCK), 0, st, keys, cells, m, pass, tiles, hist, keys_out, cells_out);
}
void wiring_successors(const u32* keys, const u32* cells, u32 m, const u32* count, u32 lg, u32 num_wires, u32 routed, u32* succ, u64* stats,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_successors, stride_blocks(m), dim3(BLOCK), 0, st, keys, cells, m, count, lg, num_wires, routed, succ, stats);
}
template <class F>
void wiring_sigmas(const typename F::T* lo, const typename F::T* hi, const typename F::T* k_is, const u32* succ, u32 routed, u32 lg,
                   u32 num_wires, typename F::T* out, hipStream_t st) {
    hipLaunchKernelGGL((k_wiring_sigmas<F>), stride_blocks(routed), dim3(BLOCK), 0, st, lo, hi, k_is, succ, routed, lg, num_wires, out);
}
void wiring_widen(const u32* parent, u32 num_targets, u64* out, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_widen, stride_blocks(num_targets), dim3(BLOCK), 0, st, parent, num_targets, out);
}
void wiring_merged(const u32* parent, u32 num_targets, u64* merged, hipStream_t st) {
    hipLaunchKernelGGL(k_wiring_merged, stride_blocks(num_targets), dim3(BLOCK), 0, st, parent, num_targets, merged);
}

template void wiring_sigmas<GlF>(const u64*, const u64*, const u64*, const u32*, u32, u32, u32, u64*, hipStream_t);
template void wiring_sigmas<BbF>(const u32*, const u32*, const u32*, const u32*, u32, u32, u32, u32*, hipStream_t);

}  // namespace gbk

// gb_circuit_decode_sigmas: the copy permutation read back out of the sigma columns, and its cycles as copy classes.
// The per-value arithmetic is sigma_decode.hpp's (GB_HD, shared with the host).
//   decode    k_sigma_decode: one thread per routed cell i = col * n + row (sigma's own numbering, the order the values lie in:
//             coalesced along rows), grid-stride; the discrete-log and coset tables in LDS while they fit, read from global
//             memory above that.  Writes {target, label = the cell's number row * num_wires + col} and sets the target's bit in
//             `seen`: a bit that was set already is a target hit twice.  A value that names no cell leaves its cell in words[0].
//   refusal   k_sigma_hits / k_sigma_shared, only after a double hit: a hit count per target, then the lowest cell whose target
//             is shared
//   classes   k_sigma_walk: every cell walks its cycle for up to 8 steps - the cycles that close (in a circuit, nearly all of
//             them) are labelled there and then, and their cells take no further part.  k_sigma_round, for the longer cycles:
//             pointer doubling, label'[i] = min(label[i], label[next[i]]), next'[i] = next[next[i]]; {next, label}
//             is one 8-byte word, so a round is a streaming pass with one dependent gather; double buffers, no atomics; a wave
//             that changed a label sets the round's flag
//   results   class statistics: a closed cycle's first cell counts it in the walk; for the rest k_sigma_sizes / k_sigma_stats
//             (every cell but the class's first adds one to the first's counter),
//             k_sigma_labels (the labels of all wire cells in cell order), k_sigma_compare (against a partition's first cells)
#include "kernels.hpp"
#include "sigma_decode.hpp"

namespace gbk {

namespace {
constexpr u32 SIGMA_BLOCK = 256, DECODE_MAX_BLOCKS = 2048, STRIDE_MAX_BLOCKS = 4096;

static inline dim3 sigma_blocks(u64 count) { return dim3((u32)((count + SIGMA_BLOCK - 1) / SIGMA_BLOCK)); }

// sigma's numbering col * n + row <-> the cell number row * num_wires + col
__device__ __forceinline__ u32 cell_of(u32 i, u32 lg, u32 num_wires) { return (i & ((1u << lg) - 1)) * num_wires + (i >> lg); }
__device__ __forceinline__ u32 index_of(u32 cell, u32 lg, u32 num_wires) { return ((cell % num_wires) << lg) + cell / num_wires; }

// What a thread has seen of the classes of two cells or more: a thread adds the classes whose first cell it holds, and the
// workgroup adds its sum to stats = {classes, their cells, the largest} - registers over a grid-stride loop, then the wave's
// lanes, the workgroup's waves through LDS, and at most three global atomics per workgroup.
struct ClassStats {
    u32 classes = 0, largest = 0;
    u64 cells = 0;
    __device__ __forceinline__ void add(u32 size) {
        classes++;
        cells += size;
        largest = size > largest ? size : largest;
    }
};
__device__ __forceinline__ void add_class_stats(ClassStats a, u64* __restrict__ stats) {
    __shared__ u32 wave_classes[SIGMA_BLOCK / 64], wave_largest[SIGMA_BLOCK / 64];
    __shared__ u64 wave_cells[SIGMA_BLOCK / 64];
    for (int d = 32; d; d >>= 1) {
        a.classes += __shfl_xor(a.classes, d);
        a.cells += __shfl_xor(a.cells, d);
        const u32 other = __shfl_xor(a.largest, d);
        a.largest = other > a.largest ? other : a.largest;
    }
    if ((threadIdx.x & 63) == 0) {
        wave_classes[threadIdx.x >> 6] = a.classes;
        wave_cells[threadIdx.x >> 6] = a.cells;
        wave_largest[threadIdx.x >> 6] = a.largest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ClassStats t;
        for (u32 w = 0; w < SIGMA_BLOCK / 64; w++) {
            t.classes += wave_classes[w];
            t.cells += wave_cells[w];
            t.largest = wave_largest[w] > t.largest ? wave_largest[w] : t.largest;
        }
        if (t.classes) {
            atomicAdd(&stats[0], (u64)t.classes);
            atomicAdd(&stats[1], t.cells);
            atomicMax(&stats[2], (u64)t.largest);
        }
    }
}
}  // namespace

template <class F, bool IN_LDS>
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_decode(SigmaDecodeParams<F> p, const typename F::T* __restrict__ sigma, u32 count,
                                                             uint2* __restrict__ state, u32* __restrict__ seen, u32* __restrict__ words) {
    typedef typename F::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_sigma[];
    sigma::DlogTables<F> t = p.t;
    const T *k_pow_n = p.k_pow_n, *k_inv = p.k_inv;
    if (IN_LDS) {   // [sorted | inv_lo | k_pow_n | k_inv | exps]
        const u32 m = 1u << p.t.a, nr = p.num_routed;
        T* s_sorted = reinterpret_cast<T*>(smem_sigma);
        T* s_inv_lo = s_sorted + m;
        T* s_k_pow_n = s_inv_lo + m;
        T* s_k_inv = s_k_pow_n + nr;
        uint16_t* s_exps = reinterpret_cast<uint16_t*>(s_k_inv + nr);
        for (u32 j = threadIdx.x; j < m; j += SIGMA_BLOCK) {
            s_sorted[j] = p.t.sorted[j];
            s_inv_lo[j] = p.t.inv_lo[j];
            s_exps[j] = p.t.exps[j];
        }
        for (u32 j = threadIdx.x; j < nr; j += SIGMA_BLOCK) {
            s_k_pow_n[j] = p.k_pow_n[j];
            s_k_inv[j] = p.k_inv[j];
        }
        __syncthreads();
        t.sorted = s_sorted;
        t.inv_lo = s_inv_lo;
        t.exps = s_exps;
        k_pow_n = s_k_pow_n;
        k_inv = s_k_inv;
    }
    const u32 lg = p.t.lg, stride = gridDim.x * SIGMA_BLOCK;
    for (u64 at = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x; at < count; at += stride) {
        const u32 i = (u32)at, cell = cell_of(i, lg, p.num_wires);
        u32 col, row, target = sigma::NO_CELL;
        if (sigma::decode_value<F>(t, k_pow_n, k_inv, p.num_routed, sigma[i], &col, &row)) {
            target = (col << lg) + row;   // (col < num_routed: below count)
            const u32 bit = 1u << (target & 31);
            if (atomicOr(&seen[target >> 5], bit) & bit) words[SIGMA_WORD_DOUBLE_HIT] = 1;
        } else {
            atomicMin(&words[SIGMA_WORD_NO_CELL], cell);
        }
        state[i] = make_uint2(target, cell);
    }
}

// hits[target]++ (the targets are valid: no cell was refused)
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_hits(const uint2* __restrict__ state, u32 count, u32* __restrict__ hits) {
    const u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    if (i < count && state[i].x < count) atomicAdd(&hits[state[i].x], 1u);
}
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_shared(const uint2* __restrict__ state, u32 count, const u32* __restrict__ hits,
                                                             u32* __restrict__ words) {
    const u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    if (i < count && state[i].x < count && hits[state[i].x] > 1) atomicMin(&words[SIGMA_WORD_SHARED], state[i].y);
}

// Short cycles close here: a cell walks its cycle for up to SIGMA_WALK steps; back at itself it knows its label for good and
// leaves {SIGMA_CLOSED, label}, and the cycle's first cell adds the cycle to the statistics.  `in` is only read (other cells
// walk through this one), the result goes to `out`.  Grid-stride.
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_walk(const uint2* __restrict__ in, uint2* __restrict__ out, u32 count,
                                                           u64* __restrict__ stats) {
    ClassStats seen;
    const u32 stride = gridDim.x * SIGMA_BLOCK;
    for (u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x; i < count; i += stride) {
        const uint2 me = in[i];
        u32 at = me.x, label = me.y, cells = 1;
        for (u32 step = 0; step < SIGMA_WALK && at != (u32)i && at < count; step++) {
            const uint2 there = in[at];
            label = there.y < label ? there.y : label;
            at = there.x;
            cells++;
        }
        const bool closed = at == (u32)i;
        out[i] = closed ? make_uint2(SIGMA_CLOSED, label) : me;
        if (closed && cells >= 2 && label == me.y) seen.add(cells);
    }
    add_class_stats(seen, stats);
}

// a closed cell keeps what it has (copy_closed: into a buffer that does not hold it yet); the cells of the longer cycles only
// ever meet each other
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_round(const uint2* __restrict__ in, uint2* __restrict__ out, u32 count,
                                                            bool copy_closed, u32* __restrict__ changed) {
    const u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    bool moved = false;
    if (i < count) {
        const uint2 me = in[i];
        if (me.x == SIGMA_CLOSED) {
            if (copy_closed) out[i] = me;
        } else {
            const uint2 there = me.x < count ? in[me.x] : me;   // (always in range: the decode pass refused everything else)
            moved = there.y < me.y;
            out[i] = make_uint2(there.x, moved ? there.y : me.y);
        }
    }
    if (__ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1;
}

// the cycles the walk left open: sizes[index of the class's first cell] = the class's cells but the first
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_sizes(const uint2* __restrict__ state, u32 count, u32 lg, u32 num_wires,
                                                            u32* __restrict__ sizes) {
    const u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    if (i >= count) return;
    const uint2 me = state[i];
    if (me.x != SIGMA_CLOSED && me.y != cell_of((u32)i, lg, num_wires)) atomicAdd(&sizes[index_of(me.y, lg, num_wires)], 1u);
}
// ... and their first cells add them to the statistics.  Grid-stride.
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_stats(const uint2* __restrict__ state, u32 count, u32 lg, u32 num_wires,
                                                            const u32* __restrict__ sizes, u64* __restrict__ stats) {
    ClassStats seen;
    const u32 stride = gridDim.x * SIGMA_BLOCK;
    for (u64 i = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x; i < count; i += stride) {
        const uint2 me = state[i];
        if (me.x != SIGMA_CLOSED && me.y == cell_of((u32)i, lg, num_wires)) seen.add(sizes[i] + 1);
    }
    add_class_stats(seen, stats);
}

// labels[cell] for every wire cell: a routed cell's label, a non-routed cell itself
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_labels(const uint2* __restrict__ state, u64 cells, u32 lg, u32 num_wires,
                                                             u32 num_routed, u32* __restrict__ labels) {
    const u64 cell = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    if (cell >= cells) return;
    const u32 col = (u32)(cell % num_wires);
    labels[cell] = col < num_routed ? state[index_of((u32)cell, lg, num_wires)].y : (u32)cell;
}

// the lowest routed cell whose partition class starts elsewhere than its decoded class
__global__ __launch_bounds__(SIGMA_BLOCK) void k_sigma_compare(const u32* __restrict__ labels, const u32* __restrict__ slots,
                                                              const u32* __restrict__ first, u32 num_slots, u64 cells, u32 num_wires,
                                                              u32 num_routed, u32* __restrict__ lowest) {
    const u64 cell = (u64)blockIdx.x * SIGMA_BLOCK + threadIdx.x;
    if (cell >= cells || (u32)(cell % num_wires) >= num_routed) return;
    const u32 slot = slots[cell];
    const u32 fc = slot < num_slots ? first[slot] : (u32)cell;
    if (fc != labels[cell]) atomicMin(lowest, (u32)cell);
}

// ---------------------------------------------------------------- launchers (kernels.hpp)
template <class F>
size_t sigma_decode_lds_bytes(u32 lg, u32 num_routed) {
    return sigma::dlog_table_bytes<F>(lg) + 2 * (size_t)num_routed * sizeof(typename F::T);
}
template <class F>
void sigma_decode(const SigmaDecodeParams<F>& p, const typename F::T* sigma, u32 count, uint2* state, u32* seen, u32* words,
                  hipStream_t st) {
    const dim3 grid(std::min<u32>(sigma_blocks(count).x, DECODE_MAX_BLOCKS));
    const size_t lds = sigma_decode_lds_bytes<F>(p.t.lg, p.num_routed);
    if (lds <= SIGMA_LDS_MAX_BYTES)
        hipLaunchKernelGGL((k_sigma_decode<F, true>), grid, dim3(SIGMA_BLOCK), lds, st, p, sigma, count, state, seen, words);
    else
        hipLaunchKernelGGL((k_sigma_decode<F, false>), grid, dim3(SIGMA_BLOCK), 0, st, p, sigma, count, state, seen, words);
}
void sigma_shared_target(const uint2* state, u32 count, u32* hits, u32* words, hipStream_t st) {
    (void)hipMemsetAsync(hits, 0, (size_t)count * sizeof(u32), st);
    hipLaunchKernelGGL(k_sigma_hits, sigma_blocks(count), dim3(SIGMA_BLOCK), 0, st, state, count, hits);
    hipLaunchKernelGGL(k_sigma_shared, sigma_blocks(count), dim3(SIGMA_BLOCK), 0, st, state, count, hits, words);
}
static inline dim3 stride_blocks(u64 count) { return dim3(std::min<u32>(sigma_blocks(count).x, STRIDE_MAX_BLOCKS)); }
void sigma_walk(const uint2* in, uint2* out, u32 count, u64* stats, hipStream_t st) {
    (void)hipMemsetAsync(stats, 0, 3 * sizeof(u64), st);
    hipLaunchKernelGGL(k_sigma_walk, stride_blocks(count), dim3(SIGMA_BLOCK), 0, st, in, out, count, stats);
}
void sigma_round(const uint2* in, uint2* out, u32 count, bool copy_closed, u32* changed, hipStream_t st) {
    hipLaunchKernelGGL(k_sigma_round, sigma_blocks(count), dim3(SIGMA_BLOCK), 0, st, in, out, count, copy_closed, changed);
}
void sigma_class_stats(const uint2* state, u32 count, u32 lg, u32 num_wires, u32* sizes, u64* stats, hipStream_t st) {
    (void)hipMemsetAsync(sizes, 0, (size_t)count * sizeof(u32), st);
    hipLaunchKernelGGL(k_sigma_sizes, sigma_blocks(count), dim3(SIGMA_BLOCK), 0, st, state, count, lg, num_wires, sizes);
    hipLaunchKernelGGL(k_sigma_stats, stride_blocks(count), dim3(SIGMA_BLOCK), 0, st, state, count, lg, num_wires, sizes, stats);
}
void sigma_labels(const uint2* state, u64 cells, u32 lg, u32 num_wires, u32 num_routed, u32* labels, hipStream_t st) {
    hipLaunchKernelGGL(k_sigma_labels, sigma_blocks(cells), dim3(SIGMA_BLOCK), 0, st, state, cells, lg, num_wires, num_routed, labels);
}
void sigma_compare(const u32* labels, const u32* slots, const u32* first, u32 num_slots, u64 cells, u32 num_wires, u32 num_routed,
                   u32* lowest, hipStream_t st) {
    hipLaunchKernelGGL(k_sigma_compare, sigma_blocks(cells), dim3(SIGMA_BLOCK), 0, st, labels, slots, first, num_slots, cells, num_wires,
                       num_routed, lowest);
}

template void sigma_decode<GlF>(const SigmaDecodeParams<GlF>&, const u64*, u32, uint2*, u32*, u32*, hipStream_t);
template void sigma_decode<BbF>(const SigmaDecodeParams<BbF>&, const u32*, u32, uint2*, u32*, u32*, hipStream_t);

}  // namespace gbk

// The witness check (gb_check_witness): the gate constraints evaluated on H itself, where a satisfied witness makes them vanish,
// and the copy constraints read off the partition's slot map - or off the labels gb_circuit_decode_sigmas left (kernels_sigma.hip).  kernels_gates.hip evaluates every gate at every point of the LDE
// coset g H and folds with alpha; here a row runs the ONE gate its selector names, unfolded, and reports the first constraint that
// is not zero.  The row logic is witness_check.hpp's (GB_HD, shared with the host).
//   preparation (per circuit)  k_check_count -> k_check_scan -> k_check_fill: a list of rows per gate, ascending, and one of the
//                              rows with a selector violation - so that a launch runs one gate kind and no wave mixes gates
//   the check                  one launch per gate that has rows, one thread per list entry: k_check_gates<LIGHT_GATES>,
//                              k_check_gates<HEAVY_GATES> (the in-circuit hash gate), k_check_programs (the interpreter, registers
//                              in LDS as in k_gate_programs).  Per entry the first failing constraint and its value; per launch a
//                              count of failing entries, one atomic per wave that has any.
//   copies                     k_first_cell once per partition (atomicMin over the slot map), k_check_copies per check
// The witness is [num_wires][n] CANONICAL words (what gb_expand_partition writes); a wire is encoded where it is read.
#include "gates.hpp"
#include "kernels.hpp"
#include "witness_check.hpp"

namespace gbk {

namespace {
constexpr u32 CHECK_BLOCK = 256, FILL_BLOCK = 1024;

template <class F>
__device__ __forceinline__ u64 selector_value(const typename F::T* __restrict__ hv, size_t n, u32 col, u32 row) {
    return F::dec(hv[(size_t)col * n + row]);
}
}  // namespace

// counts[l] += rows of this workgroup on list l (LDS first: one global atomic per list and workgroup)
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_count(gates::GateSet gs, const typename F::T* __restrict__ hv, u32 n, u32* __restrict__ counts) {
    __shared__ u32 local[check::MAX_LISTS];
    const u32 nl = gs.num_gates + 1;
    if (threadIdx.x < check::MAX_LISTS) local[threadIdx.x] = 0;
    __syncthreads();
    const u32 r = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    if (r < n) {
        bool bad = false;
        for (u32 col = 0; col < gs.num_selectors; col++) {
            const u32 g = check::active_gate<F>(gs, col, selector_value<F>(hv, n, col, r));
            if (g == check::BAD_SELECTOR) bad = true;
            else if (g != check::NO_GATE) atomicAdd(&local[g], 1u);
        }
        if (bad) atomicAdd(&local[gs.num_gates], 1u);
    }
    __syncthreads();
    if (threadIdx.x < nl && local[threadIdx.x]) atomicAdd(&counts[threadIdx.x], local[threadIdx.x]);
}

// offsets[l] = counts[0] + .. + counts[l - 1], l <= nl (at most 25 counts: one wave, each lane its own prefix)
__global__ __launch_bounds__(64) void k_check_scan(const u32* __restrict__ counts, u32 nl, u32* __restrict__ offsets) {
    const u32 l = threadIdx.x;
    if (l > nl) return;
    u32 sum = 0;
    for (u32 i = 0; i < l; i++) sum += counts[i];
    offsets[l] = sum;
}

// workgroup l writes list l: it walks the rows in order, FILL_BLOCK at a time, and appends those on its list behind a running
// base - ballot ranks inside a wave, the waves' totals through LDS - so that every list is in ascending row order
template <class F>
__global__ __launch_bounds__(FILL_BLOCK) void k_check_fill(gates::GateSet gs, const typename F::T* __restrict__ hv, u32 n,
                                                           const u32* __restrict__ offsets, u32* __restrict__ rows) {
    __shared__ u32 wave_total[FILL_BLOCK / 64];
    const u32 l = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 base = offsets[l];
    const u32 end = offsets[l + 1];
    for (u32 r0 = 0; r0 < n; r0 += FILL_BLOCK) {
        const u32 r = r0 + threadIdx.x;
        const bool in = r < n && check::row_on_list<F>(gs, l, [&](u32 col) { return selector_value<F>(hv, n, col, r); });
        const u64 m = __ballot(in);
        if (lane == 0) wave_total[wave] = (u32)__popcll(m);
        __syncthreads();
        u32 before = 0, total = 0;
        for (u32 w = 0; w < FILL_BLOCK / 64; w++) {
            before += w < wave ? wave_total[w] : 0;
            total += wave_total[w];
        }
        const u32 at = base + before + (u32)__popcll(m & (((u64)1 << lane) - 1));
        if (in && at < end) rows[at] = r;   // (at < end always holds: the count pass used the same test)
        base += total;
        __syncthreads();
    }
}

// out[i][col] = the canonical selector value of column col on row rows[i]
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_selectors(const typename F::T* __restrict__ hv, u32 n, u32 num_selectors,
                                                                const u32* __restrict__ rows, u32 count, u64* __restrict__ out) {
    const u32 i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    if (i >= count) return;
    for (u32 col = 0; col < num_selectors; col++) out[(size_t)i * num_selectors + col] = selector_value<F>(hv, n, col, rows[i]);
}

// the tail of a gate launch: entry i's result, and the launch's count of failing entries from the waves' ballots
template <class F>
__device__ __forceinline__ void store_result(bool live, u32 i, const check::FirstFail<F>& ff, u32* __restrict__ fail_index,
                                             u64* __restrict__ fail_value, u32* __restrict__ num_failed) {
    if (live) {
        fail_index[i] = ff.index;
        fail_value[i] = F::dec(ff.value);
    }
    const u64 m = __ballot(live && ff.failed());
    if (m && (threadIdx.x & 63) == 0) atomicAdd(num_failed, (u32)__popcll(m));
}

// one built-in gate `g` on the rows of its list.  SUBSET as in kernels_gates.hip: the in-circuit hash gates are compiled apart.
template <class F, int SUBSET>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_gates(CheckParams<F> p, u32 g, const u32* __restrict__ rows, u32 count,
                                                             const typename F::T* __restrict__ hv, const typename F::T* __restrict__ wit,
                                                             const typename F::T* __restrict__ pi_hash, u32* __restrict__ fail_index,
                                                             u64* __restrict__ fail_value, u32* __restrict__ num_failed) {
    typedef typename F::T T;
    const u32 i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    const bool live = i < count;
    const size_t n = p.n;
    const u32 row = live ? rows[i] : 0;
    check::FirstFail<F> ff;
    if (live) {
        auto wire = [&](u32 col) -> T { return F::enc(wit[(size_t)col * n + row]); };
        auto konst = [&](u32 k) -> T { return hv[(size_t)(p.gs.num_selectors + k) * n + row]; };
        gates::eval_gate<F, gates::BaseAlg<F>, SUBSET>(p.gs, p.gs.g[g], wire, konst, pi_hash, ff);
    }
    store_result<F>(live, i, ff, fail_index, fail_value, num_failed);
}

// a program gate on the rows of its list: gates::run_program with the register file in LDS ([max_regs][blockDim], as k_gate_programs)
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_programs(CheckParams<F> p, ProgramParams<F> pp, u32 g, const u32* __restrict__ rows,
                                                                u32 count, const typename F::T* __restrict__ hv,
                                                                const typename F::T* __restrict__ wit, u32* __restrict__ fail_index,
                                                                u64* __restrict__ fail_value, u32* __restrict__ num_failed) {
    typedef typename F::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_check[];
    const gates::LdsRegs<T> regs{reinterpret_cast<T*>(smem_check) + threadIdx.x, CHECK_BLOCK};
    const u32 i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    const bool live = i < count;   // (no barrier below: a lane only ever touches its own LDS words)
    const size_t n = p.n;
    const u32 row = live ? rows[i] : 0;
    check::FirstFail<F> ff;
    if (live) {
        const gates::ProgramInfo& pi = pp.ps.p[p.gs.g[g].param];
        auto wire = [&](u32 col) -> T { return F::enc(wit[(size_t)col * n + row]); };
        auto konst = [&](u32 k) -> T { return hv[(size_t)(p.gs.num_selectors + k) * n + row]; };
        gates::run_program<F, gates::BaseAlg<F>>(pp.instrs + pi.instr_off, pi.num_instrs, pp.lits + pi.lit_off, regs, wire, konst, ff);
    }
    store_result<F>(live, i, ff, fail_index, fail_value, num_failed);
}

// first[slot] = the lowest cell (row * num_wires + column) of the slot's class; first[] starts as all ones
__global__ __launch_bounds__(CHECK_BLOCK) void k_first_cell(const u32* __restrict__ slots, u64 cells, u32 num_slots, u32* __restrict__ first) {
    const u64 cell = (u64)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    if (cell >= cells) return;
    const u32 slot = slots[cell];
    if (slot < num_slots) atomicMin(&first[slot], (u32)cell);
}

// one thread per cell, in cell order: does it hold what the first cell of its class holds (first = null: the slot is that cell -
// the labels decoded from sigma)?  A wave writes its ballot as one word
// of `mask` (bit order = cell order, so the host reads the violations off in ascending order) and adds its count.
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_copies(const u32* __restrict__ slots, const u32* __restrict__ first, u32 num_slots,
                                                              const typename F::T* __restrict__ wit, u32 n, u32 num_wires, u64 cells,
                                                              u64* __restrict__ mask, u32* __restrict__ num_failed) {
    const u64 cell = (u64)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    bool bad = false;
    if (cell < cells) {
        const u32 slot = slots[cell];
        const u32 fc = slot < num_slots ? (first ? first[slot] : slot) : (u32)cell;
        if (fc != (u32)cell && fc < cells)
            bad = wit[(size_t)(cell % num_wires) * n + cell / num_wires] != wit[(size_t)(fc % num_wires) * n + fc / num_wires];
    }
    const u64 m = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        if (cell < cells) mask[cell >> 6] = m;   // (a workgroup starts on a multiple of 64: the wave's first cell names its word)
        if (m) atomicAdd(num_failed, (u32)__popcll(m));
    }
}

// the listed copy violations' other halves: out[i] = {the cell's value, the class's first cell, that cell's value}, canonical
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_copy_report(const u32* __restrict__ slots, const u32* __restrict__ first, u32 num_slots,
                                                             const typename F::T* __restrict__ wit, u32 n, u32 num_wires,
                                                             const u32* __restrict__ cells, u32 count, u64* __restrict__ out) {
    const u32 i = blockIdx.x * CHECK_BLOCK + threadIdx.x;
    if (i >= count) return;
    const u32 cell = cells[i], slot = slots[cell];
    const u32 fc = slot < num_slots ? (first ? first[slot] : slot) : cell;
    out[3 * (size_t)i] = wit[(size_t)(cell % num_wires) * n + cell / num_wires];
    out[3 * (size_t)i + 1] = fc;
    out[3 * (size_t)i + 2] = wit[(size_t)(fc % num_wires) * n + fc / num_wires];
}

// *flag = 1 if a word is not below p
template <class F>
__global__ __launch_bounds__(CHECK_BLOCK) void k_check_canonical(const typename F::T* __restrict__ v, size_t count, u32* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * CHECK_BLOCK + threadIdx.x;
    const bool bad = i < count && (u64)v[i] >= F::ORDER;
    const u64 m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---------------------------------------------------------------- launchers (kernels.hpp)
static inline dim3 blocks_for(u64 count) { return dim3((u32)((count + CHECK_BLOCK - 1) / CHECK_BLOCK)); }

template <class F>
void check_count_rows(const gates::GateSet& gs, const typename F::T* hv, u32 n, u32* counts, u32* offsets, hipStream_t st) {
    const u32 nl = gs.num_gates + 1;
    (void)hipMemsetAsync(counts, 0, check::MAX_LISTS * sizeof(u32), st);
    hipLaunchKernelGGL((k_check_count<F>), blocks_for(n), dim3(CHECK_BLOCK), 0, st, gs, hv, n, counts);
    hipLaunchKernelGGL(k_check_scan, dim3(1), dim3(64), 0, st, counts, nl, offsets);
}
template <class F>
void check_fill_rows(const gates::GateSet& gs, const typename F::T* hv, u32 n, const u32* offsets, u32* rows, hipStream_t st) {
    hipLaunchKernelGGL((k_check_fill<F>), dim3(gs.num_gates + 1), dim3(FILL_BLOCK), 0, st, gs, hv, n, offsets, rows);
}
template <class F>
void check_selector_values(const typename F::T* hv, u32 n, u32 num_selectors, const u32* rows, u32 count, u64* out, hipStream_t st) {
    if (count) hipLaunchKernelGGL((k_check_selectors<F>), blocks_for(count), dim3(CHECK_BLOCK), 0, st, hv, n, num_selectors, rows, count, out);
}
template <class F>
void check_gate_rows(const CheckParams<F>& p, u32 g, const ProgramParams<F>* programs, const u32* rows, u32 count, const typename F::T* hv,
                     const typename F::T* wit, const typename F::T* pi_hash, u32* fail_index, u64* fail_value, u32* num_failed, hipStream_t st) {
    if (!count) return;
    const gb_gate& gd = p.gs.g[g];
    if (gates::is_program(gd)) {
        const size_t smem = (size_t)(programs->ps.max_regs ? programs->ps.max_regs : 1u) * CHECK_BLOCK * sizeof(typename F::T);
        hipLaunchKernelGGL((k_check_programs<F>), blocks_for(count), dim3(CHECK_BLOCK), smem, st, p, *programs, g, rows, count, hv, wit,
                           fail_index, fail_value, num_failed);
    } else if (gates::is_heavy(gd)) {
        hipLaunchKernelGGL((k_check_gates<F, gates::HEAVY_GATES>), blocks_for(count), dim3(CHECK_BLOCK), 0, st, p, g, rows, count, hv, wit,
                           pi_hash, fail_index, fail_value, num_failed);
    } else {
        hipLaunchKernelGGL((k_check_gates<F, gates::LIGHT_GATES>), blocks_for(count), dim3(CHECK_BLOCK), 0, st, p, g, rows, count, hv, wit,
                           pi_hash, fail_index, fail_value, num_failed);
    }
}
void check_first_cells(const u32* slots, u64 cells, u32 num_slots, u32* first, hipStream_t st) {
    (void)hipMemsetAsync(first, 0xFF, (size_t)(num_slots ? num_slots : 1) * sizeof(u32), st);
    hipLaunchKernelGGL(k_first_cell, blocks_for(cells), dim3(CHECK_BLOCK), 0, st, slots, cells, num_slots, first);
}
template <class F>
void check_copies(const u32* slots, const u32* first, u32 num_slots, const typename F::T* wit, u32 n, u32 num_wires, u64* mask,
                  u32* num_failed, hipStream_t st) {
    const u64 cells = (u64)n * num_wires;
    hipLaunchKernelGGL((k_check_copies<F>), blocks_for(cells), dim3(CHECK_BLOCK), 0, st, slots, first, num_slots, wit, n, num_wires, cells,
                       mask, num_failed);
}
template <class F>
void check_copy_report(const u32* slots, const u32* first, u32 num_slots, const typename F::T* wit, u32 n, u32 num_wires, const u32* cells,
                       u32 count, u64* out, hipStream_t st) {
    if (count) hipLaunchKernelGGL((k_copy_report<F>), blocks_for(count), dim3(CHECK_BLOCK), 0, st, slots, first, num_slots, wit, n, num_wires,
                                  cells, count, out);
}
template <class F>
void check_canonical(const typename F::T* v, size_t count, u32* flag, hipStream_t st) {
    hipLaunchKernelGGL((k_check_canonical<F>), blocks_for(count), dim3(CHECK_BLOCK), 0, st, v, count, flag);
}

#define GB_CHECK_INSTANTIATE(FF, TT)                                                                                                   \
    template void check_count_rows<FF>(const gates::GateSet&, const TT*, u32, u32*, u32*, hipStream_t);                                \
    template void check_fill_rows<FF>(const gates::GateSet&, const TT*, u32, const u32*, u32*, hipStream_t);                           \
    template void check_selector_values<FF>(const TT*, u32, u32, const u32*, u32, u64*, hipStream_t);                                  \
    template void check_gate_rows<FF>(const CheckParams<FF>&, u32, const ProgramParams<FF>*, const u32*, u32, const TT*, const TT*,    \
                                      const TT*, u32*, u64*, u32*, hipStream_t);                                                       \
    template void check_copies<FF>(const u32*, const u32*, u32, const TT*, u32, u32, u64*, u32*, hipStream_t);                         \
    template void check_copy_report<FF>(const u32*, const u32*, u32, const TT*, u32, u32, const u32*, u32, u64*, hipStream_t);         \
    template void check_canonical<FF>(const TT*, size_t, u32*, hipStream_t);
GB_CHECK_INSTANTIATE(GlF, u64)
GB_CHECK_INSTANTIATE(BbF, u32)
#undef GB_CHECK_INSTANTIATE

}  // namespace gbk

// gb_wiring_sigmas (include/goldibear_gpu.h): the copy constraints of a circuit turned into its sigma columns and its
// representative map - "generate sigma polynomials" of CircuitBuilder::build (plonk/circuit_builder.rs:1005-1040, 1220-1224;
// plonk/permutation_argument.rs) as a stage of its own on a context.  Included by api.hip after prover_host.inc.  The kernels are
// kernels_wiring.hip's, what a thread does wiring.hpp's.  Everything is pooled and goes back when the call returns.
//   per target          4 bytes (the forest), + 8 with a representative_map_out (the widened copy that goes to the host)
//   per wire cell       4 bytes (routed cells per label)
//   per routed cell     4 bytes (the successor), + one element where sigmas_out is host memory
//   per moved cell      16 bytes (label and cell, twice: the sort's two buffers) + 1 word per digit and 1024 cells
//   per pair            nothing: the pairs pass through one 1 MiB slice

namespace {

static constexpr u32 WIRING_MAX_PASSES = 40;   // a pass divides the depth of every tree by JUMPS + 1 at least: 14 would do for 2^32

static std::string target_name(u64 t, u64 cells, u32 nw) {
    if (t < cells) return "target " + std::to_string(t) + " (row " + std::to_string(t / nw) + ", wire " + std::to_string(t % nw) + ")";
    return "target " + std::to_string(t) + " (virtual target " + std::to_string(t - cells) + ")";
}

template <class F>
gb_status wiring_sigmas(gb_ctx* ctx, u32 lg, u32 nw, u32 nr, const void* k_is_ptr, const uint64_t* pairs, u64 num_copies, u64 num_targets,
                        bool dev_out, void* sigmas_out, uint64_t* map_out, gb_wiring_info* info) {
    typedef typename F::T T;
    namespace W = gbk::wiring;
    if (lg > F::TWO_ADICITY)
        return fail(ctx, GB_ERR_UNSUPPORTED, "gb_wiring_sigmas: degree_bits exceeds the field's two-adicity (32 Goldilocks / 27 BabyBear)");
    const u64 cells = (u64)nw << lg;
    if (num_targets < cells)
        return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: num_targets " + std::to_string(num_targets) + " is below degree * num_wires = " +
                    std::to_string(cells));
    if (num_targets >> 32) return fail(ctx, GB_ERR_UNSUPPORTED, "gb_wiring_sigmas: 2^32 targets or more");
    std::vector<T> k_is(nr);
    for (u32 j = 0; j < nr; j++) {
        const T k = static_cast<const T*>(k_is_ptr)[j];
        if ((u64)k >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: k_is[" + std::to_string(j) + "] is not a canonical element");
        k_is[j] = F::enc(k);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    gb_status s;
    const typename Host<F>::Tables* tabs;
    if ((s = tables_for<F>(ctx, lg, &tabs))) return s;
    const u32 nt = (u32)num_targets, routed = (u32)((u64)nr << lg);

    TmpAlloc tmp(ctx);
    T* k_is_dev;
    if ((s = upload_tmp(ctx, tmp, k_is, &k_is_dev))) return s;
    u32* parent = tmp.get<u32>(nt);
    u64* words = tmp.get<u64>(5);                           // {pair out of range, pair not routable, classes, largest class, merged}
    u32* changed = tmp.get<u32>(WIRING_MAX_PASSES);
    if (!parent || !words || !changed) return fail(ctx, GB_ERR_OOM, "wiring: the forest");
    u64 *err = words, *stats = words + 2;
    HIP_TRY(ctx, hipMemsetAsync(err, 0xFF, 2 * sizeof(u64), st));
    HIP_TRY(ctx, hipMemsetAsync(stats, 0, 3 * sizeof(u64), st));
    HIP_TRY(ctx, hipMemsetAsync(changed, 0, WIRING_MAX_PASSES * sizeof(u32), st));
    {
        Scope sc(ctx, "wiring: classes");
        gbk::wiring_init(parent, nt, st);
    }
    if (num_copies) {   // the pairs in slices of the page-locked arena, each united as it lands
        const size_t slice = XFER_UP_BYTES / 4 / (2 * sizeof(u64));
        u64* slice_dev = tmp.get<u64>(2 * (size_t)std::min<u64>(slice, num_copies));
        if (!slice_dev) return fail(ctx, GB_ERR_OOM, "wiring: pair slice");
        for (u64 i0 = 0; i0 < num_copies; i0 += slice) {
            const size_t count = (size_t)std::min<u64>(slice, num_copies - i0), bytes = count * 2 * sizeof(u64);
            {
                Scope sc(ctx, "wiring: upload");
                if (void* stage = stage_up(ctx, bytes)) {
                    std::memcpy(stage, pairs + 2 * i0, bytes);
                    HIP_TRY(ctx, hipMemcpyAsync(slice_dev, stage, bytes, hipMemcpyHostToDevice, st));
                } else {   // no arena: a pageable copy, which the runtime stages itself
                    HIP_TRY(ctx, hipMemcpyAsync(slice_dev, pairs + 2 * i0, bytes, hipMemcpyHostToDevice, st));
                    HIP_TRY(ctx, hipStreamSynchronize(st));
                }
            }
            Scope sc(ctx, "wiring: classes");
            gbk::wiring_union(slice_dev, (u32)count, i0, parent, num_targets, cells, nw, nr, err, st);
        }
        if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        u64 bad[2];
        if ((s = read_back(ctx, bad, err, sizeof bad))) return s;
        if (bad[0] != ~(u64)0) {
            const u64 a = pairs[2 * bad[0]], b = pairs[2 * bad[0] + 1];
            return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: copy constraint " + std::to_string(bad[0]) + " names target " +
                        std::to_string(a >= num_targets ? a : b) + ", but there are " + std::to_string(num_targets) + " targets");
        }
        if (bad[1] != ~(u64)0) {
            const u64 a = pairs[2 * bad[1]], b = pairs[2 * bad[1] + 1];
            const u64 t = (a < cells && a % nw >= nr) ? a : b;
            return fail(ctx, GB_ERR_INVALID, "Tried to route a wire that isn't routable: copy constraint " + std::to_string(bad[1]) + ", " +
                        target_name(t, cells, nw));
        }
    }
    gb_wiring_info got{};
    got.routed_cells = routed;
    {
        // compression: a pass lets every target jump up to JUMPS ancestors; the pass that moves no pointer ends it, and is counted
        Scope sc(ctx, "wiring: classes");
        for (u32 r = 0;; r++) {
            if (r == WIRING_MAX_PASSES) return fail(ctx, GB_ERR_HIP, "internal: the forest is still moving after every compression pass");
            gbk::wiring_jump(parent, nt, changed + r, st);
            if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
            got.rounds = r + 1;
            u32 flag = 0;
            if ((s = read_back(ctx, &flag, changed + r, sizeof flag))) return s;
            if (!flag) break;
        }
    }
    u32* succ = tmp.get<u32>(routed);
    if (!succ) return fail(ctx, GB_ERR_OOM, "wiring: successors");
    u32 m = 0;
    {
        Scope sc(ctx, "wiring: order");
        const u32 tiles = gbk::wiring_sort_tiles(routed);
        u32* count = tmp.get<u32>((size_t)cells);
        u32* tile_start = tmp.get<u32>((size_t)tiles + 1);   // the kept cells per tile, then their scan; [tiles] = all of them
        u32* sums = tmp.get<u32>(gbk::wiring_scan_tiles(tiles + 1));
        if (!count || !tile_start || !sums) return fail(ctx, GB_ERR_OOM, "wiring: label counts");
        HIP_TRY(ctx, hipMemsetAsync(count, 0, (size_t)cells * sizeof(u32), st));
        HIP_TRY(ctx, hipMemsetAsync(tile_start, 0, ((size_t)tiles + 1) * sizeof(u32), st));
        HIP_TRY(ctx, hipMemsetAsync(succ, 0xFF, (size_t)routed * sizeof(u32), st));
        gbk::wiring_count(parent, routed, nr, nw, count, st);
        gbk::wiring_keep_count(parent, count, routed, nr, nw, tile_start, st);
        gbk::wiring_scan(tile_start, tiles + 1, sums, st);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        if ((s = read_back(ctx, &m, tile_start + tiles, sizeof m))) return s;
        if (m > routed) return fail(ctx, GB_ERR_HIP, "internal: more moved cells than routed cells");
        if (m) {
            const u32 sort_tiles = gbk::wiring_sort_tiles(m), hist_words = W::RADIX * sort_tiles;
            u32* keys[2] = {tmp.get<u32>(m), tmp.get<u32>(m)};
            u32* vals[2] = {tmp.get<u32>(m), tmp.get<u32>(m)};
            u32* hist = tmp.get<u32>(hist_words);
            u32* hist_sums = tmp.get<u32>(gbk::wiring_scan_tiles(hist_words));
            if (!keys[0] || !keys[1] || !vals[0] || !vals[1] || !hist || !hist_sums) return fail(ctx, GB_ERR_OOM, "wiring: sort buffers");
            gbk::wiring_compact(parent, count, routed, nr, nw, tile_start, m, keys[0], vals[0], st);
            u32 cur = 0;
            for (u32 pass = 0; pass < W::digit_passes(cells); pass++, cur ^= 1)   // a label is a cell: the digits above are zero
                gbk::wiring_sort_pass(keys[cur], vals[cur], m, pass, hist, hist_sums, keys[cur ^ 1], vals[cur ^ 1], st);
            gbk::wiring_successors(keys[cur], vals[cur], m, count, lg, nw, routed, succ, stats, st);
            if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        }
    }
    T* sig = dev_out ? static_cast<T*>(sigmas_out) : tmp.get<T>(routed);
    if (!sig) return fail(ctx, GB_ERR_OOM, "wiring: sigma values");
    {
        Scope sc(ctx, "wiring: sigmas");
        gbk::wiring_sigmas<F>(tabs->tw_lo_fwd, tabs->tw_hi_fwd, k_is_dev, succ, routed, lg, nw, sig, st);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        if (!dev_out) HIP_TRY(ctx, hipMemcpyAsync(sigmas_out, sig, (size_t)routed * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    if (map_out) {
        u64* wide = tmp.get<u64>(nt);
        if (!wide) return fail(ctx, GB_ERR_OOM, "wiring: representative map");
        gbk::wiring_widen(parent, nt, wide, st);
        HIP_TRY(ctx, hipMemcpyAsync(map_out, wide, (size_t)nt * sizeof(u64), hipMemcpyDeviceToHost, st));
    }
    gbk::wiring_merged(parent, nt, stats + 2, st);
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    u64 hs[3];
    if ((s = read_back(ctx, hs, stats, sizeof hs))) return s;   // (waits for the stream: the caller's blocks are written)
    got.moved_cells = m;
    got.num_classes = hs[0];
    got.largest_class = hs[1] ? hs[1] : 1;
    got.merged_targets = hs[2];
    if (info) *info = got;
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_wiring_sigmas(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t num_wires, uint32_t num_routed_wires, const void* k_is,
                           const uint64_t* copy_constraints, uint64_t num_copies, uint64_t num_targets, uint32_t flags, void* sigmas_out,
                           uint64_t* representative_map_out, void* info) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!k_is || !sigmas_out || (num_copies && !copy_constraints)) return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: null argument");
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (flags & ~(uint32_t)GB_INPUT_DEVICE) return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: flags other than GB_INPUT_DEVICE");
    if (num_routed_wires == 0 || num_routed_wires > num_wires)
        return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: num_routed_wires must be between 1 and num_wires");
    const bool dev_out = (flags & GB_INPUT_DEVICE) != 0;
    if (dev_out && (reinterpret_cast<uintptr_t>(sigmas_out) & 15))
        return fail(ctx, GB_ERR_INVALID, "gb_wiring_sigmas: a device sigmas_out must be 16-byte aligned");
    gb_wiring_info* out = static_cast<gb_wiring_info*>(info);
    const gb_status s = by_field(field, [&](auto f) {
        return wiring_sigmas<decltype(f)>(ctx, degree_bits, num_wires, num_routed_wires, k_is, copy_constraints, num_copies, num_targets, dev_out,
                                          sigmas_out, representative_map_out, out);
    });
    if (s != GB_OK) (void)hipStreamSynchronize(ctx->stream);   // nothing of a refused call still reads or writes the caller's blocks
    return s;
} GB_CATCH(ctx)

}  // extern "C"

// gb_circuit_decode_sigmas / gb_circuit_copy_classes (include/goldibear_gpu.h): the copy permutation read back out of the sigma
// columns and its cycles as copy classes.  Included at the end of prover_host.inc, after check_host.inc.  The kernels are
// kernels_sigma.hip's, the per-value arithmetic sigma_decode.hpp's.  The sigma values on H are the circuit's own: sigma_vals, which
// gb_circuit_create* keeps for the Z computation - no transform is needed.  Everything but the labels is pooled and goes back when
// the call returns; the labels go to the circuit only once every check has passed.

namespace {

// the discrete-log tables of (context, field, lg): built on the host once, kept on the device until gb_ctx_destroy
template <class F>
gb_status dlog_tables_for(gb_ctx* ctx, u32 lg, gbk::sigma::DlogTables<F>* out) {
    typedef typename F::T T;
    auto& cached = cache<F>(ctx).dlog;
    auto it = cached.find(lg);
    if (it == cached.end()) {
        const gbk::sigma::DlogTablesHost<F> h = gbk::sigma::build_dlog_tables<F>(lg);
        typename TableCache<F>::template Owner<gbk::sigma::DlogTables<F>> o;
        o.t = h.view();
        gb_status s;
        auto failed = [&](gb_status e) {
            for (void* p : o.owned) (void)hipFree(p);
            return e;
        };
        if ((s = upload<T>(ctx, h.sorted, &o.t.sorted, o.owned))) return failed(s);
        if ((s = upload<T>(ctx, h.inv_lo, &o.t.inv_lo, o.owned))) return failed(s);
        if ((s = upload<uint16_t>(ctx, h.exps, &o.t.exps, o.owned))) return failed(s);
        it = cached.emplace(lg, std::move(o)).first;
    }
    *out = it->second.t;
    return GB_OK;
}

static std::string cell_name(u64 cell, u32 nw) { return "row " + std::to_string(cell / nw) + ", wire " + std::to_string(cell % nw); }

// the partition's classes against the labels: for every routed cell the first cell of its slot must be its label
static gb_status sigma_compare_partition(gb_circuit* c, TmpAlloc& tmp, const u32* labels) {
    gb_ctx* ctx = c->ctx;
    const u32 nw = c->cfg.num_wires;
    const u64 cells = (u64)nw << c->cfg.degree_bits;
    gb_status s;
    if ((s = check_first_cells_of_partition(c))) return s;
    Scope sc(ctx, "decode sigmas: compare");
    u32* lowest = tmp.get<u32>(1);
    if (!lowest) return fail(ctx, GB_ERR_OOM, "decode sigmas: compare");
    HIP_TRY(ctx, hipMemsetAsync(lowest, 0xFF, sizeof(u32), ctx->stream));
    const u32 num_slots = (u32)c->part.reps.size();
    gbk::sigma_compare(labels, c->part.slots_dev, c->chk.first_cell, num_slots, cells, nw, c->cfg.num_routed_wires, lowest, ctx->stream);
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    u32 cell = 0;
    if ((s = read_back(ctx, &cell, lowest, sizeof cell))) return s;
    if (cell == 0xFFFFFFFFu) return GB_OK;
    u32 slot = 0, by_partition = cell, by_sigma = 0;
    {
        ReadBack rb(ctx);
        if ((s = rb.add(&slot, c->part.slots_dev + cell, sizeof slot))) return s;
        if ((s = rb.add(&by_sigma, labels + cell, sizeof by_sigma))) return s;
        if ((s = rb.finish())) return s;
    }
    if (slot < num_slots)
        if ((s = read_back(ctx, &by_partition, c->chk.first_cell + slot, sizeof by_partition))) return s;
    return fail(ctx, GB_ERR_INVALID, "partition and sigma disagree at " + cell_name(cell, nw) + " (partition: first cell " +
                std::to_string(by_partition) + ", sigma: first cell " + std::to_string(by_sigma) + ")");
}

template <class F>
gb_status decode_sigmas(Circuit<F>* c, gb_sigma_info* info) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, nw = cfg.num_wires, nr = cfg.num_routed_wires;
    const u64 cells = (u64)nw << lg, routed = (u64)nr << lg;
    if (cells > 0xFFFFFFFFull) return fail(ctx, GB_ERR_UNSUPPORTED, "decode sigmas: more than 2^32 wire cells");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    gb_circuit::Check& k = c->chk;
    gb_status s;
    const bool with_partition = c->part.set && c->part.slots_dev;
    if (k.sigma_labels) {   // decoded already: nothing to do but the comparison with a partition set since
        if (with_partition && !k.sigma_compared) {
            TmpAlloc tmp(ctx);
            if ((s = sigma_compare_partition(c, tmp, k.sigma_labels))) {
                (void)hipStreamSynchronize(st);
                c->drop_sigma_labels();
                return s;
            }
            k.sigma_compared = true;
            k.sigma_info.compared_partition = 1;
        }
        if (info) *info = k.sigma_info;
        return GB_OK;
    }
    const u32 count = (u32)routed;
    std::vector<T> k_pow_n, k_inv;
    if (!gbk::sigma::build_coset_tables<F>(c->k_is_dev_host.data(), nr, lg, &k_pow_n, &k_inv))
        return fail(ctx, GB_ERR_INVALID, "k_is do not name distinct cosets");
    gbk::SigmaDecodeParams<F> p{};
    if ((s = dlog_tables_for<F>(ctx, lg, &p.t))) return s;
    p.num_routed = nr;
    p.num_wires = nw;

    TmpAlloc tmp(ctx);
    T *k_pow_n_dev, *k_inv_dev;
    if ((s = upload_tmp(ctx, tmp, k_pow_n, &k_pow_n_dev))) return s;
    if ((s = upload_tmp(ctx, tmp, k_inv, &k_inv_dev))) return s;
    p.k_pow_n = k_pow_n_dev;
    p.k_inv = k_inv_dev;
    u32 max_rounds = 0;
    while (((u64)1 << max_rounds) < routed) max_rounds++;
    const size_t seen_words = (size_t)((routed + 31) / 32);
    uint2* state[2] = {tmp.get<uint2>(count), tmp.get<uint2>(count)};
    u32* seen = tmp.get<u32>(seen_words);
    u32* words = tmp.get<u32>(gbk::SIGMA_WORDS + max_rounds);   // the decode pass's words, then a "changed" flag per round
    u64* stats = tmp.get<u64>(3);
    if (!state[0] || !state[1] || !seen || !words || !stats) return fail(ctx, GB_ERR_OOM, "decode sigmas: work buffers");
    u32 hw[gbk::SIGMA_WORDS];
    {
        Scope sc(ctx, "decode sigmas: decode");
        HIP_TRY(ctx, hipMemsetAsync(seen, 0, seen_words * sizeof(u32), st));
        HIP_TRY(ctx, hipMemsetAsync(words, 0xFF, 2 * sizeof(u32), st));
        HIP_TRY(ctx, hipMemsetAsync(words + 2, 0, (gbk::SIGMA_WORDS - 2 + max_rounds) * sizeof(u32), st));
        gbk::sigma_decode<F>(p, c->sigma_vals, count, state[0], seen, words, st);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        if ((s = read_back(ctx, hw, words, sizeof hw))) return s;
        if (hw[gbk::SIGMA_WORD_NO_CELL] != 0xFFFFFFFFu) {
            const u32 cell = hw[gbk::SIGMA_WORD_NO_CELL];
            T v;
            if ((s = read_back(ctx, &v, c->sigma_vals + (((size_t)(cell % nw)) << lg) + cell / nw, sizeof v))) return s;
            return fail(ctx, GB_ERR_INVALID, "sigma names no routed cell at " + cell_name(cell, nw) + ": the value " +
                        std::to_string(F::dec(v)) + " is in no coset k_is[j] H, j < " + std::to_string(nr));
        }
        if (hw[gbk::SIGMA_WORD_DOUBLE_HIT]) {   // name the lowest cell whose target is shared: a hit count per target
            gbk::sigma_shared_target(state[0], count, reinterpret_cast<u32*>(state[1]), words, st);
            if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
            if ((s = read_back(ctx, hw, words, sizeof hw))) return s;
            const u32 cell = hw[gbk::SIGMA_WORD_SHARED];
            if (cell == 0xFFFFFFFFu) return fail(ctx, GB_ERR_HIP, "internal: a target was hit twice, but no cell shares its target");
            uint2 st_cell;
            if ((s = read_back(ctx, &st_cell, state[0] + (((size_t)(cell % nw)) << lg) + cell / nw, sizeof st_cell))) return s;
            const u64 target_cell = (u64)(st_cell.x & (((u32)1 << lg) - 1)) * nw + (st_cell.x >> lg);
            return fail(ctx, GB_ERR_INVALID, "sigma is not a permutation: " + cell_name(cell, nw) + " and another cell both go to " +
                        cell_name(target_cell, nw));
        }
    }
    gb_sigma_info got{};
    got.routed_cells = routed;
    u32 cur = 0;
    {
        Scope sc(ctx, "decode sigmas: classes");
        // the short cycles by walking them; then doubling rounds over the rest.  A round without a change: every cycle fits
        // 2^round cells; after max_rounds rounds every cycle does anyway
        gbk::sigma_walk(state[0], state[1], count, stats, st);
        cur = 1;
        for (u32 r = 0; r < max_rounds; r++) {
            u32* changed = words + gbk::SIGMA_WORDS + r;
            gbk::sigma_round(state[cur], state[cur ^ 1], count, r == 0, changed, st);
            if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
            cur ^= 1;
            got.rounds = r + 1;
            u32 flag = 0;
            if ((s = read_back(ctx, &flag, changed, sizeof flag))) return s;
            if (!flag) break;
        }
        gbk::sigma_class_stats(state[cur], count, lg, nw, reinterpret_cast<u32*>(state[cur ^ 1]), stats, st);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
        u64 hs[3];
        if ((s = read_back(ctx, hs, stats, sizeof hs))) return s;
        got.num_classes = hs[0];
        got.moved_cells = hs[1];
        got.largest_class = hs[2] ? hs[2] : 1;
    }
    void* lp = nullptr;
    if (hipMalloc(&lp, (size_t)cells * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GB_ERR_OOM, "hipMalloc copy class labels"); }
    u32* labels = static_cast<u32*>(lp);
    auto failed = [&](gb_status e) {   // nothing half-built stays with the circuit
        (void)hipStreamSynchronize(st);
        (void)hipFree(labels);
        return e;
    };
    {
        Scope sc(ctx, "decode sigmas: classes");
        gbk::sigma_labels(state[cur], cells, lg, nw, nr, labels, st);
        if (hipGetLastError() != hipSuccess) return failed(fail(ctx, GB_ERR_HIP, "kernel launch failed"));
    }
    if (with_partition) {
        if ((s = sigma_compare_partition(c, tmp, labels))) return failed(s);
        got.compared_partition = 1;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    k.sigma_labels = labels;
    k.sigma_info = got;
    k.sigma_compared = with_partition;
    if (info) *info = got;
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_circuit_decode_sigmas(gb_circuit* c, uint32_t flags, void* info) try {
    if (gb_status s = stage_guard(c)) return s;
    if (flags) return fail(c->ctx, GB_ERR_INVALID, "gb_circuit_decode_sigmas: flags must be 0");
    gb_sigma_info* out = static_cast<gb_sigma_info*>(info);
    return by_field(c, [&](auto* cf) { return decode_sigmas(cf, out); });
} GB_CATCH_CIRCUIT(c)

gb_status gb_circuit_copy_classes(gb_circuit* c, uint32_t* first_cell_out) try {
    if (gb_status s = stage_guard(c)) return s;
    gb_ctx* ctx = c->ctx;
    if (!first_cell_out) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (!c->chk.sigma_labels) return fail(ctx, GB_ERR_INVALID, "the sigmas of this circuit have not been decoded (gb_circuit_decode_sigmas)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)c->cfg.num_wires << c->cfg.degree_bits;
    HIP_TRY(ctx, hipMemcpyAsync(first_cell_out, c->chk.sigma_labels, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

}  // extern "C"

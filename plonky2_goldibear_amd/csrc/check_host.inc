// gb_check_witness / gb_check_partition / gb_check_inputs (include/goldibear_gpu.h): does this witness satisfy this circuit, and
// where not?  Included at the end of prover_host.inc, behind the witness fronts (witness_host.inc).  The kernels are kernels_check.hip's, the row logic
// witness_check.hpp's; this file prepares a circuit on its first check (the selector and constant columns as values on H, a row
// list per gate), runs one launch per gate that has rows and the copy pass, reads the counts back first and the per-entry results
// only where a count is not zero, and puts the violations in the order the header gives.  The copy classes are the partition's
// where the circuit has one, else those gb_circuit_decode_sigmas read out of the sigma columns (sigma_host.inc), else none.

#include "witness_check.hpp"

namespace {

// The selector and constant columns on H: the circuit keeps their coefficients and their LDE, which holds the coset g H and not H,
// so the first check runs the library's forward transform (rate 0, shift 1) over the coefficient columns; then the row lists.
template <class F>
gb_status check_prepare(Circuit<F>* c) {
    typedef typename F::T T;
    typedef Host<F> HF;
    namespace CK = gbk::check;
    gb_ctx* ctx = c->ctx;
    gb_circuit::Check& k = c->chk;
    if (k.ready) return GB_OK;
    Scope sc(ctx, "check witness: prepare");
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, ncols = cfg.num_selectors + cfg.num_constants, nl = c->gates.num_gates + 1;
    const size_t n = (size_t)1 << lg;
    hipStream_t st = ctx->stream;
    gb_status s;
    const typename HF::Tables* tabs;
    const typename HF::Cosets* cos;
    if ((s = tables_for<F>(ctx, lg, &tabs))) return s;
    if ((s = cosets_for<F>(ctx, lg, 0, F::one(), false, &cos))) return s;
    auto failed = [&](gb_status e) {   // nothing half-built stays with the circuit
        (void)hipStreamSynchronize(st);
        c->drop_check();
        return e;
    };
    PoolBlock leaf_order(ctx);
    if ((s = leaf_order.get(ncols * n * sizeof(T), "selector values"))) return s;
    if (hipMalloc(&k.hvals, ncols * n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); k.hvals = nullptr; return failed(fail(ctx, GB_ERR_OOM, "hipMalloc selector values")); }
    void* p = nullptr;
    if (hipMalloc(&p, (2 * CK::MAX_LISTS + 1) * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return failed(fail(ctx, GB_ERR_OOM, "hipMalloc row counts")); }
    k.lists_dev = static_cast<u32*>(p);
    gbk::lde_columns<F>((const T*)c->cs->coeffs, (T*)leaf_order.p, ncols, *tabs, *cos, st);
    gbk::poly_bitrev_store<F>((const T*)leaf_order.p, (T*)k.hvals, ncols, lg, false, st);
    u32* counts_dev = k.lists_dev;
    u32* offsets_dev = k.lists_dev + CK::MAX_LISTS;
    gbk::check_count_rows<F>(c->gates, (const T*)k.hvals, (u32)n, counts_dev, offsets_dev, st);
    if (hipGetLastError() != hipSuccess) return failed(fail(ctx, GB_ERR_HIP, "kernel launch failed"));
    std::vector<u32> lists(2 * CK::MAX_LISTS + 1);
    if ((s = read_back(ctx, lists.data(), k.lists_dev, lists.size() * sizeof(u32)))) return failed(s);
    k.counts.assign(lists.begin(), lists.begin() + nl);
    k.offsets.assign(lists.begin() + CK::MAX_LISTS, lists.begin() + CK::MAX_LISTS + nl + 1);
    const size_t total = k.offsets[nl];
    if (total > ((size_t)cfg.num_selectors + 1) * n) return failed(fail(ctx, GB_ERR_HIP, "internal: the row lists are longer than the circuit"));
    if (hipMalloc(&p, std::max<size_t>(1, total) * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return failed(fail(ctx, GB_ERR_OOM, "hipMalloc row lists")); }
    k.rows = static_cast<u32*>(p);
    gbk::check_fill_rows<F>(c->gates, (const T*)k.hvals, (u32)n, offsets_dev, k.rows, st);
    if (hipGetLastError() != hipSuccess) return failed(fail(ctx, GB_ERR_HIP, "kernel launch failed"));
    k.ready = true;
    return GB_OK;
}

// the first cell of every class of the partition's slot map, once per partition (the circuit has one, with fewer than 2^32 cells)
static gb_status check_first_cells_of_partition(gb_circuit* c) {
    gb_ctx* ctx = c->ctx;
    gb_circuit::Check& k = c->chk;
    if (k.first_cell) return GB_OK;
    const u32 num_slots = (u32)c->part.reps.size();
    void* p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, std::max<size_t>(1, num_slots) * sizeof(u32)));
    k.first_cell = static_cast<u32*>(p);
    gbk::check_first_cells(c->part.slots_dev, (u64)c->cfg.num_wires << c->cfg.degree_bits, num_slots, k.first_cell, c->ctx->stream);
    return GB_OK;
}

static std::string describe_violation(const gb_violation& v) {
    switch (v.kind) {
        case GB_VIOLATION_SELECTOR:
            return "selector violation at row " + std::to_string(v.row) + ": selector column " + std::to_string(v.index) + " holds " +
                   std::to_string(v.value) + ", which names no gate of its group";
        case GB_VIOLATION_GATE:
            return "gate violation at row " + std::to_string(v.row) + ": gate " + std::to_string(v.gate) + ", constraint " +
                   std::to_string(v.index) + " = " + std::to_string(v.value);
        default:
            return "copy violation at row " + std::to_string(v.row) + ", wire " + std::to_string(v.index) + " = " + std::to_string(v.value) +
                   ": the first cell of its class (row " + std::to_string(v.other_row) + ", wire " + std::to_string(v.other_wire) + ") holds " +
                   std::to_string(v.other_value);
    }
}

// wit: the device matrix [num_wires][n], canonical words
template <class F>
gb_status check_matrix(Circuit<F>* c, TmpAlloc& tmp, const typename F::T* wit, const uint64_t* public_inputs, size_t num_public_inputs,
                       gb_violation* out, size_t capacity, gb_check_result* result) {
    typedef typename F::T T;
    typedef Host<F> HF;
    namespace CK = gbk::check;
    constexpr u32 H = F::H;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 nw = cfg.num_wires, nsel = cfg.num_selectors, ng = c->gates.num_gates, nl = ng + 1;
    const size_t n = Counts(cfg).n;
    const u64 cells = (u64)n * nw;
    hipStream_t st = ctx->stream;
    gb_status s;
    if (result) *result = gb_check_result{};
    if ((s = check_prepare<F>(c))) return s;
    gb_circuit::Check& k = c->chk;
    Scope sc(ctx, "check witness");

    T pi_hash[H];
    {
        std::vector<T> pis(num_public_inputs);
        for (size_t i = 0; i < num_public_inputs; i++) pis[i] = (T)public_inputs[i];
        HF::hash_no_pad(pis.data(), pis.size(), pi_hash);   // prover.rs:244
    }
    T* pi_dev;
    {
        std::vector<T> enc(H);
        for (u32 i = 0; i < H; i++) enc[i] = F::enc(pi_hash[i]);
        if ((s = upload_tmp(ctx, tmp, enc, &pi_dev))) return s;
    }
    // words: [0] a word of the witness is not below p, [1] copy violations, [2 + g] failing entries of gate g
    const size_t nwords = 2 + (size_t)ng;
    u32* words = tmp.get<u32>(nwords);
    const size_t total = k.offsets[nl];
    u32* fail_index = tmp.get<u32>(total);
    u64* fail_value = tmp.get<u64>(total);
    if (!words || !fail_index || !fail_value) return fail(ctx, GB_ERR_OOM, "check results");
    HIP_TRY(ctx, hipMemsetAsync(words, 0, nwords * sizeof(u32), st));
    { Scope sw(ctx, "check witness: canonical words"); gbk::check_canonical<F>(wit, (size_t)cells, words, st); }
    const gbk::CheckParams<F> cp{c->gates, (u32)n};
    const gbk::ProgramParams<F> pp{c->programs, c->prog_instrs_dev, c->prog_lits_dev};
    // with profiling on, every gate launch is a scope of its own, named by the gate's kind (tools/witness_check_times.py)
    static const char* const GATE_SCOPES[] = {
        "check witness: gate kind 0",  "check witness: gate kind 1",  "check witness: gate kind 2",  "check witness: gate kind 3",
        "check witness: gate kind 4",  "check witness: gate kind 5",  "check witness: gate kind 6",  "check witness: gate kind 7",
        "check witness: gate kind 8",  "check witness: gate kind 9",  "check witness: gate kind 10", "check witness: gate kind 11",
        "check witness: gate kind 12", "check witness: gate kind 13", "check witness: gate kind 14", "check witness: gate kind 15",
        "check witness: gate kind 16", "check witness: gate kind 17", "check witness: gate kind 18"};
    for (u32 g = 0; g < ng; g++) {
        if (!k.counts[g] || gbk::gates::num_constraints<F>(c->gates.g[g], c->programs) == 0) continue;
        const u32 off = k.offsets[g];
        Scope sg(ctx, GATE_SCOPES[std::min<u32>(c->gates.g[g].kind, GB_GATE_PROGRAM)]);
        gbk::check_gate_rows<F>(cp, g, c->programs.num_programs ? &pp : nullptr, k.rows + off, k.counts[g], (const T*)k.hvals, wit, pi_dev,
                                fail_index + off, fail_value + off, words + 2 + g, st);
    }
    // copies: the classes of the partition's slot map (their first cells once per partition), or without a partition the labels
    // gb_circuit_decode_sigmas left - a slot map whose slots are the first cells themselves; then one pass over the cells
    const bool by_partition = c->part.set && c->part.slots_dev;
    const bool copies = by_partition || k.sigma_labels;
    const u32* slots = by_partition ? c->part.slots_dev : k.sigma_labels;
    const u32 num_slots = by_partition ? (u32)c->part.reps.size() : (u32)cells;
    u64* mask = nullptr;
    const size_t mask_words = (size_t)((cells + 63) / 64);
    if (copies) {
        if (cells > 0xFFFFFFFFull) return fail(ctx, GB_ERR_UNSUPPORTED, "copy check: more than 2^32 wire cells");
        if (by_partition)
            if ((s = check_first_cells_of_partition(c))) return s;
        mask = tmp.get<u64>(mask_words);
        if (!mask) return fail(ctx, GB_ERR_OOM, "copy check mask");
        Scope sp(ctx, "check witness: copies");
        gbk::check_copies<F>(slots, by_partition ? k.first_cell : nullptr, num_slots, wit, (u32)n, nw, mask, words + 1, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    std::vector<u32> hw(nwords);
    if ((s = read_back(ctx, hw.data(), words, nwords * sizeof(u32)))) return s;
    if (hw[0]) return fail(ctx, GB_ERR_INVALID, "non-canonical witness element");

    std::vector<gb_violation> listed;   // at most `capacity` of them, in the header's order
    auto room = [&] { return listed.size() < capacity; };
    // ---- selector violations, by (row, column): the rows of the last list, their selector values through the shared row logic
    u64 num_selector = 0;
    if (const u32 V = k.counts[ng]) {
        u64* vals_dev = tmp.get<u64>((size_t)V * nsel);
        if (!vals_dev) return fail(ctx, GB_ERR_OOM, "selector values");
        gbk::check_selector_values<F>((const T*)k.hvals, (u32)n, nsel, k.rows + k.offsets[ng], V, vals_dev, st);
        std::vector<u32> rows(V);
        std::vector<u64> vals((size_t)V * nsel);
        ReadBack rb(ctx);
        if ((s = rb.add(rows.data(), k.rows + k.offsets[ng], V * sizeof(u32)))) return s;
        if ((s = rb.add(vals.data(), vals_dev, vals.size() * sizeof(u64)))) return s;
        if ((s = rb.finish())) return s;
        for (u32 i = 0; i < V; i++)
            for (u32 col = 0; col < nsel; col++) {
                const u64 v = vals[(size_t)i * nsel + col];
                if (CK::active_gate<F>(c->gates, col, v) != CK::BAD_SELECTOR) continue;
                num_selector++;
                if (room()) listed.push_back(gb_violation{GB_VIOLATION_SELECTOR, 0, rows[i], col, 0, 0, v, 0});
            }
    }
    // ---- gate violations, by (row, gate)
    u64 num_gate = 0;
    {
        std::vector<gb_violation> found;
        for (u32 g = 0; g < ng; g++) {
            const u32 nf = hw[2 + g], cnt = k.counts[g], off = k.offsets[g];
            if (!nf) continue;
            num_gate += nf;
            if (!capacity) continue;
            std::vector<u32> rows(cnt), idx(cnt);
            std::vector<u64> val(cnt);
            ReadBack rb(ctx);
            if ((s = rb.add(rows.data(), k.rows + off, cnt * sizeof(u32)))) return s;
            if ((s = rb.add(idx.data(), fail_index + off, cnt * sizeof(u32)))) return s;
            if ((s = rb.add(val.data(), fail_value + off, cnt * sizeof(u64)))) return s;
            if ((s = rb.finish())) return s;
            for (u32 i = 0; i < cnt; i++)
                if (idx[i] != CK::NO_FAILURE) found.push_back(gb_violation{GB_VIOLATION_GATE, g, rows[i], idx[i], 0, 0, val[i], 0});
        }
        std::sort(found.begin(), found.end(), [](const gb_violation& a, const gb_violation& b) { return a.row != b.row ? a.row < b.row : a.gate < b.gate; });
        for (const gb_violation& v : found) {
            if (!room()) break;
            listed.push_back(v);
        }
    }
    // ---- copy violations, by cell index: the waves' ballots are in cell order
    const u64 num_copy = copies ? hw[1] : 0;
    if (num_copy && room()) {
        std::vector<u64> hm(mask_words);
        if ((s = read_back(ctx, hm.data(), mask, mask_words * sizeof(u64)))) return s;
        std::vector<u32> bad;
        const size_t want = capacity - listed.size();
        for (size_t w = 0; w < mask_words && bad.size() < want; w++)
            for (u64 m = hm[w]; m && bad.size() < want; m &= m - 1) bad.push_back((u32)(w * 64 + (u32)__builtin_ctzll(m)));
        u32* bad_dev;
        if ((s = upload_tmp(ctx, tmp, bad, &bad_dev))) return s;
        u64* rep_dev = tmp.get<u64>(3 * bad.size());
        if (!rep_dev) return fail(ctx, GB_ERR_OOM, "copy report");
        gbk::check_copy_report<F>(slots, by_partition ? k.first_cell : nullptr, num_slots, wit, (u32)n, nw, bad_dev, (u32)bad.size(), rep_dev, st);
        std::vector<u64> rep(3 * bad.size());
        if ((s = read_back(ctx, rep.data(), rep_dev, rep.size() * sizeof(u64)))) return s;
        for (size_t i = 0; i < bad.size(); i++) {
            const u64 fc = rep[3 * i + 1];
            listed.push_back(gb_violation{GB_VIOLATION_COPY, 0, bad[i] / nw, bad[i] % nw, (u32)(fc % nw), fc / nw, rep[3 * i], rep[3 * i + 2]});
        }
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    if (out) std::copy(listed.begin(), listed.end(), out);
    if (result) *result = gb_check_result{num_gate, num_selector, num_copy, copies ? (by_partition ? 1u : 2u) : 0u, (uint32_t)listed.size()};
    if (!(num_gate + num_selector + num_copy)) return GB_OK;
    std::string msg = "the witness does not satisfy the circuit: " + std::to_string(num_selector) + " selector, " + std::to_string(num_gate) +
                      " gate, " + std::to_string(num_copy) + " copy violations";
    if (!listed.empty()) msg += "; the first: " + describe_violation(listed[0]);
    return fail(ctx, GB_ERR_UNSATISFIED, msg);
}

// the caller's matrix -> a device matrix of canonical words, as gb_prove takes it: device input is read where it lies
template <class F>
gb_status check_witness_matrix(Circuit<F>* c, ColSrc witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs,
                               gb_violation* out, size_t capacity, gb_check_result* result) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << c->cfg.degree_bits, count = (size_t)c->cfg.num_wires * n;
    const bool dev = (flags & GB_INPUT_DEVICE) != 0, p3 = (flags & GB_INPUT_P3_REPR) != 0;
    if (p3 && dev) return fail(ctx, GB_ERR_INVALID, "GB_INPUT_P3_REPR describes host memory; device inputs are canonical");
    TmpAlloc tmp(ctx);
    const T* wit = static_cast<const T*>(witness.base);
    if (!dev || witness.ptrs) {
        T* copy = tmp.get<T>(count);
        if (!copy) return fail(ctx, GB_ERR_OOM, "witness copy");
        if (!copy_columns(witness, c->cfg.num_wires, n * sizeof(T), copy, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream))
            return fail(ctx, GB_ERR_HIP, "copy of the witness failed");
        if (p3) p3_to_canonical_dev<F>(copy, count, ctx->stream);
        wit = copy;
    }
    const gb_status s = check_matrix<F>(c, tmp, wit, public_inputs, num_public_inputs, out, capacity, result);
    if (!dev) (void)hipStreamSynchronize(ctx->stream);   // the witness is the caller's again, whatever the outcome
    return s;
}

// option "check_witness": prove()'s full computation checks its witness before the wires commitment
template <class F>
gb_status check_before_commit(Circuit<F>* c, ColSrc witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs) {
    return check_witness_matrix<F>(c, witness, flags, public_inputs, num_public_inputs, nullptr, 1, nullptr);
}

// gb_check_partition / gb_check_inputs: the matrix as the prove fronts make it (witness_host.inc), then the check
template <class F>
gb_status check_source(Circuit<F>* c, WitnessSource src, uint32_t flags, gb_violation* out, size_t capacity, gb_check_result* result) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> pis;
    TmpAlloc tmp(ctx);
    T* matrix = tmp.get<T>((size_t)c->cfg.num_wires << c->cfg.degree_bits);
    if (!matrix) return fail(ctx, GB_ERR_OOM, src.inputs ? "witness matrix" : "partition witness matrix");
    if (gb_status s = witness_to_device<F>(c, tmp, src, flags, matrix, &pis)) return s;
    return check_matrix<F>(c, tmp, matrix, pis.data(), pis.size(), out, capacity, result);
}

}  // namespace

extern "C" {

gb_status gb_check_witness(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs,
                           void* violations_out, size_t capacity, void* result) try {
    if (gb_status s = stage_guard(c)) return s;
    gb_ctx* ctx = c->ctx;
    if (!witness) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (capacity && !violations_out) return fail(ctx, GB_ERR_INVALID, "null violations_out with a capacity");
    if (flags & ~GB_PUBLIC_INPUT_FLAGS) return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    if (num_public_inputs && !public_inputs) return fail(ctx, GB_ERR_INVALID, "null public inputs");
    if (num_public_inputs != c->cfg.num_public_inputs) return fail(ctx, GB_ERR_INVALID, "Number of public inputs doesn't match circuit data.");
    gb_violation* out = static_cast<gb_violation*>(violations_out);
    gb_check_result* res = static_cast<gb_check_result*>(result);
    c->drop_retry();   // for gb_prove_retry a check is another call in between: what follows it is the full computation
    return by_field(c, [&](auto* cf) {
        return check_witness_matrix(cf, ColSrc(witness), flags, public_inputs, num_public_inputs, out, capacity, res);
    });
} GB_CATCH_CIRCUIT(c)

gb_status gb_check_partition(gb_circuit* c, const void* values, uint32_t flags, void* violations_out, size_t capacity, void* result) try {
    if (gb_status s = partition_guard(c, values, flags)) return s;
    if (capacity && !violations_out) return fail(c->ctx, GB_ERR_INVALID, "null violations_out with a capacity");
    gb_violation* out = static_cast<gb_violation*>(violations_out);
    gb_check_result* res = static_cast<gb_check_result*>(result);
    c->drop_retry();   // for gb_prove_retry a check is another call in between: what follows it is the full computation
    return by_field(c, [&](auto* cf) { return check_source(cf, WitnessSource{values, false}, flags, out, capacity, res); });
} GB_CATCH_CIRCUIT(c)

gb_status gb_check_inputs(gb_circuit* c, const void* input_values, uint32_t flags, void* violations_out, size_t capacity, void* result) try {
    if (gb_status s = generators_guard(c, input_values, flags)) return s;
    if (capacity && !violations_out) return fail(c->ctx, GB_ERR_INVALID, "null violations_out with a capacity");
    gb_violation* out = static_cast<gb_violation*>(violations_out);
    gb_check_result* res = static_cast<gb_check_result*>(result);
    c->drop_retry();   // for gb_prove_retry a check is another call in between: what follows it is the full computation
    return by_field(c, [&](auto* cf) { return check_source(cf, WitnessSource{input_values, true}, flags, out, capacity, res); });
} GB_CATCH_CIRCUIT(c)

}  // extern "C"

// The witness fronts (included at the end of prover_host.inc): prove() and the witness check from the partition witness or from
// the inputs of the witness generators, their stages and their entry points.

// ---------------------------------------------------------------------------------------------- the partition witness
// prove_with_partition_witness's first timed step, "compute full witness" = partition_witness.full_witness() (plonk/prover.rs:
// 160-183, iop/witness.rs:359-371), from the reference's own object: `values` holds PartitionWitness.values (None as zero), one
// entry per target.  Compaction staged[k] = values[reps[k]] (reps ascending: one streaming pass, canonicalised and range-checked as
// it goes, by the context's copy threads into page-locked memory), upload of the K staged elements, k_expand_partition.  The
// upload is not overlapped with the transforms the way the chunks of a host matrix are (DESIGN.md section 8).
template <class F>
static bool partition_value(const void* values, uint64_t target, bool p3, typename F::T* out) {
    typedef typename F::T T;
    T v = static_cast<const T*>(values)[target];
    if (p3) v = (T)Host<F>::p3_to_canonical(F::reduce_word(v));
    *out = v;
    return (u64)v < F::ORDER;
}

template <class F>
static gb_status partition_public_inputs(Circuit<F>* c, const void* values, bool p3, std::vector<uint64_t>* pis) {
    pis->resize(c->part.pi_reps.size());
    for (size_t i = 0; i < pis->size(); i++) {
        typename F::T v;
        if (!partition_value<F>(values, c->part.pi_reps[i], p3, &v)) return fail(c->ctx, GB_ERR_INVALID, "non-canonical witness element");
        (*pis)[i] = (uint64_t)v;
    }
    return GB_OK;
}

// values -> matrix_dev [num_wires][n], canonical words, on the context's stream
template <class F>
static gb_status expand_partition_stage(Circuit<F>* c, TmpAlloc& tmp, const void* values, uint32_t flags, typename F::T* matrix_dev) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    gb_circuit::Partition& part = c->part;
    hipStream_t st = ctx->stream;
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0;
    const size_t K = part.reps.size(), bytes = K * sizeof(T);
    Scope sc(ctx, "compute full witness");
    if (part.staged_host_bytes < bytes) {
        if (part.staged_host) {
            HIP_TRY(ctx, hipStreamSynchronize(st));
            (void)hipHostFree(part.staged_host);
            part.staged_host = nullptr;
            part.staged_host_bytes = 0;
        }
        HIP_TRY(ctx, hipHostMalloc(&part.staged_host, bytes, hipHostMallocDefault));
        part.staged_host_bytes = bytes;
    }
    if (!part.staged_read) HIP_TRY(ctx, hipEventCreateWithFlags(&part.staged_read, hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(part.staged_read));   // the upload of the call before has left the staging block
    {
        Scope s1(ctx, "partition compaction");
        T* staged = static_cast<T*>(part.staged_host);
        const uint32_t* reps = part.reps.data();
        std::atomic<bool> bad{false};
        auto run = [&](size_t k0, size_t k1) {
            bool ok = true;
            for (size_t k = k0; k < k1; k++) ok &= partition_value<F>(values, reps[k], p3, staged + k);
            if (!ok) bad.store(true, std::memory_order_relaxed);
        };
        const size_t nthreads = K >= ((size_t)1 << 18) && ctx->copy_threads > 1 ? (size_t)ctx->copy_threads : 1;
        if (nthreads == 1) {
            run(0, K);
        } else {
            std::vector<std::thread> workers;
            const size_t per = (K + nthreads - 1) / nthreads;
            try {   // a thread the system refuses: the calling thread takes its share
                for (size_t i = 1; i < nthreads; i++) workers.emplace_back(run, std::min(K, i * per), std::min(K, (i + 1) * per));
            } catch (...) {
            }
            const size_t started = workers.size() + 1;
            run(0, std::min(K, per));
            if (started < nthreads) run(std::min(K, started * per), K);
            for (auto& w : workers) w.join();
        }
        if (bad.load()) return fail(ctx, GB_ERR_INVALID, "non-canonical witness element");
    }
    T* staged_dev = tmp.get<T>(K);
    if (!staged_dev) return fail(ctx, GB_ERR_OOM, "partition staging");
    {
        Scope s2(ctx, "partition upload");
        HIP_TRY(ctx, hipMemcpyAsync(staged_dev, part.staged_host, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipEventRecord(part.staged_read, st));
    }
    {
        Scope s3(ctx, "partition expansion");
        gbk::expand_partition<F>(part.slots_dev, staged_dev, matrix_dev, c->cfg.degree_bits, c->cfg.num_wires, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

// ---------------------------------------------------------------------------------------------- the witness generators
// prove()'s first call, generate_partial_witness (plonk/prover.rs:136-158; "run N generators", iop/generator.rs:25-106), on the
// device: the inputs are uploaded and scattered to their classes, the schedule's launches (generators.hpp) fill the values array -
// one canonical word per class, the slots of the partition map first - and one block comes back: the public inputs' values and
// the error word.  k_expand_partition then reads the front of that array where gb_prove_partition reads its staged upload.
template <class F>
static gb_status generate_stage(Circuit<F>* c, TmpAlloc& tmp, const void* input_values, uint32_t flags, typename F::T* values_dev,
                                std::vector<uint64_t>* pis) {
    typedef typename F::T T;
    namespace GN = gbk::gen;
    gb_ctx* ctx = c->ctx;
    gb_circuit::Generators& g = c->gens;
    const GN::Schedule& sc = g.sched;
    hipStream_t st = ctx->stream;
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0;
    const size_t ni = sc.input_cls.size(), npi = sc.pi_cls.size();
    Scope scope(ctx, "run generators");
    // the inputs: canonical, below p, and equal where two of them name one class (witness.rs:340-350).  They go up in slices of
    // the context's page-locked arena (stage_up), each filled and handed to one asynchronous copy; only a context that has no
    // arena copies from pageable memory, and waits for that copy before the buffer goes
    auto canonical = [&](size_t i) {
        T v = static_cast<const T*>(input_values)[i];
        return p3 ? (T)Host<F>::p3_to_canonical(F::reduce_word(v)) : v;
    };
    HIP_TRY(ctx, hipMemsetAsync(values_dev, 0, (size_t)sc.num_classes * sizeof(T), st));
    HIP_TRY(ctx, hipMemsetAsync(g.err_dev, 0, GN::ERROR_WORDS * sizeof(uint32_t), st));
    if (ni) {
        T* in_dev = tmp.get<T>(ni);
        if (!in_dev) return fail(ctx, GB_ERR_OOM, "generator inputs");
        const size_t slice = XFER_UP_BYTES / 4 / sizeof(T);
        std::vector<T> pageable;
        for (size_t i0 = 0; i0 < ni; i0 += slice) {
            const size_t count = std::min(slice, ni - i0);
            T* host = static_cast<T*>(stage_up(ctx, count * sizeof(T)));
            const bool staged = host != nullptr;
            if (!staged) {
                pageable.resize(count);
                host = pageable.data();
            }
            for (size_t i = i0; i < i0 + count; i++) {
                const T v = canonical(i);
                if ((u64)v >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical witness element (input " + std::to_string(i) + ")");
                host[i - i0] = v;
                if (sc.input_first[i] != i && canonical(sc.input_first[i]) != v)
                    return fail(ctx, GB_ERR_INVALID, "Partition containing target " + std::to_string(sc.class_reps[sc.input_cls[i]]) +
                                " was set twice with different values (inputs " + std::to_string(sc.input_first[i]) + " and " + std::to_string(i) + ")");
            }
            HIP_TRY(ctx, hipMemcpyAsync(in_dev + i0, host, count * sizeof(T), hipMemcpyHostToDevice, st));
            if (!staged) HIP_TRY(ctx, hipStreamSynchronize(st));
        }
        gbk::scatter_inputs<F>(g.input_cls_dev, in_dev, (u32)ni, values_dev, st);
    }
    gbk::run_generators<F>(g.device, sc.launches.data(), sc.launches.size(), sc.level_off.data(), values_dev, g.err_dev, st);
    u64* back_dev = tmp.get<u64>(npi + GN::ERROR_WORDS);
    if (!back_dev) return fail(ctx, GB_ERR_OOM, "generator read-back");
    gbk::gather_public<F>(g.pi_cls_dev, (u32)npi, values_dev, g.err_dev, back_dev, st);
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    std::vector<u64> back(npi + GN::ERROR_WORDS);
    {
        ReadBack rb(ctx);
        if (gb_status rs = rb.add(back.data(), back_dev, back.size() * sizeof(u64))) return rs;
        if (gb_status rs = rb.finish()) return rs;
    }
    const u32 code = (u32)back[npi], record = (u32)back[npi + 1], cls = (u32)back[npi + 2];
    if (code != GN::ERR_NONE) {
        const std::string rec = "generator record " + std::to_string(record) + ": ";
        const std::string target = cls < sc.class_reps.size() ? std::to_string(sc.class_reps[cls]) : std::string("?");
        switch (code) {
            case GN::ERR_SET_TWICE:
                return fail(ctx, GB_ERR_INVALID, rec + "Partition containing target " + target + " was set twice with different values");
            case GN::ERR_SWAP_NOT_BOOLEAN:
                return fail(ctx, GB_ERR_INVALID, rec + "the swap wire (target " + target + ") is neither 0 nor 1");
            case GN::ERR_ACCESS_INDEX:
                return fail(ctx, GB_ERR_INVALID, rec + "Access index (target " + target + ") is larger than the vector size");
            case GN::ERR_SPLIT_TOO_LARGE:
                return fail(ctx, GB_ERR_INVALID, rec + "Integer too large to fit in given number of limbs");
            case GN::ERR_DIVIDE_BY_ZERO:
                if (cls >= sc.class_reps.size()) return fail(ctx, GB_ERR_INVALID, rec + "Tried to invert zero (INV in a generator program)");
                return fail(ctx, GB_ERR_INVALID, rec + "Tried to invert zero (the denominator at target " + target + ")");
            case GN::ERR_NO_SQUARE_ROOT:
                return fail(ctx, GB_ERR_INVALID, rec + "SQRT of a non-residue in a generator program (called `Option::unwrap()` on a `None` value)");
            case GN::ERR_INTEGER_DIVIDE_BY_ZERO:
                return fail(ctx, GB_ERR_INVALID, rec + "attempt to divide by zero (IDIV / IREM in a generator program)");
            case GN::ERR_NOT_BOOLEAN:
                return fail(ctx, GB_ERR_INVALID, rec + "not a bool (target " + target + ")");
            case GN::ERR_NO_PROGRAM_TABLES:   // the schedule always sets program_regs with a program generator: not reachable from the ABI
                return fail(ctx, GB_ERR_HIP, rec + "a program generator was run without the program tables");
            default:
                return fail(ctx, GB_ERR_HIP, rec + "unknown generator error word");
        }
    }
    if (pis) pis->assign(back.begin(), back.begin() + npi);
    return GB_OK;
}

// ---------------------------------------------------------------------------------------------- one path from either source
// Where a witness comes from: PartitionWitness.values, one entry per target (gb_*_partition), or the input values of the
// generator schedule (gb_*_inputs)
struct WitnessSource {
    const void* values;
    bool inputs;
};

// source -> matrix_dev [num_wires][n] of canonical words on the context's stream, and the public inputs (pis may be null: the
// partition's are read off `values`, which a caller may have done already; the generators' come back from the device with their
// error word either way).  The scopes are the reference's: "compute full witness" around the partition's three steps; "run
// generators", then "compute full witness" around the expansion alone - full_witness() straight from the generated values.
template <class F>
static gb_status witness_to_device(Circuit<F>* c, TmpAlloc& tmp, WitnessSource src, uint32_t flags, typename F::T* matrix_dev,
                                   std::vector<uint64_t>* pis) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    gb_status s;
    if (!src.inputs) {
        if (pis && (s = partition_public_inputs<F>(c, src.values, (flags & GB_INPUT_P3_REPR) != 0, pis))) return s;
        return expand_partition_stage<F>(c, tmp, src.values, flags, matrix_dev);
    }
    T* values_dev = tmp.get<T>(c->gens.sched.num_classes);
    if (!values_dev) return fail(ctx, GB_ERR_OOM, "generated values");
    if ((s = generate_stage<F>(c, tmp, src.values, flags, values_dev, pis))) return s;
    Scope sc(ctx, "compute full witness");
    gbk::expand_partition<F>(c->part.slots_dev, values_dev, matrix_dev, c->cfg.degree_bits, c->cfg.num_wires, ctx->stream);
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

// The retry (prover.rs:186-226): the caller re-drew ONE value, the one behind witness[hint.wire][hint.row].  May that cell of the
// matrix the failed attempt kept be re-drawn in place - is everything else of that matrix, and of the public inputs, still
// right - and with what value?
//   the partition: values[representative_map[row * num_wires + wire]] was re-drawn; yes where that slot is the cell's alone
//   (prover_data.random_wire is).  Every other used entry is the failed attempt's, which was checked then.
//   the inputs: yes where the cell is an input that no generator reads, writes or checks, no public input is in its class and
//   that cell alone carries it (input_fast, gb_circuit_set_generators)
template <class F>
static gb_status redrawn_cell(Circuit<F>* c, WitnessSource src, const RetryHint& hint, bool p3, bool* in_place, typename F::T* value) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    const u32 nw = c->cfg.num_wires;
    *in_place = false;
    if (src.inputs) {
        const gb_circuit::Generators& g = c->gens;
        const uint64_t target = hint.row * nw + hint.wire;
        auto it = std::lower_bound(g.input_index.begin(), g.input_index.end(), std::make_pair(target, (uint32_t)0));
        if (it == g.input_index.end() || it->first != target || !g.input_fast[it->second]) return GB_OK;
        T v = static_cast<const T*>(src.values)[it->second];
        if (p3) v = (T)Host<F>::p3_to_canonical(F::reduce_word(v));
        *value = v;
    } else {
        uint32_t slot = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&slot, c->part.slots_dev + hint.row * nw + hint.wire, sizeof slot, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (slot >= c->part.reps.size() || c->part.is_shared_slot(slot)) return GB_OK;
        (void)partition_value<F>(src.values, c->part.reps[slot], p3, value);
    }
    if ((u64)*value >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical witness element");
    *in_place = true;
    return GB_OK;
}

// gb_prove_partition* / gb_prove_inputs*: the matrix on the device - a fresh one, or the kept one with one cell re-drawn - then
// the proof proper, the device-witness path of prove()
template <class F>
static gb_status prove_from_source(Circuit<F>* c, WitnessSource src, uint32_t flags, const void* salts, void* proof_out, size_t proof_cap,
                                   size_t* proof_len, const RetryHint* hint) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gb_circuit_config& cfg = c->cfg;
    const size_t n = (size_t)1 << cfg.degree_bits, N = n << cfg.rate_bits;
    const u32 nw = cfg.num_wires;
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0;
    hipStream_t st = ctx->stream;
    gb_circuit::RetryKeep& keep = c->retry;
    gb_status s;
    std::vector<uint64_t> pis;
    if (!src.inputs && (s = partition_public_inputs<F>(c, src.values, p3, &pis))) return s;   // (before an earlier attempt's state is touched)
    struct MatrixGuard {   // the matrix: a pool block, handed to c->retry when the attempt leaves retry state behind
        gb_ctx* ctx; void* p; size_t bytes;
        ~MatrixGuard() { if (p) pool_free(ctx, p, bytes); }
    } matrix{ctx, nullptr, (size_t)nw * n * sizeof(T)};
    TmpAlloc tmp(ctx);
    // a kept matrix serves the partition's retry whichever front kept it (the public inputs are read off `values`); the inputs'
    // retry needs the public inputs its own front kept with it
    bool incremental = hint && !salts && keep.wires && keep.seg.state && keep.matrix && (!src.inputs || keep.by_inputs) &&
                       hint->wire < nw && hint->row < n;
    T v{};
    if (incremental && (s = redrawn_cell<F>(c, src, *hint, p3, &incremental, &v))) return s;
    if (incremental) {
        if (src.inputs) pis = keep.pis;
        matrix.p = keep.matrix;   // this call's from here on; the rest of the kept state is taken by prove()
        keep.matrix = nullptr;
        keep.matrix_bytes = 0;
        keep.by_inputs = false;
        Scope sc(ctx, "compute full witness");
        u32* cell = reinterpret_cast<u32*>(static_cast<T*>(matrix.p) + (size_t)hint->wire * n + hint->row);
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)cell, (int)(u32)(u64)v, 1, st));
        if (sizeof(T) == 8) HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(cell + 1), (int)(u32)((u64)v >> 32), 1, st));
    } else {
        hint = nullptr;
        c->drop_retry();   // (with the matrix of an earlier attempt) before the new one is allocated
        if (pool_alloc(ctx, matrix.bytes, &matrix.p) != hipSuccess) { matrix.p = nullptr; return fail(ctx, GB_ERR_OOM, src.inputs ? "witness matrix" : "partition witness matrix"); }
        if ((s = witness_to_device<F>(c, tmp, src, flags, static_cast<T*>(matrix.p), src.inputs ? &pis : nullptr))) return s;
    }
    // Host salts go to the device with the witness; a seed goes to prove() as it is
    const T* salts_dev = static_cast<const T*>(salts);
    const bool seeded = (flags & GB_SALTS_FROM_SEED) != 0;
    if (salts && !seeded) {
        const size_t count = (size_t)3 * GB_SALT_SIZE * N;
        T* sd = tmp.get<T>(count);
        if (!sd) return fail(ctx, GB_ERR_OOM, "salt staging");
        HIP_TRY(ctx, hipMemcpyAsync(sd, salts, count * sizeof(T), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));   // the salts are the caller's again
        if (p3) p3_to_canonical_dev<F>(sd, count, st);
        salts_dev = sd;
    }
    s = prove<F>(c, ColSrc(matrix.p), GB_INPUT_DEVICE | (seeded ? GB_SALTS_FROM_SEED : 0u), pis.data(), pis.size(), salts_dev, proof_out,
                 proof_cap, proof_len, hint);
    if (s == GB_ERR_PERM_ARG_ZERO && keep.wires) {   // prove() kept its wires commitment: keep the matrix it was made from
        keep.matrix = matrix.p;
        keep.matrix_bytes = matrix.bytes;
        keep.by_inputs = src.inputs;
        if (src.inputs) keep.pis = std::move(pis);
        matrix.p = nullptr;
    }
    return s;
}

// one small table of a circuit on the device, by hipMalloc (an empty one still gets a valid allocation)
static hipError_t upload_table(const void* src, size_t bytes, void** dst) {
    hipError_t e = hipMalloc(dst, std::max<size_t>(16, bytes));
    if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    return e;
}

extern "C" {

// ---- the partition witness (templates above: expand_partition_stage, witness_to_device)
gb_status gb_circuit_set_partition(gb_circuit* c, const uint64_t* representative_map, uint64_t num_targets,
                                   const uint64_t* public_input_targets, size_t num_public_inputs) try {
    if (gb_status s = stage_guard(c)) return s;
    gb_ctx* ctx = c->ctx;
    const uint64_t cells = (uint64_t)c->cfg.num_wires << c->cfg.degree_bits;
    gbk::partition::SlotMap m;
    const char* msg = "";
    if (const int ms = gbk::partition::build_slot_map(representative_map, num_targets, cells, public_input_targets, num_public_inputs,
                                                      c->cfg.num_public_inputs, &m, &msg))
        return fail(ctx, (gb_status)ms, std::string("gb_circuit_set_partition: ") + msg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->drop_retry();
    c->drop_partition();
    void* p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, std::max<size_t>(4, m.slots.size() * sizeof(uint32_t))));
    c->part.slots_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, hipMemcpy(p, m.slots.data(), m.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->part.rep_map.resize(num_targets);
    for (uint64_t t = 0; t < num_targets; t++) c->part.rep_map[t] = (uint32_t)representative_map[t];
    c->part.reps = std::move(m.reps);
    c->part.pi_reps = std::move(m.pi_reps);
    c->part.shared = std::move(m.shared);
    c->part.num_targets = num_targets;
    c->part.set = true;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

static gb_status partition_guard(gb_circuit* c, const void* values, uint32_t flags, uint32_t allowed = GB_PUBLIC_INPUT_FLAGS) {
    if (gb_status s = stage_guard(c)) return s;
    if (!values) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    if (flags & ~allowed) return fail(c->ctx, GB_ERR_INVALID, "unknown bits in flags");
    if (flags & GB_INPUT_DEVICE) return fail(c->ctx, GB_ERR_INVALID, "the partition witness is a host object: GB_INPUT_DEVICE does not apply");
    if (!c->part.set) return fail(c->ctx, GB_ERR_INVALID, "gb_circuit_set_partition has not been called on this circuit");
    return GB_OK;
}

gb_status gb_expand_partition(gb_circuit* c, const void* values, uint32_t flags, void* witness_dev_out) try {
    if (gb_status s = partition_guard(c, values, flags)) return s;
    if (!witness_dev_out) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    return by_field(c, [&](auto* cf) -> gb_status {
        typedef typename std::remove_pointer<decltype(cf)>::type::T T;
        HIP_TRY(c->ctx, hipSetDevice(c->ctx->device));
        TmpAlloc tmp(c->ctx);
        return witness_to_device(cf, tmp, WitnessSource{values, false}, flags, static_cast<T*>(witness_dev_out), nullptr);
    });
} GB_CATCH_CIRCUIT(c)

// ---- generator programs: witness generators as data (generator_programs.hpp checks them, generators.hpp gen_program runs them)
gb_status gb_circuit_set_generator_programs(gb_circuit* c, const uint64_t* program_words, const uint32_t* program_offsets,
                                            uint32_t num_programs) try {
    namespace GN = gbk::gen;
    if (gb_status s = stage_guard(c)) return s;
    gb_ctx* ctx = c->ctx;
    if (!c->part.set)
        return fail(ctx, GB_ERR_INVALID, "gb_circuit_set_generator_programs: gb_circuit_set_partition has not been called on this circuit");
    GN::GeneratorPrograms parsed;
    std::string msg;
    const uint64_t order = by_field(c->field, [](auto f) { return (uint64_t)decltype(f)::ORDER; });
    if (!GN::parse_generator_programs(program_words, program_offsets, num_programs, order, c->cfg.num_constants, &parsed, &msg))
        return fail(ctx, GB_ERR_INVALID, "gb_circuit_set_generator_programs: " + msg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->drop_retry();
    c->drop_generator_programs();   // and the schedule built on the old ones
    if (parsed.empty()) return GB_OK;
    std::vector<uint64_t> lits(parsed.lits.size());   // device form, once
    for (size_t i = 0; i < lits.size(); i++)
        lits[i] = c->field == GB_GOLDILOCKS ? (uint64_t)GlF::enc(parsed.lits[i]) : (uint64_t)BbF::enc(parsed.lits[i]);
    gb_circuit::GeneratorPrograms& gp = c->gen_programs;
    void* p = nullptr;
    HIP_TRY(ctx, upload_table(parsed.headers.data(), parsed.headers.size() * sizeof(GN::ProgramHeader), &p));
    gp.headers_dev = static_cast<GN::ProgramHeader*>(p);
    HIP_TRY(ctx, upload_table(parsed.instrs.data(), parsed.instrs.size() * sizeof(uint64_t), &p));
    gp.instrs_dev = static_cast<uint64_t*>(p);
    HIP_TRY(ctx, upload_table(lits.data(), lits.size() * sizeof(uint64_t), &p));
    gp.lits_dev = static_cast<uint64_t*>(p);
    gp.host = std::move(parsed);
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// ---- the witness generators (templates above: generate_stage, witness_to_device)
// replaces the host's generate_partial_witness (plonk/prover.rs:136-158, iop/generator.rs:25-106): the generators as data, scheduled once
gb_status gb_circuit_set_generators(gb_circuit* c, const void* generators, uint64_t num_generators, const uint64_t* input_targets,
                                    uint64_t num_inputs, const uint64_t* constants, uint32_t flags) try {
    namespace GN = gbk::gen;
    if (gb_status s = stage_guard(c)) return s;
    gb_ctx* ctx = c->ctx;
    if (flags) return fail(ctx, GB_ERR_INVALID, "gb_circuit_set_generators: unknown bits in flags");
    if (!c->part.set) return fail(ctx, GB_ERR_INVALID, "gb_circuit_set_generators: gb_circuit_set_partition has not been called on this circuit");
    static_assert(sizeof(gb_generator) == sizeof(GN::Record) && offsetof(gb_generator, a) == offsetof(GN::Record, a) &&
                  offsetof(gb_generator, b) == offsetof(GN::Record, b) && offsetof(gb_generator, gate) == offsetof(GN::Record, gate), "gb_generator");
    std::vector<GN::GateDesc> gates(c->gates.num_gates);
    for (u32 i = 0; i < c->gates.num_gates; i++) {
        const gb_gate& gg = c->gates.g[i];
        gates[i] = GN::GateDesc{gg.kind, gg.param, gg.param2, gg.param3};
    }
    GN::CircuitDesc d;
    d.representative_map = c->part.rep_map.data();
    d.num_targets = c->part.num_targets;
    d.num_wires = c->cfg.num_wires;
    d.degree_bits = c->cfg.degree_bits;
    d.num_constants = c->cfg.num_constants;
    d.ext_degree = by_field(c->field, [](auto f) { return (uint32_t)decltype(f)::D; });
    d.order = by_field(c->field, [](auto f) { return (uint64_t)decltype(f)::ORDER; });
    d.slot_reps = c->part.reps.data();
    d.num_slots = c->part.reps.size();
    d.pi_reps = c->part.pi_reps.data();
    d.num_public_inputs = c->part.pi_reps.size();
    d.gates = gates.data();
    d.num_gates = (uint32_t)gates.size();
    d.constants = constants;
    d.programs = &c->gen_programs.host;
    GN::Schedule sched;
    std::string msg;
    if (const int ss = GN::build_schedule(d, static_cast<const GN::Record*>(generators), num_generators, input_targets, num_inputs, GN::GROUP, &sched,
                                          &msg))
        return fail(ctx, (gb_status)ss, "gb_circuit_set_generators: " + msg);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->drop_retry();
    c->drop_generators();
    gb_circuit::Generators& g = c->gens;
    // the inputs that are not the first of their class are compared on the host and left out of the scatter
    std::vector<uint32_t> scatter(sched.input_cls);
    std::vector<uint32_t> per_class(sched.num_classes, 0);
    for (size_t i = 0; i < scatter.size(); i++) {
        per_class[sched.input_cls[i]]++;
        if (sched.input_first[i] != i) scatter[i] = GN::OUT_SKIP;
    }
    g.input_fast.assign(scatter.size(), 0);
    g.input_index.resize(scatter.size());
    for (size_t i = 0; i < scatter.size(); i++) {
        const uint32_t cl = sched.input_cls[i];
        g.input_index[i] = std::make_pair(input_targets[i], (uint32_t)i);
        bool fast = sched.input_free[i] && per_class[cl] == 1 && cl < sched.num_slots && !c->part.is_shared_slot(cl);
        for (uint32_t pc : sched.pi_cls) fast = fast && pc != cl;
        g.input_fast[i] = fast;
    }
    std::sort(g.input_index.begin(), g.input_index.end());
    void* p = nullptr;
    HIP_TRY(ctx, upload_table(sched.ops.data(), sched.ops.size() * sizeof(GN::Op), &p));
    g.ops_dev = static_cast<GN::Op*>(p);
    HIP_TRY(ctx, upload_table(sched.args.data(), sched.args.size() * sizeof(uint32_t), &p));
    g.args_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, upload_table(sched.level_off.data(), sched.level_off.size() * sizeof(uint32_t), &p));
    g.level_off_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, upload_table(scatter.data(), scatter.size() * sizeof(uint32_t), &p));
    g.input_cls_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, upload_table(sched.pi_cls.data(), sched.pi_cls.size() * sizeof(uint32_t), &p));
    g.pi_cls_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, upload_table(nullptr, 0, &p));
    g.err_dev = static_cast<uint32_t*>(p);
    HIP_TRY(ctx, upload_table(sched.row_constants.data(), sched.row_constants.size() * sizeof(uint64_t), &p));
    g.row_constants_dev = static_cast<uint64_t*>(p);
    if (!GN::device_schedule(sched, g.ops_dev, g.args_dev, g.level_off_dev, c->gen_programs.headers_dev, c->gen_programs.instrs_dev,
                             c->gen_programs.lits_dev, g.row_constants_dev, &g.device, &msg)) {
        c->drop_generators();
        return fail(ctx, GB_ERR_HIP, msg);
    }
    std::vector<uint64_t>().swap(sched.row_constants);
    // the kernels read ops and args from the device; the host keeps what it launches and reports with
    std::vector<GN::Op>().swap(sched.ops);
    std::vector<uint32_t>().swap(sched.args);
    g.sched = std::move(sched);
    g.set = true;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

static gb_status schedule_guard(gb_circuit* c) {   // a schedule is set
    if (gb_status s = stage_guard(c)) return s;
    if (!c->part.set || !c->gens.set) return fail(c->ctx, GB_ERR_INVALID, "gb_circuit_set_generators has not been called on this circuit");
    return GB_OK;
}
static gb_status generators_guard(gb_circuit* c, const void* input_values, uint32_t flags,
                                  uint32_t allowed = GB_PUBLIC_INPUT_FLAGS) {   // and these are inputs for it
    if (gb_status s = stage_guard(c)) return s;
    if (flags & ~allowed) return fail(c->ctx, GB_ERR_INVALID, "unknown bits in flags");
    if (flags & GB_INPUT_DEVICE) return fail(c->ctx, GB_ERR_INVALID, "the inputs are a host object: GB_INPUT_DEVICE does not apply");
    if (gb_status s = schedule_guard(c)) return s;
    if (!input_values && !c->gens.sched.input_cls.empty()) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    return GB_OK;
}

// what a host that polls "run N generators" would log (iop/generator.rs:25-30)
gb_status gb_circuit_generators_info(gb_circuit* c, uint32_t* num_levels, uint32_t* num_launches, uint32_t* num_unrunnable,
                                     uint32_t* num_checks, uint32_t* num_classes) try {
    if (gb_status s = schedule_guard(c)) return s;
    const gbk::gen::Schedule& sc = c->gens.sched;
    if (num_levels) *num_levels = sc.num_levels;
    if (num_launches) *num_launches = (uint32_t)sc.launches.size();
    if (num_unrunnable) *num_unrunnable = sc.num_unrunnable;
    if (num_checks) *num_checks = sc.num_checks;
    if (num_classes) *num_classes = sc.num_classes;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// the keys of PartitionWitness.values (iop/witness.rs:318-330) that the generated array holds, in its order
gb_status gb_circuit_generator_classes(gb_circuit* c, uint64_t* class_targets_out, uint64_t capacity) try {
    if (gb_status s = schedule_guard(c)) return s;
    const gbk::gen::Schedule& sc = c->gens.sched;
    if (!class_targets_out || capacity < sc.class_reps.size()) return fail(c->ctx, GB_ERR_INVALID, "class_targets_out holds fewer than num_classes entries");
    for (size_t k = 0; k < sc.class_reps.size(); k++) class_targets_out[k] = sc.class_reps[k];
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// generate_partial_witness (iop/generator.rs:25-106) alone
gb_status gb_generate_partition(gb_circuit* c, const void* input_values, uint32_t flags, void* values_dev_out) try {
    if (gb_status s = generators_guard(c, input_values, flags)) return s;
    if (!values_dev_out) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    return by_field(c, [&](auto* cf) -> gb_status {
        typedef typename std::remove_pointer<decltype(cf)>::type::T T;
        HIP_TRY(c->ctx, hipSetDevice(c->ctx->device));
        TmpAlloc tmp(c->ctx);
        return generate_stage(cf, tmp, input_values, flags, static_cast<T*>(values_dev_out), nullptr);
    });
} GB_CATCH_CIRCUIT(c)

// every gb_prove_partition* / gb_prove_inputs*: the source's guard, the guard of the prove entries, the one front
static gb_status prove_source_entry(gb_circuit* c, WitnessSource src, uint32_t flags, const void* salts, void* proof_out, size_t proof_cap,
                                    size_t* proof_len, const RetryHint* hint = nullptr) {
    if (gb_status s = src.inputs ? generators_guard(c, src.values, flags, GB_PROVE_FLAGS) : partition_guard(c, src.values, flags, GB_PROVE_FLAGS))
        return s;
    if (gb_status s = prove_guard(c, flags, salts, proof_len)) return s;
    return by_field(c, [&](auto* cf) { return prove_from_source(cf, src, flags, salts, proof_out, proof_cap, proof_len, hint); });
}

gb_status gb_prove_partition(gb_circuit* c, const void* values, uint32_t flags, const void* salts, void* proof_out, size_t proof_cap,
                             size_t* proof_len) try {
    return prove_source_entry(c, WitnessSource{values, false}, flags, salts, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_partition_retry(gb_circuit* c, const void* values, uint32_t flags, uint32_t wire, uint64_t row, void* proof_out,
                                   size_t proof_cap, size_t* proof_len) try {
    const RetryHint hint{wire, row};
    return prove_source_entry(c, WitnessSource{values, false}, flags, nullptr, proof_out, proof_cap, proof_len, &hint);
} GB_CATCH_CIRCUIT(c)

// prove() (plonk/prover.rs:136-158): generate_partial_witness, then prove_with_partition_witness
gb_status gb_prove_inputs(gb_circuit* c, const void* input_values, uint32_t flags, const void* salts, void* proof_out,
                          size_t proof_cap, size_t* proof_len) try {
    return prove_source_entry(c, WitnessSource{input_values, true}, flags, salts, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

// the second or third attempt of prove_with_partition_witness's loop (plonk/prover.rs:186-226)
gb_status gb_prove_inputs_retry(gb_circuit* c, const void* input_values, uint32_t flags, uint32_t wire, uint64_t row,
                                void* proof_out, size_t proof_cap, size_t* proof_len) try {
    const RetryHint hint{wire, row};
    return prove_source_entry(c, WitnessSource{input_values, true}, flags, nullptr, proof_out, proof_cap, proof_len, &hint);
} GB_CATCH_CIRCUIT(c)

}  // extern "C"

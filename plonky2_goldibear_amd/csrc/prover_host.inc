// Host orchestration of prove() on one context (included at the end of api.hip).
// Follows internal_prove_with_partition_witness (plonk/prover.rs:228-447) step by step; every
// heavy step is a kernel from kernels_prover.hip / ntt_passes.hpp / kernels_*16.hip / kernels_bb.hip / kernels_merkle.hip, the
// Fiat-Shamir transcript runs on the host (poseidon_gl_host.hpp / poseidon2_bb_host.hpp).
// One template over the field traits (field_traits.hpp) serves Goldilocks and BabyBear: F::T is the device
// form of an element (canonical u64 / Montgomery u32); the transcript and the proof bytes use canonical words
// of the same width.

#include <array>

#include "gates.hpp"
#include "generator_schedule.hpp"
#include "partition_map.hpp"

struct gb_circuit {
    uint32_t field = 0;
    gb_ctx* ctx = nullptr;
    gb_circuit_config cfg{};
    gbk::gates::GateSet gates{};      // CommonCircuitData.gates + selectors_info
    bool general_gates = false;       // false: the dummy gate set, evaluated inside k_quotient
    bool verify_only = false;         // made by gb_verifier_create: no prover state
    uint32_t num_gate_constraints = 0;  // CommonCircuitData.num_gate_constraints (max over the gates)
    // the constraint programs of the GB_GATE_PROGRAM gates (parse_programs): headers, instruction words, literals in device form
    // (one per u64 for either field)
    gbk::gates::ProgramSet programs{};
    std::vector<u64> prog_instrs, prog_lits;
    std::vector<uint32_t> arity_bits;   // FriParams.reduction_arity_bits (ConstantArityBits' list unless set through the ABI)
    // cfg.arity_bits == 0, or a (cfg.arity_bits, cfg.final_poly_bits) on which ConstantArityBits would panic: the circuit's strategy
    // is Fixed / MinSize and its list comes through gb_circuit_set_fri_reduction_arity_bits - until then nothing that needs it runs
    bool arity_pending = false;
    bool test_fail_next_perm_arg = false;   // armed by gb_test_arm_perm_arg_failure (include/goldibear_gpu_test_hooks.h), one shot
    // What a gb_prove* that ended in GB_ERR_PERM_ARG_ZERO leaves for its retry (prove_with_partition_witness's retry loop,
    // plonk/prover.rs:183-226, re-draws ONE wire): the wires commitment, the device-form witness and the leaf sponges' state in
    // front of the last column segment; from a witness front (witness_host.inc) also the canonical matrix that commitment was made
    // from - the "device witness" gb_prove_partition_retry / gb_prove_inputs_retry re-draw one cell of - and, from gb_prove_inputs,
    // the generated public inputs.  One state with one owner: nothing else remembers an attempt.  Held until the next gb_prove* /
    // gb_circuit_free on this circuit (drop_retry).
    struct RetryKeep {
        gb_batch* wires = nullptr;
        void* wit_vals = nullptr;
        size_t wit_bytes = 0;
        size_t wit_mont_cols = 0;   // BabyBear: columns below this are in Montgomery form in wit_vals, the rest canonical (commit())
        SegKeep seg;
        void* matrix = nullptr;     // [num_wires][n] canonical words, a pool block
        size_t matrix_bytes = 0;
        bool by_inputs = false;     // kept by gb_prove_inputs, with these public inputs (a partition attempt's matrix has none:
        std::vector<uint64_t> pis;  // gb_prove_inputs_retry does not build on it, gb_prove_partition_retry builds on either)
    } retry;
    // gb_circuit_set_partition: ProverOnlyCircuitData.representative_map as the slot map of partition_map.hpp - the ascending
    // representatives and the public inputs' on the host, a u32 slot per wire cell on the device - and what gb_prove_partition
    // works with: page-locked staging for the compacted values.
    struct Partition {
        bool set = false;
        std::vector<uint32_t> reps, pi_reps;
        std::vector<uint32_t> rep_map;      // the map itself (targets are below 2^32): gb_circuit_set_generators resolves targets with it
        std::vector<uint64_t> shared;
        uint64_t num_targets = 0;
        uint32_t* slots_dev = nullptr;
        void* staged_host = nullptr;
        size_t staged_host_bytes = 0;
        hipEvent_t staged_read = nullptr;   // recorded behind the upload out of staged_host
        bool is_shared_slot(uint32_t k) const { return (shared[k >> 6] >> (k & 63)) & 1; }
    } part;
    // gb_circuit_set_generators: the schedule of generator_schedule.hpp - its launches, levels and input classes on the host, the
    // ops, operands and level offsets on the device - and the device error word of the generator kernels.
    struct Generators {
        bool set = false;
        gbk::gen::Schedule sched;
        gbk::gen::Op* ops_dev = nullptr;
        uint32_t *args_dev = nullptr, *level_off_dev = nullptr, *input_cls_dev = nullptr, *pi_cls_dev = nullptr, *err_dev = nullptr;
        uint64_t* row_constants_dev = nullptr;   // the constants of the program generators' rows (Schedule::row_constants)
        gbk::gen::DeviceSchedule device{nullptr, nullptr, nullptr};   // of device_schedule(): the arrays above and the program tables
        std::vector<std::pair<uint64_t, uint32_t>> input_index;   // (target, index into input_targets), ascending
        std::vector<uint8_t> input_fast;    // the input may be re-drawn inside a kept matrix (gb_prove_inputs_retry)
    } gens;
    // gb_circuit_set_generator_programs: the checked programs on the host (the schedule reads the headers) and their tables on the
    // device, literals in the field's device form.  A schedule is built on them: replacing them drops it.
    struct GeneratorPrograms {
        gbk::gen::GeneratorPrograms host;
        gbk::gen::ProgramHeader* headers_dev = nullptr;
        uint64_t *instrs_dev = nullptr, *lits_dev = nullptr;
    } gen_programs;
    // gb_check_witness (check_host.inc): what the first check on the circuit builds and later ones reuse - the selector and constant
    // columns as values on H, the row list of every gate - and, per partition, the first cell of every copy class.  Released by
    // gb_circuit_free and gb_ctx_trim (the decoded labels too); the first cells also when gb_circuit_set_partition replaces the map.
    struct Check {
        bool ready = false;
        void* hvals = nullptr;               // [num_selectors + num_constants][n], natural order, device form
        uint32_t* lists_dev = nullptr;       // counts [MAX_LISTS], then offsets [MAX_LISTS + 1]
        uint32_t* rows = nullptr;            // the lists, one behind the other
        std::vector<uint32_t> counts, offsets;   // host copies: [num_gates + 1], [num_gates + 2]
        uint32_t* first_cell = nullptr;      // [number of slots]
        // gb_circuit_decode_sigmas (sigma_host.inc): per wire cell the lowest cell of its cycle under sigma - the copy pass reads
        // them as a slot map whose slots are first cells - and what the call reported; sigma_compared: against the partition set now
        uint32_t* sigma_labels = nullptr;    // [num_wires * n]
        gb_sigma_info sigma_info{};
        bool sigma_compared = false;
    } chk;
    void drop_check_copies() {   // (the caller has waited for the stream)
        if (chk.first_cell) (void)hipFree(chk.first_cell);
        chk.first_cell = nullptr;
        chk.sigma_compared = false;
    }
    void drop_sigma_labels() {   // (the caller has waited for the stream)
        if (chk.sigma_labels) (void)hipFree(chk.sigma_labels);
        chk.sigma_labels = nullptr;
        chk.sigma_info = gb_sigma_info{};
        chk.sigma_compared = false;
    }
    void drop_check() {          // (the caller has waited for the stream)
        drop_check_copies();
        drop_sigma_labels();
        for (void* p : {chk.hvals, (void*)chk.lists_dev, (void*)chk.rows})
            if (p) (void)hipFree(p);
        chk = Check{};
    }
    void drop_generators() {   // (the caller has waited for the stream)
        for (void* p : {(void*)gens.ops_dev, (void*)gens.args_dev, (void*)gens.level_off_dev, (void*)gens.input_cls_dev, (void*)gens.pi_cls_dev,
                        (void*)gens.err_dev, (void*)gens.row_constants_dev})
            if (p) (void)hipFree(p);
        gens = Generators{};
    }
    void drop_generator_programs() {   // (the caller has waited for the stream)
        drop_generators();
        for (void* p : {(void*)gen_programs.headers_dev, (void*)gen_programs.instrs_dev, (void*)gen_programs.lits_dev})
            if (p) (void)hipFree(p);
        gen_programs = GeneratorPrograms{};
    }
    void drop_retry() {
        if (retry.wires) gb_batch_free(retry.wires);
        if (ctx && retry.wit_vals) pool_free(ctx, retry.wit_vals, retry.wit_bytes);
        if (ctx && retry.seg.state) pool_free(ctx, retry.seg.state, retry.seg.bytes);
        if (ctx && retry.matrix) pool_free(ctx, retry.matrix, retry.matrix_bytes);
        retry = RetryKeep{};
    }
    void drop_partition() {   // (the caller has waited for the stream)
        drop_generator_programs();
        drop_check_copies();
        if (part.slots_dev) (void)hipFree(part.slots_dev);
        if (part.staged_host) (void)hipHostFree(part.staged_host);
        if (part.staged_read) (void)hipEventDestroy(part.staged_read);
        part = Partition{};
    }
    void attach(gb_ctx* cx) {
        ctx = cx;
        if (cx) cx->circuits.push_back(this);
    }
    virtual ~gb_circuit() {
        if (ctx) ctx->circuits.erase(std::remove(ctx->circuits.begin(), ctx->circuits.end(), this), ctx->circuits.end());
    }
    virtual void release() = 0;
    virtual void verifier_data(void* cap_out, void* digest_out) = 0;
};

// ---------------------------------------------------------------------------------------------- constraint programs
// The program table of gb_circuit_create_programs / gb_verifier_create_programs, decoded and checked (include/goldibear_gpu.h
// gives the words and the list of what is refused).  Host only; this is the code that reads untrusted input: every length is
// checked against the offsets before a word is read, and after it returns run_program needs no check of its own.
struct ProgramTable {   // the three program arguments of the ABI
    const uint64_t* words;
    const uint32_t* offsets;
    uint32_t num_programs;
};
struct ParsedPrograms {
    gbk::gates::ProgramSet set{};
    std::vector<u64> instrs, lits;
    void move_to(gb_circuit* c) {   // the circuit is the tables' one owner from here on
        c->programs = set;
        c->prog_instrs = std::move(instrs);
        c->prog_lits = std::move(lits);
    }
};
template <class F>
static gb_status parse_programs(gb_ctx* ctx, const gb_circuit_config* cfg, const uint64_t* words, const uint32_t* offsets,
                                uint32_t num_programs, ParsedPrograms* out) {
    namespace G = gbk::gates;
    *out = ParsedPrograms{};
    if (num_programs == 0) return GB_OK;
    if (num_programs > G::MAX_PROGRAMS)
        return fail(ctx, GB_ERR_INVALID, "more than " + std::to_string(G::MAX_PROGRAMS) + " constraint programs");
    if (!words || !offsets) return fail(ctx, GB_ERR_INVALID, "null program table");
    if (offsets[0] != 0) return fail(ctx, GB_ERR_INVALID, "program_offsets[0] is not 0");
    constexpr u64 ORDER = F::ORDER_BITS == 64 ? 0xFFFFFFFF00000001ull : 2013265921ull;
    // a program is at most a header, MAX_PROGRAM_LITERALS literals and MAX_PROGRAM_INSTRS instructions long
    constexpr u32 MAX_WORDS = G::PROGRAM_HEADER_WORDS + G::MAX_PROGRAM_LITERALS + G::MAX_PROGRAM_INSTRS;
    for (u32 pi = 0; pi < num_programs; pi++) {
        const std::string name = "program " + std::to_string(pi);
        if (offsets[pi + 1] < offsets[pi]) return fail(ctx, GB_ERR_INVALID, name + ": program_offsets are not ascending");
        const u32 len = offsets[pi + 1] - offsets[pi];
        if (len < G::PROGRAM_HEADER_WORDS || len > MAX_WORDS)
            return fail(ctx, GB_ERR_INVALID, name + ": " + std::to_string(len) + " words is no program (header " +
                        std::to_string(G::PROGRAM_HEADER_WORDS) + ", at most " + std::to_string(MAX_WORDS) + ")");
        const uint64_t* w = words + offsets[pi];
        G::ProgramInfo h{};
        h.num_wires = (u32)w[0]; h.num_constants = (u32)(w[0] >> 32);
        h.num_constraints = (u32)w[1]; h.degree = (u32)(w[1] >> 32);
        h.num_regs = (u32)w[2]; h.num_literals = (u32)(w[2] >> 32);
        h.num_instrs = (u32)w[3];
        if ((w[3] >> 32) != 0) return fail(ctx, GB_ERR_INVALID, name + ": header word 3 has bits above num_instrs");
        if (h.num_instrs > G::MAX_PROGRAM_INSTRS || h.num_regs > G::MAX_PROGRAM_REGS || h.num_literals > G::MAX_PROGRAM_LITERALS ||
            h.num_constraints > G::MAX_PROGRAM_CONSTRAINTS)
            return fail(ctx, GB_ERR_INVALID, name + ": header over the limits (" + std::to_string(h.num_instrs) + " instructions / " +
                        std::to_string(h.num_regs) + " registers / " + std::to_string(h.num_literals) + " literals / " +
                        std::to_string(h.num_constraints) + " constraints; at most 4096 / 32 / 256 / 1024)");
        if (len != G::PROGRAM_HEADER_WORDS + h.num_literals + h.num_instrs)
            return fail(ctx, GB_ERR_INVALID, name + ": the header describes " +
                        std::to_string(G::PROGRAM_HEADER_WORDS + h.num_literals + h.num_instrs) + " words, the table holds " + std::to_string(len));
        if (h.num_wires > cfg->num_wires || h.num_constants > cfg->num_constants)
            return fail(ctx, GB_ERR_INVALID, name + " needs " + std::to_string(h.num_wires) + " wires / " + std::to_string(h.num_constants) +
                        " constants, the config has " + std::to_string(cfg->num_wires) + " / " + std::to_string(cfg->num_constants));
        h.lit_off = (u32)out->lits.size();
        h.instr_off = (u32)out->instrs.size();
        for (u32 i = 0; i < h.num_literals; i++) {
            const u64 v = w[G::PROGRAM_HEADER_WORDS + i];
            if (v >= ORDER) return fail(ctx, GB_ERR_INVALID, name + ": literal " + std::to_string(i) + " is not canonical");
            out->lits.push_back((u64)F::enc((typename F::T)v));
        }
        // one pass: which registers are written, and the degree bound of what each holds
        u32 reg_deg[G::MAX_PROGRAM_REGS];
        bool written[G::MAX_PROGRAM_REGS] = {};
        u32 emits = 0;
        const uint64_t* ins = w + G::PROGRAM_HEADER_WORDS + h.num_literals;
        for (u32 pc = 0; pc < h.num_instrs; pc++) {
            const u64 iw = ins[pc];
            const std::string at = name + " instruction " + std::to_string(pc);
            if (iw >> 56) return fail(ctx, GB_ERR_INVALID, at + ": bits 56-63 are not zero");
            const u32 op = G::prog_op(iw), dst = G::prog_dst(iw);
            u32 deg[2] = {0, 0};
            const u32 nops = op == G::PROG_EMIT ? 1 : 2;
            for (u32 k = 0; k < nops; k++) {
                const u32 o = G::prog_operand(iw, k), idx = G::prog_index(o);
                switch (G::prog_space(o)) {
                    case G::PROG_REG:
                        if (idx >= h.num_regs) return fail(ctx, GB_ERR_INVALID, at + ": register " + std::to_string(idx) + " of " + std::to_string(h.num_regs));
                        if (!written[idx]) return fail(ctx, GB_ERR_INVALID, at + ": register " + std::to_string(idx) + " is read before it is written");
                        deg[k] = reg_deg[idx];
                        break;
                    case G::PROG_WIRE:
                        if (idx >= h.num_wires) return fail(ctx, GB_ERR_INVALID, at + ": wire " + std::to_string(idx) + " of " + std::to_string(h.num_wires));
                        deg[k] = 1;
                        break;
                    case G::PROG_CONST:
                        if (idx >= h.num_constants) return fail(ctx, GB_ERR_INVALID, at + ": constant " + std::to_string(idx) + " of " + std::to_string(h.num_constants));
                        deg[k] = 1;
                        break;
                    default:
                        if (idx >= h.num_literals) return fail(ctx, GB_ERR_INVALID, at + ": literal " + std::to_string(idx) + " of " + std::to_string(h.num_literals));
                        break;
                }
            }
            if (op == G::PROG_EMIT) {
                if (dst != 0 || G::prog_operand(iw, 1) != 0) return fail(ctx, GB_ERR_INVALID, at + ": EMIT with a destination or a second operand");
                if (deg[0] > h.degree)
                    return fail(ctx, GB_ERR_INVALID, at + ": constraint " + std::to_string(emits) + " has degree bound " + std::to_string(deg[0]) +
                                ", the program declares " + std::to_string(h.degree));
                emits++;
                out->instrs.push_back(iw);
                continue;
            }
            if (dst >= h.num_regs) return fail(ctx, GB_ERR_INVALID, at + ": register " + std::to_string(dst) + " of " + std::to_string(h.num_regs));
            // (a bound past any quotient degree factor is clamped: 4096 products of it cannot wrap a u32)
            const u32 d = op == G::PROG_MUL ? deg[0] + deg[1] : std::max(deg[0], deg[1]);
            reg_deg[dst] = std::min(d, 1u << 16);
            written[dst] = true;
            out->instrs.push_back(iw);
        }
        if (emits != h.num_constraints)
            return fail(ctx, GB_ERR_INVALID, name + ": " + std::to_string(emits) + " EMITs, the header declares " +
                        std::to_string(h.num_constraints) + " constraints");
        out->set.p[pi] = h;
        out->set.max_regs = std::max(out->set.max_regs, h.num_regs);
    }
    out->set.num_programs = num_programs;
    return GB_OK;
}

// A FriParams.reduction_arity_bits list for oracles of this shape: what gb_circuit_set_fri_reduction_arity_bits,
// gb_fri_prove_openings and gb_fri_verify accept (the empty list included)
static gb_status check_fri_reduction_arity_bits(gb_ctx* ctx, u32 degree_bits, u32 rate_bits, u32 cap_height, const uint32_t* arity_bits,
                                                uint32_t num_layers) {
    if (num_layers && !arity_bits) return fail(ctx, GB_ERR_INVALID, "null arity_bits");
    if (num_layers > GB_MAX_FRI_LAYERS) return fail(ctx, GB_ERR_INVALID, "more than GB_MAX_FRI_LAYERS FRI reduction layers");
    const u32 max_ab = 8u;   // a FRI leaf is 2^arity_bits extension elements; the proof format's u8 counts and the verifier stop at 2^8
    u32 db = degree_bits;
    for (u32 i = 0; i < num_layers; i++) {
        const u32 ab = arity_bits[i];
        if (ab == 0 || ab > max_ab) return fail(ctx, GB_ERR_INVALID, "FRI reduction arity outside the supported range");
        if (ab > db) return fail(ctx, GB_ERR_INVALID, "FRI reduction arities sum past degree_bits");
        if (db + rate_bits < cap_height + ab)
            return fail(ctx, GB_ERR_INVALID, "cap_height should be at most log2(leaves.len()) in a FRI layer (merkle_tree.rs:154-157)");
        db -= ab;
    }
    return GB_OK;
}
static gb_status need_arity_list(gb_circuit* c) {
    if (c && c->arity_pending)
        return fail(c->ctx, GB_ERR_INVALID, "no FRI reduction list: ConstantArityBits(arity_bits, final_poly_bits) is not defined for this circuit "
                                            "(fri/reduction_strategies.rs:45) - hand its list over with gb_circuit_set_fri_reduction_arity_bits");
    return GB_OK;
}
static void drop_all_retry_state(gb_ctx* ctx) {
    for (gb_circuit* c : ctx->circuits) c->drop_retry();
}
static void drop_all_check_state(gb_ctx* ctx) {   // gb_ctx_trim (the caller has waited for the stream)
    for (gb_circuit* c : ctx->circuits) c->drop_check();
}
// the catch-all of the entry points that take a circuit: what an interrupted attempt may have kept for gb_prove_retry goes too
static gb_status unwound_circuit(gb_circuit* c, const char* fn) noexcept {
    if (c) {
        try { c->drop_retry(); } catch (...) {}
    }
    return unwound(c ? c->ctx : nullptr, fn);
}
#define GB_CATCH_CIRCUIT(C) catch (...) { return unwound_circuit((C), __func__); }

namespace {

// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) (fri/reduction_strategies.rs:39-50).  false = the
// configuration on which the reference panics there: `assert!(degree_bits >= arity_bits)` inside the loop (an arity that does not
// fit what is left of the degree), or the usize underflow of `degree_bits + rate_bits - arity_bits`.
static inline bool constant_arity_bits(const gb_circuit_config& cfg, std::vector<uint32_t>* out) {
    out->clear();
    if (cfg.arity_bits == 0) return false;
    uint32_t db = cfg.degree_bits;
    while (db > cfg.final_poly_bits) {
        if (db + cfg.rate_bits < cfg.arity_bits) return false;
        if (db + cfg.rate_bits - cfg.arity_bits < cfg.cap_height) break;
        if (db < cfg.arity_bits) return false;
        out->push_back(cfg.arity_bits);
        db -= cfg.arity_bits;
    }
    return true;
}

// log2_ceil(quotient_degree_factor) (plonk/prover.rs:735); the factor is a power of two here (check_circuit_cfg)
static inline u32 quotient_degree_bits(const gb_circuit_config& cfg) {
    u32 qb = 0;
    while ((1u << qb) < cfg.max_quotient_degree_factor) qb++;
    return qb;
}

// what the stages derive from a circuit's config (prover.rs:305-376: partial products per challenge, quotient chunks)
struct Counts {
    u32 lg, nchunks, num_prods;
    size_t n, N, nzs, nq;
    explicit Counts(const gb_circuit_config& cfg)
        : lg(cfg.degree_bits), nchunks((cfg.num_routed_wires + cfg.max_quotient_degree_factor - 1) / cfg.max_quotient_degree_factor),
          num_prods(nchunks - 1), n((size_t)1 << lg), N(n << cfg.rate_bits), nzs((size_t)cfg.num_challenges * nchunks),
          nq((size_t)cfg.num_challenges * cfg.max_quotient_degree_factor) {}
};

template <class F>
struct Circuit : gb_circuit {
    typedef typename F::T T;
    gb_batch* cs = nullptr;        // constants || sigmas commitment (device resident for every proof)
    T* sigma_vals = nullptr;       // [routed][n] sigma values on H_n, device form (ProverOnlyCircuitData.sigmas)
    T* k_is = nullptr;             // [routed], device form
    std::vector<T> k_is_dev_host;  // device form, host copy
    std::vector<T> cap_host;       // canonical
    T digest[F::H] = {};           // canonical
    T *wn_lo = nullptr, *wn_hi = nullptr, *wN_lo = nullptr, *wN_hi = nullptr, *combine_mat = nullptr;
    T* l0 = nullptr;               // [n 2^qb] L_0 on the quotient domain, leaf order (eval_l_0, zero_poly_coset.rs:58-61)
    std::vector<T> zh, zh_inv;     // ZeroPolyOnCoset (field/src/zero_poly_coset.rs:22-37), device form
    u32* perm_err = nullptr;       // set by the partial-products kernel on a zero denominator; zero otherwise
    u64* prog_instrs_dev = nullptr;   // the constraint programs' instruction words and literals (device form), device copies
    T* prog_lits_dev = nullptr;
    std::vector<void*> owned;
    void release() override {
        if (cs) gb_batch_free(cs);
        if (sigma_vals) (void)hipFree(sigma_vals);
        for (void* p : owned) (void)hipFree(p);
        cs = nullptr; sigma_vals = nullptr; owned.clear();
    }
    void verifier_data(void* cap_out, void* digest_out) override {
        if (cap_out) std::memcpy(cap_out, cap_host.data(), cap_host.size() * sizeof(T));
        if (digest_out) std::memcpy(digest_out, digest, sizeof digest);
    }
};

// One call for either field (the tag is GB_GOLDILOCKS or GB_BABYBEAR: the entries check it).  fn is a generic lambda: by tag it
// gets the traits as a value, `[&](auto f) { typedef decltype(f) F; ... }`; by circuit it gets the circuit as its Circuit<F>*, and
// the templates it calls deduce F from that
template <class Fn>
auto by_field(uint32_t field, Fn&& fn) -> decltype(fn(GlF{})) {
    return field == GB_GOLDILOCKS ? fn(GlF{}) : fn(BbF{});
}
template <class Fn>
auto by_field(gb_circuit* c, Fn&& fn) -> decltype(fn(static_cast<Circuit<GlF>*>(c))) {
    return c->field == GB_GOLDILOCKS ? fn(static_cast<Circuit<GlF>*>(c)) : fn(static_cast<Circuit<BbF>*>(c));
}

struct TmpAlloc {  // pooled temporaries released together
    gb_ctx* ctx;
    std::vector<std::pair<void*, size_t>> blocks;
    std::vector<std::shared_ptr<void>> host_keep;  // sources of uploads still in flight (upload_tmp)
    explicit TmpAlloc(gb_ctx* c) : ctx(c) {}
    ~TmpAlloc() {
        if (!host_keep.empty()) (void)hipStreamSynchronize(ctx->stream);  // an early return may leave copies pending
        for (auto& b : blocks) pool_free(ctx, b.first, b.second);
    }
    template <typename T>
    T* get(size_t count) {
        void* p = nullptr;
        size_t bytes = (count ? count : 1) * sizeof(T);
        if (pool_alloc(ctx, bytes, &p) != hipSuccess) return nullptr;
        blocks.emplace_back(p, bytes);
        return static_cast<T*>(p);
    }
};

struct Bytes {
    uint8_t* p;
    size_t len = 0, cap;
    Bytes(void* out, size_t c) : p(static_cast<uint8_t*>(out)), cap(c) {}
    void put(const void* src, size_t n) {
        if (p && len + n <= cap) std::memcpy(p + len, src, n);
        len += n;
    }
    void u64v(u64 x) { put(&x, 8); }
    void u8v(uint8_t x) { put(&x, 1); }
};

template <class F>
std::vector<typename F::T> fpowers(typename F::T base, size_t count) {  // device form
    std::vector<typename F::T> v(count);
    typename F::T x = F::one();
    for (size_t i = 0; i < count; i++) {
        v[i] = x;
        x = F::mul(x, base);
    }
    return v;
}

// Small host table -> device, without draining the stream: the source is kept alive by `tmp` until the proof is done (every
// proof ends on a synchronised read-back), so the host can keep enqueueing behind a dozen of these per proof.
template <typename V>
gb_status upload_tmp(gb_ctx* ctx, TmpAlloc& tmp, std::vector<V> host, V** dev) {
    V* d = tmp.get<V>(host.size());
    if (!d) return fail(ctx, GB_ERR_OOM, "tmp alloc");
    const size_t bytes = host.size() * sizeof(V);
    if (void* stage = stage_up(ctx, bytes)) {   // through the context's page-locked arena: an asynchronous copy
        std::memcpy(stage, host.data(), bytes);
        HIP_TRY(ctx, hipMemcpyAsync(d, stage, bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        auto keep = std::make_shared<std::vector<V>>(std::move(host));
        tmp.host_keep.push_back(keep);
        HIP_TRY(ctx, hipMemcpyAsync(d, keep->data(), keep->size() * sizeof(V), hipMemcpyHostToDevice, ctx->stream));
    }
    *dev = d;
    return GB_OK;
}
template <typename V>
gb_status upload_owned(gb_ctx* ctx, const std::vector<V>& host, V** dev, std::vector<void*>* owned) {
    void* p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, host.size() * sizeof(V)));
    HIP_TRY(ctx, hipMemcpy(p, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice));
    *dev = static_cast<V*>(p);
    owned->push_back(p);
    return GB_OK;
}

// split power tables z^e = lo[e & 1023] * hi[e >> 10] of `count` (<= 5) points on the device (pooled), one launch; with `plain`
// non-null also the plain list z^0 .. z^(nplain - 1) of one more point
template <class F>
gb_status make_ext_powtabs(gb_ctx* ctx, TmpAlloc& tmp, u32 count, const typename F::E* z, const size_t* n, gbk::ExtPowTab<F>** out,
                           const typename F::E* plain_z = nullptr, size_t nplain = 0, typename F::E** plain = nullptr) {
    typedef typename F::E E;
    gbk::ExtPowJobs<F> jobs{};
    u32 nj = 0;
    for (u32 i = 0; i < count; i++, nj++) {
        const size_t nhi = n[i] > 1024 ? n[i] / 1024 : 1;
        E* dlo = tmp.get<E>(1024);
        E* dhi = tmp.get<E>(nhi);
        if (!dlo || !dhi) return fail(ctx, GB_ERR_OOM, "tmp alloc");
        jobs.j[nj] = gbk::ExtPowJob<F>{z[i], dlo, dhi, 1024u, (u32)nhi};
        out[i]->lo = dlo; out[i]->hi = dhi; out[i]->lo_bits = 10;
    }
    if (plain) {
        E* d = tmp.get<E>(nplain ? nplain : 1);
        if (!d) return fail(ctx, GB_ERR_OOM, "tmp alloc");
        jobs.j[nj++] = gbk::ExtPowJob<F>{*plain_z, d, nullptr, (u32)nplain, 0u};
        *plain = d;
    }
    gbk::ext_powtabs<F>(jobs, nj, ctx->stream);   // built on the device: no host products, no uploads
    return GB_OK;
}
template <class F>
gb_status make_ext_powtab(gb_ctx* ctx, TmpAlloc& tmp, typename F::E z, size_t n, gbk::ExtPowTab<F>* out) {
    return make_ext_powtabs<F>(ctx, tmp, 1, &z, &n, &out);
}

template <class F>
gb_status read_cap(gb_batch* b, std::vector<typename F::T>& cap) {
    cap.resize((size_t)F::H << b->cap_height);
    return gb_batch_cap(b, cap.data());
}

// What a quotient on the first 2^qb coset blocks of size-n LDEs needs, in device form (circuit_create for the PLONK quotient,
// gb_constraint_quotient for any other): Z_H and 1 / Z_H on the cosets, and the combine matrix of the coset_ifft's last step.
template <class F>
void quotient_domain_tables(u32 lg, u32 qb, std::vector<typename F::T>* zh, std::vector<typename F::T>* zh_inv, std::vector<typename F::T>* mat) {
    typedef typename F::T T;
    // ZeroPolyOnCoset::new(degree_bits, quotient_degree_bits): Z_H(g w_Q^i) = g^n w_R^(i mod R) - 1, R = 2^qb
    const u32 R = 1u << qb;
    const size_t n = (size_t)1 << lg;
    T g_pow_n = F::pow(F::generator(), n), wR = F::two_adic_generator(qb), x = F::one();
    for (u32 i = 0; i < R; i++) {
        T v = F::sub(F::mul(g_pow_n, x), F::one());
        zh->push_back(v);
        zh_inv->push_back(F::inv(v));
        x = F::mul(x, wR);
    }
    // combine matrix: mat[m][c] = g^(-n m) / R * zeta_c^(-m), zeta_c = w_R^bitrev_r(c)
    mat->assign((size_t)R * R, F::zero());
    T g_inv = F::inv(g_pow_n), r_inv = F::inv(F::enc(R));
    for (u32 m = 0; m < R; m++)
        for (u32 cc = 0; cc < R; cc++) {
            T zeta = F::pow(wR, bitrev32(cc, qb));
            (*mat)[m * R + cc] = F::mul(F::mul(F::pow(g_inv, m), r_inv), F::pow(F::inv(zeta), m));
        }
}

// ---------------------------------------------------------------------------------------------- build()
template <class F>
gb_status circuit_create(gb_ctx* ctx, const gb_circuit_config* cfg, const gbk::gates::GateSet& gset, bool general,
                         ColSrc constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out,
                         ParsedPrograms* progs = nullptr) {
    typedef typename F::T T;
    typedef Host<F> HF;
    constexpr u32 H = F::H;
    const u32 lg = cfg->degree_bits, r = cfg->rate_bits;
    // the security asserts of circuit_builder.rs:1187-1192
    if (F::D * F::ORDER_BITS < lg + 100)
        return fail(ctx, GB_ERR_INVALID, "The degree of the extension is not enough for the soundness of the evaluation point");
    if ((F::ORDER_BITS - lg) * cfg->num_challenges < 100)
        return fail(ctx, GB_ERR_INVALID, "num_challenges is not sufficient for the soundness of the permutation argument (circuit_builder.rs:1191-1192)");
    if (lg + r > F::TWO_ADICITY) return fail(ctx, GB_ERR_INVALID, "LDE size exceeds the field's two-adicity");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    Circuit<F>* c = new (std::nothrow) Circuit<F>();
    if (!c) return fail(ctx, GB_ERR_OOM, "host allocation failed");
    c->field = F::TAG;
    c->attach(ctx);
    c->cfg = *cfg;
    c->gates = gset;
    c->general_gates = general;
    if (progs) progs->move_to(c);
    for (u32 g = 0; g < gset.num_gates; g++)
        c->num_gate_constraints = std::max(c->num_gate_constraints, gbk::gates::num_constraints<F>(gset.g[g], c->programs));
    auto cleanup = [&](gb_status s) { gb_circuit_free(c); return s; };
    const size_t n = (size_t)1 << lg;
    const size_t ncs = cfg->num_selectors + cfg->num_constants + cfg->num_routed_wires;
    gb_status s;
    // constants_sigmas_commitment (circuit_builder.rs:1230-1239), blinding = false
    if ((s = commit<F>(ctx, constants_sigmas, ncs, lg, r, cfg->cap_height, nullptr, flags, false, &c->cs)))
        return cleanup((flags & GB_INPUT_DEVICE) ? s : finish_host_commit(ctx, s, nullptr));   // no copy from the caller's buffer left in flight
    // sigma values stay resident for the Z computation (ProverOnlyCircuitData.sigmas)
    void* p = nullptr;
    const size_t sig_count = (size_t)cfg->num_routed_wires * n;
    if (hipMalloc(&p, sig_count * sizeof(T)) != hipSuccess) return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc sigma"));
    c->sigma_vals = (T*)p;
    const size_t first_sigma = cfg->num_selectors + cfg->num_constants;
    const ColSrc sig_src = constants_sigmas.ptrs ? ColSrc::columns(constants_sigmas.ptrs + first_sigma)
                                                 : ColSrc(static_cast<const T*>(constants_sigmas.base) + first_sigma * n);
    if (!copy_columns(sig_src, cfg->num_routed_wires, n * sizeof(T), c->sigma_vals,
                      (flags & GB_INPUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream))
        return cleanup(fail(ctx, GB_ERR_HIP, "copy of sigma values failed"));
    if (flags & GB_INPUT_P3_REPR) gbk::reduce_words<F>(c->sigma_vals, sig_count, ctx->stream);   // the field types' in-memory words
    else HF::to_device_form(c->sigma_vals, c->sigma_vals, sig_count, ctx->stream);
    std::vector<T> k_canon(cfg->num_routed_wires);
    if (flags & GB_INPUT_DEVICE) {
        if (hipMemcpy(k_canon.data(), k_is, k_canon.size() * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)
            return cleanup(fail(ctx, GB_ERR_HIP, "copy of k_is failed"));
    } else {
        std::memcpy(k_canon.data(), k_is, k_canon.size() * sizeof(T));
    }
    if (flags & GB_INPUT_P3_REPR)
        for (T& k : k_canon) k = (T)HF::p3_to_canonical(k);
    for (T k : k_canon) c->k_is_dev_host.push_back(F::enc(k));
    if ((s = upload_owned(ctx, c->k_is_dev_host, &c->k_is, &c->owned))) return cleanup(s);
    if ((s = upload_owned(ctx, std::vector<u32>(1, 0u), &c->perm_err, &c->owned))) return cleanup(s);
    if (c->programs.num_programs) {   // the tables k_gate_programs reads (an empty table still gets a valid one-word allocation)
        std::vector<T> lits(c->prog_lits.begin(), c->prog_lits.end());
        if (lits.empty()) lits.push_back(F::zero());
        const std::vector<u64> no_instrs(1, 0);
        if ((s = upload_owned(ctx, c->prog_instrs.empty() ? no_instrs : c->prog_instrs, &c->prog_instrs_dev, &c->owned))) return cleanup(s);
        if ((s = upload_owned(ctx, lits, &c->prog_lits_dev, &c->owned))) return cleanup(s);
    }
    // compute_quotient_polys works on every step-th point of the LDE, step = 2^(rate_bits - quotient_degree_bits)
    // (plonk/prover.rs:735-749): in leaf order those are the first 2^qb coset blocks of a column, so everything the quotient stage
    // needs - domain powers, Z_H on the cosets, L_0, the combine matrix of the coset_ifft - is the rate-qb table
    const u32 qb = quotient_degree_bits(*cfg);
    // subgroup / quotient-domain power tables
    {
        T wn = F::two_adic_generator(lg), wN = F::two_adic_generator(lg + qb);
        size_t nhi_n = n > 4096 ? n / 4096 : 1, nhi_N = (n << qb) > 4096 ? (n << qb) / 4096 : 1;
        if ((s = upload_owned(ctx, fpowers<F>(wn, 4096), &c->wn_lo, &c->owned))) return cleanup(s);
        if ((s = upload_owned(ctx, fpowers<F>(F::pow(wn, 4096), nhi_n), &c->wn_hi, &c->owned))) return cleanup(s);
        if ((s = upload_owned(ctx, fpowers<F>(wN, 4096), &c->wN_lo, &c->owned))) return cleanup(s);
        if ((s = upload_owned(ctx, fpowers<F>(F::pow(wN, 4096), nhi_N), &c->wN_hi, &c->owned))) return cleanup(s);
    }
    {
        std::vector<T> mat;
        quotient_domain_tables<F>(lg, qb, &c->zh, &c->zh_inv, &mat);
        if ((s = upload_owned(ctx, mat, &c->combine_mat, &c->owned))) return cleanup(s);
        // L_0 table for the quotient kernel
        T* zh_dev;
        if ((s = upload_owned(ctx, c->zh, &zh_dev, &c->owned))) return cleanup(s);
        void* lp = nullptr;
        if (hipMalloc(&lp, (n << qb) * sizeof(T)) != hipSuccess) return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc L_0 table"));
        c->owned.push_back(lp);
        c->l0 = (T*)lp;
        gbk::l0_table<F>(lg, qb, gbk::PowTab<F>{c->wN_lo, c->wN_hi, 12}, zh_dev, c->l0, ctx->stream);
    }
    // FriReductionStrategy::ConstantArityBits (fri/reduction_strategies.rs:39-50); a circuit with another strategy replaces the list
    // (where ConstantArityBits would panic the list is left open - ADVICE r5: such a circuit carries a Fixed / MinSize list)
    if (!constant_arity_bits(*cfg, &c->arity_bits)) { c->arity_bits.clear(); c->arity_pending = true; }
    // circuit_digest = hash_no_pad(cap.flatten() || hash_pad([]) || [degree_bits]) (circuit_builder.rs:1300-1312)
    if ((s = read_cap<F>(c->cs, c->cap_host))) return cleanup(s);
    {
        std::vector<T> parts(c->cap_host);
        T pad[8] = {1, 0, 0, 0, 0, 0, 0, 1}, dom[H];  // hash_pad of the empty separator (plonk/config.rs:58-66), rate 8
        HF::hash_no_pad(pad, 8, dom);
        parts.insert(parts.end(), dom, dom + H);
        parts.push_back((T)lg);
        HF::hash_no_pad(parts.data(), parts.size(), c->digest);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = c;
    return GB_OK;
}

// fri_proof_of_work (fri/prover.rs:136-188): the MINIMUM candidate whose duplex response has >= min_lz leading zeros
template <class F>
gb_status pow_search(gb_ctx* ctx, u64* res /* a device word the caller has already filled with 0xFF bytes */, const gbk::PowState<F>& ps,
                     u32 min_lz, u64* nonce) {
    hipStream_t st = ctx->stream;
    const u64 none = ~0ull;
    const u64 limit = F::ORDER_BITS == 64 ? ((u64)1 << 40) : (((u64)1 << 31) - ((u64)1 << 27) + 1);  // candidates are field elements
    // A candidate passes with probability 2^-bits (bits = proof_of_work_bits): the first batch is 4 x 2^bits candidates (98 %
    // of the proofs end there; at 16 bits that is one wave per SIMD instead of sixteen), later ones 2^20.  Batches ascend and
    // each returns its minimum, so the result is the minimum valid nonce whatever the batch sizes.
    const u32 bits = min_lz - (64 - F::ORDER_BITS);
    u64 batch = std::min<u64>((u64)1 << 20, std::max<u64>((u64)1 << 12, (u64)4 << std::min(bits, 30u)));
    u64 found = none;
    for (u64 start = 0; found == none; start += batch, batch = (u64)1 << 20) {
        if (start >= limit) return fail(ctx, GB_ERR_HIP, "Proof of work failed. This is highly unlikely!");
        if (start) HIP_TRY(ctx, hipMemsetAsync(res, 0xFF, 8, st));   // `none` again (the first batch finds the caller's fill)
        gbk::pow_grind<F>(ps, start, std::min(batch, limit - start), min_lz, res, st);
        if (gb_status rs = read_back(ctx, &found, res, 8)) return rs;
    }
    *nonce = found;
    return GB_OK;
}

// ---------------------------------------------------------------------------------------------- the stages of prove()
// Each stage is also an entry point of the C ABI (gb_zs_partial_products, gb_quotient_polys, gb_prove_openings) for a host that
// keeps the reference's prover loop and its Challenger (SURVEY.md 8(b)).

// Has the partial-products kernel met a zero denominator?  One read-back - together with `also` (the next commitment's cap) when the
// caller has deferred the question to there.
template <class F>
gb_status perm_arg_check(Circuit<F>* c, void* also_host, size_t also_bytes, const void* also_dev) {
    gb_ctx* ctx = c->ctx;
    u32 herr = 0;
    ReadBack rb(ctx);
    if (also_bytes) if (gb_status rs = rb.add(also_host, also_dev, also_bytes)) return rs;
    if (gb_status rs = rb.add(&herr, c->perm_err, 4)) return rs;
    if (gb_status rs = rb.finish()) return rs;
    if (herr) {
        HIP_TRY(ctx, hipMemsetAsync(c->perm_err, 0, 4, ctx->stream));
        return fail(ctx, GB_ERR_PERM_ARG_ZERO, "permutation argument division by zero (ProverError::InvZeroPermArg)");
    }
    return GB_OK;
}

// wires_permutation_partial_products_and_zs + all_wires_permutation_partial_products (plonk/prover.rs:449-546).
// wit_dev: the routed wire VALUES [>= num_routed][n] in device form; out: [nch * (1 + num_prods)][n] values in device form, in
// the order prover.rs:318-329 commits them (all Zs, then each challenge's partial products); GB_ERR_PERM_ARG_ZERO = InvZeroPermArg.
template <class F>
gb_status stage_zs_partial_products(Circuit<F>* c, TmpAlloc& tmp, const typename F::T* wit_dev, const std::vector<typename F::T>& betas_d,
                                    const std::vector<typename F::T>& gammas_d, typename F::T** zs_vals_out, bool defer_check = false) {
    typedef typename F::T T;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, nch = cfg.num_challenges, nr = cfg.num_routed_wires, qdf = cfg.max_quotient_degree_factor;
    const Counts cnt(cfg);
    const u32 nchunks = cnt.nchunks;
    const size_t n = cnt.n, nzs = cnt.nzs;
    hipStream_t st = ctx->stream;
    gbk::ZsParams<F> zp{lg, nr, nch, qdf, nchunks, gbk::PowTab<F>{c->wn_lo, c->wn_hi, 12}, {}, {}};
    std::copy(betas_d.begin(), betas_d.end(), zp.betas);
    std::copy(gammas_d.begin(), gammas_d.end(), zp.gammas);
    const u32 nb1024 = (u32)((n + 1023) / 1024);
    T* q_tmp = tmp.get<T>((size_t)nch * nchunks * n);
    T* zloc = tmp.get<T>((size_t)nch * n);
    T* totals = tmp.get<T>((size_t)nch * nb1024);
    T* zs_vals = tmp.get<T>(nzs * n);
    if (!q_tmp || !zloc || !totals || !zs_vals) return fail(ctx, GB_ERR_OOM, "partial products workspace");
    // c->perm_err: the circuit's own word, zero between proofs - a kernel sets it on a zero denominator, the host clears it again
    gbk::zs_partial_products<F>(zp, wit_dev, c->sigma_vals, c->k_is, q_tmp, zloc, totals, c->perm_err, zs_vals, st);
    *zs_vals_out = zs_vals;
    return defer_check ? GB_OK : perm_arg_check<F>(c, nullptr, 0, nullptr);
}

// The tail of a quotient stage: coset_ifft of size n 2^qb (prover.rs:921-925) = per-coset size-n inverse NTTs + radix-2^qb combine,
// which leaves the degree-n chunks.  qv: [nch 2^qb][n] quotient values as the quotient kernels store them; qc: workspace of the same
// size; combine_mat: quotient_domain_tables' matrix on the device; `scope`: the timing scope of the transforms (a scope of its
// own: not a commitment's transform).
template <class F>
gb_status quotient_coset_ifft(gb_ctx* ctx, u32 lg, u32 qb, u32 nch, const typename F::T* qv, typename F::T* qc,
                              const typename F::T* combine_mat, typename F::T* chunks, const char* scope) {
    typedef typename F::T T;
    typedef Host<F> HF;
    const size_t n = (size_t)1 << lg, nq = (size_t)nch << qb;
    hipStream_t st = ctx->stream;
    gb_status s;
    const typename HF::Tables* tabs;
    const typename HF::Cosets* inv_cos;
    if ((s = tables_for<F>(ctx, lg, &tabs))) return s;
    if ((s = cosets_for<F>(ctx, lg, qb, F::generator(), true, &inv_cos))) return s;
    if ((s = ensure(ctx, ctx->scratch, nq * n * sizeof(T)))) return s;
    { Scope sq(ctx, scope); gbk::intt_columns<F>(qv, qc, (T*)ctx->scratch.p, nq, *tabs, st); }
    gbk::CosetPow<F> ip{inv_cos->pow_lo, inv_cos->pow_hi, (u32)(n < 4096 ? n : 4096), (u32)(n > 4096 ? n / 4096 : 1)};
    gbk::quotient_combine<F>(lg, qb, nch, qc, combine_mat, ip, chunks, st);
    return GB_OK;
}

// compute_quotient_polys (plonk/prover.rs:712-926) and the split into degree-n chunks (:345-376): out = [nch * qdf][n] chunk
// COEFFICIENTS in device form.  pi_hash: canonical [H]; betas_d / gammas_d: device form; alphas: canonical.
template <class F>
gb_status stage_quotient_polys(Circuit<F>* c, TmpAlloc& tmp, gb_batch* wires, gb_batch* zs, const typename F::T* pi_hash,
                               const std::vector<typename F::T>& betas_d, const std::vector<typename F::T>& gammas_d,
                               const std::vector<typename F::T>& alphas, typename F::T** chunks_out) {
    typedef typename F::T T;
    constexpr u32 H = F::H;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, r = cfg.rate_bits, nch = cfg.num_challenges, nr = cfg.num_routed_wires;
    const Counts cnt(cfg);
    const u32 qdf = cfg.max_quotient_degree_factor, nchunks = cnt.nchunks;
    const u32 qb = quotient_degree_bits(cfg);   // the quotient domain: n 2^qb points = the first 2^qb coset blocks of the LDEs
    const size_t n = cnt.n, nq = cnt.nq;
    hipStream_t st = ctx->stream;
    gb_status s;
    const u32 t0 = nch + nch * nchunks, nterms = t0 + c->num_gate_constraints;
    std::vector<T> uni;
    for (u32 k = 0; k < nch; k++) uni.push_back(F::cform(betas_d[k]));   // multipliers go in constant form (F::mulc)
    uni.insert(uni.end(), gammas_d.begin(), gammas_d.end());
    for (u32 k = 0; k < nch; k++)
        for (u32 j = 0; j < nr; j++) uni.push_back(F::cform(F::mul(betas_d[k], c->k_is_dev_host[j])));
    for (u32 k = 0; k < nch; k++) {
        T x = F::one(), a = F::enc(alphas[k]);
        for (u32 t = 0; t < nterms; t++) { uni.push_back(x); x = F::mul(x, a); }
    }
    uni.insert(uni.end(), c->zh.begin(), c->zh.end());
    uni.insert(uni.end(), c->zh_inv.begin(), c->zh_inv.end());
    for (u32 i = 0; i < H; i++) uni.push_back(F::enc(pi_hash[i]));
    {   // the alpha powers once more in constant form, for k_quotient's own alpha-fold (the gate kernels read the plain ones)
        const size_t a0 = 2 * (size_t)nch + (size_t)nch * nr, na = (size_t)nch * nterms;
        for (size_t i = 0; i < na; i++) uni.push_back(F::cform(uni[a0 + i]));
    }
    T* uni_dev;
    if ((s = upload_tmp(ctx, tmp, uni, &uni_dev))) return s;
    gbk::QuotientParams<F> qp{lg, qb, nch, nr, cfg.num_selectors + cfg.num_constants, cfg.num_selectors, qdf, nchunks, nterms,
                              cfg.gate_constant, cfg.gate_pi, cfg.num_constants, gbk::PowTab<F>{c->wN_lo, c->wN_hi, 12}, c->l0,
                              c->general_gates ? 1u : 0u, lg + r, 0, nch};
    T* qv = tmp.get<T>(nq * n);
    T* qc = tmp.get<T>(nq * n);
    T* chunks = tmp.get<T>(nq * n);
    if (!qv || !qc || !chunks) return fail(ctx, GB_ERR_OOM, "quotient workspace");
    if (c->general_gates) {  // the gate terms first (kernels_gates.hip); k_quotient adds the permutation argument to them
        gbk::GateParams<F> gp{lg, qb, nch, nterms, t0, c->gates, lg + r};
        const T* apow_dev = uni_dev + 2 * (size_t)nch + (size_t)nch * nr;
        const T* pi_dev = apow_dev + (size_t)nch * nterms + 2 * ((size_t)1 << qb);
        const gbk::ProgramParams<F> pp{c->programs, c->prog_instrs_dev, c->prog_lits_dev};
        if (!gbk::gate_constraints<F>(gp, (const T*)c->cs->lde, (const T*)wires->lde, apow_dev, pi_dev, qv, st,
                                      c->programs.num_programs ? &pp : nullptr,
                                      gbk::GateLaunchOptions{ctx->test_force_gate_fallback, &ctx->test_gate_fallback_launches}))
            return fail(ctx, GB_ERR_UNSUPPORTED, "no gate-constraint kernel for this num_challenges");
    }
    if (!gbk::quotient_values<F>(qp, (const T*)c->cs->lde, (const T*)wires->lde, (const T*)zs->lde, uni_dev, qv, st))
        return fail(ctx, GB_ERR_UNSUPPORTED, "no quotient kernel for this (degree factor, num_challenges)");
    if ((s = quotient_coset_ifft<F>(ctx, lg, qb, nch, qv, qc, c->combine_mat, chunks, "quotient IFFT"))) return s;
    *chunks_out = chunks;
    return GB_OK;
}

// ---------------------------------------------------------------------------------------------- prove_openings
// A FriInstanceInfo (fri/structure.rs) compiled for k_reduce_batches: the batches in passes of at most REDUCE_SLOTS consecutive
// ones, each pass a list of runs.  A run is a maximal stretch of consecutive polynomial_index in one oracle whose columns are in
// the same slots of the pass with consecutive powers in each - what FriPolynomialInfo::from_range yields.  Lists in any other order
// fall apart into runs of one column, and a polynomial listed twice in one batch gets a run per mention: nothing below depends
// on runs being merged.
struct FriPlan {
    struct Run {
        u32 oracle, col, ncols;
        u32 apow0[gbk::REDUCE_SLOTS];
    };
    struct Pass {
        u32 batch0, nslots, run0, nruns;
    };
    std::vector<u32> batch_sizes;
    std::vector<Pass> passes;
    std::vector<Run> runs;
    u32 longest = 0;   // the longest batch: alpha^0 .. alpha^(longest - 1) are needed
};
// polynomials: [sum of batch_sizes][2] = (oracle_index, polynomial_index), batch after batch (validated by the caller)
static FriPlan compile_fri_instance(const u32* batch_sizes, u32 num_batches, const u32* polynomials) {
    constexpr u32 S = gbk::REDUCE_SLOTS, ABSENT = gbk::REDUCE_ABSENT;
    FriPlan plan;
    plan.batch_sizes.assign(batch_sizes, batch_sizes + num_batches);
    size_t at = 0;
    for (u32 b0 = 0; b0 < num_batches; b0 += S) {
        const u32 ns = std::min(S, num_batches - b0);
        // (oracle, polynomial) -> one cell per mention that cannot share a read: its power index in every slot
        std::map<std::pair<u32, u32>, std::vector<std::array<u32, S>>> cells;
        for (u32 s = 0; s < ns; s++) {
            plan.longest = std::max(plan.longest, batch_sizes[b0 + s]);
            for (u32 j = 0; j < batch_sizes[b0 + s]; j++, at++) {
                auto& v = cells[{polynomials[2 * at], polynomials[2 * at + 1]}];
                size_t i = 0;
                while (i < v.size() && v[i][s] != ABSENT) i++;
                if (i == v.size()) { v.emplace_back(); v.back().fill(ABSENT); }
                v[i][s] = j;
            }
        }
        FriPlan::Pass pass{b0, ns, (u32)plan.runs.size(), 0};
        for (const auto& kv : cells)
            for (size_t i = 0; i < kv.second.size(); i++) {
                const auto& pw = kv.second[i];
                if (i == 0 && plan.runs.size() > pass.run0) {   // does it continue the run before it?
                    FriPlan::Run& r = plan.runs.back();
                    bool joins = r.oracle == kv.first.first && r.col + r.ncols == kv.first.second;
                    for (u32 s = 0; s < S && joins; s++)
                        joins = r.apow0[s] == ABSENT ? pw[s] == ABSENT : pw[s] == r.apow0[s] + r.ncols;
                    if (joins) { r.ncols++; continue; }
                }
                FriPlan::Run r{kv.first.first, kv.first.second, 1, {}};
                std::copy(pw.begin(), pw.end(), r.apow0);
                plan.runs.push_back(r);
            }
        pass.nruns = (u32)plan.runs.size() - pass.run0;
        plan.passes.push_back(pass);
    }
    return plan;
}
// the table k_reduce_batches reads: the plan's runs over these oracles' coefficient blocks
template <class F>
std::vector<gbk::ReduceRun<F>> fri_run_table(const FriPlan& plan, gb_batch* const* oracles) {
    typedef typename F::T T;
    std::vector<gbk::ReduceRun<F>> t(plan.runs.size());
    for (size_t i = 0; i < t.size(); i++) {
        const FriPlan::Run& r = plan.runs[i];
        t[i].base = (const T*)oracles[r.oracle]->coeffs + ((size_t)r.col << oracles[r.oracle]->log_n);
        t[i].ncols = r.ncols;
        std::copy(r.apow0, r.apow0 + gbk::REDUCE_SLOTS, t[i].apow0);
    }
    return t;
}

struct FriShape {   // the oracles' common shape and what fri_proof needs of FriParams
    u32 degree_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    const std::vector<uint32_t>* reduction_arity_bits;
};

template <class F>
typename F::E get_ext_challenge(typename Host<F>::Challenger& chl) {  // get_extension_challenge: D base challenges -> device form
    typename F::E e = F::ezero();
    for (u32 k = 0; k < F::D; k++) F::set_coord(e, k, F::enc(chl.get()));
    return e;
}

// The rest of prove_openings once final_poly = sum over the batches of alpha-shifted quotients is there (fri/oracle.rs:226-246):
// its lde + coset_fft, then fri_proof (fri/prover.rs:29-81): commit phase, proof of work (minimum nonce), query rounds over every
// oracle's tree.  opening_scope: the caller's "compute opening proofs" scope, open since its reduction.  Appends the FriProof bytes (util/serialization/mod.rs:1679-1695) to `ob`; `ch` leaves as the reference's does.
template <class F>
gb_status fri_proof_of_final_poly(gb_ctx* ctx, TmpAlloc& tmp, const FriShape& fs, gb_batch* const* oracles, u32 num_oracles,
                                  const typename F::E* final_poly, std::unique_ptr<Scope>& opening_scope,
                                  typename Host<F>::Challenger& ch, Bytes& ob) {
    typedef typename F::T T;
    typedef typename F::E E;
    typedef Host<F> HF;
    constexpr u32 D = F::D, H = F::H;
    const u32 lg = fs.degree_bits, r = fs.rate_bits, capH = fs.cap_height, lgN = lg + r;
    const size_t n = (size_t)1 << lg, N = n << r;
    const size_t cap_elems = (size_t)H << capH, es = sizeof(T);
    const std::vector<uint32_t>& arity_bits = *fs.reduction_arity_bits;
    hipStream_t st = ctx->stream;
    gb_status s;
    auto get_ext = get_ext_challenge<F>;
    const u32 nlayers = (u32)arity_bits.size();
    std::vector<T*> layer_vals(nlayers + 1, nullptr), layer_levels(nlayers, nullptr);
    std::vector<u32> layer_lgN(nlayers + 1, 0);
    std::vector<T> fri_caps, final_coeffs;
    u64* pow_res = nullptr;
    {   // still inside the caller's "compute opening proofs" scope, which ends where the final polynomial has been observed
        T* fcols = tmp.get<T>(D * n);
        if (!fcols) return fail(ctx, GB_ERR_OOM, "prove_openings workspace");
        gbk::ext_split<F>(final_poly, n, fcols, st);

        // lde + coset_fft of the final polynomial, coordinate-wise, in leaf order (oracle.rs:226-231)
        const typename HF::Tables* tabs;
        const typename HF::Cosets* cos;
        T shift = F::generator();
        u32 cur_lg = lg;
        T* cur_coeffs = fcols;
        for (u32 li = 0; li < nlayers; li++) {
            const size_t cur_n = (size_t)1 << cur_lg, cur_N = cur_n << r;
            if ((s = tables_for<F>(ctx, cur_lg, &tabs))) return s;
            if ((s = cosets_for<F>(ctx, cur_lg, r, shift, false, &cos))) return s;
            T* vals = tmp.get<T>(D * cur_N);
            if (!vals) return fail(ctx, GB_ERR_OOM, "FRI values");
            { Scope sl(ctx, "FRI LDE"); gbk::lde_columns<F>(cur_coeffs, vals, D, *tabs, *cos, st); }
            layer_vals[li] = vals;
            layer_lgN[li] = cur_lg + r;
            // fri_committed_trees (fri/prover.rs:83-133)
            const u32 ab = arity_bits[li];
            const u32 tree_lg = cur_lg + r - ab;
            const u64 L = (u64)1 << tree_lg;
            T* levels = tmp.get<T>((size_t)(2 * H) << tree_lg);
            if (!levels) return fail(ctx, GB_ERR_OOM, "FRI tree");
            gbk::fri_leaves<F>(vals, cur_N, ab, L, levels, st);
            for (u32 k = 0; k < tree_lg - capH; k++)
                HF::merkle_level(levels + H * level_offset(L, k), levels + H * level_offset(L, k + 1), L >> (k + 1), st);
            layer_levels[li] = levels;
            std::vector<T> lcap(cap_elems);
            if (gb_status rs = read_back(ctx, lcap.data(), levels + H * level_offset(L, tree_lg - capH), cap_elems * es)) return rs;
            fri_caps.insert(fri_caps.end(), lcap.begin(), lcap.end());
            ch.observe(lcap.data(), lcap.size());
            const E beta = get_ext(ch);
            T* folded = tmp.get<T>(D * (cur_n >> ab));
            if (!folded) return fail(ctx, GB_ERR_OOM, "FRI fold");
            gbk::fri_fold<F>(cur_coeffs, cur_n, ab, beta, folded, st);
            cur_coeffs = folded;
            cur_lg -= ab;
            shift = F::pow(shift, (u64)1 << ab);
        }
        // final polynomial: coeffs truncated to len >> rate_bits = the 2^cur_lg folded coefficients
        const size_t fl = (size_t)1 << cur_lg;
        std::vector<T> fc(D * fl);
        pow_res = tmp.get<u64>(1);      // the proof-of-work search's result word: filled while the stream is busy anyway
        if (!pow_res) return fail(ctx, GB_ERR_OOM, "pow result");
        HIP_TRY(ctx, hipMemsetAsync(pow_res, 0xFF, 8, st));
        if (gb_status rs = read_back(ctx, fc.data(), cur_coeffs, D * fl * es)) return rs;
        final_coeffs.resize(D * fl);
        for (size_t t = 0; t < fl; t++)
            for (u32 k = 0; k < D; k++) final_coeffs[D * t + k] = (T)F::dec(fc[k * fl + t]);
        ch.observe(final_coeffs.data(), final_coeffs.size());
        opening_scope.reset();
    }

    // ---- fri_proof_of_work (fri/prover.rs:136-188): the minimum nonce
    u64 pow_witness = 0;
    {
        Scope sc(ctx, "find proof-of-work witness");
        gbk::PowState<F> ps;
        std::memcpy(ps.s, ch.state, sizeof ps.s);
        for (int i = 0; i < ch.nin; i++) ps.s[i] = ch.in[i];
        ps.pos = (u32)ch.nin;
        const u32 min_lz = fs.proof_of_work_bits + (64 - F::ORDER_BITS);  // fri/prover.rs:147
        u64 found = 0;
        if ((s = pow_search<F>(ctx, pow_res, ps, min_lz, &found))) return s;
        pow_witness = found;
        ch.observe((T)pow_witness);
        u64 resp = ch.get();
        if (min_lz && (resp >> (64 - min_lz))) return fail(ctx, GB_ERR_HIP, "proof-of-work response check failed");
    }

    // ---- query rounds (fri/prover.rs:190-255)
    {
        Scope sc(ctx, "fri query rounds");
        const u32 nqr = fs.num_query_rounds;
        std::vector<u64> idx(nqr);
        for (auto& x : idx) x = (u64)ch.get() % N;
        u64* idx_dev = nullptr;
        if (nqr > gbk::QUERY_IDX_INLINE) if ((s = upload_tmp(ctx, tmp, idx, &idx_dev))) return s;
        const u32 layers0 = lgN - capH;
        // every opened row and path of the proof: one job per tree, one launch per twelve jobs, one buffer, one read-back
        std::vector<gbk::QueryJob<F>> jobs;
        size_t total = 0;
        auto add_job = [&](gbk::QueryJob<F> j) {
            j.out = total;
            total += (size_t)nqr * (j.width + (size_t)j.layers * H);
            jobs.push_back(j);
        };
        for (u32 o = 0; o < num_oracles; o++)
            add_job(gbk::QueryJob<F>{(const T*)oracles[o]->lde, (const T*)oracles[o]->levels, (u64)N, 0, (u32)(oracles[o]->ncols + oracles[o]->nsalt),
                                     lgN, layers0, 0, 0, 0});
        for (u32 li = 0, shift = 0; li < nlayers; li++) {
            const u32 ab = arity_bits[li];
            shift += ab;
            const u32 tree_lg = layer_lgN[li] - ab;
            add_job(gbk::QueryJob<F>{layer_vals[li], layer_levels[li], (u64)1 << layer_lgN[li], 0, (u32)(D << ab), tree_lg, tree_lg - capH, shift, ab, 1});
        }
        T* dq = tmp.get<T>(total);
        if (!dq) return fail(ctx, GB_ERR_OOM, "query workspace");
        for (size_t j0 = 0; j0 < jobs.size(); j0 += gbk::QUERY_JOBS) {
            gbk::QueryJobs<F> pack{};
            const u32 nj = (u32)std::min<size_t>(gbk::QUERY_JOBS, jobs.size() - j0);
            std::copy(jobs.begin() + j0, jobs.begin() + j0 + nj, pack.j);
            gbk::query_gather<F>(pack, nj, idx.data(), idx_dev, nqr, dq, st);
        }
        std::vector<T> opened(total);
        if (gb_status rs = read_back(ctx, opened.data(), dq, total * es)) return rs;
        // FriProof bytes (serialization/mod.rs:1679-1695, 1642-1659)
        ob.put(fri_caps.data(), fri_caps.size() * es);
        for (u32 qi = 0; qi < nqr; qi++) {
            for (const auto& j : jobs) {
                const T* rows = opened.data() + j.out;
                const T* paths = rows + (size_t)nqr * j.width;
                ob.put(rows + (size_t)qi * j.width, (size_t)j.width * es);
                ob.u8v((uint8_t)j.layers);
                ob.put(paths + (size_t)qi * j.layers * H, (size_t)j.layers * H * es);
            }
        }
    }
    ob.put(final_coeffs.data(), final_coeffs.size() * es);
    {
        T pw = (T)pow_witness;
        ob.put(&pw, es);
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}


// PolynomialBatch::prove_openings (fri/oracle.rs:187-246) on a compiled instance: oracles[num_oracles] with the shape `fs`, batch b
// opened at points[b].  One k_reduce_batches pass per REDUCE_SLOTS batches, then per batch, in instance order, divide_by_linear and
// alpha.shift_poly(final_poly) += quotient (:216-223).  The instance's run table is made and uploaded here, for the call.
template <class F>
gb_status fri_prove_instance(gb_ctx* ctx, TmpAlloc& tmp, const FriShape& fs, const FriPlan& plan, gb_batch* const* oracles, u32 num_oracles, const typename F::E* points,
                             typename Host<F>::Challenger& ch, Bytes& ob) {
    typedef typename F::E E;
    const size_t n = (size_t)1 << fs.degree_bits;
    const u32 nb = (u32)plan.batch_sizes.size();
    hipStream_t st = ctx->stream;
    gb_status s;
    const E fri_alpha = get_ext_challenge<F>(ch);
    // every point's powers and those of its inverse (the division runs on z^-1), EXT_POW_JOBS tables per launch
    std::vector<gbk::ExtPowTab<F>> ztab(2 * (size_t)nb);
    E* apow_dev = nullptr;   // alpha^0 .. alpha^(longest batch - 1)
    {
        std::vector<E> pts(2 * (size_t)nb);
        std::vector<size_t> ns(2 * (size_t)nb);
        std::vector<gbk::ExtPowTab<F>*> out(2 * (size_t)nb);
        for (u32 b = 0; b < nb; b++) {
            pts[2 * b] = points[b]; pts[2 * b + 1] = F::einv(points[b]);
            ns[2 * b] = n; ns[2 * b + 1] = n + 1;
            out[2 * b] = &ztab[2 * b]; out[2 * b + 1] = &ztab[2 * b + 1];
        }
        for (size_t i = 0; i < pts.size();) {   // (the first launch also carries alpha's plain list)
            const u32 cnt = (u32)std::min<size_t>(pts.size() - i, gbk::EXT_POW_JOBS - (i ? 0 : 1));
            if (i == 0) s = make_ext_powtabs<F>(ctx, tmp, cnt, pts.data(), ns.data(), out.data(), &fri_alpha, plan.longest, &apow_dev);
            else s = make_ext_powtabs<F>(ctx, tmp, cnt, pts.data() + i, ns.data() + i, out.data() + i);
            if (s) return s;
            i += cnt;
        }
    }
    E* final_poly = tmp.get<E>(n);
    std::unique_ptr<Scope> opening_scope(new Scope(ctx, "compute opening proofs"));
    {
        E* comp = tmp.get<E>(gbk::REDUCE_SLOTS * n);
        E* sloc = tmp.get<E>(n);
        E* dtot = tmp.get<E>(std::max<size_t>(1024, (n + 1023) / 1024));   // one suffix total per block of 1024 coefficients
        if (!comp || !sloc || !dtot || !final_poly) return fail(ctx, GB_ERR_OOM, "prove_openings workspace");
        gbk::ReduceRun<F>* runs_dev = nullptr;
        if ((s = upload_tmp(ctx, tmp, fri_run_table<F>(plan, oracles), &runs_dev))) return s;
        for (const FriPlan::Pass& pass : plan.passes) {
            gbk::reduce_batches<F>(runs_dev + pass.run0, pass.nruns, pass.nslots, n, apow_dev, comp, st);
            for (u32 k = 0; k < pass.nslots; k++) {
                const u32 b = pass.batch0 + k;
                const E sh = gbk::epow<F>(fri_alpha, plan.batch_sizes[b]);   // alpha.shift_poly: the count of the batch just reduced
                gbk::divide_by_linear_accumulate<F>(comp + (size_t)k * n, n, ztab[2 * b], ztab[2 * b + 1], sh, b == 0, sloc, dtot, final_poly, st);
            }
        }
    }
    return fri_proof_of_final_poly<F>(ctx, tmp, fs, oracles, num_oracles, final_poly, opening_scope, ch, ob);
}

// PolynomialBatch::prove_openings (fri/oracle.rs:187-246) for the PLONK instance get_fri_instance(zeta) (plonk/circuit_data.rs:
// 438-520: every polynomial of the four oracles opened at zeta, the Zs also at g zeta), then fri_proof (fri/prover.rs:29-81):
// commit phase, proof of work (minimum nonce), query rounds.  `ch` is the Challenger after observe_openings; it leaves in the
// state the reference's leaves in.  Appends the FriProof bytes (util/serialization/mod.rs:1679-1695) to `ob`.  Its two batches
// are fixed, so they are reduced by the two launches of k_reduce_polys; everything behind the final polynomial is the routine
// fri_prove_instance ends in as well.
template <class F>
gb_status stage_prove_openings(Circuit<F>* c, TmpAlloc& tmp, gb_batch* wires, gb_batch* zs, gb_batch* quot, typename F::E zeta,
                               typename Host<F>::Challenger& ch, Bytes& ob) {
    typedef typename F::T T;
    typedef typename F::E E;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, r = cfg.rate_bits, nch = cfg.num_challenges, capH = cfg.cap_height, nw = cfg.num_wires;
    const Counts cnt(cfg);
    const size_t n = cnt.n, ncs = c->cs->ncols, nzs = cnt.nzs, nq = cnt.nq;
    hipStream_t st = ctx->stream;
    gb_status s;
    auto get_ext = get_ext_challenge<F>;
    const E zeta_next = F::escale(zeta, F::two_adic_generator(lg));
    gbk::ExtPowTab<F> zt, zt_inv, znt, znt_inv;
    const E fri_alpha = get_ext(ch);
    E* apow_dev = nullptr;   // alpha^0 .. alpha^(total_polys - 1)
    {
        const E pts[4] = {zeta, F::einv(zeta), zeta_next, F::einv(zeta_next)};
        const size_t ns[4] = {n, n + 1, n, n + 1};
        gbk::ExtPowTab<F>* tabs4[4] = {&zt, &zt_inv, &znt, &znt_inv};
        if ((s = make_ext_powtabs<F>(ctx, tmp, 4, pts, ns, tabs4, &fri_alpha, ncs + nw + nzs + nq, &apow_dev))) return s;
    }
    E* final_poly = tmp.get<E>(n);
    std::unique_ptr<Scope> opening_scope(new Scope(ctx, "compute opening proofs"));
    {
        E* comp = tmp.get<E>(n);
        E* sloc = tmp.get<E>(n);
        E* dtot = tmp.get<E>(std::max<size_t>(1024, (n + 1023) / 1024));   // one suffix total per block of 1024 coefficients (round 6: 1024 of
                                                                            // them overflowed into final_poly from 2^21 rows up - found by the byte comparison)
        if (!comp || !sloc || !dtot || !final_poly) return fail(ctx, GB_ERR_OOM, "prove_openings workspace");
        gbk::PolyGroups<F> g0{{(const T*)c->cs->coeffs, (const T*)wires->coeffs, (const T*)zs->coeffs, (const T*)quot->coeffs},
                              {(u32)ncs, nw, (u32)nzs, (u32)nq}, 4};
        gbk::PolyGroups<F> g1{{(const T*)zs->coeffs, nullptr, nullptr, nullptr}, {nch, 0, 0, 0}, 1};
        gbk::reduce_polys<F>(g0, n, apow_dev, comp, st);
        gbk::divide_by_linear_accumulate<F>(comp, n, zt, zt_inv, F::efrom(F::one()), 1, sloc, dtot, final_poly, st);
        gbk::reduce_polys<F>(g1, n, apow_dev, comp, st);
        const E sh = gbk::epow<F>(fri_alpha, nch);  // alpha.shift_poly: count of the second batch
        gbk::divide_by_linear_accumulate<F>(comp, n, znt, znt_inv, sh, 0, sloc, dtot, final_poly, st);
    }
    gb_batch* oracles[4] = {c->cs, wires, zs, quot};
    const FriShape fs{lg, r, capH, cfg.proof_of_work_bits, cfg.num_query_rounds, &c->arity_bits};
    return fri_proof_of_final_poly<F>(ctx, tmp, fs, oracles, 4, final_poly, opening_scope, ch, ob);
}

// ---------------------------------------------------------------------------------------------- prove()
struct RetryHint {   // gb_prove_retry: the one wire that differs from the witness of the attempt that failed
    uint32_t wire;
    uint64_t row;
};
// option "check_witness" (check_host.inc): GB_ERR_UNSATISFIED where the witness breaks a gate or a copy constraint
template <class F>
gb_status check_before_commit(Circuit<F>* c, ColSrc witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs);

// prover.rs:399-404: an opening point inside the subgroup would divide by zero in prove_openings
template <class F>
gb_status check_opening_point(gb_ctx* ctx, typename F::E zeta, u32 degree_bits) {
    for (u32 i = 0; i < degree_bits; i++) zeta = F::emul(zeta, zeta);
    if (gbk::eis_one<F>(zeta)) return fail(ctx, GB_ERR_OPENING_IN_SUBGROUP, "Opening point is in the subgroup.");
    return GB_OK;
}

// The routed wire VALUES [num_routed][n] on the device in device form, as the Z computation reads them (only these columns:
// prover.rs:497-505): the caller's device matrix where canonical words are the device form, else a pooled copy, converted
template <class F>
gb_status routed_wires_device_form(Circuit<F>* c, TmpAlloc& tmp, ColSrc witness, uint32_t flags, const typename F::T** out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    gb_ctx* ctx = c->ctx;
    const bool dev = (flags & GB_INPUT_DEVICE) != 0;
    if (HF::device_form_is_canonical && dev && witness.base) {
        *out = static_cast<const T*>(witness.base);
        return GB_OK;
    }
    const u32 nr = c->cfg.num_routed_wires;
    const size_t n = (size_t)1 << c->cfg.degree_bits;
    T* copy = tmp.get<T>((size_t)nr * n);
    if (!copy) return fail(ctx, GB_ERR_OOM, "witness copy");
    if (!copy_columns(witness, nr, n * sizeof(T), copy, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream))
        return fail(ctx, GB_ERR_HIP, "copy of the routed wires failed");
    if (flags & GB_INPUT_P3_REPR) gbk::reduce_words<F>(copy, (size_t)nr * n, ctx->stream);
    else HF::to_device_form(copy, copy, (size_t)nr * n, ctx->stream);
    *out = copy;
    return GB_OK;
}

// zero-knowledge (config.zero_knowledge && PlonkOracle::*.blinding, prover.rs:267,334,382): the wires, Zs and quotient
// leaves end in SALT_SIZE salt elements.  salts = [3][SALT_SIZE][N] canonical values in LDE-point order, in the same
// memory space as the witness; the Zs / quotient commitments run on device data, so host salts are staged once.
// GB_SALTS_FROM_SEED: `salts` is 32 seed bytes on the host (checked non-null by the entries); column j of commitment s is the
// stream (seed, (GB_STREAM_SALTS, s, j)), elements 0 .. N - 1, generated just before the commitment that consumes it into ONE
// block of SALT_SIZE x N elements the three commitments share - the stream orders commitment s's bitrev_copy out of the block
// before the generator of commitment s + 1 writes it.
template <class F>
struct SaltPlan {
    typedef typename F::T T;
    const T *w = nullptr, *z = nullptr, *q = nullptr;   // of the wires / Zs / quotient commitment; null: no salts
    bool seeded = false;
    gbk::rnd::Key key{};
    size_t N = 0;
    gb_status init(gb_ctx* ctx, TmpAlloc& tmp, const void* salts, bool from_seed, uint32_t flags, size_t lde_size) {
        seeded = from_seed;
        N = lde_size;
        w = static_cast<const T*>(salts);
        const size_t per = (size_t)GB_SALT_SIZE * N;
        if (seeded) {
            const u32 nonce[3] = {gbk::rnd::STREAM_SALTS, 0, 0};
            key = gbk::rnd::make_key(static_cast<const uint8_t*>(salts), nonce);
            T* block = tmp.get<T>(per);
            if (!block) return fail(ctx, GB_ERR_OOM, "salt block");
            w = z = q = block;
        } else if (salts && (flags & GB_INPUT_DEVICE)) {
            z = w + per;
            q = w + 2 * per;
        } else if (salts) {
            T* stage = tmp.get<T>(2 * per);
            if (!stage) return fail(ctx, GB_ERR_OOM, "salt staging");
            HIP_TRY(ctx, hipMemcpyAsync(stage, w + per, 2 * per * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
            if (flags & GB_INPUT_P3_REPR) p3_to_canonical_dev<F>(stage, 2 * per, ctx->stream);   // the Zs / quotient commits take device salts: canonical
            z = stage;
            q = stage + per;
        }
        return GB_OK;
    }
    gb_status generate(gb_ctx* ctx, u32 commitment) {   // the seeded block for this commitment; no-op without the flag
        if (!seeded) return GB_OK;
        key.nonce[1] = commitment;
        if (!gbk::random_elements<F>(key, 0, N, GB_SALT_SIZE, const_cast<T*>(w), N, ctx->stream))
            return fail(ctx, GB_ERR_HIP, "launch of k_random_elements failed");
        return GB_OK;
    }
};

// gb_prove_retry, the retry of an attempt that failed on this circuit with one wire re-drawn: everything of that attempt's wires
// commitment is still right except the column of that wire - its coefficients, its LDE - and what the leaf sponges absorbed from
// it on.  The kept state moves into the caller's guarded variables first: from there on it is that call's to release or to keep.
template <class F>
gb_status recommit_retry_column(Circuit<F>* c, TmpAlloc& tmp, ColSrc witness, uint32_t flags, const RetryHint& hint, gb_batch** wires_out,
                                typename F::T** wit_vals_out, SegKeep* seg_out, size_t* wit_mont_cols_out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    constexpr u32 H = F::H;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = cfg.degree_bits, r = cfg.rate_bits, capH = cfg.cap_height, nw = cfg.num_wires;
    const size_t n = (size_t)1 << lg, N = n << r, col_bytes = n * sizeof(T), wit_bytes = (size_t)nw * col_bytes;
    const bool dev_witness = (flags & GB_INPUT_DEVICE) != 0;
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0;   // host words of the reference's field types (commit() rejects it for device input)
    hipStream_t st = ctx->stream;
    gb_status s;
    Scope sc(ctx, "compute wires commitment");
    gb_batch* const wires = *wires_out = c->retry.wires;
    T*& wit_vals = *wit_vals_out = (T*)c->retry.wit_vals;
    const SegKeep seg = *seg_out = c->retry.seg;
    const size_t wit_mont_cols = *wit_mont_cols_out = c->retry.wit_mont_cols;
    c->retry.wires = nullptr; c->retry.wit_vals = nullptr; c->retry.seg = SegKeep{};   // owned by the call from here on
    c->drop_retry();                                          // (a witness front's matrix, had it not taken it: not this witness)
    const T* col_src;                                         // the wire's column of the new witness, device form
    bool canonical_col = false;                               // ... or canonical, where commit() left the kept copy so
    if (dev_witness) {                                        // the caller's device matrix holds it: copy, convert
        if (wit_vals) { pool_free(ctx, wit_vals, wit_bytes); wit_vals = nullptr; }   // (a host attempt's copy: not this one's)
        T* colbuf = tmp.get<T>(n);
        if (!colbuf) return fail(ctx, GB_ERR_OOM, "witness column");
        HIP_TRY(ctx, hipMemcpyAsync(colbuf, witness.col(hint.wire, col_bytes), col_bytes, hipMemcpyDeviceToDevice, st));
        HF::to_device_form(colbuf, colbuf, n, st);
        col_src = colbuf;
    } else {                                                  // host matrix: the kept device copy, one element re-written
        if (ctx->retry_verify) {   // option "retry_verify": is the caller's matrix the kept one but for that element?  (a debugging
                                   // aid: one column at a time through a host buffer of n elements)
            std::unique_ptr<T[]> back(new (std::nothrow) T[n]);
            if (!back) return fail(ctx, GB_ERR_OOM, "host allocation failed");
            for (u32 w = 0; w < nw; w++) {
                HIP_TRY(ctx, hipMemcpyAsync(back.get(), wit_vals + (size_t)w * n, col_bytes, hipMemcpyDeviceToHost, st));
                HIP_TRY(ctx, hipStreamSynchronize(st));
                const T* hw = reinterpret_cast<const T*>(witness.col(w, col_bytes));
                for (size_t i = 0; i < n; i++) {
                    if (w == hint.wire && i == hint.row) continue;
                    const T canon = p3 ? (T)HF::p3_to_canonical(hw[i]) : hw[i];
                    if (back[i] != (w < wit_mont_cols ? F::enc(canon) : canon))   // the caller's guards release wires / wit_vals / seg
                        return fail(ctx, GB_ERR_INVALID, "gb_prove_retry: the witness differs from the failed attempt's in more than witness[wire][row]");
                }
            }
        }
        T v = reinterpret_cast<const T*>(witness.col(hint.wire, col_bytes))[hint.row];
        if (p3) v = (T)HF::p3_to_canonical(v);
        if ((u64)v >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical witness element");
        canonical_col = !HF::device_form_is_canonical && hint.wire >= wit_mont_cols;   // that column of the kept copy is as uploaded
        const T vd = canonical_col ? v : F::enc(v);
        T* cell = wit_vals + (size_t)hint.wire * n + hint.row;
        if (sizeof(T) == 8) {
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)cell, (int)(u32)(u64)vd, 1, st));
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)((u32*)cell + 1), (int)(u32)((u64)vd >> 32), 1, st));
        } else {
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)cell, (int)(u32)vd, 1, st));
        }
        col_src = wit_vals + (size_t)hint.wire * n;
    }
    const typename HF::Tables* tabs;
    const typename HF::Cosets* cos;
    if ((s = tables_for<F>(ctx, lg, &tabs))) return s;
    if ((s = cosets_for<F>(ctx, lg, r, F::generator(), false, &cos))) return s;
    if ((s = ensure(ctx, ctx->scratch, 2 * n * sizeof(T)))) return s;
    T* coeffs_col = (T*)wires->coeffs + (size_t)hint.wire * n;
    T* lde_col = (T*)wires->lde + (size_t)hint.wire * N;
    {
        Scope si(ctx, "IFFT");
        if (canonical_col) {
            if (!HF::intt_canonical(const_cast<T*>(col_src), coeffs_col, (T*)ctx->scratch.p, 1, *tabs, st))
                return fail(ctx, GB_ERR_INVALID, "internal: canonical-input transform not available for this size");
        } else {
            gbk::intt_columns<F>(col_src, coeffs_col, (T*)ctx->scratch.p, 1, *tabs, st);
        }
    }
    { Scope sf(ctx, "FFT + blinding"); gbk::lde_columns<F>(coeffs_col, lde_col, 1, *tabs, *cos, st); }
    {
        Scope sm(ctx, "build Merkle tree");
        T* lv = (T*)wires->levels;
        { Scope sl(ctx, "hash leaves"); HF::merkle_leaves_segment((const T*)wires->lde, N, seg.start, nw, (T*)seg.state, true, 0, lv, st); }
        for (u32 k = 0; k < lg + r - capH; k++)
            HF::merkle_level(lv + H * level_offset(N, k), lv + H * level_offset(N, k + 1), N >> (k + 1), st);
    }
    return GB_OK;
}

// The opening set at zeta and g zeta (plonk/proof.rs:346-387), then the front of the proof bytes - the three caps and the
// OpeningSet (serialization/mod.rs:2103-2118, 1514-1529) - and observe_openings (plonk/proof.rs:388-440)
template <class F>
gb_status open_and_serialize(Circuit<F>* c, TmpAlloc& tmp, gb_batch* wires, gb_batch* zs, gb_batch* quot, typename F::E zeta,
                             const typename F::T* const caps[3], typename Host<F>::Challenger& ch, Bytes& ob) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 D = F::D, H = F::H;
    gb_ctx* ctx = c->ctx;
    const gb_circuit_config& cfg = c->cfg;
    const Counts cnt(cfg);
    const u32 nch = cfg.num_challenges, nw = cfg.num_wires;
    const size_t n = cnt.n, ncs = c->cs->ncols, nzs = cnt.nzs, nq = cnt.nq, cap_elems = (size_t)H << cfg.cap_height;
    hipStream_t st = ctx->stream;
    const E zeta_next = F::escale(zeta, F::two_adic_generator(cnt.lg));
    // o_* hold D canonical words per opened polynomial
    std::vector<T> o_cs(D * ncs), o_w(D * nw), o_z(D * nzs), o_zn(D * nzs), o_q(D * nq);
    {
        Scope sc(ctx, "construct the opening set");
        gbk::ExtPowTab<F> zt, znt;
        {
            const E pts[2] = {zeta, zeta_next};
            const size_t ns[2] = {n, n};
            gbk::ExtPowTab<F>* tabs2[2] = {&zt, &znt};
            if (gb_status s = make_ext_powtabs<F>(ctx, tmp, 2, pts, ns, tabs2)) return s;
        }
        E* ztab = tmp.get<E>(n);
        E* zntab = tmp.get<E>(n);
        const size_t nchk = (n + 4095) / 4096;
        const size_t nout = ncs + nw + 2 * nzs + nq;
        E* partial = tmp.get<E>(nchk * nout);
        E* outs = tmp.get<E>(nout);
        if (!ztab || !zntab || !partial || !outs) return fail(ctx, GB_ERR_OOM, "openings workspace");
        gbk::ext_pow_tables<F>(gbk::ExtPowTables<F>{{zt, znt}, {ztab, zntab}}, 2, n, st);
        const gbk::EvalJobs<F> ej{{{(const T*)c->cs->coeffs, ztab, (u32)ncs}, {(const T*)wires->coeffs, ztab, nw}, {(const T*)zs->coeffs, ztab, (u32)nzs},
                                   {(const T*)zs->coeffs, zntab, (u32)nzs}, {(const T*)quot->coeffs, ztab, (u32)nq}}};
        gbk::eval_columns<F>(ej, 5, n, partial, outs, st);
        std::vector<E> host(nout);
        if (gb_status rs = read_back(ctx, host.data(), outs, nout * sizeof(E))) return rs;
        const E* h = host.data();
        auto take = [&](std::vector<T>& dst, size_t count) {
            for (size_t i = 0; i < count; i++, h++)
                for (u32 k = 0; k < D; k++) dst[D * i + k] = (T)F::dec(F::coord(*h, k));
        };
        take(o_cs, ncs); take(o_w, nw); take(o_z, nzs); take(o_zn, nzs); take(o_q, nq);
    }
    const size_t es = sizeof(T);
    for (u32 i = 0; i < 3; i++) ob.put(caps[i], cap_elems * es);            // wires, Zs, quotient
    const size_t nconst = cfg.num_selectors + cfg.num_constants;
    ob.put(o_cs.data(), D * nconst * es);                                   // constants
    ob.put(o_cs.data() + D * nconst, D * (ncs - nconst) * es);             // plonk_sigmas
    ob.put(o_w.data(), o_w.size() * es);                                    // wires
    ob.put(o_z.data(), D * nch * es);                                       // plonk_zs
    ob.put(o_zn.data(), D * nch * es);                                      // plonk_zs_next
    ob.put(o_z.data() + D * nch, D * (nzs - nch) * es);                     // partial_products
    ob.put(o_q.data(), o_q.size() * es);                                    // quotient_polys
    // observe_openings: zeta batch then zeta_next batch
    ch.observe(o_cs.data(), o_cs.size());
    ch.observe(o_w.data(), o_w.size());
    ch.observe(o_z.data(), D * nch);
    ch.observe(o_z.data() + D * nch, D * (nzs - nch));
    ch.observe(o_q.data(), o_q.size());
    ch.observe(o_zn.data(), D * nch);
    return GB_OK;
}

template <class F>
gb_status prove(Circuit<F>* c, ColSrc witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs,
                const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len, const RetryHint* hint = nullptr) {
    typedef typename F::T T;
    typedef typename F::E E;
    typedef Host<F> HF;
    constexpr u32 H = F::H;
    const bool seeded = (flags & GB_SALTS_FROM_SEED) != 0;
    flags &= ~(uint32_t)GB_SALTS_FROM_SEED;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gb_circuit_config& cfg = c->cfg;
    const Counts cnt(cfg);
    const u32 lg = cfg.degree_bits, r = cfg.rate_bits, nch = cfg.num_challenges, capH = cfg.cap_height, nw = cfg.num_wires;
    const size_t n = cnt.n, N = cnt.N, cap_elems = (size_t)H << capH;
    hipStream_t st = ctx->stream;
    TmpAlloc tmp(ctx);
    gb_status s;
    gb_batch *wires = nullptr, *zs = nullptr, *quot = nullptr;
    struct Guard {
        gb_batch **a, **b, **c;
        ~Guard() { gb_batch_free(*a); gb_batch_free(*b); gb_batch_free(*c); }
    } guard{&wires, &zs, &quot};
    auto enc_all = [](const std::vector<T>& canon) {
        std::vector<T> v(canon.size());
        for (size_t i = 0; i < canon.size(); i++) v[i] = F::enc(canon[i]);
        return v;
    };

    std::vector<T> pis(num_public_inputs);
    for (size_t i = 0; i < num_public_inputs; i++) pis[i] = (T)public_inputs[i];
    T pi_hash[H];
    HF::hash_no_pad(pis.data(), pis.size(), pi_hash);  // prover.rs:244
    SaltPlan<F> salt;
    if ((s = salt.init(ctx, tmp, salts, seeded, flags, N))) return s;

    // ---- wires commitment (prover.rs:261-272)
    // A host witness crosses PCIe once: commit() uploads it in column chunks into `wit_vals` (device form), overlapped with the
    // inverse NTTs, and the permutation argument below reads the routed columns from there.
    // `wit_vals` and the sponge state in front of the last column segment outlive this call when it ends in InvZeroPermArg
    // (c->retry): they are pool blocks of their own, released by the guard unless they are kept.
    T* wit_vals = nullptr;
    const size_t wit_bytes = (size_t)nw * n * sizeof(T);
    size_t wit_mont_cols = cfg.num_routed_wires;   // leading columns of wit_vals in device form: what the Z computation reads (commit() may convert more)
    SegKeep seg;
    struct KeepGuard {
        gb_ctx* ctx; T** wit; size_t wit_bytes; SegKeep* seg;
        ~KeepGuard() {
            if (*wit) pool_free(ctx, *wit, wit_bytes);
            if (seg->state) pool_free(ctx, seg->state, seg->bytes);
        }
    } keep_guard{ctx, &wit_vals, wit_bytes, &seg};
    const bool dev_witness = (flags & GB_INPUT_DEVICE) != 0;
    const bool incremental = hint && c->retry.wires && c->retry.seg.state && !salts && (dev_witness || c->retry.wit_vals) &&
                             hint->wire < nw && hint->wire >= c->retry.seg.start && hint->row < n;
    if (incremental) {
        if ((s = recommit_retry_column<F>(c, tmp, witness, flags, *hint, &wires, &wit_vals, &seg, &wit_mont_cols))) return s;
    } else {
        c->drop_retry();
        if (ctx->check_witness && (s = check_before_commit<F>(c, witness, flags, public_inputs, num_public_inputs))) return s;
        if (!dev_witness && lg >= 12) {
            void* p = nullptr;
            if (pool_alloc(ctx, wit_bytes, &p) != hipSuccess) return fail(ctx, GB_ERR_OOM, "witness staging");
            wit_vals = (T*)p;
        }
        Scope sc(ctx, "compute wires commitment");
        if ((s = salt.generate(ctx, 0))) return s;
        if ((s = commit<F>(ctx, witness, nw, lg, r, capH, salt.w, flags | (seeded ? GB_SALTS_DEVICE : 0u), false, &wires, wit_vals,
                           salts ? nullptr : &seg, &wit_mont_cols)))
            return dev_witness ? s : finish_host_commit(ctx, s, nullptr);   // the witness is the caller's again
    }
    const T* wit_dev = wit_vals;   // the Z computation needs the routed wire VALUES on the device (device form) as well
    if (!wit_dev && (s = routed_wires_device_form<F>(c, tmp, witness, flags, &wit_dev))) return s;
    std::vector<T> cap;
    typename HF::Challenger ch;
    ch.observe(c->digest, H);
    ch.observe(pi_hash, H);
    if ((s = read_cap<F>(wires, cap))) return s;
    ch.observe(cap.data(), cap.size());
    const std::vector<T> cap_wires(cap);   // the proof carries the three caps too: kept, not read a second time
    std::vector<T> betas(nch), gammas(nch), alphas(nch);  // canonical
    for (auto& b : betas) b = ch.get();
    for (auto& g : gammas) g = ch.get();
    const std::vector<T> betas_d = enc_all(betas), gammas_d = enc_all(gammas);

    // ---- Z and partial products (prover.rs:305-339)
    {
        Scope sc(ctx, "compute partial products");
        T* zs_vals = nullptr;
        // Up to 2^16 rows the question "was a denominator zero?" travels with the Z commitment's cap - one host round trip fewer per
        // proof, against a wasted commitment (cheap at these sizes) on the rare proof that fails; above, it is asked at once.
        const bool defer = lg <= 16;
        auto failed = [&](gb_status st_) {
            if (st_ == GB_ERR_PERM_ARG_ZERO && seg.state && (wit_vals || dev_witness)) {   // keep what gb_prove_retry can build on
                c->retry.wires = wires; wires = nullptr;
                c->retry.wit_vals = wit_vals; c->retry.wit_bytes = wit_bytes; wit_vals = nullptr;
                c->retry.wit_mont_cols = wit_mont_cols;
                c->retry.seg = seg; seg = SegKeep{};
            }
            return st_;
        };
        s = stage_zs_partial_products<F>(c, tmp, wit_dev, betas_d, gammas_d, &zs_vals, defer);
        if (s == GB_OK && c->test_fail_next_perm_arg) {
            c->test_fail_next_perm_arg = false;
            if (defer) (void)perm_arg_check<F>(c, nullptr, 0, nullptr);   // settle the kernel's own answer before the armed one is given
            s = fail(ctx, GB_ERR_PERM_ARG_ZERO, "InvZeroPermArg (armed by gb_test_arm_perm_arg_failure)");
        }
        if (s) return failed(s);
        if ((s = salt.generate(ctx, 1))) return s;
        if ((s = commit<F>(ctx, zs_vals, cnt.nzs, lg, r, capH, salt.z, GB_INPUT_DEVICE | GB_INPUT_DEVICE_FORM, false, &zs))) {
            if (defer) (void)hipMemsetAsync(c->perm_err, 0, 4, st);   // nobody will ask the deferred question: leave the word zero
            return s;
        }
        if (defer) {
            cap.resize(cap_elems);
            const T* cap_dev = (const T*)zs->levels + H * level_offset(N, lg + r - capH);
            if ((s = perm_arg_check<F>(c, cap.data(), cap_elems * sizeof(T), cap_dev))) return failed(s);
        }
    }
    if (lg > 16) if ((s = read_cap<F>(zs, cap))) return s;
    ch.observe(cap.data(), cap.size());
    const std::vector<T> cap_zs(cap);
    for (auto& a : alphas) a = ch.get();

    // ---- quotient polynomials (prover.rs:345-387)
    {
        Scope sc(ctx, "compute quotient polys");
        T* chunks = nullptr;
        if ((s = stage_quotient_polys<F>(c, tmp, wires, zs, pi_hash, betas_d, gammas_d, alphas, &chunks))) return s;
        if ((s = salt.generate(ctx, 2))) return s;
        if ((s = commit<F>(ctx, chunks, cnt.nq, lg, r, capH, salt.q, GB_INPUT_DEVICE | GB_INPUT_DEVICE_FORM, true, &quot))) return s;
    }
    if ((s = read_cap<F>(quot, cap))) return s;
    ch.observe(cap.data(), cap.size());
    const E zeta = get_ext_challenge<F>(ch);
    if ((s = check_opening_point<F>(ctx, zeta, lg))) return s;

    // ---- openings (plonk/proof.rs:346-440), then prove_openings (fri/oracle.rs:187-246) -> FriProof bytes
    Bytes ob(proof_out, proof_cap);
    const T* const caps[3] = {cap_wires.data(), cap_zs.data(), cap.data()};   // (the quotient's, read for zeta above)
    if ((s = open_and_serialize<F>(c, tmp, wires, zs, quot, zeta, caps, ch, ob))) return s;
    if ((s = stage_prove_openings<F>(c, tmp, wires, zs, quot, zeta, ch, ob))) return s;
    ob.u64v(num_public_inputs);  // ProofWithPublicInputs (serialization/mod.rs:2134-2151)
    ob.put(pis.data(), pis.size() * sizeof(T));
    *proof_len = ob.len;
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    if (!proof_out || ob.len > proof_cap) return fail(ctx, GB_ERR_BUFFER_TOO_SMALL, "proof buffer too small");
    return GB_OK;
}

// PolynomialBatch columns evaluated at one extension point (plonk/proof.rs:359-363 eval_commitment)
template <class F>
gb_status batch_eval_ext(gb_batch* b, const void* z_canon, void* out) {
    typedef typename F::T T;
    typedef typename F::E E;
    gb_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)1 << b->log_n, ncols = b->ncols;
    TmpAlloc tmp(ctx);
    E z = F::ezero();
    for (u32 k = 0; k < F::D; k++) F::set_coord(z, k, F::enc(static_cast<const T*>(z_canon)[k]));
    gbk::ExtPowTab<F> zt;
    gb_status s;
    if ((s = make_ext_powtab<F>(ctx, tmp, z, n, &zt))) return s;
    const size_t nchk = (n + 4095) / 4096;
    E* ztab = tmp.get<E>(n);
    E* partial = tmp.get<E>(nchk * ncols);
    E* outs = tmp.get<E>(ncols);
    if (!ztab || !partial || !outs) return fail(ctx, GB_ERR_OOM, "eval workspace");
    gbk::ext_pow_tables<F>(gbk::ExtPowTables<F>{{zt, zt}, {ztab, ztab}}, 1, n, ctx->stream);
    gbk::eval_columns<F>(gbk::EvalJobs<F>{{{(const T*)b->coeffs, ztab, (u32)ncols}}}, 1, n, partial, outs, ctx->stream);
    std::vector<E> host(ncols);
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), outs, ncols * sizeof(E), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    T* o = static_cast<T*>(out);
    for (size_t i = 0; i < ncols; i++)
        for (u32 k = 0; k < F::D; k++) o[F::D * i + k] = (T)F::dec(F::coord(host[i], k));
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

}  // namespace


// ---- stage-level entry points (the templates; the extern "C" wrappers are at the end of the file)
template <class F>
static gb_status abi_zs_partial_products(Circuit<F>* c, ColSrc witness, uint32_t flags, const void* betas, const void* gammas,
                                         void* values_out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gb_circuit_config& cfg = c->cfg;
    const Counts cnt(cfg);
    const u32 nch = cfg.num_challenges;
    const size_t n = cnt.n, nzs = cnt.nzs;
    hipStream_t st = ctx->stream;
    TmpAlloc tmp(ctx);
    const bool dev = flags & GB_INPUT_DEVICE, p3 = flags & GB_INPUT_P3_REPR;
    if (p3 && dev) return fail(ctx, GB_ERR_INVALID, "GB_INPUT_P3_REPR describes host memory; device inputs are canonical");
    const T* wit_dev;
    if (gb_status s = routed_wires_device_form<F>(c, tmp, witness, flags, &wit_dev)) return s;
    std::vector<T> bd(nch), gd(nch);
    for (u32 k = 0; k < nch; k++) {
        const T b = static_cast<const T*>(betas)[k], g = static_cast<const T*>(gammas)[k];
        if ((u64)b >= F::ORDER || (u64)g >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical challenge");
        bd[k] = F::enc(b);
        gd[k] = F::enc(g);
    }
    T* zs_vals = nullptr;
    if (gb_status s = stage_zs_partial_products<F>(c, tmp, wit_dev, bd, gd, &zs_vals)) return s;
    HF::from_device_form(zs_vals, zs_vals, nzs * n, st);
    HIP_TRY(ctx, hipMemcpyAsync(values_out, zs_vals, nzs * n * sizeof(T), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

template <class F>
static gb_status check_stage_batch(Circuit<F>* c, const gb_batch* b, size_t ncols, const char* what) {
    const gb_circuit_config& cfg = c->cfg;
    if (!b) return fail(c->ctx, GB_ERR_INVALID, std::string("null ") + what + " batch");
    if (!b->coeffs) return fail(c->ctx, GB_ERR_INVALID, std::string(what) + " is a stand-alone Merkle tree, not a polynomial batch");
    if (b->ctx != c->ctx || b->field != c->field) return fail(c->ctx, GB_ERR_INVALID, std::string(what) + " batch belongs to another context or field");
    if (b->log_n != cfg.degree_bits || b->rate_bits != cfg.rate_bits || b->cap_height != cfg.cap_height || b->ncols != ncols ||
        b->nsalt != (cfg.zero_knowledge ? (size_t)GB_SALT_SIZE : 0))
        return fail(c->ctx, GB_ERR_INVALID, std::string(what) + " batch does not have the circuit's shape");
    return GB_OK;
}

template <class F>
static gb_status abi_quotient_polys(Circuit<F>* c, gb_batch* wires, gb_batch* zs, const void* pi_hash, const void* betas,
                                    const void* gammas, const void* alphas, uint32_t flags, void* chunks_out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gb_circuit_config& cfg = c->cfg;
    const Counts cnt(cfg);
    const u32 nch = cfg.num_challenges;
    const size_t n = cnt.n, nzs = cnt.nzs, nq = cnt.nq;
    if (gb_status s = check_stage_batch<F>(c, wires, cfg.num_wires, "wires")) return s;
    if (gb_status s = check_stage_batch<F>(c, zs, nzs, "zs_partial_products")) return s;
    hipStream_t st = ctx->stream;
    TmpAlloc tmp(ctx);
    std::vector<T> bd(nch), gd(nch), al(nch);
    for (u32 k = 0; k < nch; k++) {
        const T b = static_cast<const T*>(betas)[k], g = static_cast<const T*>(gammas)[k], a = static_cast<const T*>(alphas)[k];
        if ((u64)b >= F::ORDER || (u64)g >= F::ORDER || (u64)a >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical challenge");
        bd[k] = F::enc(b);
        gd[k] = F::enc(g);
        al[k] = a;
    }
    T ph[F::H];
    for (u32 i = 0; i < F::H; i++) {
        ph[i] = static_cast<const T*>(pi_hash)[i];
        if ((u64)ph[i] >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical public inputs hash");
    }
    T* chunks = nullptr;
    if (gb_status s = stage_quotient_polys<F>(c, tmp, wires, zs, ph, bd, gd, al, &chunks)) return s;
    HF::from_device_form(chunks, chunks, nq * n, st);
    HIP_TRY(ctx, hipMemcpyAsync(chunks_out, chunks, nq * n * sizeof(T), (flags & GB_INPUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

// Challenger<F, H> by value (gb_challenger_state) <-> the host transcript
template <class F>
static gb_status challenger_from_state(gb_ctx* ctx, const gb_challenger_state* chs, typename Host<F>::Challenger& ch) {
    typedef typename F::T T;
    constexpr u32 W = F::SPONGE_W;  // SPONGE_WIDTH of the configuration's hasher
    if (chs->input_len >= 8 || chs->output_len > 8) return fail(ctx, GB_ERR_INVALID, "challenger buffers hold at most SPONGE_RATE elements");
    for (u32 i = 0; i < W; i++) {
        if (chs->sponge_state[i] >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical challenger state");
        ch.state[i] = (T)chs->sponge_state[i];
    }
    for (u32 i = 0; i < 8; i++)
        if ((i < chs->input_len && chs->input_buffer[i] >= F::ORDER) || (i < chs->output_len && chs->output_buffer[i] >= F::ORDER))
            return fail(ctx, GB_ERR_INVALID, "non-canonical challenger buffer");
    ch.nin = (int)chs->input_len;
    ch.nout = (int)chs->output_len;
    for (int i = 0; i < ch.nin; i++) ch.in[i] = (T)chs->input_buffer[i];
    for (int i = 0; i < ch.nout; i++) ch.out[i] = (T)chs->output_buffer[i];
    return GB_OK;
}
template <class F>
static void challenger_to_state(const typename Host<F>::Challenger& ch, gb_challenger_state* chs) {
    std::memset(chs, 0, sizeof *chs);
    for (u32 i = 0; i < F::SPONGE_W; i++) chs->sponge_state[i] = ch.state[i];
    chs->input_len = (uint32_t)ch.nin;
    chs->output_len = (uint32_t)ch.nout;
    for (int i = 0; i < ch.nin; i++) chs->input_buffer[i] = ch.in[i];
    for (int i = 0; i < ch.nout; i++) chs->output_buffer[i] = ch.out[i];
}

template <class F>
static gb_status abi_prove_openings(Circuit<F>* c, gb_batch* wires, gb_batch* zs, gb_batch* quot, const void* zeta_canon,
                                    gb_challenger_state* chs, void* out, size_t out_cap, size_t* out_len) {
    typedef typename F::T T;
    typedef typename F::E E;
    typedef Host<F> HF;
    gb_ctx* ctx = c->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gb_circuit_config& cfg = c->cfg;
    const Counts cnt(cfg);
    const size_t nzs = cnt.nzs, nq = cnt.nq;
    if (gb_status s = check_stage_batch<F>(c, wires, cfg.num_wires, "wires")) return s;
    if (gb_status s = check_stage_batch<F>(c, zs, nzs, "zs_partial_products")) return s;
    if (gb_status s = check_stage_batch<F>(c, quot, nq, "quotient")) return s;
    typename HF::Challenger ch;
    if (gb_status s = challenger_from_state<F>(ctx, chs, ch)) return s;
    E zeta = F::ezero();
    for (u32 k = 0; k < F::D; k++) {
        const T z = static_cast<const T*>(zeta_canon)[k];
        if ((u64)z >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical zeta");
        F::set_coord(zeta, k, F::enc(z));
    }
    if (gb_status s = check_opening_point<F>(ctx, zeta, cfg.degree_bits)) return s;
    TmpAlloc tmp(ctx);
    Bytes ob(out, out_cap);
    if (gb_status s = stage_prove_openings<F>(c, tmp, wires, zs, quot, zeta, ch, ob)) return s;
    *out_len = ob.len;
    // the caller's Challenger advances only with the proof it belongs to: after a size query (GB_ERR_BUFFER_TOO_SMALL) or any other
    // error *chs is untouched, so the retry with a big enough buffer draws the same fri_alpha / betas / PoW and returns these bytes
    if (!out || ob.len > out_cap) return fail(ctx, GB_ERR_BUFFER_TOO_SMALL, "FriProof buffer too small");
    challenger_to_state<F>(ch, chs);
    return GB_OK;
}

// The description of a FriInstanceInfo as it crosses the ABI (flat arrays), checked against `num_polys[o]` polynomials per oracle
static gb_status check_fri_instance_lists(gb_ctx* ctx, const uint32_t* num_polys, uint32_t num_oracles, const uint32_t* batch_sizes,
                                          uint32_t num_batches, const uint32_t* polynomials) {
    if (!num_oracles) return fail(ctx, GB_ERR_INVALID, "a FRI instance needs at least one oracle");
    if (!num_batches) return fail(ctx, GB_ERR_INVALID, "a FRI instance needs at least one batch");
    if (!batch_sizes || !polynomials) return fail(ctx, GB_ERR_INVALID, "null argument");
    size_t at = 0;
    for (u32 b = 0; b < num_batches; b++) {
        if (!batch_sizes[b]) return fail(ctx, GB_ERR_INVALID, "batch " + std::to_string(b) + " opens no polynomial");
        for (u32 j = 0; j < batch_sizes[b]; j++, at++) {
            const u32 o = polynomials[2 * at], k = polynomials[2 * at + 1];
            if (o >= num_oracles)
                return fail(ctx, GB_ERR_INVALID, "batch " + std::to_string(b) + ": oracle_index " + std::to_string(o) + " out of range");
            if (k >= num_polys[o])
                return fail(ctx, GB_ERR_INVALID, "batch " + std::to_string(b) + ": polynomial_index " + std::to_string(k) + " out of range for oracle " +
                                                     std::to_string(o) + " (salt columns are not polynomials)");
        }
    }
    return GB_OK;
}

template <class F>
static gb_status abi_fri_prove_openings(gb_ctx* ctx, gb_batch* const* oracles, u32 num_oracles, const void* points_canon,
                                        const uint32_t* batch_sizes, u32 num_batches, const uint32_t* polynomials,
                                        const std::vector<uint32_t>& arity_bits, u32 pow_bits, u32 nqr, gb_challenger_state* chs,
                                        void* out, size_t out_cap, size_t* out_len) {
    typedef typename F::T T;
    typedef typename F::E E;
    typedef Host<F> HF;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    typename HF::Challenger ch;
    if (gb_status s = challenger_from_state<F>(ctx, chs, ch)) return s;
    std::vector<E> points(num_batches);
    for (u32 b = 0; b < num_batches; b++) {
        E z = F::ezero();
        bool zero = true;
        for (u32 k = 0; k < F::D; k++) {
            const T w = static_cast<const T*>(points_canon)[(size_t)b * F::D + k];
            if ((u64)w >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "non-canonical coordinate in the point of batch " + std::to_string(b));
            zero = zero && w == 0;
            F::set_coord(z, k, F::enc(w));
        }
        if (zero) return fail(ctx, GB_ERR_UNSUPPORTED, "the point of batch " + std::to_string(b) + " is zero: the division by X - z runs on 1 / z");
        points[b] = z;
    }
    const FriPlan plan = compile_fri_instance(batch_sizes, num_batches, polynomials);
    const FriShape fs{oracles[0]->log_n, oracles[0]->rate_bits, oracles[0]->cap_height, pow_bits, nqr, &arity_bits};
    TmpAlloc tmp(ctx);
    Bytes ob(out, out_cap);
    if (gb_status s = fri_prove_instance<F>(ctx, tmp, fs, plan, oracles, num_oracles, points.data(), ch, ob)) return s;
    *out_len = ob.len;
    if (!out || ob.len > out_cap) return fail(ctx, GB_ERR_BUFFER_TOO_SMALL, "FriProof buffer too small");   // *chs untouched, as gb_prove_openings
    challenger_to_state<F>(ch, chs);
    return GB_OK;
}

// CommonCircuitData.gates + selectors_info -> GateSet, with the shape checks the reference's builder guarantees
template <class F>
static gb_status build_gate_set(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                gbk::gates::GateSet* out, const gbk::gates::ProgramSet* programs = nullptr) {
    typedef typename F::T T;
    namespace G = gbk::gates;
    if (!gates || num_gates == 0) return fail(ctx, GB_ERR_INVALID, "No gates?");
    if (num_gates > G::MAX_GATES) return fail(ctx, GB_ERR_UNSUPPORTED, "too many gate types");
    if (cfg->num_selectors == 0 || cfg->num_selectors > num_gates) return fail(ctx, GB_ERR_INVALID, "bad num_selectors");
    G::GateSet gs{};
    gs.num_gates = num_gates;
    gs.num_selectors = cfg->num_selectors;
    for (u32 g = 0; g < num_gates; g++) {
        const gb_gate& d = gates[g];
        const std::string name = "gate " + std::to_string(g);
        if (d.selector_index >= cfg->num_selectors || d.group_start > g || d.group_end <= g || d.group_end > num_gates)
            return fail(ctx, GB_ERR_INVALID, name + ": selector group does not contain the gate");
        bool needs_param = false;
        switch (d.kind) {
            case GB_GATE_NOOP:
            case GB_GATE_PUBLIC_INPUT: break;
            case GB_GATE_CONSTANT:
            case GB_GATE_ARITHMETIC:
            case GB_GATE_ARITHMETIC_EXTENSION:
            case GB_GATE_MUL_EXTENSION:
            case GB_GATE_BASE_SUM:
            case GB_GATE_REDUCING:
            case GB_GATE_REDUCING_EXTENSION:
            case GB_GATE_APPLY_MAT4:
            case GB_GATE_EXPONENTIATION: needs_param = true; break;
            case GB_GATE_ADD_MANY:
                if (d.param2 == 0) return fail(ctx, GB_ERR_INVALID, name + ": AddManyGate with no operations");
                needs_param = true;
                break;
            case GB_GATE_POSEIDON2_INTERNAL_PERMUTATION:
                if (F::TAG != GB_BABYBEAR)
                    return fail(ctx, GB_ERR_UNSUPPORTED, name + ": Poseidon2InternalPermutationGate is the BabyBear gate");
                break;
            case GB_GATE_POSEIDON:
            case GB_GATE_POSEIDON_MDS:
                if (F::TAG != GB_GOLDILOCKS)
                    return fail(ctx, GB_ERR_UNSUPPORTED, name + ": PoseidonGate / PoseidonMdsGate are the Goldilocks gates");
                break;
            case GB_GATE_POSEIDON2_BABYBEAR:
                if (F::TAG != GB_BABYBEAR) return fail(ctx, GB_ERR_UNSUPPORTED, name + ": Poseidon2BabyBearGate is the BabyBear gate");
                needs_param = true;
                break;
            case GB_GATE_RANDOM_ACCESS:
                if (d.param > G::MAX_RANDOM_ACCESS_BITS || d.param2 == 0)
                    return fail(ctx, GB_ERR_UNSUPPORTED, name + ": RandomAccessGate needs bits <= 6 and num_copies >= 1");
                break;
            case GB_GATE_COSET_INTERPOLATION: {
                const u32 npts = 1u << (d.param & 31);
                if (d.param == 0 || d.param > G::MAX_INTERPOLATION_BITS || d.param2 < 2 || d.param2 > npts)
                    return fail(ctx, GB_ERR_UNSUPPORTED, name + ": CosetInterpolationGate needs 1 <= subgroup_bits <= 4 and 2 <= degree <= 2^subgroup_bits");
                // with_max_degree (coset_interpolation.rs:70-99): the degree is the minimal one for its number of intermediates
                const u32 nint = G::interpolation_intermediates(d);
                if (d.param2 != (npts - 2) / (nint + 1) + 2)
                    return fail(ctx, GB_ERR_INVALID, name + ": CosetInterpolationGate degree is not the one with_max_degree() yields");
                break;
            }
            case GB_GATE_PROGRAM: {
                if (!programs)
                    return fail(ctx, GB_ERR_INVALID, name + ": a program gate needs the program table of gb_circuit_create_programs / gb_verifier_create_programs");
                if (d.param >= programs->num_programs)
                    return fail(ctx, GB_ERR_INVALID, name + ": program " + std::to_string(d.param) + " of " + std::to_string(programs->num_programs));
                // the bound selectors.rs:125-209 keeps for every gate it groups: gate degree + filter degree <= max degree
                const u32 filter_deg = d.group_end - d.group_start - 1 + (cfg->num_selectors > 1 ? 1 : 0);
                if ((u64)programs->p[d.param].degree + filter_deg > (u64)cfg->max_quotient_degree_factor + 1)
                    return fail(ctx, GB_ERR_INVALID, name + ": program " + std::to_string(d.param) + " of degree " +
                                std::to_string(programs->p[d.param].degree) + " with a filter of degree " + std::to_string(filter_deg) +
                                " exceeds max_quotient_degree_factor + 1 = " + std::to_string(cfg->max_quotient_degree_factor + 1));
                break;
            }
            default:
                return fail(ctx, GB_ERR_UNSUPPORTED, name + ": kind " + std::to_string(d.kind) + " has no constraint evaluator (csrc/gates.hpp)");
        }
        if (needs_param && d.param == 0) return fail(ctx, GB_ERR_INVALID, name + ": param 0");
        if (d.kind == GB_GATE_BASE_SUM && G::base_sum_base(d) > cfg->max_quotient_degree_factor)
            return fail(ctx, GB_ERR_INVALID, name + ": BaseSumGate base exceeds the quotient degree factor");
        static const G::ProgramSet no_programs{};
        const G::ProgramSet& ps = programs ? *programs : no_programs;
        const u32 wires = G::num_wires<F>(d, ps), consts = G::num_constants<F>(d, ps);
        if (wires > cfg->num_wires || consts > cfg->num_constants)
            return fail(ctx, GB_ERR_INVALID, name + " needs " + std::to_string(wires) + " wires / " + std::to_string(consts) +
                        " constants, the config has " + std::to_string(cfg->num_wires) + " / " + std::to_string(cfg->num_constants));
        gs.g[g] = d;
    }
    // CosetInterpolationGate tables: two_adic_subgroup(4) (field/src/types.rs:14-17) and 1 / 2^b
    {
        const T g16 = F::two_adic_generator(G::MAX_INTERPOLATION_BITS);
        T x = F::one();
        for (u32 i = 0; i < 16; i++) { gs.subgroup16[i] = x; x = F::mul(x, g16); }
        for (u32 b = 0; b <= G::MAX_INTERPOLATION_BITS; b++) gs.inv_pow2[b] = F::inv(F::enc(1u << b));
    }
    *out = gs;
    return GB_OK;
}

// CommonCircuitData + VerifierOnlyCircuitData -> a circuit object that can only verify (no device state; ctx may be NULL)
template <class F>
static gb_status verifier_create(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates, const void* k_is,
                                 const void* cap, const void* digest, gb_circuit** out, const ProgramTable* table = nullptr) {
    typedef typename F::T T;
    gbk::gates::GateSet gs{};
    ParsedPrograms progs;
    if (table)
        if (gb_status s = parse_programs<F>(ctx, cfg, table->words, table->offsets, table->num_programs, &progs)) return s;
    if (gb_status s = build_gate_set<F>(ctx, cfg, gates, num_gates, &gs, table ? &progs.set : nullptr)) return s;
    Circuit<F>* c = new (std::nothrow) Circuit<F>();
    if (!c) return fail(ctx, GB_ERR_OOM, "host allocation failed");
    c->field = F::TAG;
    c->attach(ctx);
    c->cfg = *cfg;
    c->gates = gs;
    c->general_gates = true;
    c->verify_only = true;
    progs.move_to(c);
    for (u32 g = 0; g < gs.num_gates; g++)
        c->num_gate_constraints = std::max(c->num_gate_constraints, gbk::gates::num_constraints<F>(gs.g[g], c->programs));
    const T* k = static_cast<const T*>(k_is);
    for (u32 j = 0; j < cfg->num_routed_wires; j++) c->k_is_dev_host.push_back(F::enc(k[j]));
    c->cap_host.assign(static_cast<const T*>(cap), static_cast<const T*>(cap) + ((size_t)F::H << cfg->cap_height));
    std::memcpy(c->digest, digest, sizeof c->digest);
    if (!constant_arity_bits(*cfg, &c->arity_bits)) { c->arity_bits.clear(); c->arity_pending = true; }
    *out = c;
    return GB_OK;
}

extern "C" {

gb_status gb_pow_grind(gb_ctx* ctx, uint32_t field, const void* sponge_state, uint32_t witness_pos, uint32_t min_leading_zeros,
                       uint64_t* nonce) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!sponge_state || !nonce) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (witness_pos >= 8 || min_leading_zeros > 64) return fail(ctx, GB_ERR_INVALID, "witness_pos must be inside the rate (< 8)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TmpAlloc tmp(ctx);
    u64* res = tmp.get<u64>(1);
    if (!res) return fail(ctx, GB_ERR_OOM, "pow result");
    HIP_TRY(ctx, hipMemsetAsync(res, 0xFF, 8, ctx->stream));
    if (field == GB_GOLDILOCKS) {
        gbk::PowState<GlF> ps;
        std::memcpy(ps.s, sponge_state, sizeof ps.s);
        ps.pos = witness_pos;
        return pow_search<GlF>(ctx, res, ps, min_leading_zeros, reinterpret_cast<u64*>(nonce));
    }
    gbk::PowState<BbF> ps;
    std::memcpy(ps.s, sponge_state, sizeof ps.s);
    ps.pos = witness_pos;
    return pow_search<BbF>(ctx, res, ps, min_leading_zeros, reinterpret_cast<u64*>(nonce));
} GB_CATCH(ctx)

gb_status gb_batch_eval_ext(gb_batch* b, const void* z, void* out) try {
    if (!b) return fail(nullptr, GB_ERR_INVALID, "null batch");
    if (!z || !out) return fail(b->ctx, GB_ERR_INVALID, "null argument");
    if (!b->coeffs) return fail(b->ctx, GB_ERR_INVALID, "a stand-alone Merkle tree holds no polynomials");
    return by_field(b->field, [&](auto f) { return batch_eval_ext<decltype(f)>(b, z, out); });
} GB_CATCH(b ? b->ctx : nullptr)

static gb_status check_circuit_cfg(gb_ctx* ctx, const gb_circuit_config* cfg, ColSrc constants_sigmas, const void* k_is,
                                   uint32_t flags, gb_circuit** out) {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!cfg || !constants_sigmas || !k_is || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (constants_sigmas.ptrs)
        for (size_t i = 0; i < (size_t)cfg->num_selectors + cfg->num_constants + cfg->num_routed_wires; i++)
            if (!constants_sigmas.ptrs[i]) return fail(ctx, GB_ERR_INVALID, "null constants_sigmas column pointer");
    if (cfg->field != GB_GOLDILOCKS && cfg->field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (flags & ~GB_PUBLIC_INPUT_FLAGS) return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    {   // the security assert of circuit_builder.rs:1190-1192, before any question of what the kernels are compiled for
        const u32 order_bits = cfg->field == GB_GOLDILOCKS ? 64u : 31u;
        if (cfg->degree_bits < order_bits && (order_bits - cfg->degree_bits) * (uint64_t)cfg->num_challenges < 100)
            return fail(ctx, GB_ERR_INVALID, "num_challenges is not sufficient for the soundness of the permutation argument (circuit_builder.rs:1191-1192)");
    }
    const u32 qdf = cfg->max_quotient_degree_factor;
    if (qdf == 0 || (qdf & (qdf - 1))) return fail(ctx, GB_ERR_UNSUPPORTED, "quotient_degree_factor must be a power of two");
    if (qdf > (1u << cfg->rate_bits))
        return fail(ctx, GB_ERR_INVALID, "Having constraints of degree higher than the rate is not supported yet. (plonk/prover.rs:736-740)");
    if (cfg->num_challenges == 0 || cfg->num_challenges > gbk::MAX_CHALLENGES || cfg->rate_bits > 8 || cfg->num_constants > 4)
        return fail(ctx, GB_ERR_UNSUPPORTED, "config outside the supported range (num_challenges <= 16, rate_bits <= 8, num_constants <= 4)");
    if (!gbk::quotient_shape_supported(cfg->field, qdf, cfg->num_challenges))
        return fail(ctx, GB_ERR_UNSUPPORTED,
                    "quotient kernel: degree factor 2, 4, 8 or 16; BabyBear num_challenges >= 4");
    if (cfg->num_routed_wires > cfg->num_wires || cfg->num_routed_wires == 0) return fail(ctx, GB_ERR_INVALID, "bad wire counts");
    // as gb_verifier_create: no proof of a wider circuit verifies, and a gate's constraint count (<= its wires) stays where the
    // unreduced fold sums of the gate kernels were checked (fold_acc.hpp FOLD_ACC_MAX_TERMS)
    if (cfg->num_wires > 4096) return fail(ctx, GB_ERR_INVALID, "bad wire counts: more than 4096 wires");
    const u32 nchunks = (cfg->num_routed_wires + cfg->max_quotient_degree_factor - 1) / cfg->max_quotient_degree_factor;
    if (nchunks > gbk::MAX_CHUNKS) return fail(ctx, GB_ERR_UNSUPPORTED, "too many partial products");
    // no size cap below the two-adicity (plonk/prover.rs:228-447, field/src/fft.rs:168-205); what does not fit the device is GB_ERR_OOM
    if (cfg->degree_bits < 2) return fail(ctx, GB_ERR_UNSUPPORTED, "degree_bits below 2");
    if (cfg->degree_bits + cfg->rate_bits > (cfg->field == GB_GOLDILOCKS ? 32u : 27u))
        return fail(ctx, GB_ERR_INVALID, "LDE size exceeds the field's two-adicity (32 Goldilocks / 27 BabyBear)");
    if (cfg->arity_bits > 8) return fail(ctx, GB_ERR_UNSUPPORTED, "arity_bits outside [0, 8] (0: the list comes through gb_circuit_set_fri_reduction_arity_bits)");
    return GB_OK;
}

static gb_status circuit_create_dummy(gb_ctx* ctx, const gb_circuit_config* cfg, ColSrc constants_sigmas, const void* k_is,
                                      uint32_t flags, gb_circuit** out) {
    if (gb_status s = check_circuit_cfg(ctx, cfg, constants_sigmas, k_is, flags, out)) return s;
    if (cfg->num_selectors != 1 || cfg->gate_constant > 2 || cfg->gate_pi > 2 || cfg->gate_constant == cfg->gate_pi)
        return fail(ctx, GB_ERR_UNSUPPORTED, "gb_circuit_create takes the dummy circuit's gate set {Noop, Constant, PublicInput}; "
                                             "use gb_circuit_create_gates for other gate sets");
    // the same gate set in table form (the verifier reads it): [Noop, Constant, PublicInput] at the selector values given
    gbk::gates::GateSet gs{};
    gs.num_gates = 3;
    gs.num_selectors = 1;
    const u32 hout = cfg->field == GB_GOLDILOCKS ? 4 : 8;
    for (u32 g = 0; g < 3; g++) gs.g[g] = gb_gate{GB_GATE_NOOP, 0, 0, 0, 3};
    gs.g[cfg->gate_constant] = gb_gate{GB_GATE_CONSTANT, cfg->num_constants, 0, 0, 3};
    gs.g[cfg->gate_pi] = gb_gate{GB_GATE_PUBLIC_INPUT, hout, 0, 0, 3};
    return by_field(cfg->field, [&](auto f) { return circuit_create<decltype(f)>(ctx, cfg, gs, false, constants_sigmas, k_is, flags, out); });
}

gb_status gb_circuit_create(gb_ctx* ctx, const gb_circuit_config* cfg, const void* constants_sigmas, const void* k_is,
                            uint32_t flags, gb_circuit** out) try {
    return circuit_create_dummy(ctx, cfg, constants_sigmas, k_is, flags, out);
} GB_CATCH(ctx)
// constants_sigmas_vecs as build() holds them (circuit_builder.rs:1198-1229: Vec<PolynomialValues<F>>): one pointer per column
gb_status gb_circuit_create_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const void* const* constants_sigmas_cols, const void* k_is,
                                 uint32_t flags, gb_circuit** out) try {
    return circuit_create_dummy(ctx, cfg, ColSrc::columns(constants_sigmas_cols), k_is, flags, out);
} GB_CATCH(ctx)

static gb_status circuit_create_general(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                        ColSrc constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out,
                                        const ProgramTable* table = nullptr) {
    if (gb_status s = check_circuit_cfg(ctx, cfg, constants_sigmas, k_is, flags, out)) return s;
    gbk::gates::GateSet gs{};
    ParsedPrograms progs;
    return by_field(cfg->field, [&](auto f) -> gb_status {
        typedef decltype(f) F;
        if (table)
            if (gb_status s = parse_programs<F>(ctx, cfg, table->words, table->offsets, table->num_programs, &progs)) return s;
        if (gb_status s = build_gate_set<F>(ctx, cfg, gates, num_gates, &gs, table ? &progs.set : nullptr)) return s;
        return circuit_create<F>(ctx, cfg, gs, true, constants_sigmas, k_is, flags, out, &progs);
    });
}

gb_status gb_circuit_create_gates(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                  const void* constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out) try {
    return circuit_create_general(ctx, cfg, gates, num_gates, constants_sigmas, k_is, flags, out);
} GB_CATCH(ctx)
gb_status gb_circuit_create_gates_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                       const void* const* constants_sigmas_cols, const void* k_is, uint32_t flags, gb_circuit** out) try {
    return circuit_create_general(ctx, cfg, gates, num_gates, ColSrc::columns(constants_sigmas_cols), k_is, flags, out);
} GB_CATCH(ctx)

gb_status gb_circuit_create_programs(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                     const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                     const void* constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out) try {
    const ProgramTable table{program_words, program_offsets, num_programs};
    return circuit_create_general(ctx, cfg, gates, num_gates, constants_sigmas, k_is, flags, out, &table);
} GB_CATCH(ctx)
gb_status gb_circuit_create_programs_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                          const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                          const void* const* constants_sigmas_cols, const void* k_is, uint32_t flags,
                                          gb_circuit** out) try {
    const ProgramTable table{program_words, program_offsets, num_programs};
    return circuit_create_general(ctx, cfg, gates, num_gates, ColSrc::columns(constants_sigmas_cols), k_is, flags, out, &table);
} GB_CATCH(ctx)

static gb_status verifier_create_checked(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                         const void* k_is, const void* constants_sigmas_cap, const void* circuit_digest,
                                         gb_circuit** out, const ProgramTable* table) {
    if (!cfg || !k_is || !constants_sigmas_cap || !circuit_digest || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->field != GB_GOLDILOCKS && cfg->field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (cfg->num_challenges == 0 || cfg->num_routed_wires == 0 || cfg->num_routed_wires > cfg->num_wires ||
        cfg->max_quotient_degree_factor == 0 || cfg->arity_bits > 8 || cfg->cap_height > 24 ||
        cfg->degree_bits + cfg->rate_bits > (cfg->field == GB_GOLDILOCKS ? 32u : 27u) || cfg->num_wires > 4096)
        return fail(ctx, GB_ERR_INVALID, "bad circuit config");
    return by_field(cfg->field, [&](auto f) {
        return verifier_create<decltype(f)>(ctx, cfg, gates, num_gates, k_is, constants_sigmas_cap, circuit_digest, out, table);
    });
}
gb_status gb_verifier_create(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates, const void* k_is,
                             const void* constants_sigmas_cap, const void* circuit_digest, gb_circuit** out) try {
    return verifier_create_checked(ctx, cfg, gates, num_gates, k_is, constants_sigmas_cap, circuit_digest, out, nullptr);
} GB_CATCH(ctx)
gb_status gb_verifier_create_programs(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                      const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                      const void* k_is, const void* constants_sigmas_cap, const void* circuit_digest,
                                      gb_circuit** out) try {
    const ProgramTable table{program_words, program_offsets, num_programs};
    return verifier_create_checked(ctx, cfg, gates, num_gates, k_is, constants_sigmas_cap, circuit_digest, out, &table);
} GB_CATCH(ctx)

gb_status gb_circuit_free(gb_circuit* c) try {
    if (!c) return GB_OK;
    if (c->ctx) {
        (void)hipSetDevice(c->ctx->device);
        (void)hipStreamSynchronize(c->ctx->stream);
    }
    c->drop_retry();
    c->drop_partition();
    c->drop_check();
    c->release();
    delete c;
    return GB_OK;
} GB_CATCH(nullptr)   // (the object may be gone: the message goes to the thread's own slot)

gb_status gb_circuit_constants_sigmas_commitment(gb_circuit* c, gb_batch** out) try {
    if (!c || !out) return fail(c ? c->ctx : nullptr, GB_ERR_INVALID, "null argument");
    if (c->verify_only) return fail(c->ctx, GB_ERR_INVALID, "this circuit object was made by gb_verifier_create: it holds no commitment");
    *out = by_field(c, [](auto* cf) { return cf->cs; });
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

gb_status gb_circuit_verifier_data(gb_circuit* c, void* cap_out, void* digest_out) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    c->verifier_data(cap_out, digest_out);
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// FriParams.reduction_arity_bits for a circuit whose FriReductionStrategy is not ConstantArityBits (fri/reduction_strategies.rs:29-56)
gb_status gb_circuit_set_fri_reduction_arity_bits(gb_circuit* c, const uint32_t* arity_bits, uint32_t num_layers) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    gb_ctx* ctx = c->ctx;
    if (gb_status s = check_fri_reduction_arity_bits(ctx, c->cfg.degree_bits, c->cfg.rate_bits, c->cfg.cap_height, arity_bits, num_layers)) return s;
    c->arity_bits.assign(arity_bits, arity_bits + num_layers);
    c->arity_pending = false;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

gb_status gb_circuit_fri_reduction_arity_bits(gb_circuit* c, uint32_t* arity_bits_out, uint32_t* num_layers_out) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (!arity_bits_out || !num_layers_out) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    const size_t nl = std::min<size_t>(c->arity_bits.size(), GB_MAX_FRI_LAYERS);
    for (size_t i = 0; i < nl; i++) arity_bits_out[i] = c->arity_bits[i];
    *num_layers_out = (uint32_t)nl;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// What every gb_prove* entry checks of its proof buffer and its salts, behind the checks of its own witness argument (all of
// them GB_ERR_INVALID): the matrix entries below, the witness fronts of witness_host.inc
static gb_status prove_guard(gb_circuit* c, uint32_t flags, const void* salts, const size_t* proof_len) {
    gb_ctx* ctx = c->ctx;
    if (!proof_len) return fail(ctx, GB_ERR_INVALID, "null argument");
    if ((flags & GB_SALTS_FROM_SEED) && !salts) return fail(ctx, GB_ERR_INVALID, "GB_SALTS_FROM_SEED without a seed (salts is null)");
    if (c->cfg.zero_knowledge && !salts)
        return fail(ctx, GB_ERR_INVALID, "a zero-knowledge circuit is proved with salts (a host input, as for gb_prove_salted)");
    if (!c->cfg.zero_knowledge && salts) return fail(ctx, GB_ERR_INVALID, "salts given for a circuit without zero_knowledge");
    return need_arity_list(c);
}

static gb_status prove_entry(gb_circuit* c, ColSrc witness, uint32_t flags, const uint64_t* public_inputs,
                             size_t num_public_inputs, const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len,
                             const RetryHint* hint = nullptr) {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    gb_ctx* ctx = c->ctx;
    if (!witness) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (flags & ~GB_PROVE_FLAGS) return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    if (witness.ptrs && !c->verify_only)
        for (u32 w = 0; w < c->cfg.num_wires; w++)
            if (!witness.ptrs[w]) return fail(ctx, GB_ERR_INVALID, "null wire column pointer");
    if (num_public_inputs && !public_inputs) return fail(ctx, GB_ERR_INVALID, "null public inputs");
    if (num_public_inputs != c->cfg.num_public_inputs)  // the reference reads them off the witness: always CommonCircuitData's count
        return fail(ctx, GB_ERR_INVALID, "Number of public inputs doesn't match circuit data.");
    if (c->verify_only) return fail(ctx, GB_ERR_INVALID, "this circuit object was made by gb_verifier_create: it can only verify");
    if (gb_status s = prove_guard(c, flags, salts, proof_len)) return s;
    return by_field(c, [&](auto* cf) {
        return prove(cf, witness, flags, public_inputs, num_public_inputs, salts, proof_out, proof_cap, proof_len, hint);
    });
}

gb_status gb_prove(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs,
                   void* proof_out, size_t proof_cap, size_t* proof_len) try {
    return prove_entry(c, witness, flags, public_inputs, num_public_inputs, nullptr, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_retry(gb_circuit* c, const void* witness, uint32_t flags, uint32_t wire, uint64_t row, const uint64_t* public_inputs,
                         size_t num_public_inputs, void* proof_out, size_t proof_cap, size_t* proof_len) try {
    const RetryHint hint{wire, row};
    return prove_entry(c, witness, flags, public_inputs, num_public_inputs, nullptr, proof_out, proof_cap, proof_len, &hint);
} GB_CATCH_CIRCUIT(c)

gb_status gb_circuit_drop_retry(gb_circuit* c) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (c->ctx && (c->retry.wires || c->retry.wit_vals || c->retry.seg.state)) {
        HIP_TRY(c->ctx, hipSetDevice(c->ctx->device));
        HIP_TRY(c->ctx, hipStreamSynchronize(c->ctx->stream));
    }
    c->drop_retry();
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_salted(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs,
                          size_t num_public_inputs, const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len) try {
    if (c && !salts) return fail(c->ctx, GB_ERR_INVALID, "null salts");
    return prove_entry(c, witness, flags, public_inputs, num_public_inputs, salts, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

// the same three over MatrixWitness.wire_values as the reference holds it: num_wires separately allocated columns
gb_status gb_prove_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const uint64_t* public_inputs,
                        size_t num_public_inputs, void* proof_out, size_t proof_cap, size_t* proof_len) try {
    return prove_entry(c, ColSrc::columns(wire_cols), flags, public_inputs, num_public_inputs, nullptr, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_retry_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, uint32_t wire, uint64_t row,
                              const uint64_t* public_inputs, size_t num_public_inputs, void* proof_out, size_t proof_cap,
                              size_t* proof_len) try {
    const RetryHint hint{wire, row};
    return prove_entry(c, ColSrc::columns(wire_cols), flags, public_inputs, num_public_inputs, nullptr, proof_out, proof_cap, proof_len, &hint);
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_salted_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const uint64_t* public_inputs,
                               size_t num_public_inputs, const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len) try {
    if (c && !salts) return fail(c->ctx, GB_ERR_INVALID, "null salts");
    return prove_entry(c, ColSrc::columns(wire_cols), flags, public_inputs, num_public_inputs, salts, proof_out, proof_cap, proof_len);
} GB_CATCH_CIRCUIT(c)

// test hook (include/goldibear_gpu_test_hooks.h): the next gb_prove* on the circuit reports InvZeroPermArg once its Z computation is done
gb_status gb_test_arm_perm_arg_failure(gb_circuit* c) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    c->test_fail_next_perm_arg = true;
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

// test hooks (include/goldibear_gpu_test_hooks.h): the dispatch of kernels_gates.hip's short-gate launch on this context, and how
// often it took the lane-per-point kernel
gb_status gb_test_force_gate_fallback(gb_ctx* ctx, int on) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null context");
    ctx->test_force_gate_fallback = on != 0;
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_test_gate_fallback_launches(gb_ctx* ctx, uint64_t* count) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null context");
    if (!count) return fail(ctx, GB_ERR_INVALID, "null argument");
    *count = ctx->test_gate_fallback_launches;
    return GB_OK;
} GB_CATCH(ctx)

static gb_status stage_guard(gb_circuit* c) {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (c->verify_only) return fail(c->ctx, GB_ERR_INVALID, "this circuit object was made by gb_verifier_create: it can only verify");
    return GB_OK;
}

static gb_status zs_entry(gb_circuit* c, ColSrc witness, uint32_t flags, const void* betas, const void* gammas, void* values_out) {
    if (gb_status s = stage_guard(c)) return s;
    if (!witness || !betas || !gammas || !values_out) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    if (flags & ~GB_PUBLIC_INPUT_FLAGS) return fail(c->ctx, GB_ERR_INVALID, "unknown bits in flags");
    if (witness.ptrs)
        for (u32 w = 0; w < c->cfg.num_routed_wires; w++)
            if (!witness.ptrs[w]) return fail(c->ctx, GB_ERR_INVALID, "null wire column pointer");
    return by_field(c, [&](auto* cf) { return abi_zs_partial_products(cf, witness, flags, betas, gammas, values_out); });
}

gb_status gb_zs_partial_products(gb_circuit* c, const void* witness, uint32_t flags, const void* betas, const void* gammas,
                                 void* values_out) try {
    return zs_entry(c, witness, flags, betas, gammas, values_out);
} GB_CATCH_CIRCUIT(c)

gb_status gb_zs_partial_products_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const void* betas, const void* gammas,
                                      void* values_out) try {
    return zs_entry(c, ColSrc::columns(wire_cols), flags, betas, gammas, values_out);
} GB_CATCH_CIRCUIT(c)

gb_status gb_quotient_polys(gb_circuit* c, gb_batch* wires, gb_batch* zs_partial_products, const void* public_inputs_hash,
                            const void* betas, const void* gammas, const void* alphas, uint32_t flags, void* chunks_out) try {
    if (gb_status s = stage_guard(c)) return s;
    if (!public_inputs_hash || !betas || !gammas || !alphas || !chunks_out) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    return by_field(c, [&](auto* cf) {
        return abi_quotient_polys(cf, wires, zs_partial_products, public_inputs_hash, betas, gammas, alphas, flags, chunks_out);
    });
} GB_CATCH_CIRCUIT(c)

gb_status gb_prove_openings(gb_circuit* c, gb_batch* wires, gb_batch* zs_partial_products, gb_batch* quotient, const void* zeta,
                            gb_challenger_state* challenger, void* fri_proof_out, size_t fri_proof_cap, size_t* fri_proof_len) try {
    if (gb_status s = stage_guard(c)) return s;
    if (gb_status s = need_arity_list(c)) return s;
    if (!zeta || !challenger || !fri_proof_len) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    return by_field(c, [&](auto* cf) {
        return abi_prove_openings(cf, wires, zs_partial_products, quotient, zeta, challenger, fri_proof_out, fri_proof_cap, fri_proof_len);
    });
} GB_CATCH_CIRCUIT(c)

gb_status gb_fri_prove_openings(gb_ctx* ctx, gb_batch* const* oracles, uint32_t num_oracles, const void* points,
                                const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials,
                                const uint32_t* reduction_arity_bits, uint32_t num_layers, uint32_t proof_of_work_bits,
                                uint32_t num_query_rounds, gb_challenger_state* challenger, void* fri_proof_out,
                                size_t fri_proof_cap, size_t* fri_proof_len) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null context");
    if (!num_oracles) return fail(ctx, GB_ERR_INVALID, "a FRI instance needs at least one oracle");
    if (!oracles || !points || !challenger || !fri_proof_len) return fail(ctx, GB_ERR_INVALID, "null argument");
    std::vector<uint32_t> num_polys(num_oracles);
    for (u32 o = 0; o < num_oracles; o++) {
        const gb_batch* b = oracles[o];
        const std::string what = "oracle " + std::to_string(o);
        if (!b) return fail(ctx, GB_ERR_INVALID, what + " is null");
        if (b->ctx != ctx || b->field != oracles[0]->field) return fail(ctx, GB_ERR_INVALID, what + " belongs to another context or field");
        if (!b->coeffs) return fail(ctx, GB_ERR_INVALID, what + " is a stand-alone Merkle tree, not a polynomial batch");
        if (b->log_n != oracles[0]->log_n || b->rate_bits != oracles[0]->rate_bits || b->cap_height != oracles[0]->cap_height)
            return fail(ctx, GB_ERR_INVALID, what + " differs from oracle 0 in degree_bits, rate_bits or cap_height");
        num_polys[o] = (uint32_t)b->ncols;
    }
    if (gb_status s = check_fri_instance_lists(ctx, num_polys.data(), num_oracles, batch_sizes, num_batches, polynomials)) return s;
    const gb_batch* b0 = oracles[0];
    if (gb_status s = check_fri_reduction_arity_bits(ctx, b0->log_n, b0->rate_bits, b0->cap_height, reduction_arity_bits, num_layers)) return s;
    if (proof_of_work_bits > 31) return fail(ctx, GB_ERR_INVALID, "proof_of_work_bits above 31");
    if (num_query_rounds == 0) return fail(ctx, GB_ERR_INVALID, "num_query_rounds is zero: a proof without queries proves nothing");
    if (num_query_rounds > GB_MAX_FRI_QUERY_ROUNDS) return fail(ctx, GB_ERR_INVALID, "more than GB_MAX_FRI_QUERY_ROUNDS query rounds");
    const std::vector<uint32_t> arity(reduction_arity_bits, reduction_arity_bits + num_layers);
    return by_field(b0->field, [&](auto f) {
        return abi_fri_prove_openings<decltype(f)>(ctx, oracles, num_oracles, points, batch_sizes, num_batches, polynomials, arity, proof_of_work_bits,
                                                   num_query_rounds, challenger, fri_proof_out, fri_proof_cap, fri_proof_len);
    });
} GB_CATCH(ctx)

}  // extern "C"

#include "witness_host.inc"
#include "check_host.inc"
#include "sigma_host.inc"

// gb_constraint_quotient and gb_constraint_eval (include/goldibear_gpu.h, "constraint systems over committed oracles"; included at
// the end of api.hip): the quotient of a caller's own constraints over any committed oracles, and the same constraints at the
// verifier's point.  Both run the table through constraint_system.hpp first; what it accepts needs no further check.  The quotient
// stage is k_constraint_quotient (kernels_constraints.hpp) on the first 2^qb coset blocks of the oracles' LDEs, then the tail
// gb_quotient_polys has (quotient_coset_ifft, prover_host.inc).

namespace {

template <class F>
gb_status abi_constraint_quotient(gb_ctx* ctx, gb_batch* const* oracles, u32 num_oracles, const gbk::constraints::System& sys,
                                  const void* params, u32 num_params, const void* alphas, u32 nch, u32 qb, uint32_t flags,
                                  void* chunks_out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const u32 lg = oracles[0]->log_n, r = oracles[0]->rate_bits, R = 1u << qb;
    const size_t n = (size_t)1 << lg, points = n << qb, nq = (size_t)nch << qb;
    hipStream_t st = ctx->stream;
    TmpAlloc tmp(ctx);
    gb_status s;
    // uniform tables, device form: [literals][params][alpha powers nch x nterms][zh R][zh_inv R] - every part at least one word, so
    // that no kernel argument is a null or a one-past-the-end pointer
    const u32 nterms = std::max(sys.total_constraints, 1u);
    std::vector<T> zh, zh_inv, mat, uni;
    quotient_domain_tables<F>(lg, qb, &zh, &zh_inv, &mat);
    for (u64 v : sys.lits) uni.push_back(F::enc((T)v));
    if (sys.lits.empty()) uni.push_back(F::zero());
    const size_t params_at = uni.size();
    for (u32 k = 0; k < num_params; k++) uni.push_back(F::enc(static_cast<const T*>(params)[k]));
    if (!num_params) uni.push_back(F::zero());
    const size_t apow_at = uni.size();
    for (u32 k = 0; k < nch; k++) {
        T x = F::one(), a = F::enc(static_cast<const T*>(alphas)[k]);
        for (u32 t = 0; t < nterms; t++) { uni.push_back(x); x = F::mul(x, a); }
    }
    const size_t zh_at = uni.size();
    uni.insert(uni.end(), zh.begin(), zh.end());
    uni.insert(uni.end(), zh_inv.begin(), zh_inv.end());
    std::vector<u64> code(sys.instrs.begin(), sys.instrs.end());   // [instruction words][cell words]
    if (code.empty()) code.push_back(0);
    const size_t cells_at = code.size();
    code.insert(code.end(), sys.cells.begin(), sys.cells.end());
    if (sys.cells.empty()) code.push_back(0);
    T *uni_dev, *mat_dev, *lo_dev, *hi_dev;
    u64* code_dev;
    if ((s = upload_tmp(ctx, tmp, uni, &uni_dev))) return s;
    if ((s = upload_tmp(ctx, tmp, code, &code_dev))) return s;
    if ((s = upload_tmp(ctx, tmp, mat, &mat_dev))) return s;
    // the quotient domain's generator powers, split as the circuits' tables are (circuit_create)
    const T wN = F::two_adic_generator(lg + qb);
    if ((s = upload_tmp(ctx, tmp, fpowers<F>(wN, 4096), &lo_dev))) return s;
    if ((s = upload_tmp(ctx, tmp, fpowers<F>(F::pow(wN, 4096), points > 4096 ? points / 4096 : 1), &hi_dev))) return s;
    T* qv = tmp.get<T>(nq * n);
    T* qc = tmp.get<T>(nq * n);
    T* chunks = tmp.get<T>(nq * n);
    T* l0 = sys.reads_lagrange ? tmp.get<T>(points) : nullptr;
    if (!qv || !qc || !chunks || (sys.reads_lagrange && !l0)) return fail(ctx, GB_ERR_OOM, "constraint quotient workspace");
    gbk::ConstraintParams<F> cp{};
    cp.log_n = lg; cp.rate_bits = qb; cp.stride_bits = lg + r; cp.num_programs = sys.num_programs; cp.nterms = nterms;
    cp.w_N = gbk::PowTab<F>{lo_dev, hi_dev, 12};
    cp.l0 = l0;
    for (u32 o = 0; o < num_oracles; o++) cp.lde[o] = (const T*)oracles[o]->lde;
    for (u32 i = 0; i < sys.num_programs; i++) cp.p[i] = sys.p[i];
    cp.max_regs = sys.max_regs;
    cp.instrs = code_dev; cp.cells = code_dev + cells_at;
    cp.lits = uni_dev; cp.params = uni_dev + params_at;
    {
        Scope sv(ctx, "constraint quotient: values");
        if (l0) gbk::l0_table<F>(lg, qb, cp.w_N, uni_dev + zh_at, l0, st);
        if (!gbk::constraint_quotient_values<F>(cp, nch, uni_dev + apow_at, uni_dev + zh_at + R, qv, st))
            return fail(ctx, GB_ERR_UNSUPPORTED, "no constraint-quotient kernel for this num_challenges");
    }
    if ((s = quotient_coset_ifft<F>(ctx, lg, qb, nch, qv, qc, mat_dev, chunks, "constraint quotient: IFFT"))) return s;
    HF::from_device_form(chunks, chunks, nq * n, st);
    HIP_TRY(ctx, hipMemcpyAsync(chunks_out, chunks, nq * n * sizeof(T), (flags & GB_INPUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    return GB_OK;
}

template <class F>
gb_status abi_constraint_eval(gb_ctx* ctx, u32 degree_bits, const gbk::constraints::System& sys, const void* cell_values,
                              const void* params, u32 num_params, const void* zeta_canon, const void* alphas, u32 nch, void* folded_out) {
    typedef typename F::T T;
    typedef typename F::E E;
    typedef gbk::gates::ExtAlg<F> A;
    namespace CS = gbk::constraints;
    constexpr u32 D = F::D;
    auto read_ext = [&](const T* w, const char* what, E* out) -> gb_status {
        E z = F::ezero();
        for (u32 k = 0; k < D; k++) {
            if ((u64)w[k] >= F::ORDER) return fail(ctx, GB_ERR_INVALID, std::string("non-canonical coordinate in ") + what);
            F::set_coord(z, k, F::enc(w[k]));
        }
        *out = z;
        return GB_OK;
    };
    E zeta;
    if (gb_status s = read_ext(static_cast<const T*>(zeta_canon), "zeta", &zeta)) return s;
    if (gb_status s = check_opening_point<F>(ctx, zeta, degree_bits)) return s;
    std::vector<E> cells(sys.total_cells);
    for (u32 i = 0; i < sys.total_cells; i++)
        if (gb_status s = read_ext(static_cast<const T*>(cell_values) + (size_t)i * D, "cell_values", &cells[i])) return s;
    // Z_H(zeta) = zeta^n - 1; L_first(zeta) = Z_H(zeta) / (n (zeta - 1)) (eval_l_0, plonk_common.rs:56-66; zeta is outside H, so
    // neither denominator is zero); L_last(zeta) = L_first(zeta w_n)
    const u64 n = (u64)1 << degree_bits;
    const E one = F::efrom(F::one());
    E zn = zeta;
    for (u32 i = 0; i < degree_bits; i++) zn = F::emul(zn, zn);
    const E z_h = F::esub(zn, one);
    auto l_first_at = [&](E x) { return F::emul(z_h, F::einv(F::escale(F::esub(x, one), F::enc(n)))); };
    const E l_first = l_first_at(zeta), l_last = l_first_at(F::escale(zeta, F::two_adic_generator(degree_bits)));
    std::vector<T> lits, pars(num_params);
    for (u64 v : sys.lits) lits.push_back(F::enc((T)v));
    if (lits.empty()) lits.push_back(F::zero());
    for (u32 k = 0; k < num_params; k++) pars[k] = F::enc(static_cast<const T*>(params)[k]);
    std::vector<E> cons;
    cons.reserve(sys.total_constraints);
    std::vector<E> regs(gbk::gates::MAX_PROGRAM_REGS, F::ezero());
    std::vector<u64> instrs(sys.instrs.begin(), sys.instrs.end());
    if (instrs.empty()) instrs.push_back(0);
    for (u32 g = 0; g < sys.num_programs; g++) {
        const CS::ProgramInfo& pi = sys.p[g];
        auto cell = [&](u32 c) { return cells[pi.cell_off + c]; };
        auto input = [&](u32 k) -> E {
            return k == CS::INPUT_X ? zeta : k == CS::INPUT_L_FIRST ? l_first : k == CS::INPUT_L_LAST ? l_last
                                                                                                      : F::efrom(pars[k - CS::NUM_BUILTIN_INPUTS]);
        };
        auto emit = [&](E v) { cons.push_back(v); };
        gbk::gates::run_program<F, A>(instrs.data() + pi.instr_off, pi.num_instrs, lits.data() + pi.lit_off,
                                      gbk::gates::ArrayRegs<E>{regs.data()}, cell, input, emit);
    }
    for (u32 k = 0; k < nch; k++) {
        const T a = F::enc(static_cast<const T*>(alphas)[k]);
        E acc = F::ezero();
        for (size_t t = cons.size(); t-- > 0;) acc = F::eadd(cons[t], F::escale(acc, a));   // Horner: sum_i alpha^i constraint_i
        for (u32 d = 0; d < D; d++) static_cast<T*>(folded_out)[(size_t)k * D + d] = (T)F::dec(F::coord(acc, d));
    }
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_constraint_quotient(gb_ctx* ctx, gb_batch* const* oracles, uint32_t num_oracles, const uint64_t* program_words,
                                 const uint32_t* program_offsets, uint32_t num_programs, const void* params, uint32_t num_params,
                                 const void* alphas, uint32_t num_challenges, uint32_t quotient_degree_bits, uint32_t flags,
                                 void* chunks_out) try {
    namespace CS = gbk::constraints;
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null context");
    if (!num_oracles) return fail(ctx, GB_ERR_INVALID, "a constraint system needs at least one oracle");
    if (num_oracles > CS::MAX_ORACLES) return fail(ctx, GB_ERR_INVALID, "more than GB_MAX_CONSTRAINT_ORACLES oracles");
    if (!oracles || !chunks_out) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (flags & ~(uint32_t)GB_INPUT_DEVICE) return fail(ctx, GB_ERR_INVALID, "flags other than GB_INPUT_HOST / GB_INPUT_DEVICE");
    uint32_t num_polys[CS::MAX_ORACLES];
    for (u32 o = 0; o < num_oracles; o++) {
        const gb_batch* b = oracles[o];
        const std::string what = "oracle " + std::to_string(o);
        if (!b) return fail(ctx, GB_ERR_INVALID, what + " is null");
        if (b->ctx != ctx || b->field != oracles[0]->field) return fail(ctx, GB_ERR_INVALID, what + " belongs to another context or field");
        if (!b->coeffs) return fail(ctx, GB_ERR_INVALID, what + " is a stand-alone Merkle tree, not a polynomial batch");
        if (b->log_n != oracles[0]->log_n || b->rate_bits != oracles[0]->rate_bits)
            return fail(ctx, GB_ERR_INVALID, what + " differs from oracle 0 in degree_bits or rate_bits");
        num_polys[o] = (uint32_t)std::min<size_t>(b->ncols, 0xFFFFFFFFu);
    }
    const gb_batch* b0 = oracles[0];
    if (quotient_degree_bits < 1 || quotient_degree_bits > CS::MAX_QUOTIENT_DEGREE_BITS)
        return fail(ctx, GB_ERR_INVALID, "quotient_degree_bits " + std::to_string(quotient_degree_bits) + " outside 1 .. 4");
    if (quotient_degree_bits > b0->rate_bits)
        return fail(ctx, GB_ERR_INVALID, "quotient_degree_bits " + std::to_string(quotient_degree_bits) + " above the oracles' rate_bits " +
                                             std::to_string(b0->rate_bits) + ": the quotient domain is part of their LDE");
    std::string msg;
    if (CS::check_counts(num_challenges, num_params, params, alphas, &msg)) return fail(ctx, GB_ERR_INVALID, msg);
    const bool gl = b0->field == GB_GOLDILOCKS;
    const u64 order = gl ? GlF::ORDER : BbF::ORDER;
    if (CS::check_canonical_words(params, num_params, gl ? 8 : 4, order, "param", &msg) ||
        CS::check_canonical_words(alphas, num_challenges, gl ? 8 : 4, order, "alpha", &msg))
        return fail(ctx, GB_ERR_INVALID, msg);
    CS::Shape sh;
    sh.order = order; sh.num_oracles = num_oracles; sh.oracle_num_polys = num_polys; sh.num_rows = (u64)1 << b0->log_n;
    sh.num_params = num_params; sh.max_degree = (1u << quotient_degree_bits) + 1;
    CS::System sys;
    if (CS::parse_system(program_words, program_offsets, num_programs, sh, &sys, &msg)) return fail(ctx, GB_ERR_INVALID, msg);
    return by_field(b0->field, [&](auto f) {
        return abi_constraint_quotient<decltype(f)>(ctx, oracles, num_oracles, sys, params, num_params, alphas, num_challenges,
                                                    quotient_degree_bits, flags, chunks_out);
    });
} GB_CATCH(ctx)

gb_status gb_constraint_eval(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, const uint64_t* program_words,
                             const uint32_t* program_offsets, uint32_t num_programs, const void* cell_values, const void* params,
                             uint32_t num_params, const void* zeta, const void* alphas, uint32_t num_challenges, void* folded_out) try {
    namespace CS = gbk::constraints;
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field");
    const bool gl = field == GB_GOLDILOCKS;
    if (degree_bits > (gl ? GlF::TWO_ADICITY : BbF::TWO_ADICITY)) return fail(ctx, GB_ERR_INVALID, "degree_bits exceeds the field's two-adicity");
    if (!zeta || !folded_out) return fail(ctx, GB_ERR_INVALID, "null argument");
    std::string msg;
    if (CS::check_counts(num_challenges, num_params, params, alphas, &msg)) return fail(ctx, GB_ERR_INVALID, msg);
    const u64 order = gl ? GlF::ORDER : BbF::ORDER;
    if (CS::check_canonical_words(params, num_params, gl ? 8 : 4, order, "param", &msg) ||
        CS::check_canonical_words(alphas, num_challenges, gl ? 8 : 4, order, "alpha", &msg))
        return fail(ctx, GB_ERR_INVALID, msg);
    CS::Shape sh;
    sh.order = order; sh.num_oracles = CS::MAX_ORACLES; sh.num_rows = (u64)1 << degree_bits; sh.num_params = num_params;
    CS::System sys;
    if (CS::parse_system(program_words, program_offsets, num_programs, sh, &sys, &msg)) return fail(ctx, GB_ERR_INVALID, msg);
    if (sys.total_cells && !cell_values) return fail(ctx, GB_ERR_INVALID, "null argument");
    return by_field(field, [&](auto f) {
        return abi_constraint_eval<decltype(f)>(ctx, degree_bits, sys, cell_values, params, num_params, zeta, alphas, num_challenges, folded_out);
    });
} GB_CATCH(ctx)

}  // extern "C"

// Host-side verify() for the proofs gb_prove produces (included at the end of api.hip, after prover_host.inc).
// The reference verifies on the CPU as well; this is its restatement for the gate sets of gates.hpp, so that a
// proof can be checked where it was made without the Rust crate (SURVEY.md 8(f).2):
//   plonk/verifier.rs:17-128          verify_with_challenges: vanishing(zeta) == Z_H(zeta) * sum_j zeta^(n j) t_j(zeta), then FRI
//   plonk/get_challenges.rs:26-101    the Fiat-Shamir replay (fri/challenges.rs:24-68 for the FRI part)
//   plonk/vanishing_poly.rs:40-170    eval_vanishing_poly for {NoopGate, ConstantGate, PublicInputGate<H>}
//   fri/verifier.rs:23-250            proof of work, initial Merkle paths, fri_combine_initial, the folding checks
//   hash/merkle_proofs.rs:54-76       verify_merkle_proof_to_cap
// Arithmetic runs on the field traits' device form (canonical u64 / Montgomery u32), hashes on canonical words.

namespace {

struct VerifyFail {
    gb_status code;
    std::string msg;
    // what gb_verify_batch reports beside the status (gb_verify_result): the GB_VCHECK_* of the checks gb_verify runs, the
    // query round and the oracle / layer of the FRI query checks
    u32 check = GB_VCHECK_NONE, query_round = UINT32_MAX, index = UINT32_MAX;
};
// The text gb_verify leaves in gb_last_error for each of its checks (gb_verify_check_text) and the status it returns
inline const char* vcheck_text(u32 check) {
    switch (check) {
    case GB_VCHECK_TRUNCATED: return "proof bytes are truncated";
    case GB_VCHECK_NON_CANONICAL: return "non-canonical field element in the proof";
    case GB_VCHECK_PI_IMPLAUSIBLE: return "implausible public input count";
    case GB_VCHECK_PI_COUNT: return "Number of public inputs doesn't match circuit data.";
    case GB_VCHECK_TRAILING: return "trailing bytes in proof";
    case GB_VCHECK_VANISHING: return "vanishing polynomial identity failed at zeta (plonk/verifier.rs:87-95)";
    case GB_VCHECK_POW: return "Invalid proof of work witness. (fri/verifier.rs:51-65)";
    case GB_VCHECK_INITIAL_PATH_LEN: return "Merkle path of the wrong length";
    case GB_VCHECK_INITIAL_PATH: return "initial Merkle path does not lead to the cap";
    case GB_VCHECK_CONSISTENCY: return "FRI consistency check failed (fri/verifier.rs:213-216)";
    case GB_VCHECK_LAYER_PATH_LEN: return "FRI layer Merkle path of the wrong length";
    case GB_VCHECK_LAYER_PATH: return "FRI layer Merkle path does not lead to the cap";
    case GB_VCHECK_FINAL_POLY: return "Final polynomial evaluation is invalid. (fri/verifier.rs:240-247)";
    // what a compressed proof alone can fail on (compress_host.inc), as gb_verify_compressed words it
    case GB_VCHECK_COMPRESSED_INDICES: return "the compressed proof's query indices are not the transcript's";
    case GB_VCHECK_COMPRESSED_MISSING_SIBLING: return "compressed Merkle proof is missing a sibling";
    case GB_VCHECK_COMPRESSED_TRAILING: return "trailing bytes in compressed proof";
    default: return "";
    }
}
inline gb_status vcheck_status(u32 check) {
    switch (check) {
    case GB_VCHECK_NONE: return GB_OK;
    case GB_VCHECK_VANISHING: case GB_VCHECK_POW: case GB_VCHECK_INITIAL_PATH: case GB_VCHECK_CONSISTENCY: case GB_VCHECK_LAYER_PATH:
    case GB_VCHECK_FINAL_POLY: case GB_VCHECK_COMPRESSED_INDICES: return GB_ERR_VERIFY;
    default: return GB_ERR_INVALID;
    }
}
[[noreturn]] inline void vfail(u32 check, u32 query_round = UINT32_MAX, u32 index = UINT32_MAX) {
    throw VerifyFail{vcheck_status(check), vcheck_text(check), check, query_round, index};
}

template <class F>
struct ProofReader {
    typedef typename F::T T;
    typedef typename F::E E;
    const uint8_t* p;
    size_t len, off = 0;
    void need(size_t n) {
        if (off + n > len) vfail(GB_VCHECK_TRUNCATED);
    }
    uint8_t u8() { need(1); return p[off++]; }
    u64 usize() { need(8); u64 v; std::memcpy(&v, p + off, 8); off += 8; return v; }
    T field_canonical() {  // hash/hash_types.rs:33-37 / :67-71
        need(sizeof(T));
        T v;
        std::memcpy(&v, p + off, sizeof(T));
        off += sizeof(T);
        const u64 order = F::ORDER_BITS == 64 ? 0xFFFFFFFF00000001ULL : 2013265921ULL;
        if ((u64)v >= order) vfail(GB_VCHECK_NON_CANONICAL);
        return v;
    }
    void canon_vec(std::vector<T>& out, size_t n) { out.resize(n); for (auto& x : out) x = field_canonical(); }
    E ext() {  // device form
        E e = F::ezero();
        for (u32 k = 0; k < F::D; k++) F::set_coord(e, k, F::enc(field_canonical()));
        return e;
    }
    void ext_vec(std::vector<E>& out, std::vector<T>& canon, size_t n) {  // device form + the canonical words for the transcript
        out.resize(n);
        for (size_t i = 0; i < n; i++) {
            E e = F::ezero();
            for (u32 k = 0; k < F::D; k++) {
                T c = field_canonical();
                canon.push_back(c);
                F::set_coord(e, k, F::enc(c));
            }
            out[i] = e;
        }
    }
};

template <class F>
struct HostHash;
template <>
struct HostHash<GlF> {
    u64 s[12] = {};   // the hasher policy of verify_query.hpp: one sponge state, canonical words
    void set_canonical(int i, u64 v) { s[i] = v; }
    void permute() { poseidon_gl_host::permute(s); }
    u64 out(int i) const { return s[i]; }
    static void two_to_one(const u64* l, const u64* r, u64* out) {  // hash/hashing.rs:76-96
        u64 st[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
        poseidon_gl_host::permute(st);
        std::memcpy(out, st, 4 * sizeof(u64));
    }
};
template <>
struct HostHash<BbF> {
    u32 s[16] = {};
    void set_canonical(int i, u32 v) { s[i] = v; }
    void permute() { poseidon2_bb_host::permute(s); }
    u32 out(int i) const { return s[i]; }
    static void two_to_one(const u32* l, const u32* r, u32* out) {
        u32 st[16];
        std::memcpy(st, l, 8 * sizeof(u32));
        std::memcpy(st + 8, r, 8 * sizeof(u32));
        poseidon2_bb_host::permute(st);
        std::memcpy(out, st, 8 * sizeof(u32));
    }
};

// hash/merkle_proofs.rs:54-76 (leaf and siblings canonical): verify_query.hpp's walk over the host permutation
template <class F>
bool merkle_verify(const std::vector<typename F::T>& leaf, u64 index, const typename F::T* cap, const std::vector<typename F::T>& siblings) {
    HostHash<F> h;
    return gbk::vq::merkle_path_ok<F>(h, reinterpret_cast<const unsigned char*>(leaf.data()), (u32)leaf.size(), index,
                                      reinterpret_cast<const unsigned char*>(siblings.data()), (u32)(siblings.size() / F::H), cap);
}

inline u64 rev_bits64(u64 x, u32 bits) { return gbk::vq::rev_bits(x, bits); }

template <class F>
bool eeq(const typename F::E& a, const typename F::E& b) { return gbk::vq::eeq<F>(a, b); }

// Shape of a proof for one circuit (what the (de)serialisers need from CommonCircuitData)
template <class F>
struct ProofShape {
    u32 lg, r, nch, capH, lgN, nr, nw, qdf, nchunks, num_prods, nconst, nlayers, nqr;
    u64 n, N;
    size_t ncs, nzs, nq, cap_elems, salt, final_len;
    size_t widths[4], row_widths[4];  // polynomials per oracle; leaf width = that + salt for the blinded oracles
    explicit ProofShape(const Circuit<F>* c) {
        const gb_circuit_config& cfg = c->cfg;
        lg = cfg.degree_bits; r = cfg.rate_bits; nch = cfg.num_challenges; capH = cfg.cap_height;
        lgN = lg + r; n = (u64)1 << lg; N = n << r;
        nr = cfg.num_routed_wires; nw = cfg.num_wires; qdf = cfg.max_quotient_degree_factor;
        nchunks = (nr + qdf - 1) / qdf; num_prods = nchunks - 1;
        nconst = cfg.num_selectors + cfg.num_constants;
        ncs = nconst + nr; nzs = (size_t)nch * (1 + num_prods); nq = (size_t)nch * qdf;
        cap_elems = (size_t)F::H << capH;
        nlayers = (u32)c->arity_bits.size();
        nqr = cfg.num_query_rounds;
        // FriParams.hiding: the blinded oracles' leaves end in SALT_SIZE salt elements, which the Merkle hash covers and
        // fri_combine_initial skips (fri/verifier.rs:155-162 unsalted_eval; plonk_common.rs:25-40: every oracle but constants/sigmas)
        salt = cfg.zero_knowledge ? GB_SALT_SIZE : 0;
        const size_t w[4] = {ncs, nw, nzs, nq};
        for (int o = 0; o < 4; o++) { widths[o] = w[o]; row_widths[o] = w[o] + (o ? salt : 0); }
        u32 total_arity = 0;
        for (u32 ab : c->arity_bits) total_arity += ab;
        final_len = (size_t)1 << (lg - total_arity);
    }
};

// A proof in memory: canonical words as they are serialised (and observed by the transcript) plus the openings in device form
template <class F>
struct ParsedProof {
    typedef typename F::T T;
    typedef typename F::E E;
    std::vector<T> wires_cap, zs_cap, quot_cap;
    std::vector<E> o_const, o_sig, o_w, o_z, o_zn, o_pp, o_q;
    std::vector<T> t_const, t_sig, t_w, t_z, t_zn, t_pp, t_q;  // canonical words, transcript order inside each list
    std::vector<std::vector<T>> layer_caps;
    struct Query {
        std::vector<std::vector<T>> rows = std::vector<std::vector<T>>(4), paths = rows;   // per oracle (four in a PLONK proof)
        std::vector<std::vector<T>> step_rows, step_paths;  // step_rows: D * arity canonical words
    };
    std::vector<Query> queries;
    std::vector<E> final_poly;
    std::vector<T> t_final;
    T pow_witness = 0;
    std::vector<T> pis;
};

// FriProof (util/serialization/mod.rs:1679-1695 read side) in two pieces - a compressed proof shares only the first:
// commit_phase_merkle_caps, then query_round_proofs, final_poly and pow_witness.  row_widths[o]: the leaf width of oracle o.
template <class F>
void parse_fri_caps(ProofReader<F>& rd, u32 nlayers, size_t cap_elems, ParsedProof<F>& p) {
    p.layer_caps.resize(nlayers);
    for (auto& lc : p.layer_caps) rd.canon_vec(lc, cap_elems);
}
template <class F>
void parse_fri_queries(ProofReader<F>& rd, const size_t* row_widths, u32 num_oracles, const std::vector<uint32_t>& arity_bits, u32 nqr,
                       size_t final_len, ParsedProof<F>& p) {
    constexpr u32 D = F::D, H = F::H;
    const u32 nlayers = (u32)arity_bits.size();
    p.queries.resize(nqr);
    for (auto& q : p.queries) {
        q.rows.resize(num_oracles);
        q.paths.resize(num_oracles);
        for (u32 o = 0; o < num_oracles; o++) {
            rd.canon_vec(q.rows[o], row_widths[o]);
            rd.canon_vec(q.paths[o], (size_t)rd.u8() * H);
        }
        q.step_rows.resize(nlayers);
        q.step_paths.resize(nlayers);
        for (u32 li = 0; li < nlayers; li++) {
            rd.canon_vec(q.step_rows[li], (size_t)D << arity_bits[li]);
            rd.canon_vec(q.step_paths[li], (size_t)rd.u8() * H);
        }
    }
    rd.ext_vec(p.final_poly, p.t_final, final_len);
    p.pow_witness = rd.field_canonical();
}

template <class F>
void parse_caps_and_openings(ProofReader<F>& rd, const ProofShape<F>& sh, ParsedProof<F>& p) {
    rd.canon_vec(p.wires_cap, sh.cap_elems);
    rd.canon_vec(p.zs_cap, sh.cap_elems);
    rd.canon_vec(p.quot_cap, sh.cap_elems);
    rd.ext_vec(p.o_const, p.t_const, sh.nconst);
    rd.ext_vec(p.o_sig, p.t_sig, sh.nr);
    rd.ext_vec(p.o_w, p.t_w, sh.nw);
    rd.ext_vec(p.o_z, p.t_z, sh.nch);
    rd.ext_vec(p.o_zn, p.t_zn, sh.nch);
    rd.ext_vec(p.o_pp, p.t_pp, (size_t)sh.nch * sh.num_prods);
    rd.ext_vec(p.o_q, p.t_q, sh.nq);
    parse_fri_caps(rd, sh.nlayers, sh.cap_elems, p);
}

// util/serialization/mod.rs:2103-2151 read side
template <class F>
void parse_proof(const Circuit<F>* c, const ProofShape<F>& sh, const uint8_t* bytes, size_t len, ParsedProof<F>& p) {
    ProofReader<F> rd{bytes, len};
    parse_caps_and_openings(rd, sh, p);
    parse_fri_queries(rd, sh.row_widths, 4, c->arity_bits, sh.nqr, sh.final_len, p);
    const u64 npis = rd.usize();
    if (npis > (1u << 20)) vfail(GB_VCHECK_PI_IMPLAUSIBLE);
    // validate_proof_with_pis_shape (plonk/validate_shape.rs:22-25): hash_no_pad does not pad, so a proof re-serialised with
    // zero public inputs appended or stripped keeps its transcript - only the count tells it from the honest one
    if (npis != c->cfg.num_public_inputs) vfail(GB_VCHECK_PI_COUNT);
    rd.canon_vec(p.pis, (size_t)npis);
    if (rd.off != len) vfail(GB_VCHECK_TRAILING);
}

// plonk/get_challenges.rs:26-101 (fri/challenges.rs:24-68 for the FRI part); field challenges in device form
template <class F>
struct Challenges {
    typedef typename F::T T;
    typedef typename F::E E;
    T pi_hash[F::H];
    std::vector<T> betas, gammas, alphas;
    E zeta, fri_alpha;
    std::vector<E> fri_betas;
    u64 pow_response;
    std::vector<u64> x_indices;
};
// fri/challenges.rs:24-68 from the transcript after the openings were observed
template <class F>
void get_fri_challenges(typename Host<F>::Challenger& ch, const ParsedProof<F>& p, u32 nqr, u64 N, Challenges<F>& out) {
    out.fri_alpha = get_ext_challenge<F>(ch);
    out.fri_betas.resize(p.layer_caps.size());
    for (size_t li = 0; li < p.layer_caps.size(); li++) {
        ch.observe(p.layer_caps[li].data(), p.layer_caps[li].size());
        out.fri_betas[li] = get_ext_challenge<F>(ch);
    }
    ch.observe(p.t_final.data(), p.t_final.size());
    ch.observe(p.pow_witness);
    out.pow_response = ch.get();
    out.x_indices.resize(nqr);
    for (auto& x : out.x_indices) x = (u64)ch.get() % N;
}
template <class F>
void get_challenges(const Circuit<F>* c, const ProofShape<F>& sh, const ParsedProof<F>& p, Challenges<F>& out) {
    typedef typename F::E E;
    typedef Host<F> HF;
    constexpr u32 D = F::D, H = F::H;
    HF::hash_no_pad(p.pis.data(), p.pis.size(), out.pi_hash);
    typename HF::Challenger ch;
    auto get_ext = [&]() {
        E e = F::ezero();
        for (u32 k = 0; k < D; k++) F::set_coord(e, k, F::enc(ch.get()));
        return e;
    };
    ch.observe(c->digest, H);
    ch.observe(out.pi_hash, H);
    ch.observe(p.wires_cap.data(), p.wires_cap.size());
    out.betas.resize(sh.nch); out.gammas.resize(sh.nch); out.alphas.resize(sh.nch);
    for (auto& b : out.betas) b = F::enc(ch.get());
    for (auto& g : out.gammas) g = F::enc(ch.get());
    ch.observe(p.zs_cap.data(), p.zs_cap.size());
    for (auto& a : out.alphas) a = F::enc(ch.get());
    ch.observe(p.quot_cap.data(), p.quot_cap.size());
    out.zeta = get_ext();
    // observe_openings (plonk/proof.rs:388-440): zeta batch, then the zeta_next batch
    ch.observe(p.t_const.data(), p.t_const.size());
    ch.observe(p.t_sig.data(), p.t_sig.size());
    ch.observe(p.t_w.data(), p.t_w.size());
    ch.observe(p.t_z.data(), p.t_z.size());
    ch.observe(p.t_pp.data(), p.t_pp.size());
    ch.observe(p.t_q.data(), p.t_q.size());
    ch.observe(p.t_zn.data(), p.t_zn.size());
    get_fri_challenges<F>(ch, p, sh.nqr, sh.N, out);
}

// FriInstanceInfo (fri/structure.rs) with what the checks need of FriParams
template <class F>
struct FriInstance {
    u32 lg = 0, r = 0, capH = 0, lgN = 0;
    std::vector<size_t> widths, row_widths;   // per oracle: its polynomials; its leaf width (salted = hiding && blinding: + SALT_SIZE)
    struct Batch {
        typename F::E point;
        std::vector<std::pair<u32, u32>> polys;   // (oracle_index, polynomial_index)
    };
    std::vector<Batch> batches;
};
// get_fri_instance(zeta) (plonk/circuit_data.rs:438-520): every polynomial of the four oracles at zeta, the Zs also at g zeta -
// and the proof's opening set in that order (FriOpenings, plonk/proof.rs:388-440)
template <class F>
FriInstance<F> plonk_fri_instance(const ProofShape<F>& sh, typename F::E zeta) {
    FriInstance<F> in;
    in.lg = sh.lg; in.r = sh.r; in.capH = sh.capH; in.lgN = sh.lgN;
    in.widths.assign(sh.widths, sh.widths + 4);
    in.row_widths.assign(sh.row_widths, sh.row_widths + 4);
    in.batches.resize(2);
    in.batches[0].point = zeta;
    for (u32 o = 0; o < 4; o++)
        for (u32 i = 0; i < sh.widths[o]; i++) in.batches[0].polys.emplace_back(o, i);
    in.batches[1].point = F::escale(zeta, F::two_adic_generator(sh.lg));
    for (u32 i = 0; i < sh.nch; i++) in.batches[1].polys.emplace_back(2u, i);
    return in;
}
template <class F>
std::vector<std::vector<typename F::E>> plonk_fri_openings(const ParsedProof<F>& p) {
    std::vector<std::vector<typename F::E>> o(2);
    for (const auto* l : {&p.o_const, &p.o_sig, &p.o_w, &p.o_z, &p.o_pp, &p.o_q}) o[0].insert(o[0].end(), l->begin(), l->end());
    o[1] = p.o_zn;
    return o;
}

// The arithmetic of one FRI query (fri/verifier.rs:23-49, 121-165): the combined initial evaluation and the fold of a coset
template <class F>
struct FriQueryMath {
    typedef typename F::T T;
    typedef typename F::E E;
    const FriInstance<F> inst;
    const E fri_alpha;
    std::vector<E> red_open, alpha_shift;   // per batch: reduce(openings) (PrecomputedReducedOpenings), alpha^(size of the batch)
    std::vector<E> points;                  // per batch, and its size: the flat form verify_query.hpp takes
    std::vector<u32> sizes;
    T wN;
    // openings[b]: the claimed values of batch b's polynomials at its point, in the batch's order
    FriQueryMath(FriInstance<F> in, const std::vector<std::vector<E>>& openings, E alpha) : inst(std::move(in)), fri_alpha(alpha) {
        for (size_t b = 0; b < inst.batches.size(); b++) {
            E acc = F::ezero();   // ReducingFactor::reduce (util/reducing.rs:56-59)
            for (size_t i = openings[b].size(); i-- > 0;) acc = F::eadd(F::emul(fri_alpha, acc), openings[b][i]);
            red_open.push_back(acc);
            alpha_shift.push_back(gbk::epow<F>(fri_alpha, inst.batches[b].polys.size()));
            points.push_back(inst.batches[b].point);
            sizes.push_back((u32)inst.batches[b].polys.size());
        }
        wN = F::two_adic_generator(inst.lgN);
    }
    FriQueryMath(const ProofShape<F>& s, const ParsedProof<F>& p, const Challenges<F>& c)
        : FriQueryMath(plonk_fri_instance<F>(s, c.zeta), plonk_fri_openings<F>(p), c.fri_alpha) {}
    T subgroup_x(u64 x_index) const { return gbk::vq::subgroup_x<F>(inst.lgN, x_index); }
    // fri_combine_initial: rows[o] = the opened leaf of oracle o (salts, if any, at the end and never indexed)
    E combine_initial(const std::vector<T>* rows, T x) const {
        return gbk::vq::combine_initial<F>((u32)sizes.size(), sizes.data(), points.data(), red_open.data(), alpha_shift.data(), fri_alpha, x,
                                           [&](u32 b, u32 i) {
                                               const std::pair<u32, u32>& pl = inst.batches[b].polys[i];
                                               return rows[pl.first][pl.second];
                                           });
    }
    // compute_evaluation: interpolate the coset's values (bit-reversed order) at beta
    static E compute_evaluation(T x, u64 within, u32 ab, const std::vector<E>& evals, E beta) {
        return gbk::vq::compute_evaluation<F>(x, within, ab, beta, [&](u32 k) { return evals[k]; });
    }
    static std::vector<E> to_ext(const std::vector<T>& canon) {
        std::vector<E> out(canon.size() / F::D);
        for (size_t k = 0; k < out.size(); k++) {
            E e = F::ezero();
            for (u32 d = 0; d < F::D; d++) F::set_coord(e, d, F::enc(canon[F::D * k + d]));
            out[k] = e;
        }
        return out;
    }
};

// verify_fri_proof (fri/verifier.rs:67-250) after the transcript, in the two pieces gb_verify_batch needs apart: the proof of
// work, then per query round the initial Merkle paths, fri_combine_initial and the folding checks down to the final polynomial
// (verify_query.hpp).  initial_caps[o]: the cap of oracle o.
template <class F>
void check_pow(u32 proof_of_work_bits, const Challenges<F>& chal) {
    const u32 min_lz = proof_of_work_bits + (64 - F::ORDER_BITS);
    const u32 lz = chal.pow_response ? (u32)__builtin_clzll(chal.pow_response) : 64;
    if (lz < min_lz) vfail(GB_VCHECK_POW);
}
template <class F>
void verify_fri_queries(const FriQueryMath<F>& fri, const typename F::T* const* initial_caps, const std::vector<uint32_t>& arity_bits,
                        const ParsedProof<F>& pp, const Challenges<F>& chal) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 H = F::H;
    namespace vq = gbk::vq;
    const FriInstance<F>& in = fri.inst;
    const u32 nlayers = (u32)arity_bits.size(), noracles = (u32)in.widths.size();
    for (size_t qi = 0; qi < pp.queries.size(); qi++) {
        const typename ParsedProof<F>::Query& q = pp.queries[qi];
        const u64 x_index = chal.x_indices[qi];
        for (u32 o = 0; o < noracles; o++) {
            // the path length is part of the statement (hash/merkle_proofs.rs:62-75 indexes the cap with what is left of the index)
            if (q.paths[o].size() != (size_t)H * (in.lgN - in.capH)) vfail(GB_VCHECK_INITIAL_PATH_LEN, (u32)qi, o);
            if (!merkle_verify<F>(q.rows[o], x_index, initial_caps[o], q.paths[o])) vfail(GB_VCHECK_INITIAL_PATH, (u32)qi, o);
        }
        const T subgroup_x = fri.subgroup_x(x_index);
        const E old_eval = fri.combine_initial(q.rows.data(), subgroup_x);
        u32 height = in.lgN;
        const u32 pos = vq::fold_checks<F>(
            noracles, nlayers, arity_bits.data(), x_index, subgroup_x, old_eval, (u32)pp.final_poly.size(),
            [&](u32 li) { return reinterpret_cast<const unsigned char*>(q.step_rows[li].data()); },
            [&](u32 li) { return chal.fri_betas[li]; }, [&](u32 i) { return pp.final_poly[i]; },
            [&](u32 li, u64 coset_index) {
                height -= arity_bits[li];
                if (height < in.capH || q.step_paths[li].size() != (size_t)H * (height - in.capH)) vfail(GB_VCHECK_LAYER_PATH_LEN, (u32)qi, li);
                return merkle_verify<F>(q.step_rows[li], coset_index, pp.layer_caps[li].data(), q.step_paths[li]);
            });
        if (pos == ~0u) continue;
        if (pos == vq::pos_final(noracles, nlayers)) vfail(GB_VCHECK_FINAL_POLY, (u32)qi);
        const u32 li = (pos - noracles) / 2;
        vfail((pos - noracles) & 1 ? GB_VCHECK_LAYER_PATH : GB_VCHECK_CONSISTENCY, (u32)qi, li);
    }
}
template <class F>
void verify_fri_parsed(const FriQueryMath<F>& fri, const typename F::T* const* initial_caps, const std::vector<uint32_t>& arity_bits,
                       u32 proof_of_work_bits, const ParsedProof<F>& pp, const Challenges<F>& chal) {
    check_pow<F>(proof_of_work_bits, chal);
    verify_fri_queries<F>(fri, initial_caps, arity_bits, pp, chal);
}

// vanishing(zeta) == Z_H(zeta) * quotient(zeta)  (plonk/verifier.rs:60-95, vanishing_poly.rs:40-170)
template <class F>
void check_vanishing(const Circuit<F>* c, const ProofShape<F>& sh, const ParsedProof<F>& pp, const Challenges<F>& chal) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 H = F::H;
    const gb_circuit_config& cfg = c->cfg;
    const u32 lg = sh.lg, nch = sh.nch, nr = sh.nr, qdf = sh.qdf, nchunks = sh.nchunks, num_prods = sh.num_prods;
    const u64 n = sh.n;
    const E one = F::efrom(F::one());
    const std::vector<E>&o_const = pp.o_const, &o_sig = pp.o_sig, &o_w = pp.o_w, &o_z = pp.o_z, &o_zn = pp.o_zn, &o_pp = pp.o_pp,
                        &o_q = pp.o_q;
    const std::vector<T>&betas = chal.betas, &gammas = chal.gammas, &alphas = chal.alphas;
    const E zeta = chal.zeta;
    const T* pi_hash = chal.pi_hash;

    {
        E zn = zeta;
        for (u32 i = 0; i < lg; i++) zn = F::emul(zn, zn);
        const E z_h = F::esub(zn, one);
        // eval_l_0 (plonk_common.rs:56-66)
        E l0 = one;
        if (!eeq<F>(zeta, one))
            l0 = F::emul(z_h, F::einv(F::escale(F::esub(zeta, one), F::enc(n))));
        std::vector<E> terms;
        for (u32 i = 0; i < nch; i++) terms.push_back(F::emul(l0, F::esub(o_z[i], one)));
        for (u32 i = 0; i < nch; i++) {
            std::vector<E> nums(nr), dens(nr);
            for (u32 j = 0; j < nr; j++) {
                const E wg = F::eadd(o_w[j], F::efrom(gammas[i]));
                nums[j] = F::eadd(wg, F::escale(zeta, F::mul(betas[i], c->k_is_dev_host[j])));
                dens[j] = F::eadd(wg, F::escale(o_sig[j], betas[i]));
            }
            for (u32 m = 0; m < nchunks; m++) {
                E np = one, dp = one;
                for (u32 j = m * qdf; j < std::min((m + 1) * qdf, nr); j++) {
                    np = F::emul(np, nums[j]);
                    dp = F::emul(dp, dens[j]);
                }
                const E prev = m == 0 ? o_z[i] : o_pp[(size_t)i * num_prods + m - 1];
                const E next = m == num_prods ? o_zn[i] : o_pp[(size_t)i * num_prods + m];
                terms.push_back(F::esub(F::emul(prev, np), F::emul(next, dp)));
            }
        }
        // gate constraints: sum over the gate set of filter * unfiltered, per constraint index (vanishing_poly.rs:129-170,
        // gates/gate.rs:165-186, 391-404); the evaluators are the ones the quotient kernel runs (gates.hpp)
        {
            typedef gbk::gates::ExtAlg<F> A;
            std::vector<E> cons(c->num_gate_constraints, F::ezero());
            T pi_dev[H];
            for (u32 i = 0; i < H; i++) pi_dev[i] = F::enc(pi_hash[i]);
            auto wire = [&](u32 col) { return o_w[col]; };
            auto konst = [&](u32 i) { return o_const[cfg.num_selectors + i]; };
            const std::vector<T> prog_lits(c->prog_lits.begin(), c->prog_lits.end());   // device form, the field's word
            std::vector<E> prog_regs(gbk::gates::MAX_PROGRAM_REGS, F::ezero());
            for (u32 g = 0; g < c->gates.num_gates; g++) {
                const gb_gate& gd = c->gates.g[g];
                const E f = gbk::gates::filter<F, A>(g, gd, o_const[gd.selector_index], c->gates.num_selectors > 1);
                u32 idx = 0;
                auto emit = [&](E v) { cons[idx] = F::eadd(cons[idx], F::emul(f, v)); idx++; };
                if (gbk::gates::is_program(gd)) {   // the gate as data: the interpreter the quotient kernel runs, over the extension
                    const gbk::gates::ProgramInfo& pi = c->programs.p[gd.param];
                    gbk::gates::run_program<F, A>(c->prog_instrs.data() + pi.instr_off, pi.num_instrs, prog_lits.data() + pi.lit_off,
                                                  gbk::gates::ArrayRegs<E>{prog_regs.data()}, wire, konst, emit);
                    continue;
                }
                gbk::gates::eval_gate<F, A>(c->gates, gd, wire, konst, pi_dev, emit);
            }
            terms.insert(terms.end(), cons.begin(), cons.end());
        }
        for (u32 i = 0; i < nch; i++) {
            E van = F::ezero();
            for (size_t t = terms.size(); t-- > 0;) van = F::eadd(terms[t], F::escale(van, alphas[i]));
            E acc = F::ezero();
            for (u32 j = qdf; j-- > 0;) acc = F::eadd(F::emul(acc, zn), o_q[(size_t)i * qdf + j]);
            if (!eeq<F>(van, F::emul(z_h, acc))) vfail(GB_VCHECK_VANISHING);
        }
    }
}

template <class F>
void verify_parsed(Circuit<F>* c, const ProofShape<F>& sh, const ParsedProof<F>& pp) {
    typedef typename F::T T;
    const gb_circuit_config& cfg = c->cfg;
    Challenges<F> chal;
    get_challenges(c, sh, pp, chal);
    check_vanishing<F>(c, sh, pp, chal);

    // ---- FRI (fri/verifier.rs:67-250) on the PLONK instance
    const FriQueryMath<F> fri(sh, pp, chal);
    const T* initial_caps[4] = {c->cap_host.data(), pp.wires_cap.data(), pp.zs_cap.data(), pp.quot_cap.data()};
    verify_fri_parsed<F>(fri, initial_caps, c->arity_bits, cfg.proof_of_work_bits, pp, chal);
}

template <class F>
void verify_impl(Circuit<F>* c, const uint8_t* bytes, size_t len) {
    const ProofShape<F> sh(c);
    ParsedProof<F> pp;
    parse_proof(c, sh, bytes, len, pp);
    verify_parsed(c, sh, pp);
}

// An instance described by flat arrays (include/goldibear_gpu.h), for gb_fri_verify and gb_fri_verify_batch's host stage alike - the
// two must answer alike, so what they do to an item is written once:
//   fri_shape_instance   the shape (the lists have been checked) as a FriInstance whose points are still zero
//   fri_read_item        an item's points, openings and caps: canonical checks in gb_fri_verify's order, device form; a word >= p
//                        goes to bad(what), which throws
//   fri_read_proof       the FriProof bytes and the challenges drawn from `ch`; bytes left over go to trailing(), which throws
template <class F>
FriInstance<F> fri_shape_instance(u32 degree_bits, u32 rate_bits, u32 cap_height, bool hiding, const uint32_t* num_polys,
                                  const uint32_t* blinding, u32 num_oracles, const uint32_t* batch_sizes, u32 num_batches,
                                  const uint32_t* polynomials) {
    FriInstance<F> in;
    in.lg = degree_bits; in.r = rate_bits; in.capH = cap_height; in.lgN = degree_bits + rate_bits;
    for (u32 o = 0; o < num_oracles; o++) {
        in.widths.push_back(num_polys[o]);
        in.row_widths.push_back(num_polys[o] + (hiding && blinding[o] ? (size_t)GB_SALT_SIZE : 0));   // salted = hiding && blinding
    }
    in.batches.resize(num_batches);
    size_t at = 0;
    for (u32 b = 0; b < num_batches; b++) {
        in.batches[b].point = F::ezero();
        for (u32 j = 0; j < batch_sizes[b]; j++, at++) in.batches[b].polys.emplace_back(polynomials[2 * at], polynomials[2 * at + 1]);
    }
    return in;
}
template <class F, class Bad>
void fri_read_item(FriInstance<F>& in, const void* points, const void* openings, const void* caps, size_t cap_elems,
                   std::vector<std::vector<typename F::E>>& open, std::vector<const typename F::T*>& cap_ptrs, Bad bad) {
    typedef typename F::T T;
    typedef typename F::E E;
    auto ext_at = [&bad](const void* base, size_t i, const char* what) {
        E e = F::ezero();
        for (u32 k = 0; k < F::D; k++) {
            const T w = static_cast<const T*>(base)[i * F::D + k];
            if ((u64)w >= F::ORDER) bad(what);
            F::set_coord(e, k, F::enc(w));
        }
        return e;
    };
    open.assign(in.batches.size(), {});
    size_t at = 0;
    for (size_t b = 0; b < in.batches.size(); b++) {
        in.batches[b].point = ext_at(points, b, "the points");
        for (size_t j = 0; j < in.batches[b].polys.size(); j++, at++) open[b].push_back(ext_at(openings, at, "the openings"));
    }
    cap_ptrs.resize(in.widths.size());
    for (size_t o = 0; o < in.widths.size(); o++) {
        cap_ptrs[o] = static_cast<const T*>(caps) + o * cap_elems;
        for (size_t i = 0; i < cap_elems; i++)
            if ((u64)cap_ptrs[o][i] >= F::ORDER) bad("the initial caps");
    }
}
template <class F, class Trailing>
void fri_read_proof(const FriInstance<F>& in, const std::vector<uint32_t>& arity_bits, u32 nqr, size_t cap_elems, size_t final_len,
                    typename Host<F>::Challenger& ch, const uint8_t* bytes, size_t len, ParsedProof<F>& pp, Challenges<F>& chal,
                    Trailing trailing) {
    ProofReader<F> rd{bytes, len};
    parse_fri_caps(rd, (u32)arity_bits.size(), cap_elems, pp);
    parse_fri_queries(rd, in.row_widths.data(), (u32)in.widths.size(), arity_bits, nqr, final_len, pp);
    if (rd.off != len) trailing();
    get_fri_challenges<F>(ch, pp, nqr, (u64)1 << in.lgN, chal);
}
inline size_t fri_final_len(u32 degree_bits, const std::vector<uint32_t>& arity_bits) {
    u32 total_arity = 0;
    for (u32 ab : arity_bits) total_arity += ab;
    return (size_t)1 << (degree_bits - total_arity);
}

// verify_fri_proof (fri/verifier.rs:67-250) on an instance described by flat arrays; the lists have been checked, `ch` is the
// caller's transcript by value
template <class F>
void fri_verify_impl(u32 degree_bits, u32 rate_bits, u32 cap_height, bool hiding, const uint32_t* num_polys, const uint32_t* blinding,
                     u32 num_oracles, const void* points, const uint32_t* batch_sizes, u32 num_batches, const uint32_t* polynomials,
                     const void* openings, const void* caps, const std::vector<uint32_t>& arity_bits, u32 proof_of_work_bits, u32 nqr,
                     typename Host<F>::Challenger ch, const uint8_t* bytes, size_t len) {
    typedef typename F::T T;
    typedef typename F::E E;
    FriInstance<F> in = fri_shape_instance<F>(degree_bits, rate_bits, cap_height, hiding, num_polys, blinding, num_oracles, batch_sizes,
                                              num_batches, polynomials);
    const size_t cap_elems = (size_t)F::H << cap_height;
    std::vector<std::vector<E>> open;
    std::vector<const T*> cap_ptrs;
    fri_read_item<F>(in, points, openings, caps, cap_elems, open, cap_ptrs, [](const char* what) {
        throw VerifyFail{GB_ERR_INVALID, std::string("non-canonical field element in ") + what};
    });
    ParsedProof<F> pp;
    Challenges<F> chal;
    fri_read_proof<F>(in, arity_bits, nqr, cap_elems, fri_final_len(degree_bits, arity_bits), ch, bytes, len, pp, chal,
                      [] { throw VerifyFail{GB_ERR_INVALID, "trailing bytes in proof"}; });
    const FriQueryMath<F> fri(std::move(in), open, chal.fri_alpha);
    verify_fri_parsed<F>(fri, cap_ptrs.data(), arity_bits, proof_of_work_bits, pp, chal);
}

}  // namespace

extern "C" {

gb_status gb_fri_verify(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t hiding,
                        const uint32_t* oracle_num_polys, const uint32_t* oracle_blinding, uint32_t num_oracles, const void* points,
                        const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials, const void* openings,
                        const void* initial_caps, const uint32_t* reduction_arity_bits, uint32_t num_layers,
                        uint32_t proof_of_work_bits, uint32_t num_query_rounds, const gb_challenger_state* challenger,
                        const void* fri_proof, size_t fri_proof_len) try {
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field");
    if (!oracle_num_polys || !oracle_blinding || !points || !openings || !initial_caps || !challenger || !fri_proof)
        return fail(ctx, GB_ERR_INVALID, "null argument");
    const u32 two_adicity = field == GB_GOLDILOCKS ? GlF::TWO_ADICITY : BbF::TWO_ADICITY;
    if (degree_bits > two_adicity || rate_bits > two_adicity || degree_bits + rate_bits > two_adicity)
        return fail(ctx, GB_ERR_INVALID, "LDE size exceeds the field's two-adicity");
    if (cap_height > degree_bits + rate_bits) return fail(ctx, GB_ERR_INVALID, "cap_height should be at most log2(leaves.len())");
    if (gb_status s = check_fri_instance_lists(ctx, oracle_num_polys, num_oracles, batch_sizes, num_batches, polynomials)) return s;
    if (gb_status s = check_fri_reduction_arity_bits(ctx, degree_bits, rate_bits, cap_height, reduction_arity_bits, num_layers)) return s;
    if (proof_of_work_bits > 31) return fail(ctx, GB_ERR_INVALID, "proof_of_work_bits above 31");
    // every query round is at least one opened word per oracle: a count the bytes cannot hold is refused before anything is sized by it
    if (num_query_rounds == 0) return fail(ctx, GB_ERR_INVALID, "num_query_rounds is zero: a proof without queries proves nothing");
    if (num_query_rounds > GB_MAX_FRI_QUERY_ROUNDS) return fail(ctx, GB_ERR_INVALID, "more than GB_MAX_FRI_QUERY_ROUNDS query rounds");
    if (num_query_rounds > fri_proof_len) return fail(ctx, GB_ERR_INVALID, "proof bytes are truncated: fewer bytes than query rounds");
    const std::vector<uint32_t> arity(reduction_arity_bits, reduction_arity_bits + num_layers);
    const uint8_t* bytes = static_cast<const uint8_t*>(fri_proof);
    try {
        if (field == GB_GOLDILOCKS) {
            Host<GlF>::Challenger ch;
            if (gb_status s = challenger_from_state<GlF>(ctx, challenger, ch)) return s;
            fri_verify_impl<GlF>(degree_bits, rate_bits, cap_height, hiding != 0, oracle_num_polys, oracle_blinding, num_oracles, points, batch_sizes,
                                 num_batches, polynomials, openings, initial_caps, arity, proof_of_work_bits, num_query_rounds, ch, bytes, fri_proof_len);
        } else {
            Host<BbF>::Challenger ch;
            if (gb_status s = challenger_from_state<BbF>(ctx, challenger, ch)) return s;
            fri_verify_impl<BbF>(degree_bits, rate_bits, cap_height, hiding != 0, oracle_num_polys, oracle_blinding, num_oracles, points, batch_sizes,
                                 num_batches, polynomials, openings, initial_caps, arity, proof_of_work_bits, num_query_rounds, ch, bytes, fri_proof_len);
        }
    } catch (const VerifyFail& f) {
        return fail(ctx, f.code, f.msg);
    }
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_verify(gb_circuit* c, const void* proof, size_t proof_len) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (!proof) return fail(c->ctx, GB_ERR_INVALID, "null proof");
    if (gb_status s = need_arity_list(c)) return s;
    try {
        if (c->field == GB_GOLDILOCKS) verify_impl<GlF>(static_cast<Circuit<GlF>*>(c), static_cast<const uint8_t*>(proof), proof_len);
        else verify_impl<BbF>(static_cast<Circuit<BbF>*>(c), static_cast<const uint8_t*>(proof), proof_len);
    } catch (const VerifyFail& f) {
        return fail(c->ctx, f.code, f.msg);
    }
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

}  // extern "C"

// Compressed proofs on the host (included at the end of api.hip, after verifier_host.inc whose parser, transcript and FRI
// query arithmetic it shares).  The reference does this on the CPU as well:
//   hash/path_compression.rs:12-117     compress_merkle_proofs / decompress_merkle_proofs
//   fri/proof.rs:137-232, 237-384       FriProof::compress / CompressedFriProof::decompress
//   plonk/proof.rs:96-140, 183-260      ProofWithPublicInputs::compress, CompressedProofWithPublicInputs::{decompress, verify}
//   plonk/get_challenges.rs:129-180     get_inferred_elements (the value each FRI layer's fold must reproduce)
//   util/serialization/mod.rs:1102-1150, 2168-2256   byte layout of the compressed form

namespace {

template <class F>
struct ProofWriter {
    typedef typename F::T T;
    std::vector<uint8_t> out;
    void put(const void* p, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(p); out.insert(out.end(), b, b + n); }
    void words(const std::vector<T>& v) { if (!v.empty()) put(v.data(), v.size() * sizeof(T)); }
    void u8(uint8_t x) { out.push_back(x); }
    void u32le(u32 x) { put(&x, 4); }
    void u64le(u64 x) { put(&x, 8); }
    void path(const std::vector<T>& siblings) {  // write_merkle_proof: u8 length, then the hashes
        u8((uint8_t)(siblings.size() / F::H));
        words(siblings);
    }
    void caps_and_openings(const ParsedProof<F>& p) {
        words(p.wires_cap); words(p.zs_cap); words(p.quot_cap);
        words(p.t_const); words(p.t_sig); words(p.t_w); words(p.t_z); words(p.t_zn); words(p.t_pp); words(p.t_q);
        for (const auto& lc : p.layer_caps) words(lc);
    }
};

// hash/path_compression.rs:12-54.  paths[k] = siblings (H words each) of the proof for indices[k]; returns the compressed ones.
template <class F>
std::vector<std::vector<typename F::T>> compress_paths(u32 cap_height, const std::vector<u64>& indices,
                                                       const std::vector<const std::vector<typename F::T>*>& paths) {
    typedef typename F::T T;
    constexpr u32 H = F::H;
    const u32 layers = (u32)(paths[0]->size() / H), height = cap_height + layers;
    const u64 num_leaves = (u64)1 << height;
    std::set<u64> known;
    for (u64 i : indices)
        for (u32 j = 0; j < layers; j++) known.insert((i + num_leaves) >> j);
    std::vector<std::vector<T>> out(paths.size());
    for (size_t k = 0; k < paths.size(); k++) {
        u64 index = indices[k] + num_leaves;
        for (u32 l = 0; l < layers; l++) {
            if (known.insert(index ^ 1).second) out[k].insert(out[k].end(), paths[k]->begin() + (size_t)l * H, paths[k]->begin() + (size_t)(l + 1) * H);
            index >>= 1;
            known.insert(index);
        }
    }
    return out;
}

// hash/path_compression.rs:56-117
template <class F>
std::vector<std::vector<typename F::T>> decompress_paths(const std::vector<const std::vector<typename F::T>*>& leaves,
                                                         const std::vector<u64>& indices,
                                                         const std::vector<const std::vector<typename F::T>*>& compressed, u32 height,
                                                         u32 cap_height) {
    typedef typename F::T T;
    typedef std::array<T, F::H> Hash;
    constexpr u32 H = F::H;
    const u64 num_leaves = (u64)1 << height;
    std::map<u64, Hash> seen;
    for (size_t k = 0; k < indices.size(); k++) {
        Hash h{};
        const std::vector<T>& leaf = *leaves[k];
        if (leaf.size() <= H) std::copy(leaf.begin(), leaf.end(), h.begin());  // hash_or_noop (plonk/config.rs:70-84)
        else Host<F>::hash_no_pad(leaf.data(), leaf.size(), h.data());
        seen[indices[k] + num_leaves] = h;
    }
    std::vector<size_t> next(indices.size(), 0);
    for (u32 layer = 0; layer + cap_height < height; layer++)
        for (size_t k = 0; k < indices.size(); k++) {
            const u64 index = (indices[k] + num_leaves) >> layer;
            const Hash cur = seen.at(index);
            auto it = seen.find(index ^ 1);
            if (it == seen.end()) {
                if ((next[k] + 1) * H > compressed[k]->size()) vfail(GB_VCHECK_COMPRESSED_MISSING_SIBLING);
                Hash sib;
                std::copy(compressed[k]->begin() + next[k] * H, compressed[k]->begin() + (next[k] + 1) * H, sib.begin());
                next[k]++;
                it = seen.emplace(index ^ 1, sib).first;
            }
            Hash parent;
            if (index & 1) HostHash<F>::two_to_one(it->second.data(), cur.data(), parent.data());
            else HostHash<F>::two_to_one(cur.data(), it->second.data(), parent.data());
            seen[index >> 1] = parent;
        }
    std::vector<std::vector<T>> out(indices.size());
    for (size_t k = 0; k < indices.size(); k++) {
        u64 index = indices[k] + num_leaves;
        for (u32 l = 0; l + cap_height < height; l++) {
            const Hash& h = seen.at(index ^ 1);
            out[k].insert(out[k].end(), h.begin(), h.end());
            index >>= 1;
        }
    }
    return out;
}

// ProofWithPublicInputs::compress -> bytes of CompressedProofWithPublicInputs
template <class F>
std::vector<uint8_t> compress_impl(Circuit<F>* c, const uint8_t* bytes, size_t len) {
    typedef typename F::T T;
    constexpr u32 D = F::D;
    const ProofShape<F> sh(c);
    ParsedProof<F> p;
    parse_proof(c, sh, bytes, len, p);
    Challenges<F> chal;
    get_challenges(c, sh, p, chal);  // fri_query_indices (plonk/get_challenges.rs:103-127)
    const std::vector<u64>& indices = chal.x_indices;
    const u32 nq = sh.nqr, nl = sh.nlayers;
    for (const auto& q : p.queries) {  // untrusted bytes: every path must have its tree's depth before it is indexed by layer
        for (int o = 0; o < 4; o++)
            if (q.paths[o].size() != (size_t)F::H * (sh.lgN - sh.capH)) throw VerifyFail{GB_ERR_INVALID, "Merkle path of the wrong length"};
        u32 height = sh.lgN;
        for (u32 li = 0; li < nl; li++) {
            height -= c->arity_bits[li];
            if (height < sh.capH || q.step_paths[li].size() != (size_t)F::H * (height - sh.capH))
                throw VerifyFail{GB_ERR_INVALID, "FRI layer Merkle path of the wrong length"};
        }
    }

    // "transpose": per tree, the indices / paths of every query; then compress each tree's paths together
    std::vector<std::vector<T>> init_paths[4];
    for (int o = 0; o < 4; o++) {
        std::vector<const std::vector<T>*> ps;
        for (const auto& q : p.queries) ps.push_back(&q.paths[o]);
        init_paths[o] = compress_paths<F>(sh.capH, indices, ps);
    }
    std::vector<std::vector<u64>> step_idx(nl, std::vector<u64>(nq));
    std::vector<std::vector<std::vector<T>>> step_evals(nl, std::vector<std::vector<T>>(nq)), step_paths(nl);
    {
        std::vector<u64> cur(indices);
        for (u32 li = 0; li < nl; li++) {
            const u32 ab = c->arity_bits[li];
            std::vector<const std::vector<T>*> ps;
            for (u32 k = 0; k < nq; k++) {
                const u64 within = cur[k] & ((1u << ab) - 1);
                cur[k] >>= ab;
                step_idx[li][k] = cur[k];
                const std::vector<T>& row = p.queries[k].step_rows[li];
                std::vector<T>& ev = step_evals[li][k];  // the element the verifier can infer is removed (fri/proof.rs:178-180)
                ev.assign(row.begin(), row.begin() + (size_t)within * D);
                ev.insert(ev.end(), row.begin() + (size_t)(within + 1) * D, row.end());
                ps.push_back(&p.queries[k].step_paths[li]);
            }
            step_paths[li] = compress_paths<F>(sh.capH, step_idx[li], ps);
        }
    }
    // write: caps, openings, layer caps, the indices (u32), then per tree the entries keyed by index - FIRST occurrence wins
    // (HashMap::entry().or_insert) - in ascending index order (serialization/mod.rs:2177-2191)
    ProofWriter<F> w;
    w.caps_and_openings(p);
    for (u64 i : indices) w.u32le((u32)i);
    {
        std::map<u64, u32> first;
        for (u32 k = 0; k < nq; k++) first.emplace(indices[k], k);
        for (const auto& kv : first)
            for (int o = 0; o < 4; o++) { w.words(p.queries[kv.second].rows[o]); w.path(init_paths[o][kv.second]); }
    }
    for (u32 li = 0; li < nl; li++) {
        std::map<u64, u32> first;
        for (u32 k = 0; k < nq; k++) first.emplace(step_idx[li][k], k);
        for (const auto& kv : first) { w.words(step_evals[li][kv.second]); w.path(step_paths[li][kv.second]); }
    }
    w.words(p.t_final);
    w.put(&p.pow_witness, sizeof(T));
    w.words(p.pis);  // no length prefix (serialization/mod.rs:2255)
    return std::move(w.out);
}

// The bytes of a CompressedProofWithPublicInputs, read once for gb_proof_decompress, gb_verify_compressed and the batch verifier's
// host stage (read_compressed_fri_query_rounds, serialization/mod.rs:1102-1150): caps, openings, the stored query indices, per
// tree the entries of the distinct indices in ascending order, the final polynomial, the proof-of-work witness, the public inputs
// (no count: what is left).  Every word is checked canonical where it stands; an entry is kept as its place in the bytes.
struct CompressedEntry {
    u64 index;          // the leaf (an oracle tree: the query index; a layer tree: the coset index)
    size_t row[4];      // byte offset of the row per oracle ([0] alone for a layer: the coset without its inferred element)
    u32 siblings[4];    // the length byte behind the row; the stored siblings follow it
};
struct CompressedIndex {
    std::vector<u64> stored;                        // the query indices as stored
    std::vector<CompressedEntry> initial;           // ascending
    std::vector<std::vector<CompressedEntry>> steps;   // per layer, ascending
    size_t queries_begin = 0, queries_end = 0;      // the entries' bytes
    static const CompressedEntry& at(const std::vector<CompressedEntry>& v, u64 index) {
        auto it = std::lower_bound(v.begin(), v.end(), index, [](const CompressedEntry& e, u64 i) { return e.index < i; });
        if (it == v.end() || it->index != index) throw std::out_of_range("compressed entry");
        return *it;
    }
};
template <class F>
size_t canon_span(ProofReader<F>& rd, size_t n) {   // n canonical words: where they begin
    const size_t at = rd.off;
    for (size_t i = 0; i < n; i++) (void)rd.field_canonical();
    return at;
}
template <class F>
void parse_compressed(const Circuit<F>* c, const ProofShape<F>& sh, const uint8_t* bytes, size_t len, ParsedProof<F>& p, CompressedIndex& ix) {
    typedef typename F::T T;
    constexpr u32 D = F::D, H = F::H;
    const u32 nq = sh.nqr, nl = sh.nlayers;
    ProofReader<F> rd{bytes, len};
    parse_caps_and_openings(rd, sh, p);
    ix.stored.resize(nq);
    for (auto& i : ix.stored) { rd.need(4); u32 v; std::memcpy(&v, rd.p + rd.off, 4); rd.off += 4; i = v; }
    ix.queries_begin = rd.off;
    std::vector<u64> idx(ix.stored);
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
    ix.initial.resize(idx.size());
    for (size_t e = 0; e < idx.size(); e++) {
        CompressedEntry& en = ix.initial[e];
        en.index = idx[e];
        for (int o = 0; o < 4; o++) {
            en.row[o] = canon_span(rd, sh.row_widths[o]);
            en.siblings[o] = rd.u8();
            canon_span(rd, (size_t)en.siblings[o] * H);
        }
    }
    ix.steps.resize(nl);
    for (u32 li = 0; li < nl; li++) {
        const u32 ab = c->arity_bits[li];
        for (auto& i : idx) i >>= ab;
        idx.erase(std::unique(idx.begin(), idx.end()), idx.end());   // (still ascending)
        ix.steps[li].resize(idx.size());
        for (size_t e = 0; e < idx.size(); e++) {
            CompressedEntry& en = ix.steps[li][e];
            en = CompressedEntry{};
            en.index = idx[e];
            en.row[0] = canon_span(rd, (size_t)D * ((1u << ab) - 1));
            en.siblings[0] = rd.u8();
            canon_span(rd, (size_t)en.siblings[0] * H);
        }
    }
    ix.queries_end = rd.off;
    rd.ext_vec(p.final_poly, p.t_final, sh.final_len);
    p.pow_witness = rd.field_canonical();
    if ((len - rd.off) % sizeof(T)) vfail(GB_VCHECK_COMPRESSED_TRAILING);
    if ((len - rd.off) / sizeof(T) != c->cfg.num_public_inputs) vfail(GB_VCHECK_PI_COUNT);  // plonk/validate_shape.rs:22-25 (the compressed form has no count)
    rd.canon_vec(p.pis, (len - rd.off) / sizeof(T));
}

// CompressedProofWithPublicInputs::decompress -> bytes of ProofWithPublicInputs
template <class F>
std::vector<uint8_t> decompress_impl(Circuit<F>* c, const uint8_t* bytes, size_t len) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 D = F::D, H = F::H;
    const ProofShape<F> sh(c);
    const u32 nq = sh.nqr, nl = sh.nlayers;
    ParsedProof<F> p;
    CompressedIndex ix;
    parse_compressed(c, sh, bytes, len, p, ix);
    const std::vector<u64>& stored = ix.stored;
    struct Initial { std::vector<T> rows[4], paths[4]; };
    struct Step { std::vector<T> evals, path; };
    std::map<u64, Initial> initial;
    std::vector<std::map<u64, Step>> steps(nl);
    {
        auto words = [&](std::vector<T>& out, size_t at, size_t n) {
            out.resize(n);
            if (n) std::memcpy(out.data(), bytes + at, n * sizeof(T));
        };
        for (const CompressedEntry& en : ix.initial) {
            Initial& e = initial[en.index];
            for (int o = 0; o < 4; o++) {
                words(e.rows[o], en.row[o], sh.row_widths[o]);
                words(e.paths[o], en.row[o] + sh.row_widths[o] * sizeof(T) + 1, (size_t)en.siblings[o] * H);
            }
        }
        for (u32 li = 0; li < nl; li++) {
            const size_t ne = (size_t)D * ((1u << c->arity_bits[li]) - 1);
            for (const CompressedEntry& en : ix.steps[li]) {
                Step& e = steps[li][en.index];
                words(e.evals, en.row[0], ne);
                words(e.path, en.row[0] + ne * sizeof(T) + 1, (size_t)en.siblings[0] * H);
            }
        }
    }

    Challenges<F> chal;
    get_challenges(c, sh, p, chal);
    const std::vector<u64>& indices = chal.x_indices;
    if (indices != stored) vfail(GB_VCHECK_COMPRESSED_INDICES);

    // the inferred elements (get_inferred_elements) and the re-inflated evals, per query
    const FriQueryMath<F> fri(sh, p, chal);
    p.queries.resize(nq);
    std::vector<std::vector<u64>> step_idx(nl, std::vector<u64>(nq));
    std::vector<std::map<u64, std::vector<T>>> evals_by_depth(nl);
    for (u32 k = 0; k < nq; k++) {
        const Initial& in = initial.at(indices[k]);
        typename ParsedProof<F>::Query& q = p.queries[k];
        for (int o = 0; o < 4; o++) q.rows[o] = in.rows[o];
        q.step_rows.resize(nl);
        q.step_paths.resize(nl);
        T x = fri.subgroup_x(indices[k]);
        E old_eval = fri.combine_initial(in.rows, x);
        u64 index = indices[k];
        for (u32 li = 0; li < nl; li++) {
            const u32 ab = c->arity_bits[li];
            const u64 within = index & ((1u << ab) - 1);
            index >>= ab;
            step_idx[li][k] = index;
            auto seen = evals_by_depth[li].find(index);
            if (seen == evals_by_depth[li].end()) {
                const std::vector<T>& ev = steps[li].at(index).evals;
                std::vector<T> full(ev.begin(), ev.begin() + (size_t)within * D);
                for (u32 d = 0; d < D; d++) full.push_back((T)F::dec(F::coord(old_eval, d)));
                full.insert(full.end(), ev.begin() + (size_t)within * D, ev.end());
                seen = evals_by_depth[li].emplace(index, std::move(full)).first;
            }
            q.step_rows[li] = seen->second;
            old_eval = FriQueryMath<F>::compute_evaluation(x, within, ab, FriQueryMath<F>::to_ext(q.step_rows[li]), chal.fri_betas[li]);
            x = F::pow(x, (u64)1 << ab);
        }
    }
    // decompress every tree's paths together
    for (int o = 0; o < 4; o++) {
        std::vector<const std::vector<T>*> leaves, comp;
        for (u32 k = 0; k < nq; k++) { leaves.push_back(&p.queries[k].rows[o]); comp.push_back(&initial.at(indices[k]).paths[o]); }
        auto paths = decompress_paths<F>(leaves, indices, comp, sh.lgN, sh.capH);
        for (u32 k = 0; k < nq; k++) p.queries[k].paths[o] = std::move(paths[k]);
    }
    u32 height = sh.lgN;
    for (u32 li = 0; li < nl; li++) {
        height -= c->arity_bits[li];
        std::vector<const std::vector<T>*> leaves, comp;
        for (u32 k = 0; k < nq; k++) { leaves.push_back(&p.queries[k].step_rows[li]); comp.push_back(&steps[li].at(step_idx[li][k]).path); }
        auto paths = decompress_paths<F>(leaves, step_idx[li], comp, height, sh.capH);
        for (u32 k = 0; k < nq; k++) p.queries[k].step_paths[li] = std::move(paths[k]);
    }
    // write_proof_with_public_inputs (serialization/mod.rs:2103-2151)
    ProofWriter<F> w;
    w.caps_and_openings(p);
    for (const auto& q : p.queries) {
        for (int o = 0; o < 4; o++) { w.words(q.rows[o]); w.path(q.paths[o]); }
        for (u32 li = 0; li < nl; li++) { w.words(q.step_rows[li]); w.path(q.step_paths[li]); }
    }
    w.words(p.t_final);
    w.put(&p.pow_witness, sizeof(T));
    w.u64le(p.pis.size());
    w.words(p.pis);
    return std::move(w.out);
}

template <class Fn>
gb_status run_bytes(gb_circuit* c, const void* in, void* out, size_t out_cap, size_t* out_len, Fn&& fn) {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (!in || !out_len) return fail(c->ctx, GB_ERR_INVALID, "null argument");
    if (gb_status s = need_arity_list(c)) return s;
    try {
        const std::vector<uint8_t> bytes = fn();
        *out_len = bytes.size();
        if (!out || out_cap < bytes.size()) return fail(c->ctx, GB_ERR_BUFFER_TOO_SMALL, "output buffer too small (*out_len holds the size needed)");
        std::memcpy(out, bytes.data(), bytes.size());
    } catch (const VerifyFail& f) {
        return fail(c->ctx, f.code, f.msg);
    } catch (const std::out_of_range&) {
        return fail(c->ctx, GB_ERR_INVALID, "compressed proof lacks an entry its query indices need");
    }   // (std::bad_alloc and the rest: the entry point's own guard)
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_proof_compress(gb_circuit* c, const void* proof, size_t proof_len, void* out, size_t out_cap, size_t* out_len) try {
    return run_bytes(c, proof, out, out_cap, out_len, [&] {
        return by_field(c, [&](auto* cf) { return compress_impl(cf, static_cast<const uint8_t*>(proof), proof_len); });
    });
} GB_CATCH_CIRCUIT(c)

gb_status gb_proof_decompress(gb_circuit* c, const void* compressed, size_t compressed_len, void* out, size_t out_cap, size_t* out_len) try {
    return run_bytes(c, compressed, out, out_cap, out_len, [&] {
        return by_field(c, [&](auto* cf) { return decompress_impl(cf, static_cast<const uint8_t*>(compressed), compressed_len); });
    });
} GB_CATCH_CIRCUIT(c)

gb_status gb_verify_compressed(gb_circuit* c, const void* compressed, size_t compressed_len) try {
    if (!c) return fail(nullptr, GB_ERR_INVALID, "null circuit");
    if (!compressed) return fail(c->ctx, GB_ERR_INVALID, "null proof");
    if (gb_status s = need_arity_list(c)) return s;
    try {
        // CompressedProofWithPublicInputs::verify (plonk/proof.rs:238-265): decompress, then verify_with_challenges
        by_field(c, [&](auto* cf) {
            const auto bytes = decompress_impl(cf, static_cast<const uint8_t*>(compressed), compressed_len);
            verify_impl(cf, bytes.data(), bytes.size());
        });
    } catch (const VerifyFail& f) {
        return fail(c->ctx, f.code, f.msg);
    } catch (const std::out_of_range&) {
        return fail(c->ctx, GB_ERR_INVALID, "compressed proof lacks an entry its query indices need");
    }
    return GB_OK;
} GB_CATCH_CIRCUIT(c)

}  // extern "C"

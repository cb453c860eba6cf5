// gb_verify_batch: gb_verify of many proofs of one circuit, the query rounds on the device (included at the end of api.hip, after
// verifier_host.inc, whose pieces it shares: parse_proof, get_challenges, check_vanishing, check_pow, FriQueryMath and - for a
// proof whose query section is not of the circuit's shape - verify_fri_queries itself).
//
// Per chunk of proofs: the HOST STAGE runs per proof, independent, over the context's copy threads - everything gb_verify does in
// front of the query rounds, then the proof's query bytes (as they stand) and its record (kernels.hpp: VerifyLayout) into a
// page-locked slot; a proof that fails here, or that the host checks whole, takes no place in the slot.  Then one upload and the
// two kernels of kernels_verify.hip on the context's stream.  There are two slots, so the host stage of chunk k+1 runs while the
// kernels of chunk k do.  The failure keys of every chunk are read back once, at the end.
//
// gb_verify_compressed_batch is the same call over a second plan (CompressedBatchPlan): its host stage reads a compressed proof with
// compress_host.inc's parser, decides from the query indices alone how many siblings every stored path must hold, and stages the
// query section as it stands with a directory of its entries; its kernels are the k_vc_ pair of kernels_verify.hip.
//
// gb_fri_verify_batch is the same call over a third plan (FriBatchPlan): the items are FriProof bytes on one instance shape described
// by flat arrays, its host stage is gb_fri_verify's up to the query rounds, its kernels the k_fri_verify_ pair over the shape's
// tables in device memory.

#include "verify_compressed.hpp"

namespace {

template <class F>
struct BatchPlan {
    typedef typename F::T T;
    typedef typename F::E E;
    ProofShape<F> sh;
    gbk::VerifyLayout L{};
    size_t head_bytes = 0, query_bytes = 0, tail_fixed_bytes = 0, per_proof_bytes = 0;
    size_t stride = 0;          // a proof's place among the staged query sections
    size_t scratch_bytes = 0;   // per proof, on the device alone
    explicit BatchPlan(const Circuit<F>* c) : sh(c) {
        constexpr size_t TS = sizeof(T);
        constexpr u32 D = F::D, H = F::H;
        const u32 nl = sh.nlayers;
        L.nqr = sh.nqr; L.lgN = sh.lgN; L.num_layers = nl; L.final_len = (u32)sh.final_len;
        size_t batch0 = 0;
        for (int o = 0; o < 4; o++) { L.widths[o] = (u32)sh.widths[o]; batch0 += sh.widths[o]; }
        L.batch_sizes[0] = (u32)batch0;
        L.batch_sizes[1] = sh.nch;
        // one query round (util/serialization/mod.rs:1679-1695): per oracle the row and its path behind a length byte, then per
        // layer the coset and its path likewise
        size_t off = 0;
        u32 t = 0, shift = 0;
        for (int o = 0; o < 4; o++, t++) {
            gbk::VerifyTree& tr = L.trees[t];
            tr.row_off = (u32)off; tr.num_words = (u32)sh.row_widths[o];
            off += sh.row_widths[o] * TS + 1;
            tr.path_off = (u32)off; tr.path_len = sh.lgN - sh.capH;
            off += (size_t)tr.path_len * H * TS;
            tr.shift = 0;
            tr.cap_word = o == 0 ? ~0u : (u32)((o - 1) * sh.cap_elems);
        }
        for (u32 li = 0; li < nl; li++, t++) {
            const u32 ab = c->arity_bits[li];
            shift += ab;
            gbk::VerifyTree& tr = L.trees[t];
            L.arity_bits[li] = ab;
            tr.row_off = (u32)off; tr.num_words = D << ab;
            off += ((size_t)D << ab) * TS + 1;
            tr.path_off = (u32)off; tr.path_len = sh.lgN - shift - sh.capH;   // >= 0: check_fri_reduction_arity_bits
            off += (size_t)tr.path_len * H * TS;
            tr.shift = shift;
            tr.cap_word = (u32)((3 + li) * sh.cap_elems);
        }
        L.round_bytes = (u32)off;
        query_bytes = off * sh.nqr;
        const size_t openings = sh.nconst + sh.nr + sh.nw + 2 * (size_t)sh.nch + (size_t)sh.nch * sh.num_prods + sh.nq;
        head_bytes = ((3 + nl) * sh.cap_elems + D * openings) * TS;
        tail_fixed_bytes = (D * sh.final_len + 1) * TS + 8;   // final_poly, pow_witness, the public-input count
        const size_t ext_bytes = (7 + nl + sh.final_len) * sizeof(E);
        L.rec_x_off = (u32)ext_bytes;
        L.rec_caps_off = (u32)(ext_bytes + 8 * (size_t)sh.nqr);
        L.rec_bytes = (u32)((L.rec_caps_off + (3 + nl) * sh.cap_elems * TS + 15) & ~(size_t)15);
        stride = query_bytes;
        per_proof_bytes = query_bytes + L.rec_bytes;
    }
    static constexpr u32 num_oracles() { return gbk::VERIFY_ORACLES; }
    static const char* scope(int i) {
        static const char* const names[4] = {"verify batch: host stage", "verify batch: upload", "verify batch: paths", "verify batch: queries"};
        return names[i];
    }
};

// gb_verify_compressed_batch: the circuit's shape as above (an upper bound of every compressed query section), a directory in
// each record, the inferred elements as device scratch
template <class F>
struct CompressedBatchPlan : BatchPlan<F> {
    gbk::VerifyCompressedLayout C{};
    bool device_ok = true;   // a proof's query rounds share a workgroup
    explicit CompressedBatchPlan(const Circuit<F>* c) : BatchPlan<F>(c) {
        constexpr size_t TS = sizeof(typename F::T);
        gbk::VerifyLayout& L = this->L;
        const u32 ntrees = gbk::VERIFY_ORACLES + L.num_layers;
        u32 max_path = 0;
        for (u32 t = 0; t < ntrees; t++) max_path = std::max(max_path, L.trees[t].path_len);
        // (the kernels bound a path by its tree's height: the padding keeps such a read inside the slot whatever the entry)
        this->stride = (this->query_bytes + (size_t)max_path * F::H * TS + 15) & ~(size_t)15;
        C.rec_dir_off = L.rec_bytes;
        L.rec_bytes = (u32)((L.rec_bytes + 4 * (size_t)ntrees * L.nqr + 15) & ~(size_t)15);
        this->scratch_bytes = ((size_t)L.num_layers * L.nqr * F::D * TS + 15) & ~(size_t)15;
        this->per_proof_bytes = this->stride + L.rec_bytes + this->scratch_bytes;
        device_ok = L.nqr <= gbk::VERIFY_COMPRESSED_MAX_QUERIES && this->stride <= 0x7FFFFFFFu;
        C.proof_stride = (u32)this->stride;
    }
    static const char* scope(int i) {
        static const char* const names[4] = {"verify compressed batch: host stage", "verify compressed batch: upload",
                                             "verify compressed batch: queries", "verify compressed batch: paths"};
        return names[i];
    }
};

inline gb_verify_result vresult(const VerifyFail& f) { return gb_verify_result{(uint32_t)f.code, f.check, f.query_round, f.index}; }

// a proof's record (kernels.hpp: VerifyLayout)
template <class F>
void stage_record(const ProofShape<F>& sh, const gbk::VerifyLayout& L, const ParsedProof<F>& pp, const Challenges<F>& chal,
                  const FriQueryMath<F>& fri, unsigned char* rec_dst) {
    typedef typename F::T T;
    typedef typename F::E E;
    E* e = reinterpret_cast<E*>(rec_dst);
    e[0] = chal.fri_alpha;
    for (u32 b = 0; b < 2; b++) { e[1 + b] = fri.red_open[b]; e[3 + b] = fri.alpha_shift[b]; e[5 + b] = fri.points[b]; }
    for (u32 li = 0; li < L.num_layers; li++) e[7 + li] = chal.fri_betas[li];
    for (u32 i = 0; i < L.final_len; i++) e[7 + L.num_layers + i] = pp.final_poly[i];
    std::memcpy(rec_dst + L.rec_x_off, chal.x_indices.data(), 8 * (size_t)L.nqr);
    T* caps = reinterpret_cast<T*>(rec_dst + L.rec_caps_off);
    const size_t ce = sh.cap_elems;
    std::memcpy(caps, pp.wires_cap.data(), ce * sizeof(T));
    std::memcpy(caps + ce, pp.zs_cap.data(), ce * sizeof(T));
    std::memcpy(caps + 2 * ce, pp.quot_cap.data(), ce * sizeof(T));
    for (u32 li = 0; li < L.num_layers; li++) std::memcpy(caps + (3 + li) * ce, pp.layer_caps[li].data(), ce * sizeof(T));
}

// The host stage of one proof.  true: its query rounds and record stand at rounds_dst / rec_dst for the device; false: *res is final.
template <class F>
bool host_stage(Circuit<F>* c, const BatchPlan<F>& plan, const uint8_t* bytes, size_t len, gb_verify_result* res,
                unsigned char* rounds_dst, unsigned char* rec_dst) {
    typedef typename F::T T;
    constexpr u32 H = F::H;
    const ProofShape<F>& sh = plan.sh;
    const gbk::VerifyLayout& L = plan.L;
    *res = gb_verify_result{GB_OK, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
    try {
        ParsedProof<F> pp;
        parse_proof(c, sh, bytes, len, pp);
        Challenges<F> chal;
        get_challenges(c, sh, pp, chal);
        check_vanishing<F>(c, sh, pp, chal);
        const FriQueryMath<F> fri(sh, pp, chal);
        check_pow<F>(c->cfg.proof_of_work_bits, chal);
        // the regular shape: every path as long as the circuit says, so that the query rounds stand at the circuit's offsets
        bool regular = len == plan.head_bytes + plan.query_bytes + plan.tail_fixed_bytes + pp.pis.size() * sizeof(T);
        for (const auto& q : pp.queries) {
            for (u32 o = 0; o < 4 && regular; o++) regular = q.paths[o].size() == (size_t)H * L.trees[o].path_len;
            for (u32 li = 0; li < L.num_layers && regular; li++) regular = q.step_paths[li].size() == (size_t)H * L.trees[4 + li].path_len;
        }
        if (!regular) {   // the host's own walk: GB_ERR_INVALID and GB_ERR_VERIFY in gb_verify's order by construction
            const T* initial_caps[4] = {c->cap_host.data(), pp.wires_cap.data(), pp.zs_cap.data(), pp.quot_cap.data()};
            verify_fri_queries<F>(fri, initial_caps, c->arity_bits, pp, chal);
            return false;
        }
        std::memcpy(rounds_dst, bytes + plan.head_bytes, plan.query_bytes);
        stage_record<F>(sh, L, pp, chal, fri, rec_dst);
        return true;
    } catch (const VerifyFail& f) {
        *res = vresult(f);
        return false;
    }
}

// The host stage of one COMPRESSED proof: gb_verify_compressed up to the query rounds, in its order.  What decompress_impl finds while
// it re-inflates the paths - a path that holds too few siblings - follows from the indices (verify_compressed.hpp:
// sibling_counts), so it is decided here, in front of the vanishing identity as there.
template <class F>
bool host_stage(Circuit<F>* c, const CompressedBatchPlan<F>& plan, const uint8_t* bytes, size_t len, gb_verify_result* res,
                unsigned char* rounds_dst, unsigned char* rec_dst) {
    const ProofShape<F>& sh = plan.sh;
    const gbk::VerifyLayout& L = plan.L;
    *res = gb_verify_result{GB_OK, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
    try {
        ParsedProof<F> pp;
        CompressedIndex ix;
        parse_compressed(c, sh, bytes, len, pp, ix);
        Challenges<F> chal;
        get_challenges(c, sh, pp, chal);
        if (chal.x_indices != ix.stored) vfail(GB_VCHECK_COMPRESSED_INDICES);
        // the sibling plan: per tree what every entry must hold against what it holds, and the directory
        const u32 nqr = L.nqr, ntrees = gbk::VERIFY_ORACLES + L.num_layers;
        u32* dir = reinterpret_cast<u32*>(rec_dst + plan.C.rec_dir_off);
        std::vector<u64> leaf(nqr);
        std::vector<u32> need(nqr), entry_need;
        bool missing = false, surplus = false;
        for (u32 t = 0; t < ntrees; t++) {
            const gbk::VerifyTree& tr = L.trees[t];
            const std::vector<CompressedEntry>& entries = t < gbk::VERIFY_ORACLES ? ix.initial : ix.steps[t - gbk::VERIFY_ORACLES];
            const u32 o = t < gbk::VERIFY_ORACLES ? t : 0;
            for (u32 k = 0; k < nqr; k++) leaf[k] = chal.x_indices[k] >> tr.shift;
            gbk::vc::sibling_counts(leaf.data(), nqr, tr.path_len, need.data());
            entry_need.assign(entries.size(), 0);
            for (u32 k = 0; k < nqr; k++) {
                const CompressedEntry& en = CompressedIndex::at(entries, leaf[k]);
                entry_need[&en - entries.data()] += need[k];   // (zero but for the first query round of the entry)
                dir[(size_t)t * nqr + k] = (u32)(en.row[o] - ix.queries_begin);
            }
            for (size_t e = 0; e < entries.size(); e++) {
                missing = missing || entries[e].siblings[o] < entry_need[e];
                surplus = surplus || entries[e].siblings[o] > entry_need[e];
            }
        }
        if (missing) vfail(GB_VCHECK_COMPRESSED_MISSING_SIBLING);
        check_vanishing<F>(c, sh, pp, chal);
        const FriQueryMath<F> fri(sh, pp, chal);
        check_pow<F>(c->cfg.proof_of_work_bits, chal);
        const size_t section = ix.queries_end - ix.queries_begin;
        if (surplus || !plan.device_ok || section > plan.query_bytes) {
            // gb_verify_compressed ignores what a path holds beyond its need: its own walk, which is right by construction
            const std::vector<uint8_t> full = decompress_impl(c, bytes, len);
            verify_impl(c, full.data(), full.size());
            return false;
        }
        std::memcpy(rounds_dst, bytes + ix.queries_begin, section);
        stage_record<F>(sh, L, pp, chal, fri, rec_dst);
        return true;
    } catch (const VerifyFail& f) {
        *res = vresult(f);
        return false;
    }
}

template <class F>
void launch_chunk(gb_ctx* ctx, const BatchPlan<F>& plan, const gbk::VerifyLayout& L, const unsigned char* d_rounds, const unsigned char* d_recs,
                  const typename F::T* d_cap, unsigned char*, u64* keys) {
    {
        Scope sc(ctx, plan.scope(2));
        gbk::verify_paths<F>(L, d_rounds, d_recs, d_cap, keys, ctx->stream);
    }
    {
        Scope sc(ctx, plan.scope(3));
        gbk::verify_queries<F>(L, d_rounds, d_recs, keys, ctx->stream);
    }
}
template <class F>
void launch_chunk(gb_ctx* ctx, const CompressedBatchPlan<F>& plan, const gbk::VerifyLayout& L, const unsigned char* d_rounds,
                  const unsigned char* d_recs, const typename F::T* d_cap, unsigned char* d_scratch, u64* keys) {
    gbk::VerifyCompressedLayout C = plan.C;
    C.L = L;
    typename F::T* inferred = reinterpret_cast<typename F::T*>(d_scratch);
    {
        Scope sc(ctx, plan.scope(2));
        gbk::verify_compressed_queries<F>(C, d_rounds, d_recs, inferred, keys, ctx->stream);
    }
    {
        Scope sc(ctx, plan.scope(3));
        gbk::verify_compressed_paths<F>(C, d_rounds, d_recs, d_cap, inferred, keys, ctx->stream);
    }
}

// the key a proof's checks left on the device -> its result
inline gb_verify_result vresult_of_key(u64 key, u32 no, u32 num_layers) {   // no: the instance's oracles
    if (key == gbk::vq::KEY_NONE) return gb_verify_result{GB_OK, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
    const u32 qr = (u32)(key >> gbk::vq::POS_BITS), pos = (u32)(key & ((1u << gbk::vq::POS_BITS) - 1));
    if (pos < no) return gb_verify_result{GB_ERR_VERIFY, GB_VCHECK_INITIAL_PATH, qr, pos};
    if (pos == gbk::vq::pos_final(no, num_layers)) return gb_verify_result{GB_ERR_VERIFY, GB_VCHECK_FINAL_POLY, qr, UINT32_MAX};
    return gb_verify_result{GB_ERR_VERIFY, (pos - no) & 1 ? (uint32_t)GB_VCHECK_LAYER_PATH : (uint32_t)GB_VCHECK_CONSISTENCY, qr, (pos - no) / 2};
}

gb_status verify_stage_ready(gb_ctx* ctx, size_t slot_bytes, size_t key_bytes) {
    if (ctx->vstage_bytes < slot_bytes) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (int s = 0; s < 2; s++) {
            if (ctx->vstage_host[s]) (void)hipHostFree(ctx->vstage_host[s]);
            if (ctx->vstage_dev[s]) (void)hipFree(ctx->vstage_dev[s]);
            ctx->vstage_host[s] = nullptr; ctx->vstage_dev[s] = nullptr;
        }
        ctx->vstage_bytes = 0;
        for (int s = 0; s < 2; s++) {
            void* h = nullptr;
            if (hipHostMalloc(&h, slot_bytes, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, GB_ERR_OOM, "hipHostMalloc of the batch verifier's staging slot failed (lower \"verify_chunk_bytes\")");
            }
            ctx->vstage_host[s] = static_cast<char*>(h);
            void* d = nullptr;
            if (hipMalloc(&d, slot_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, GB_ERR_OOM, "hipMalloc of the batch verifier's chunk buffer failed");
            }
            ctx->vstage_dev[s] = static_cast<char*>(d);
            if (!ctx->vstage_read[s]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->vstage_read[s], hipEventDisableTiming));
        }
        ctx->vstage_bytes = slot_bytes;
    }
    return ensure(ctx, ctx->vkeys, key_bytes);
}

// fn(i) for every i below count, over `nthreads` threads (the calling one among them).  What one of them throws (std::bad_alloc: the
// call fails as a whole) stops the others at their next item and is thrown again here.
template <class Fn>
void run_on_threads(unsigned nthreads, size_t count, Fn fn) {
    std::atomic<size_t> next{0};
    std::exception_ptr thrown;
    std::mutex thrown_lock;
    auto work = [&]() {
        try {
            for (size_t i; (i = next.fetch_add(1)) < count;) fn(i);
        } catch (...) {
            std::lock_guard<std::mutex> g(thrown_lock);
            if (!thrown) thrown = std::current_exception();
            next.store(count);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthreads; t++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    if (thrown) std::rethrow_exception(thrown);
}

// stage(i, result, rounds_dst, rec_dst): the plan's host stage of item i.  `front`: front_words words that ride in front of every
// chunk (the circuit's own cap; none for gb_fri_verify_batch).  *device_items, where asked for: how many items the kernels decided.
template <class F, class Plan, class Stage>
gb_status verify_batch_impl(gb_ctx* ctx, const Plan& plan, const typename F::T* front, size_t front_words, u32 num_proofs,
                            gb_verify_result* results, Stage stage, u64* device_items = nullptr) {
    typedef typename F::T T;
    auto L = plan.L;
    const size_t cap_bytes = ((front_words * sizeof(T)) + 15) & ~(size_t)15;
    // proofs per chunk: what "verify_chunk_bytes" holds, at least one; rounds * proofs stays a 32-bit count in the kernels
    size_t per_chunk = std::max<size_t>(1, ctx->verify_chunk_bytes / plan.per_proof_bytes);
    per_chunk = std::min<size_t>(per_chunk, std::min<size_t>(num_proofs, (size_t)0x7FFFFFFF / std::max<u32>(1, L.nqr)));
    // a slot: the circuit's cap, the proofs' query rounds back to back (of any byte length), then - aligned again - their records
    // and, on the device alone, the plan's scratch
    const size_t rounds_region = (per_chunk * plan.stride + 15) & ~(size_t)15;
    const size_t recs_region = per_chunk * (size_t)L.rec_bytes;
    const size_t slot_bytes = cap_bytes + rounds_region + recs_region + per_chunk * plan.scratch_bytes;
    if (gb_status s = verify_stage_ready(ctx, slot_bytes, 8 * (size_t)num_proofs)) return s;
    u64* keys_dev = static_cast<u64*>(ctx->vkeys.p);
    HIP_TRY(ctx, hipMemsetAsync(keys_dev, 0xFF, 8 * (size_t)num_proofs, ctx->stream));
    std::vector<u32> slot_proof(num_proofs, 0);   // device slot (chunk base + place in the chunk) -> proof
    const unsigned nthreads = (unsigned)std::max(1, std::min<int>(ctx->copy_threads, (int)per_chunk));
    u32 chunk_no = 0;
    for (size_t base = 0; base < num_proofs; base += per_chunk, chunk_no++) {
        const size_t count = std::min<size_t>(per_chunk, num_proofs - base);
        const int s = (int)(chunk_no & 1);
        if (chunk_no >= 2) HIP_TRY(ctx, hipEventSynchronize(ctx->vstage_read[s]));   // the slot's last upload has left it
        char* host = ctx->vstage_host[s];
        char* dev = ctx->vstage_dev[s];
        unsigned char* h_rounds = reinterpret_cast<unsigned char*>(host) + cap_bytes;
        unsigned char* h_recs = h_rounds + rounds_region;
        std::vector<unsigned char> act(count, 0);   // place i of the slot holds a proof for the device
        std::vector<u32> owner(count);
        size_t lo = 0, hi = count;
        {
            Scope sc(ctx, plan.scope(0));
            run_on_threads(nthreads, count, [&](size_t i) {   // proof base + i stages into place i
                const size_t pi = base + i;
                act[i] = stage(pi, &results[pi], h_rounds + i * plan.stride, h_recs + i * L.rec_bytes);
            });
            // the places of proofs that ended on the host are filled from the end of the slot
            for (size_t i = 0; i < count; i++) owner[i] = (u32)(base + i);
            while (true) {
                while (lo < hi && act[lo]) lo++;
                while (hi > lo && !act[hi - 1]) hi--;
                if (lo >= hi) break;
                std::memcpy(h_rounds + lo * plan.stride, h_rounds + (hi - 1) * plan.stride, plan.stride);
                std::memcpy(h_recs + lo * L.rec_bytes, h_recs + (hi - 1) * L.rec_bytes, L.rec_bytes);
                owner[lo] = owner[hi - 1];
                act[lo] = 1;
                act[hi - 1] = 0;
            }
            for (size_t i = 0; i < count; i++) slot_proof[base + i] = i < lo ? owner[i] : UINT32_MAX;
        }
        const u32 active = (u32)lo;
        if (!active) continue;
        L.num_proofs = active;
        unsigned char* d_rounds = reinterpret_cast<unsigned char*>(dev) + cap_bytes;
        unsigned char* d_recs = d_rounds + rounds_region;
        {
            Scope sc(ctx, plan.scope(1));
            if (front_words) std::memcpy(host, front, front_words * sizeof(T));   // the circuit's cap rides in front of every chunk
            HIP_TRY(ctx, hipMemcpyAsync(dev, host, cap_bytes + (size_t)active * plan.stride, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(d_recs, h_recs, (size_t)active * L.rec_bytes, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipEventRecord(ctx->vstage_read[s], ctx->stream));
        }
        launch_chunk<F>(ctx, plan, L, d_rounds, d_recs, reinterpret_cast<const T*>(dev), d_recs + recs_region, keys_dev + base);
        HIP_TRY(ctx, hipGetLastError());
    }
    std::vector<u64> keys(num_proofs);
    if (gb_status s = read_back(ctx, keys.data(), keys_dev, 8 * (size_t)num_proofs)) return s;
    for (size_t slot = 0; slot < num_proofs; slot++)
        if (slot_proof[slot] != UINT32_MAX) {
            results[slot_proof[slot]] = vresult_of_key(keys[slot], plan.num_oracles(), L.num_layers);
            if (device_items) ++*device_items;
        }
    return GB_OK;
}

// proofs of one circuit through one of its two plans
template <class F, class Plan>
gb_status circuit_batch(gb_ctx* ctx, Circuit<F>* c, const void* const* proofs, const size_t* lens, u32 num_proofs, gb_verify_result* results) {
    const Plan plan(c);
    return verify_batch_impl<F>(ctx, plan, c->cap_host.data(), plan.sh.cap_elems, num_proofs, results,
                                [&](size_t pi, gb_verify_result* res, unsigned char* rounds_dst, unsigned char* rec_dst) {
                                    return host_stage<F>(c, plan, static_cast<const uint8_t*>(proofs[pi]), lens[pi], res, rounds_dst, rec_dst);
                                });
}

// gb_verify_compressed_batch without a context: the host stage alone, proof by proof on the calling thread.  What it decides is
// final; a proof it would hand to the device is answered GB_ERR_INVALID, for there is none.
template <class F>
void compressed_host_stage_only(Circuit<F>* c, const void* const* proofs, const size_t* lens, u32 num_proofs, gb_verify_result* results) {
    const CompressedBatchPlan<F> plan(c);
    std::vector<unsigned char> rounds(plan.stride), rec(plan.L.rec_bytes);
    for (u32 i = 0; i < num_proofs; i++)
        if (!proofs[i] || host_stage<F>(c, plan, static_cast<const uint8_t*>(proofs[i]), lens[i], &results[i], rounds.data(), rec.data()))
            results[i] = gb_verify_result{GB_ERR_INVALID, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
}

// gb_verify_batch and gb_verify_compressed_batch: one call, two plans
gb_status verify_batch_call(gb_ctx* ctx, gb_circuit* c, const void* const* proofs, const size_t* proof_lens, uint32_t num_proofs,
                            uint32_t flags, void* results, bool compressed) {
    if (!ctx) {
        if (compressed && c && flags == 0 && num_proofs && proofs && proof_lens && results && !c->arity_pending) {
            gb_verify_result* res = static_cast<gb_verify_result*>(results);
            if (c->field == GB_GOLDILOCKS) compressed_host_stage_only(static_cast<Circuit<GlF>*>(c), proofs, proof_lens, num_proofs, res);
            else compressed_host_stage_only(static_cast<Circuit<BbF>*>(c), proofs, proof_lens, num_proofs, res);
        }
        return fail(nullptr, GB_ERR_INVALID, "null ctx");
    }
    if (!c) return fail(ctx, GB_ERR_INVALID, "null circuit");
    if (c->ctx && c->ctx != ctx) return fail(ctx, GB_ERR_INVALID, "the circuit belongs to a different context");
    if (flags != 0) return fail(ctx, GB_ERR_INVALID, compressed ? "gb_verify_compressed_batch: flags must be 0" : "gb_verify_batch: flags must be 0");
    if (num_proofs == 0) return GB_OK;
    if (!proofs || !proof_lens || !results) return fail(ctx, GB_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < num_proofs; i++)
        if (!proofs[i]) return fail(ctx, GB_ERR_INVALID, "null proof");
    if (c->arity_pending) {
        (void)need_arity_list(c);   // (writes the message where gb_verify leaves it)
        return fail(ctx, GB_ERR_INVALID, "no FRI reduction list for this circuit - hand its list over with gb_circuit_set_fri_reduction_arity_bits");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gb_verify_result* res = static_cast<gb_verify_result*>(results);
    gb_status s;
    try {
        if (c->field == GB_GOLDILOCKS) {
            Circuit<GlF>* cf = static_cast<Circuit<GlF>*>(c);
            s = compressed ? circuit_batch<GlF, CompressedBatchPlan<GlF>>(ctx, cf, proofs, proof_lens, num_proofs, res)
                           : circuit_batch<GlF, BatchPlan<GlF>>(ctx, cf, proofs, proof_lens, num_proofs, res);
        } else {
            Circuit<BbF>* cf = static_cast<Circuit<BbF>*>(c);
            s = compressed ? circuit_batch<BbF, CompressedBatchPlan<BbF>>(ctx, cf, proofs, proof_lens, num_proofs, res)
                           : circuit_batch<BbF, BatchPlan<BbF>>(ctx, cf, proofs, proof_lens, num_proofs, res);
        }
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);   // earlier chunks may still read the staging slots
        throw;
    }
    if (s != GB_OK) {
        (void)hipStreamSynchronize(ctx->stream);   // nothing of the call may still read the staging slots
        return s;
    }
    uint32_t bad = 0, first = 0;
    for (uint32_t i = num_proofs; i-- > 0;)
        if (res[i].status != GB_OK) { bad++; first = i; }
    if (!bad) return GB_OK;
    return fail(ctx, GB_ERR_VERIFY, std::to_string(bad) + " of " + std::to_string(num_proofs) + " proofs did not verify; the first is proof " +
                                        std::to_string(first) + ": " + vcheck_text(res[first].check));
}

// ---- gb_fri_verify_batch: gb_fri_verify of many proofs on one instance shape, the query rounds through the general layout
// (kernels.hpp: FriVerifyLayout).  The shape has been checked by the entry point exactly as gb_fri_verify checks it.
struct FriShapeArgs {
    u32 degree_bits, rate_bits, cap_height;
    bool hiding;
    const uint32_t *num_polys, *blinding;
    u32 num_oracles;
    const uint32_t* batch_sizes;
    u32 num_batches;
    const uint32_t* polynomials;
    std::vector<uint32_t> arity_bits;
    u32 pow_bits, nqr;
};
struct FriItemArgs {
    const void* const* points;
    const void* const* openings;
    const void* const* caps;
    const void* const* proofs;
    const size_t* lens;
};

template <class F>
struct FriBatchPlan {
    typedef typename F::T T;
    typedef typename F::E E;
    const FriShapeArgs& a;
    FriInstance<F> proto;   // the instance without its points
    gbk::FriVerifyLayout L{};
    std::vector<gbk::VerifyTree> trees;
    std::vector<u32> batch_base, poly_off;
    size_t cap_elems = 0, final_len = 0, total_polys = 0;
    size_t head_bytes = 0, query_bytes = 0, tail_bytes = 0, per_proof_bytes = 0, stride = 0, scratch_bytes = 0;
    bool device_ok = false;   // the shape is inside the device path's limits (include/goldibear_gpu.h)
    explicit FriBatchPlan(const FriShapeArgs& args) : a(args) {
        constexpr size_t TS = sizeof(T);
        constexpr u32 D = F::D, H = F::H;
        const u32 no = a.num_oracles, nl = (u32)a.arity_bits.size(), lgN = a.degree_bits + a.rate_bits;
        proto = fri_shape_instance<F>(a.degree_bits, a.rate_bits, a.cap_height, a.hiding, a.num_polys, a.blinding, no, a.batch_sizes,
                                      a.num_batches, a.polynomials);
        for (u32 b = 0; b < a.num_batches; b++) {
            batch_base.push_back((u32)total_polys);
            total_polys += a.batch_sizes[b];
        }
        cap_elems = (size_t)H << a.cap_height;
        final_len = fri_final_len(a.degree_bits, a.arity_bits);
        head_bytes = (size_t)nl * cap_elems * TS;
        tail_bytes = (D * final_len + 1) * TS;
        // one query round, as BatchPlan lays it out: per oracle the row and its path behind a length byte, then the layers likewise
        trees.resize((size_t)no + nl);
        size_t off = 0;
        u32 t = 0, shift = 0;
        for (u32 o = 0; o < no; o++, t++) {
            gbk::VerifyTree& tr = trees[t];
            tr.row_off = (u32)off; tr.num_words = (u32)proto.row_widths[o];
            off += proto.row_widths[o] * TS + 1;
            tr.path_off = (u32)off; tr.path_len = lgN - a.cap_height;
            off += (size_t)tr.path_len * H * TS;
            tr.shift = 0;
            tr.cap_word = (u32)(o * cap_elems);
        }
        for (u32 li = 0; li < nl; li++, t++) {
            const u32 ab = a.arity_bits[li];
            shift += ab;
            gbk::VerifyTree& tr = trees[t];
            tr.row_off = (u32)off; tr.num_words = D << ab;
            off += ((size_t)D << ab) * TS + 1;
            tr.path_off = (u32)off; tr.path_len = lgN - shift - a.cap_height;   // >= 0: check_fri_reduction_arity_bits
            off += (size_t)tr.path_len * H * TS;
            tr.shift = shift;
            tr.cap_word = (u32)((no + li) * cap_elems);
        }
        query_bytes = off * a.nqr;
        const size_t ext_bytes = (1 + 3 * (size_t)a.num_batches + nl + final_len) * sizeof(E);
        const size_t caps_off = ext_bytes + 8 * (size_t)a.nqr;
        const size_t rec_bytes = (caps_off + ((size_t)no + nl) * cap_elems * TS + 15) & ~(size_t)15;
        device_ok = no <= GB_FRI_VERIFY_BATCH_MAX_ORACLES && a.num_batches <= GB_FRI_VERIFY_BATCH_MAX_BATCHES &&
                    total_polys <= GB_FRI_VERIFY_BATCH_MAX_POLYNOMIALS && nl <= GB_MAX_FRI_LAYERS && a.nqr <= GB_MAX_FRI_QUERY_ROUNDS &&
                    (size_t)no + 2 * (size_t)nl + 1 < ((size_t)1 << gbk::vq::POS_BITS) && query_bytes + rec_bytes <= (size_t)GB_FRI_VERIFY_BATCH_MAX_ITEM_BYTES;   // (a staging slot holds at least one item)
        if (!device_ok) return;
        for (u32 b = 0; b < a.num_batches; b++)
            for (const std::pair<u32, u32>& pl : proto.batches[b].polys) poly_off.push_back(trees[pl.first].row_off + (u32)(pl.second * TS));
        L.nqr = a.nqr; L.lgN = lgN; L.num_oracles = no; L.num_batches = a.num_batches; L.num_layers = nl; L.final_len = (u32)final_len;
        L.round_bytes = (u32)off;
        L.rec_x_off = (u32)ext_bytes; L.rec_caps_off = (u32)caps_off; L.rec_bytes = (u32)rec_bytes;
        stride = query_bytes;
        per_proof_bytes = query_bytes + rec_bytes;
    }
    u32 num_oracles() const { return a.num_oracles; }
    // the shape's tables as one block of u32 words: trees, arity_bits, batch_sizes, batch_base, poly_off
    std::vector<u32> tables() const {
        std::vector<u32> w;
        for (const gbk::VerifyTree& tr : trees) w.insert(w.end(), {tr.row_off, tr.num_words, tr.path_off, tr.path_len, tr.shift, tr.cap_word});
        w.insert(w.end(), a.arity_bits.begin(), a.arity_bits.end());
        w.insert(w.end(), a.batch_sizes, a.batch_sizes + a.num_batches);
        w.insert(w.end(), batch_base.begin(), batch_base.end());
        w.insert(w.end(), poly_off.begin(), poly_off.end());
        return w;
    }
    void point_tables(const u32* dev) {
        static_assert(sizeof(gbk::VerifyTree) == 6 * sizeof(u32), "VerifyTree is six words");
        L.trees = reinterpret_cast<const gbk::VerifyTree*>(dev);
        L.arity_bits = dev + 6 * trees.size();
        L.batch_sizes = L.arity_bits + a.arity_bits.size();
        L.batch_base = L.batch_sizes + a.num_batches;
        L.poly_off = L.batch_base + a.num_batches;
    }
    static const char* scope(int i) {
        static const char* const names[4] = {"fri verify batch: host stage", "fri verify batch: upload", "fri verify batch: paths",
                                             "fri verify batch: queries"};
        return names[i];
    }
};

// The host stage of one item, in gb_fri_verify's order (fri_verify_impl): the item's words, the proof's bytes, the transcript, the
// proof of work.  true: the item is regular and the device can take it - its query rounds and record stand at rounds_dst / rec_dst
// (where the plan has a device layout and they are not NULL); false: *res is final.
template <class F>
bool fri_host_stage(const FriBatchPlan<F>& plan, const FriItemArgs& items, size_t i, typename Host<F>::Challenger ch, gb_verify_result* res,
                    unsigned char* rounds_dst, unsigned char* rec_dst) {
    typedef typename F::T T;
    typedef typename F::E E;
    constexpr u32 H = F::H;
    const FriShapeArgs& a = plan.a;
    *res = gb_verify_result{GB_OK, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
    try {
        const uint8_t* bytes = static_cast<const uint8_t*>(items.proofs[i]);
        const size_t len = items.lens[i];
        const u32 nl = (u32)a.arity_bits.size();
        FriInstance<F> in = plan.proto;
        std::vector<std::vector<E>> open;
        std::vector<const T*> cap_ptrs;
        fri_read_item<F>(in, items.points[i], items.openings[i], items.caps[i], plan.cap_elems, open, cap_ptrs,
                         [](const char*) { vfail(GB_VCHECK_NON_CANONICAL); });
        const T* caps = static_cast<const T*>(items.caps[i]);
        ParsedProof<F> pp;
        Challenges<F> chal;
        fri_read_proof<F>(in, a.arity_bits, a.nqr, plan.cap_elems, plan.final_len, ch, bytes, len, pp, chal, [] { vfail(GB_VCHECK_TRAILING); });
        const FriQueryMath<F> fri(std::move(in), open, chal.fri_alpha);
        check_pow<F>(a.pow_bits, chal);
        // the regular shape: every path as long as the shape says, so that the query rounds stand at the shape's offsets
        bool regular = plan.device_ok && len == plan.head_bytes + plan.query_bytes + plan.tail_bytes;
        for (const auto& q : pp.queries) {
            for (u32 o = 0; o < a.num_oracles && regular; o++) regular = q.paths[o].size() == (size_t)H * plan.trees[o].path_len;
            for (u32 li = 0; li < nl && regular; li++) regular = q.step_paths[li].size() == (size_t)H * plan.trees[a.num_oracles + li].path_len;
        }
        if (!regular) {   // the host's own walk: GB_ERR_INVALID and GB_ERR_VERIFY in gb_fri_verify's order by construction
            verify_fri_queries<F>(fri, cap_ptrs.data(), a.arity_bits, pp, chal);
            return false;
        }
        if (!rounds_dst || !rec_dst) return true;
        const gbk::FriVerifyLayout& L = plan.L;
        std::memcpy(rounds_dst, bytes + plan.head_bytes, plan.query_bytes);
        E* e = reinterpret_cast<E*>(rec_dst);
        const u32 nb = a.num_batches;
        e[0] = chal.fri_alpha;
        for (u32 b = 0; b < nb; b++) { e[1 + b] = fri.red_open[b]; e[1 + nb + b] = fri.alpha_shift[b]; e[1 + 2 * nb + b] = fri.points[b]; }
        for (u32 li = 0; li < nl; li++) e[1 + 3 * nb + li] = chal.fri_betas[li];
        for (size_t k = 0; k < plan.final_len; k++) e[1 + 3 * nb + nl + k] = pp.final_poly[k];
        std::memcpy(rec_dst + L.rec_x_off, chal.x_indices.data(), 8 * (size_t)L.nqr);
        T* rc = reinterpret_cast<T*>(rec_dst + L.rec_caps_off);
        std::memcpy(rc, caps, a.num_oracles * plan.cap_elems * sizeof(T));
        for (u32 li = 0; li < nl; li++) std::memcpy(rc + (a.num_oracles + li) * plan.cap_elems, pp.layer_caps[li].data(), plan.cap_elems * sizeof(T));
        return true;
    } catch (const VerifyFail& f) {
        *res = vresult(f);
        return false;
    }
}

template <class F>
void launch_chunk(gb_ctx* ctx, const FriBatchPlan<F>& plan, const gbk::FriVerifyLayout& L, const unsigned char* d_rounds,
                  const unsigned char* d_recs, const typename F::T*, unsigned char*, u64* keys) {
    {
        Scope sc(ctx, plan.scope(2));
        gbk::fri_verify_paths<F>(L, d_rounds, d_recs, keys, ctx->stream);
    }
    {
        Scope sc(ctx, plan.scope(3));
        gbk::fri_verify_queries<F>(L, d_rounds, d_recs, keys, ctx->stream);
    }
}

template <class F>
gb_status fri_verify_batch_impl(gb_ctx* ctx, const FriShapeArgs& shape, const FriItemArgs& items, const gb_challenger_state* challengers,
                                u32 num_items, gb_verify_result* results) {
    typedef typename Host<F>::Challenger Challenger;
    FriBatchPlan<F> plan(shape);
    // the transcripts, by value; one the library cannot read is that item's GB_ERR_INVALID, as gb_fri_verify answers it
    std::vector<Challenger> chs(num_items);
    std::vector<unsigned char> bad_ch(num_items, 0);
    for (u32 i = 0; i < num_items; i++) bad_ch[i] = challenger_from_state<F>(ctx, &challengers[i], chs[i]) != GB_OK;
    auto stage = [&](size_t i, gb_verify_result* res, unsigned char* rounds_dst, unsigned char* rec_dst) {
        // gb_fri_verify's first two refusals of an item, in its order: fewer bytes than query rounds, a challenger it cannot read
        if (shape.nqr > items.lens[i]) {
            *res = gb_verify_result{GB_ERR_INVALID, GB_VCHECK_TRUNCATED, UINT32_MAX, UINT32_MAX};
            return false;
        }
        if (bad_ch[i]) {
            *res = gb_verify_result{GB_ERR_INVALID, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
            return false;
        }
        return fri_host_stage<F>(plan, items, i, chs[i], res, rounds_dst, rec_dst);
    };
    if (!ctx) {   // the host stage alone, on the calling thread: what it would hand to the device is GB_ERR_INVALID, for there is none
        for (u32 i = 0; i < num_items; i++)
            if (stage(i, &results[i], nullptr, nullptr)) results[i] = gb_verify_result{GB_ERR_INVALID, GB_VCHECK_NONE, UINT32_MAX, UINT32_MAX};
        return GB_OK;
    }
    if (!plan.device_ok) {   // beyond the device path's limits: every item is walked on the host, over the copy threads
        const unsigned nthreads = (unsigned)std::max(1, std::min<int>(ctx->copy_threads, (int)num_items));
        run_on_threads(nthreads, num_items, [&](size_t i) { (void)stage(i, &results[i], nullptr, nullptr); });
        ctx->fri_batch_host_items += num_items;
        return GB_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<u32> words = plan.tables();   // (alive until the call's last read-back: the copy below may still read it)
    if (gb_status s = ensure(ctx, ctx->vshape, words.size() * sizeof(u32))) return s;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->vshape.p, words.data(), words.size() * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
    plan.point_tables(static_cast<const u32*>(ctx->vshape.p));
    u64 device_items = 0;
    const gb_status s = verify_batch_impl<F>(ctx, plan, nullptr, 0, num_items, results, stage, &device_items);
    if (s == GB_OK) {
        ctx->fri_batch_device_items += device_items;
        ctx->fri_batch_host_items += num_items - device_items;
    }
    return s;
}

// GB_CATCH of an entry point that returns text instead of a status: the empty string
struct TextEntryPoint {};
const char* unwound(TextEntryPoint, const char*) noexcept { return ""; }

}  // namespace

extern "C" {

gb_status gb_verify_batch(gb_ctx* ctx, gb_circuit* c, const void* const* proofs, const size_t* proof_lens, uint32_t num_proofs,
                          uint32_t flags, void* results) try {
    return verify_batch_call(ctx, c, proofs, proof_lens, num_proofs, flags, results, false);
} GB_CATCH(ctx)

gb_status gb_verify_compressed_batch(gb_ctx* ctx, gb_circuit* c, const void* const* proofs, const size_t* proof_lens,
                                     uint32_t num_proofs, uint32_t flags, void* results) try {
    return verify_batch_call(ctx, c, proofs, proof_lens, num_proofs, flags, results, true);
} GB_CATCH(ctx)

gb_status gb_fri_verify_batch(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t hiding,
                              const uint32_t* oracle_num_polys, const uint32_t* oracle_blinding, uint32_t num_oracles,
                              const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials,
                              const uint32_t* reduction_arity_bits, uint32_t num_layers, uint32_t proof_of_work_bits,
                              uint32_t num_query_rounds, const void* const* points, const void* const* openings,
                              const void* const* initial_caps, const gb_challenger_state* challengers, const void* const* fri_proofs,
                              const size_t* fri_proof_lens, uint32_t num_items, uint32_t flags, void* results) try {
    // the shape: gb_fri_verify's checks, statuses and messages
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field");
    if (flags != 0) return fail(ctx, GB_ERR_INVALID, "gb_fri_verify_batch: flags must be 0");
    if (!oracle_num_polys || !oracle_blinding) return fail(ctx, GB_ERR_INVALID, "null argument");
    const u32 two_adicity = field == GB_GOLDILOCKS ? GlF::TWO_ADICITY : BbF::TWO_ADICITY;
    if (degree_bits > two_adicity || rate_bits > two_adicity || degree_bits + rate_bits > two_adicity)
        return fail(ctx, GB_ERR_INVALID, "LDE size exceeds the field's two-adicity");
    if (cap_height > degree_bits + rate_bits) return fail(ctx, GB_ERR_INVALID, "cap_height should be at most log2(leaves.len())");
    if (gb_status s = check_fri_instance_lists(ctx, oracle_num_polys, num_oracles, batch_sizes, num_batches, polynomials)) return s;
    if (gb_status s = check_fri_reduction_arity_bits(ctx, degree_bits, rate_bits, cap_height, reduction_arity_bits, num_layers)) return s;
    if (proof_of_work_bits > 31) return fail(ctx, GB_ERR_INVALID, "proof_of_work_bits above 31");
    if (num_query_rounds == 0) return fail(ctx, GB_ERR_INVALID, "num_query_rounds is zero: a proof without queries proves nothing");
    if (num_query_rounds > GB_MAX_FRI_QUERY_ROUNDS) return fail(ctx, GB_ERR_INVALID, "more than GB_MAX_FRI_QUERY_ROUNDS query rounds");
    // the items
    if (num_items) {
        if (!points || !openings || !initial_caps || !challengers || !fri_proofs || !fri_proof_lens || !results)
            return fail(ctx, GB_ERR_INVALID, "null argument");
        for (uint32_t i = 0; i < num_items; i++)
            if (!points[i] || !openings[i] || !initial_caps[i] || !fri_proofs[i])
                return fail(ctx, GB_ERR_INVALID, "null entry for item " + std::to_string(i));
    }
    FriShapeArgs shape{degree_bits, rate_bits, cap_height, hiding != 0, oracle_num_polys, oracle_blinding, num_oracles, batch_sizes,
                       num_batches, polynomials, std::vector<uint32_t>(reduction_arity_bits, reduction_arity_bits + num_layers),
                       proof_of_work_bits, num_query_rounds};
    const FriItemArgs items{points, openings, initial_caps, fri_proofs, fri_proof_lens};
    gb_verify_result* res = static_cast<gb_verify_result*>(results);
    if (!ctx) {   // the host stage alone (tests/sanitize drives it this way)
        if (num_items) {
            if (field == GB_GOLDILOCKS) (void)fri_verify_batch_impl<GlF>(nullptr, shape, items, challengers, num_items, res);
            else (void)fri_verify_batch_impl<BbF>(nullptr, shape, items, challengers, num_items, res);
        }
        return fail(nullptr, GB_ERR_INVALID, "null ctx");
    }
    if (num_items == 0) return GB_OK;
    gb_status s;
    try {
        s = field == GB_GOLDILOCKS ? fri_verify_batch_impl<GlF>(ctx, shape, items, challengers, num_items, res)
                                   : fri_verify_batch_impl<BbF>(ctx, shape, items, challengers, num_items, res);
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);   // earlier chunks may still read the staging slots
        throw;
    }
    if (s != GB_OK) {
        (void)hipStreamSynchronize(ctx->stream);   // nothing of the call may still read the staging slots
        return s;
    }
    uint32_t bad = 0, first = 0;
    for (uint32_t i = num_items; i-- > 0;)
        if (res[i].status != GB_OK) { bad++; first = i; }
    if (!bad) return GB_OK;
    return fail(ctx, GB_ERR_VERIFY, std::to_string(bad) + " of " + std::to_string(num_items) + " FRI proofs did not verify; the first is item " +
                                        std::to_string(first) + ": " + vcheck_text(res[first].check));
} GB_CATCH(ctx)

gb_status gb_fri_verify_batch_counts(gb_ctx* ctx, uint64_t* device_items, uint64_t* host_items) try {
    if (!ctx || !device_items || !host_items) return fail(ctx, GB_ERR_INVALID, "null argument");
    *device_items = ctx->fri_batch_device_items;
    *host_items = ctx->fri_batch_host_items;
    return GB_OK;
} GB_CATCH(ctx)

const char* gb_verify_check_text(uint32_t check) try {
    return vcheck_text(check);
} GB_CATCH(TextEntryPoint{})

}  // extern "C"

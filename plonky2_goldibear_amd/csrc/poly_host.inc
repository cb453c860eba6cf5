// The primitives PolynomialBatch and prove() are made of, as entry points of their own (include/goldibear_gpu.h, "polynomials and
// Merkle trees on their own"): PolynomialCoeffs::fft / coset_fft, PolynomialValues::ifft / coset_ifft / lde / lde_onto_coset
// (field/src/polynomial/mod.rs) and MerkleTree::new (hash/merkle_tree.rs).  The transforms are commit()'s - intt_columns and
// lde_columns with the coset set of the caller's shift - between the passes of kernels_poly.hip that bring the caller's layout
// (canonical words, natural order, extension elements as interleaved words, row-major leaves) to the kernels' and back.
// Included by api.hip.

namespace {

// a block of the context's pool for the length of one call
struct PoolBlock {
    gb_ctx* ctx;
    void* p = nullptr;
    size_t bytes = 0;
    explicit PoolBlock(gb_ctx* c) : ctx(c) {}
    PoolBlock(const PoolBlock&) = delete;
    ~PoolBlock() { if (p) pool_free(ctx, p, bytes); }   // stream-ordered reuse: every reader is enqueued before the next taker
    gb_status get(size_t b, const char* what) {
        if (pool_alloc(ctx, b, &p) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(ctx, GB_ERR_OOM, std::string("hipMalloc ") + what);
        }
        bytes = b;
        return GB_OK;
    }
};

enum class PolyOp { Fft, Ifft, Lde };

template <class F>
gb_status poly_transform(gb_ctx* ctx, PolyOp op, const void* in, void* out, size_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t ext,
                         const void* shift_ptr, uint32_t flags) {
    typedef typename F::T T;
    typedef Host<F> HF;
    if (ext > 1) return fail(ctx, GB_ERR_INVALID, "ext is 0 (base-field elements) or 1 (extension-field elements)");
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0, dev_in = (flags & GB_INPUT_DEVICE) != 0;
    if (p3 && dev_in) return fail(ctx, GB_ERR_INVALID, "GB_INPUT_P3_REPR describes host memory; device inputs are canonical");
    if (log_n > F::TWO_ADICITY || rate_bits > F::TWO_ADICITY || log_n + rate_bits > F::TWO_ADICITY)
        return fail(ctx, GB_ERR_INVALID, "transform size exceeds the field's two-adicity (32 Goldilocks / 27 BabyBear; fft.rs:174-180)");
    T shift = F::one();
    if (shift_ptr) {
        const T s = *static_cast<const T*>(shift_ptr);
        if (s == 0 || (u64)s >= F::ORDER) return fail(ctx, GB_ERR_INVALID, "shift must be a canonical non-zero base-field element");
        shift = F::enc(s);
    }
    if (ncols == 0) return GB_OK;
    if (!in || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const u32 D = ext ? F::D : 1, log_N = log_n + rate_bits;
    const size_t cc = ncols * D;   // coordinate columns
    size_t in_bytes, out_bytes;
    if (__builtin_mul_overflow(cc, sizeof(T) << log_n, &in_bytes) || __builtin_mul_overflow(cc, sizeof(T) << log_N, &out_bytes) ||
        cc / D != ncols || (out_bytes / sizeof(T)) >> 38)
        return fail(ctx, GB_ERR_OOM, "the transform does not fit the device");
    hipStream_t st = ctx->stream;
    gb_status s;

    // host blocks: up in one copy, down in one copy (a pageable block is staged by the runtime)
    PoolBlock up(ctx), down(ctx);
    const T* src = static_cast<const T*>(in);
    T* dst = static_cast<T*>(out);
    if (!dev_in) {
        if ((s = up.get(in_bytes, "input"))) return s;
        if (out_bytes != in_bytes && (s = down.get(out_bytes, "output"))) return s;
        HIP_TRY(ctx, hipMemcpyAsync(up.p, in, in_bytes, hipMemcpyHostToDevice, st));
        if (p3) p3_to_canonical_dev<F>((T*)up.p, in_bytes / sizeof(T), st);
        src = (const T*)up.p;
        dst = (T*)(down.p ? down.p : up.p);   // same length: transformed in place, as the reference consumes `self`
    }
    // the sets of the shifts the library's own callers use stay in the context's cache; any other shift's live for this call
    TempCosets<F> tmp(ctx);
    TempCosets<F>* const tc = (shift == F::one() || shift == F::generator()) ? nullptr : &tmp;
    const typename HF::Tables* tabs;
    if ((s = tables_for<F>(ctx, log_n, &tabs))) return s;

    // The passes run on the caller's canonical words as they are, BabyBear's too (linear maps whose factors are table values in
    // Montgomery form: kernels_poly.hip).  A block of the library's own holds the coordinate columns of extension elements, and
    // the coefficients between gb_lde's two transforms.
    PoolBlock work(ctx);
    const T* a = src;
    if (ext || op == PolyOp::Lde) {
        if ((s = work.get(in_bytes, "coefficients"))) return s;
        if (ext) {
            gbk::ext_load<F>(src, (T*)work.p, ncols, log_n, st);
            a = (const T*)work.p;
        }
    }
    if (op != PolyOp::Fft) {   // values on H_n -> coefficients
        T* coeffs = work.p ? (T*)work.p : dst;   // (base-field ifft: straight into the output)
        if ((s = ensure(ctx, ctx->scratch, in_bytes))) return s;
        { Scope sc(ctx, "IFFT"); gbk::intt_columns<F>(a, coeffs, (T*)ctx->scratch.p, cc, *tabs, st); }
        a = coeffs;
    }
    if (op == PolyOp::Ifft) {
        // coset_ifft (polynomial/mod.rs:62-72): coefficient i times shift^-i - the split powers of the inverse shift's one coset
        const typename HF::Cosets* inv = nullptr;
        if (shift != F::one() && (s = cosets_for<F>(ctx, log_n, 0, shift, true, &inv, tc))) return s;
        if (inv || ext)   // (base field, no shift: the inverse transform has written the output)
            gbk::poly_store<F>(a, dst, ncols, log_n, ext != 0, inv ? inv->pow_lo : nullptr, inv ? inv->pow_hi : nullptr, st);
    } else {   // coefficients -> values on shift H_N: leaf order from the LDE passes, then the permutation to natural order
        const typename HF::Cosets* cos;
        if ((s = cosets_for<F>(ctx, log_n, rate_bits, shift, false, &cos, tc))) return s;
        PoolBlock lde(ctx);
        if ((s = lde.get(out_bytes, "transform output"))) return s;
        { Scope sc(ctx, "FFT + blinding"); gbk::lde_columns<F>(a, (T*)lde.p, cc, *tabs, *cos, st); }
        gbk::poly_bitrev_store<F>((const T*)lde.p, dst, ncols, log_N, ext != 0, st);
    }
    if (hipGetLastError() != hipSuccess) return fail(ctx, GB_ERR_HIP, "kernel launch failed");
    if (!dev_in) {
        HIP_TRY(ctx, hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return GB_OK;
}

gb_status poly_entry(gb_ctx* ctx, PolyOp op, uint32_t field, const void* in, void* out, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                     uint32_t ext, const void* shift, uint32_t flags) {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (flags & ~GB_PUBLIC_INPUT_FLAGS) return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    gb_status s;
    if (field == GB_GOLDILOCKS) s = poly_transform<GlF>(ctx, op, in, out, ncols, log_n, rate_bits, ext, shift, flags);
    else if (field == GB_BABYBEAR) s = poly_transform<BbF>(ctx, op, in, out, ncols, log_n, rate_bits, ext, shift, flags);
    else return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    // after an error nothing of a host call may still be reading or writing the caller's blocks
    if (s != GB_OK && !(flags & GB_INPUT_DEVICE)) (void)hipStreamSynchronize(ctx->stream);
    return s;
}

// MerkleTree::new: the tree is a batch without polynomials - its `lde` block the leaves, column-major in device form like a
// commitment's, its digest levels the same - so cap, rows, paths and the reference's digest layout are the batch's read-backs
template <class F>
gb_status merkle_tree_create(gb_ctx* ctx, const void* leaves, uint32_t log_leaves, uint32_t leaf_len, uint32_t cap_height, uint32_t flags,
                             gb_batch** out) {
    typedef typename F::T T;
    typedef Host<F> HF;
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0, dev_in = (flags & GB_INPUT_DEVICE) != 0;
    if (p3 && dev_in) return fail(ctx, GB_ERR_INVALID, "GB_INPUT_P3_REPR describes host memory; device inputs are canonical");
    if (!leaves) return fail(ctx, GB_ERR_INVALID, "null leaves");
    if (leaf_len == 0) return fail(ctx, GB_ERR_INVALID, "leaf_len is zero: a leaf holds at least one element");
    if (log_leaves > 40) return fail(ctx, GB_ERR_INVALID, "more than 2^40 leaves");
    if (cap_height > log_leaves)   // merkle_tree.rs:154-157
        return fail(ctx, GB_ERR_INVALID, "cap_height=" + std::to_string(cap_height) + " should be at most log2(leaves.len())=" + std::to_string(log_leaves));
    if (leaf_len > gbk::ROWS_MAX_WIDTH) return fail(ctx, GB_ERR_UNSUPPORTED, "leaves of more than 64 * 65535 elements");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const u64 L = (u64)1 << log_leaves;
    size_t leaf_bytes;
    if (__builtin_mul_overflow((size_t)leaf_len * sizeof(T), (size_t)L, &leaf_bytes)) return fail(ctx, GB_ERR_OOM, "the leaves do not fit the device");

    gb_batch* b = new (std::nothrow) gb_batch();
    if (!b) return fail(ctx, GB_ERR_OOM, "host allocation failed");
    b->ctx = ctx; b->field = F::TAG; b->log_n = log_leaves; b->rate_bits = 0; b->cap_height = cap_height; b->nsalt = 0; b->ncols = leaf_len;
    auto cleanup = [&](gb_status s) {
        gb_batch_free(b);
        return s;
    };
    void* p = nullptr;
    if (pool_alloc(ctx, leaf_bytes, &p) != hipSuccess) { (void)hipGetLastError(); return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc leaves")); }
    b->lde = (u64*)p; b->lde_bytes = leaf_bytes;
    if (pool_alloc(ctx, 2 * (size_t)L * 32, &p) != hipSuccess) { (void)hipGetLastError(); return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc digests")); }
    b->levels = (u64*)p; b->levels_bytes = 2 * (size_t)L * 32;

    hipStream_t st = ctx->stream;
    PoolBlock up(ctx);
    const T* rows = static_cast<const T*>(leaves);
    if (!dev_in) {
        if (gb_status s = up.get(leaf_bytes, "leaf upload")) return cleanup(s);
        if (hipMemcpyAsync(up.p, leaves, leaf_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return cleanup(fail(ctx, GB_ERR_HIP, "copy of the leaves failed"));
        if (p3) p3_to_canonical_dev<F>((T*)up.p, leaf_bytes / sizeof(T), st);
        rows = (const T*)up.p;
    }
    T* const cols = (T*)b->lde;
    T* const lv = (T*)b->levels;
    {
        Scope sc(ctx, "build Merkle tree");
        gbk::rows_to_columns<F>(rows, cols, L, leaf_len, st);
        {
            Scope sl(ctx, "hash leaves");
            HF::merkle_leaves(cols, L, leaf_len, lv, st);
        }
        for (u32 k = 0; k < log_leaves - cap_height; k++)
            HF::merkle_level(lv + F::H * level_offset(L, k), lv + F::H * level_offset(L, k + 1), L >> (k + 1), st);
    }
    if (hipGetLastError() != hipSuccess) return cleanup(fail(ctx, GB_ERR_HIP, "kernel launch failed"));
    if (!dev_in && hipStreamSynchronize(st) != hipSuccess) return cleanup(fail(ctx, GB_ERR_HIP, "waiting for the upload of the leaves failed"));
    *out = b;
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_fft(gb_ctx* ctx, uint32_t field, const void* coeffs, void* values, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                 uint32_t ext, const void* shift, uint32_t flags) try {
    return poly_entry(ctx, PolyOp::Fft, field, coeffs, values, ncols, log_n, rate_bits, ext, shift, flags);
} GB_CATCH(ctx)

gb_status gb_ifft(gb_ctx* ctx, uint32_t field, const void* values, void* coeffs, size_t ncols, uint32_t log_n, uint32_t ext,
                  const void* shift, uint32_t flags) try {
    return poly_entry(ctx, PolyOp::Ifft, field, values, coeffs, ncols, log_n, 0, ext, shift, flags);
} GB_CATCH(ctx)

gb_status gb_lde(gb_ctx* ctx, uint32_t field, const void* values, void* out, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                 uint32_t ext, const void* shift, uint32_t flags) try {
    return poly_entry(ctx, PolyOp::Lde, field, values, out, ncols, log_n, rate_bits, ext, shift, flags);
} GB_CATCH(ctx)

gb_status gb_merkle_tree_create(gb_ctx* ctx, uint32_t field, const void* leaves, uint32_t log_leaves, uint32_t leaf_len,
                                uint32_t cap_height, uint32_t flags, gb_batch** out) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!out) return fail(ctx, GB_ERR_INVALID, "null out");
    *out = nullptr;
    if (flags & ~GB_PUBLIC_INPUT_FLAGS) return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    gb_status s;
    if (field == GB_GOLDILOCKS) s = merkle_tree_create<GlF>(ctx, leaves, log_leaves, leaf_len, cap_height, flags, out);
    else if (field == GB_BABYBEAR) s = merkle_tree_create<BbF>(ctx, leaves, log_leaves, leaf_len, cap_height, flags, out);
    else return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (s != GB_OK && !(flags & GB_INPUT_DEVICE)) (void)hipStreamSynchronize(ctx->stream);   // nothing still reads `leaves`
    return s;
} GB_CATCH(ctx)

gb_status gb_merkle_tree_free(gb_batch* tree) try {
    return gb_batch_free(tree);
} GB_CATCH(nullptr)   // (the object may be gone: the message goes to the thread's own slot)

gb_status gb_merkle_tree_info(const gb_batch* tree, uint32_t* field, uint32_t* log_leaves, uint32_t* leaf_len, uint32_t* cap_height) try {
    if (!tree) return fail(nullptr, GB_ERR_INVALID, "null tree");
    if (field) *field = tree->field;
    if (log_leaves) *log_leaves = tree->log_n + tree->rate_bits;
    if (leaf_len) *leaf_len = (uint32_t)(tree->ncols + tree->nsalt);
    if (cap_height) *cap_height = tree->cap_height;
    return GB_OK;
} GB_CATCH(tree ? tree->ctx : nullptr)

gb_status gb_merkle_tree_cap(gb_batch* tree, void* out) try {
    return gb_batch_cap(tree, out);
} GB_CATCH(tree ? tree->ctx : nullptr)

gb_status gb_merkle_tree_leaf(gb_batch* tree, uint64_t leaf_index, void* row, void* siblings, uint32_t* nsib) try {
    return gb_batch_leaf(tree, leaf_index, row, siblings, nsib);
} GB_CATCH(tree ? tree->ctx : nullptr)

gb_status gb_merkle_tree_digests(gb_batch* tree, void* out) try {
    return gb_batch_digests(tree, out);
} GB_CATCH(tree ? tree->ctx : nullptr)

}  // extern "C"

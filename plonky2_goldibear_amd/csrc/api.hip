// C-ABI implementation (include/goldibear_gpu.h): contexts, device-resident PolynomialBatch
// handles, twiddle/coset table caches and the reference's timing scopes.
#include "../../include/goldibear_gpu.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "bb_field.hpp"
#include "gl_field.hpp"
#include "kernels.hpp"
#include "poseidon2_bb_host.hpp"
#include "poseidon_gl_host.hpp"
#include "verify_query.hpp"

using gbk::BbF;
using gbk::GlF;
using gbk::u32;
using gbk::u64;

namespace {

thread_local std::string g_null_ctx_error;

struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct ScopeAcc {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans;
};

// A context's twiddle and coset tables of one field (device form), built on first use and kept until gb_ctx_destroy
template <class F>
struct TableCache {
    typedef typename F::T T;
    typedef gbk::NttTables<F> Tables;
    typedef gbk::CosetTables<F> Cosets;
    template <class X>
    struct Owner {   // a table set and the device blocks it owns
        X t{};
        std::vector<void*> owned;
        std::vector<size_t> pooled_bytes;   // TempCosets only: `owned` are pool blocks of these sizes
    };
    const T *tw4096_fwd = nullptr, *tw4096_inv = nullptr;
    const T *tw4096_fwd_m = nullptr, *tw4096_inv_m = nullptr;   // Goldilocks: the same times R (Montgomery form)
    std::vector<void*> owned;                                    // the shared 4096-point tables above
    std::map<u32, Owner<Tables>> tables;                         // by log_n
    std::map<std::tuple<u32, u32, T, int>, Owner<Cosets>> cosets;   // by (log_n, rate_bits, shift (device form), inverse)
    std::map<u32, Owner<gbk::sigma::DlogTables<F>>> dlog;           // by log_n: gb_circuit_decode_sigmas' discrete-log tables
    void release() {
        for (void* p : owned) hipFree(p);
        for (auto& kv : dlog) for (void* p : kv.second.owned) hipFree(p);
        for (auto& kv : tables) for (void* p : kv.second.owned) hipFree(p);
        for (auto& kv : cosets) for (void* p : kv.second.owned) hipFree(p);
    }
};

struct Stager;   // page-locked staging ring + copy threads for pageable host columns (below)

}  // namespace

struct gb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host -> device uploads that overlap kernels on `stream` (commit() of host input)
    std::string err;
    bool profiling = false;
    std::map<std::string, ScopeAcc> scopes;
    std::tuple<TableCache<GlF>, TableCache<BbF>> tables;    // cache<F>(ctx)
    std::multimap<size_t, void*> pool;                      // freed batch blocks by size (stream-ordered reuse)
    DeviceBuf scratch;                                      // grow-only workspace
    DeviceBuf small;                                        // small gather staging (rows, siblings)
    DeviceBuf big_work[3];                                  // log_n > 22: work buffers of the outer radix steps (ntt_outer.hpp), one per nesting level
    hipEvent_t upload_mark = nullptr;                       // recorded on `stream` after the last host -> device copy of a commit
    bool upload_marked = false;
    std::vector<gb_circuit*> circuits;                      // live circuits of this context: what they keep for gb_prove_retry is
                                                            // released by gb_ctx_trim and when an allocation would fail
    Stager* stager = nullptr;                               // made on first use by a pageable host input
    // the prover's small transfers - uniform tables up, caps / openings / query rows down - go through page-locked memory of the
    // context (stage_up / ReadBack below): from pageable memory every one of them is a blocking, staged copy of 70-90 us
    char *xfer_up = nullptr, *xfer_down = nullptr;
    size_t xfer_up_off = 0;
    bool xfer_failed = false;
    // gb_ctx_set_option
    int copy_threads = 4;                                   // "copy_threads": -1 = no staging ring (hipMemcpyAsync straight from pageable memory)
    bool retry_verify = false;                              // "retry_verify": gb_prove_retry compares the whole matrix with the kept copy
    bool check_witness = false;                             // "check_witness": gb_prove* check their device witness before the wires commitment
    size_t verify_chunk_bytes = (size_t)8 << 20;            // "verify_chunk_bytes": gb_verify_batch stages and uploads at most this much per chunk
    // gb_verify_batch (verify_batch_host.inc): two page-locked staging slots and their device twins, grow-only, and the failure keys
    char *vstage_host[2] = {nullptr, nullptr}, *vstage_dev[2] = {nullptr, nullptr};
    size_t vstage_bytes = 0;
    hipEvent_t vstage_read[2] = {nullptr, nullptr};         // recorded behind the uploads out of a slot
    DeviceBuf vkeys;
    DeviceBuf vshape;                                       // gb_fri_verify_batch: the shape's tables (kernels.hpp FriVerifyLayout), resident for a call
    u64 fri_batch_device_items = 0, fri_batch_host_items = 0;   // gb_fri_verify_batch_counts
    // include/goldibear_gpu_test_hooks.h: gb_test_force_gate_fallback / gb_test_gate_fallback_launches (kernels.hpp GateLaunchOptions)
    bool test_force_gate_fallback = false;
    u64 test_gate_fallback_launches = 0;
};
static void drop_all_retry_state(gb_ctx* ctx);              // prover_host.inc
static void drop_all_check_state(gb_ctx* ctx);              // prover_host.inc: what gb_check_witness keeps with the circuits

struct gb_batch {
    gb_ctx* ctx = nullptr;
    size_t coeffs_bytes = 0, lde_bytes = 0, levels_bytes = 0;
    u32 field = 0, log_n = 0, rate_bits = 0, cap_height = 0, nsalt = 0;
    size_t ncols = 0;
    u64* coeffs = nullptr;  // [ncols][n]
    u64* lde = nullptr;     // [ncols + nsalt][N], leaf order
    u64* levels = nullptr;  // level-major digests, level k at hash offset 2N - (2N >> k); last level = cap
};

namespace {

gb_status fail(gb_ctx* ctx, gb_status code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_null_ctx_error = msg;
    return code;
}

// ---- "never unwinds" (include/goldibear_gpu.h): EVERY extern "C" definition of this library is a function-try-block that ends in
// GB_CATCH / GB_CATCH_CIRCUIT (tests/test_abi_guards.py parses csrc/ and fails on one that does not) - a Rust caller's
// `panic = unwind` never crosses extern "C" either.  std::bad_alloc -> GB_ERR_OOM, any other std::exception -> GB_ERR_INVALID,
// anything else -> GB_ERR_HIP; device blocks and retry state are released by the guards of the frames the exception unwinds
// through (TmpAlloc, the batch / pool guards of commit() and prove()).  Writing the message must not throw either.
gb_status unwound(gb_ctx* ctx, const char* fn) noexcept {
    gb_status code = GB_ERR_HIP;
    std::string& dst = ctx ? ctx->err : g_null_ctx_error;
    try {
        try {
            throw;
        } catch (const std::bad_alloc&) {
            code = GB_ERR_OOM;
            dst = std::string(fn) + ": host allocation failed";
        } catch (const std::exception& e) {
            code = GB_ERR_INVALID;
            dst = std::string(fn) + ": " + e.what();
        } catch (...) {
            dst = std::string(fn) + ": unknown exception";
        }
    } catch (...) {
        dst.clear();   // no memory for the message either: the status code says it
    }
    return code;
}
#define GB_CATCH(CTX) catch (...) { return unwound((CTX), __func__); }

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(ctx, e_ == hipErrorOutOfMemory ? GB_ERR_OOM : GB_ERR_HIP,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                        \
    } while (0)

struct Scope {
    gb_ctx* ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    hipStream_t on;
    Scope(gb_ctx* c, const char* n, hipStream_t stream = nullptr) : ctx(c), name(n), on(stream ? stream : c->stream) {
        if (!ctx->profiling) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        hipEventRecord(a, on);
    }
    ~Scope() {
        if (!a) return;
        hipEventRecord(b, on);
        ctx->scopes[name].spans.emplace_back(a, b);
    }
};

// Host inputs of the public commit entry points stay the caller's only until the call returns (the reference moves its Vecs in):
// commit() marks the last host -> device copy it enqueues on the main stream, and gb_commit_* wait for that mark and for the copy
// stream before returning - the kernels behind the copies keep running asynchronously.
void mark_upload(gb_ctx* ctx) {
    if (!ctx->upload_mark && hipEventCreateWithFlags(&ctx->upload_mark, hipEventDisableTiming) != hipSuccess) {
        ctx->upload_mark = nullptr;
        (void)hipStreamSynchronize(ctx->stream);   // no event to wait on later: wait here
        return;
    }
    if (hipEventRecord(ctx->upload_mark, ctx->stream) == hipSuccess) ctx->upload_marked = true;
    else (void)hipStreamSynchronize(ctx->stream);
}
gb_status wait_uploads(gb_ctx* ctx) {
    hipError_t e = hipStreamSynchronize(ctx->copy_stream);
    if (e == hipSuccess && ctx->upload_marked) e = hipEventSynchronize(ctx->upload_mark);
    ctx->upload_marked = false;
    return e == hipSuccess ? GB_OK : fail(ctx, GB_ERR_HIP, "waiting for the upload of the host input failed");
}
// Every exit of a commit from HOST input: on success wait for the uploads (the kernels behind them keep running); after an error
// nothing of the call is worth keeping, so wait for both streams - copies from the caller's buffer and into pool blocks that
// commit()'s cleanup has already handed back may still be in flight - and keep the error that was reported first.  A batch
// whose uploads cannot be confirmed is freed, not returned.
gb_status finish_host_commit(gb_ctx* ctx, gb_status s, gb_batch** out) {
    if (!ctx) return s;
    if (s == GB_OK) {
        s = wait_uploads(ctx);
        if (s != GB_OK && out && *out) { gb_batch_free(*out); *out = nullptr; }
        return s;
    }
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->upload_marked = false;
    return s;
}

// ---- small transfers through page-locked memory (round 6).  A 2^12-row proof spent 1.1 of its 4.3 ms in 13 host round trips of
// ~80 us each (profiles/r06_recursion_shape.txt): hipMemcpyAsync from a std::vector is a synchronous, runtime-staged copy.
static constexpr size_t XFER_UP_BYTES = (size_t)4 << 20, XFER_DOWN_BYTES = (size_t)1 << 20;
bool xfer_ready(gb_ctx* ctx) {
    if (ctx->xfer_up) return true;
    if (ctx->xfer_failed) return false;
    void *u = nullptr, *d = nullptr;
    if (hipHostMalloc(&u, XFER_UP_BYTES, hipHostMallocDefault) != hipSuccess || hipHostMalloc(&d, XFER_DOWN_BYTES, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        if (u) (void)hipHostFree(u);
        ctx->xfer_failed = true;   // no page-locked memory to be had: the plain copies still work
        return false;
    }
    ctx->xfer_up = static_cast<char*>(u);
    ctx->xfer_down = static_cast<char*>(d);
    return true;
}
// `bytes` of page-locked memory to fill and hand to ONE hipMemcpyAsync on ctx->stream; it is not written again before the stream
// has passed that copy (the arena is a ring; wrapping around waits for the stream).  nullptr: too big or no arena - copy directly.
void* stage_up(gb_ctx* ctx, size_t bytes) {
    bytes = (bytes + 63) & ~(size_t)63;
    if (bytes > XFER_UP_BYTES / 4 || !xfer_ready(ctx)) return nullptr;
    if (ctx->xfer_up_off + bytes > XFER_UP_BYTES) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return nullptr;
        ctx->xfer_up_off = 0;
    }
    void* p = ctx->xfer_up + ctx->xfer_up_off;
    ctx->xfer_up_off += bytes;
    return p;
}
// device -> host copies that end in one wait: add() enqueues each into the page-locked buffer (or straight into the destination when
// it does not fit), finish() waits for the stream and hands the bytes out
struct ReadBack {
    gb_ctx* ctx;
    struct Item { void* dst; const char* src; size_t bytes; };
    Item items[48];
    unsigned n = 0;
    size_t off = 0;
    explicit ReadBack(gb_ctx* c) : ctx(c) {}
    gb_status add(void* host_dst, const void* dev, size_t bytes) {
        if (!bytes) return GB_OK;
        const size_t padded = (bytes + 63) & ~(size_t)63;
        if (n < 48 && off + padded <= XFER_DOWN_BYTES && xfer_ready(ctx)) {
            char* p = ctx->xfer_down + off;
            HIP_TRY(ctx, hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
            items[n++] = Item{host_dst, p, bytes};
            off += padded;
            return GB_OK;
        }
        HIP_TRY(ctx, hipMemcpyAsync(host_dst, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GB_OK;
    }
    gb_status finish() {   // (polling an event before blocking was tried: no gain - the wake-up is not what these waits cost)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (unsigned i = 0; i < n; i++) std::memcpy(items[i].dst, items[i].src, items[i].bytes);
        n = 0; off = 0;
        return GB_OK;
    }
};
gb_status read_back(gb_ctx* ctx, void* host_dst, const void* dev, size_t bytes) {
    ReadBack rb(ctx);
    if (gb_status s = rb.add(host_dst, dev, bytes)) return s;
    return rb.finish();
}

gb_status ensure(gb_ctx* ctx, DeviceBuf& buf, size_t bytes) {
    if (buf.bytes >= bytes) return GB_OK;
    if (buf.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(buf.p));
        buf.p = nullptr;
        buf.bytes = 0;
    }
    HIP_TRY(ctx, hipMalloc(&buf.p, bytes));
    buf.bytes = bytes;
    return GB_OK;
}

// Batch storage comes from a per-context pool: a prover commits batches of the same few shapes
// over and over, and hipMalloc/hipFree of multi-GiB blocks would otherwise dominate.  All work of
// a context is on one stream, so handing a freed block to a later commit is stream-ordered.
hipError_t pool_alloc(gb_ctx* ctx, size_t bytes, void** out) {
    auto it = ctx->pool.find(bytes);
    if (it != ctx->pool.end()) {
        *out = it->second;
        ctx->pool.erase(it);
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        drop_all_retry_state(ctx);   // what failed attempts left for gb_prove_retry goes first (it lands in the pool)
        for (auto& kv : ctx->pool) (void)hipFree(kv.second);
        ctx->pool.clear();
        e = hipMalloc(out, bytes);
    }
    return e;
}
void pool_free(gb_ctx* ctx, void* p, size_t bytes) noexcept {   // (called from destructors of guards: must not throw)
    if (!p) return;
    try {
        ctx->pool.emplace(bytes, p);
    } catch (...) {   // no memory for the map node: hand the block back to HIP instead (hipFree waits for the device)
        (void)hipFree(p);
    }
}

template <class F>
TableCache<F>& cache(gb_ctx* ctx) { return std::get<TableCache<F>>(ctx->tables); }
template <class F>
constexpr bool is_goldilocks = std::is_same<F, GlF>::value;

template <class T>
gb_status upload(gb_ctx* ctx, const std::vector<T>& host, const T** dev, std::vector<void*>& owned, std::vector<size_t>* pooled_bytes = nullptr) {
    void* p = nullptr;
    if (pooled_bytes) {   // a table of one call (TempCosets): a pool block, written in stream order behind whoever read it last
        const size_t bytes = host.size() * sizeof(T);
        if (pool_alloc(ctx, bytes, &p) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, GB_ERR_OOM, "hipMalloc shift tables"); }
        owned.push_back(p);
        pooled_bytes->push_back(bytes);
        HIP_TRY(ctx, hipMemcpyAsync(p, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // `host` is the caller's local
        *dev = static_cast<const T*>(p);
        return GB_OK;
    }
    HIP_TRY(ctx, hipMalloc(&p, host.size() * sizeof(T)));
    HIP_TRY(ctx, hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *dev = static_cast<const T*>(p);
    owned.push_back(p);
    return GB_OK;
}

template <class F>
std::vector<typename F::T> powers(typename F::T base, size_t count) {
    std::vector<typename F::T> v(count);
    typename F::T x = F::one();
    for (size_t i = 0; i < count; i++) {
        v[i] = x;
        x = F::mul(x, base);
    }
    return v;
}

u32 bitrev32(u32 x, u32 bits) {
    u32 r = 0;
    for (u32 i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

std::vector<u64> times_r(std::vector<u64> v) {   // Goldilocks' Montgomery form of a table: x R mod p, R = 2^64 mod p
    for (u64& x : v) x = GlF::cform(x);
    return v;
}

template <class F>
gb_status tables_for(gb_ctx* ctx, u32 log_n, const typename TableCache<F>::Tables** out) {
    typedef typename F::T T;
    TableCache<F>& tc = cache<F>(ctx);
    auto it = tc.tables.find(log_n);
    if (it != tc.tables.end()) { *out = &it->second.t; return GB_OK; }
    gb_status s;
    if (!tc.tw4096_fwd) {
        const T w = F::two_adic_generator(12);
        std::vector<T> fwd = powers<F>(w, 4096);
        const std::vector<T> inv = powers<F>(F::inv(w), 4096);
        if constexpr (is_goldilocks<F>) {
            // [0, 4096): w_4096^j.  [4096, 8192): the same powers in the order k_gl_lde_pb16's first stage reads them,
            // T[s][m] = w_4096^(brev4(s) m), s < 16, m < 256 - a wave's 64 lanes then read 512 contiguous bytes per slot instead of
            // gathering at stride brev4(s) (up to 60 cache lines per load instruction).
            fwd.resize(8192);
            for (u32 sl = 0; sl < 16; sl++)
                for (u32 m = 0; m < 256; m++) fwd[4096 + sl * 256 + m] = fwd[(bitrev32(sl, 4) * m) & 4095];
        }
        if ((s = upload(ctx, fwd, &tc.tw4096_fwd, tc.owned))) return s;
        if ((s = upload(ctx, inv, &tc.tw4096_inv, tc.owned))) return s;
        if constexpr (is_goldilocks<F>) {
            if ((s = upload(ctx, times_r(fwd), &tc.tw4096_fwd_m, tc.owned))) return s;
            if ((s = upload(ctx, times_r(inv), &tc.tw4096_inv_m, tc.owned))) return s;
        }
    }
    typename TableCache<F>::template Owner<typename TableCache<F>::Tables> set;
    set.t.log_n = log_n;
    set.t.outer_bits = gbk::ntt_outer_bits(log_n);
    if (set.t.outer_bits) {   // the outer radix step (ntt_outer.hpp) runs smaller transforms: their tables first (std::map nodes do not move)
        if ((s = tables_for<F>(ctx, log_n - set.t.outer_bits, &set.t.sub))) return s;
    } else if (log_n > 20) {  // 2^21 / 2^22 rows: the middle inverse pass is a radix-32 / radix-64 DFT with twiddles w_{2^14}^-j
        if constexpr (!is_goldilocks<F>)
            if (log_n == 22)   // BabyBear: the strided LDE pass of 2^22 rows works with the 2^20-row twiddles (k_bb_lde_pa16x2w)
                if ((s = tables_for<F>(ctx, 20, &set.t.wide))) return s;
        const std::vector<T> t16 = powers<F>(F::inv(F::two_adic_generator(14)), (size_t)1 << 14);
        if constexpr (is_goldilocks<F>) s = upload(ctx, times_r(t16), &set.t.tw16k_inv_m, set.owned);   // Montgomery form
        else s = upload(ctx, t16, &set.t.tw16k_inv, set.owned);
        if (s) return s;
    }
    set.t.tw4096_fwd = tc.tw4096_fwd;
    set.t.tw4096_inv = tc.tw4096_inv;
    const T w = F::two_adic_generator(log_n), wi = F::inv(w);
    const size_t n = (size_t)1 << log_n, nhi = n > 1024 ? n / 1024 : 1;
    const std::vector<T> vlo_f = powers<F>(w, 1024), vhi_f = powers<F>(F::pow(w, 1024), nhi), vlo_i = powers<F>(wi, 1024),
                         vhi_i = powers<F>(F::pow(wi, 1024), nhi);
    if ((s = upload(ctx, vlo_f, &set.t.tw_lo_fwd, set.owned))) return s;
    if ((s = upload(ctx, vhi_f, &set.t.tw_hi_fwd, set.owned))) return s;
    if ((s = upload(ctx, vlo_i, &set.t.tw_lo_inv, set.owned))) return s;
    if ((s = upload(ctx, vhi_i, &set.t.tw_hi_inv, set.owned))) return s;
    set.t.n_inv = F::inv(F::enc(n % F::ORDER));
    if (set.t.outer_bits) {
        const u32 log_m = log_n - set.t.outer_bits;
        std::vector<T> top(256);
        for (u32 j = 0; j < 256; j++) top[j] = F::pow(w, (u64)bitrev32(j, 8) << (log_m - 8));
        if ((s = upload(ctx, top, &set.t.tw_top_fwd, set.owned))) return s;
    }
    if constexpr (is_goldilocks<F>) {   // Goldilocks: the Montgomery twins the register-radix passes read (inv16_tables, lde_tables)
        set.t.tw4096_fwd_m = tc.tw4096_fwd_m;
        set.t.tw4096_inv_m = tc.tw4096_inv_m;
        if ((s = upload(ctx, times_r(vlo_f), &set.t.tw_lo_fwd_m, set.owned))) return s;
        if ((s = upload(ctx, times_r(vhi_f), &set.t.tw_hi_fwd_m, set.owned))) return s;
        if ((s = upload(ctx, times_r(vlo_i), &set.t.tw_lo_inv_m, set.owned))) return s;
        if ((s = upload(ctx, times_r(vhi_i), &set.t.tw_hi_inv_m, set.owned))) return s;
        set.t.n_inv_m = GlF::cform(set.t.n_inv);
    }
    auto res = tc.tables.emplace(log_n, std::move(set));
    *out = &res.first->second.t;
    return GB_OK;
}

// coset c (block c of n leaves) has shift s_c = shift * w_N^bitrev_r(c): leaf j = c*n + jl is the LDE
// point shift * w_N^bitrev_logN(j) (fri/oracle.rs:109 + polynomial/mod.rs:282-295; shift = 7, or
// 7^(arity^l) for FRI layer l, fri/prover.rs:122-123).  inverse: tables of s_c^-1 instead.
// log_n > 22: the work buffers of the outer radix steps (de-interleaved coefficients + sub-LDEs of a group of columns), one per nesting
// level, grown on demand before every use: the coset tables hold the ADDRESS of the context's pointer, not the pointer
inline u32 big_work_level(u32 log_n) { return (log_n - gbk::NTT_NATIVE_LOG - 1) / gbk::NTT_OUTER_MAX_BITS; }
gb_status ensure_big_work(gb_ctx* ctx, u32 log_n, u32 rate_bits, size_t es) {
    for (; log_n > gbk::NTT_NATIVE_LOG; log_n -= gbk::ntt_outer_bits(log_n)) {
        const size_t n = (size_t)1 << log_n, per_col = (n + (n << rate_bits)) * es;
        const size_t cols = std::min<size_t>(8, std::max<size_t>(1, ((size_t)8 << 30) / per_col));   // groups of up to 8 columns within 8 GiB
        if (gb_status s = ensure(ctx, ctx->big_work[big_work_level(log_n)], cols * per_col)) return s;
    }
    return GB_OK;
}
// The cache is keyed by the shift and never evicts, so it holds the sets of the shifts the library chooses itself.  The tables of a
// caller-chosen shift (gb_fft / gb_ifft / gb_lde) are built into a TempCosets instead: pool blocks that go back when the call ends.
template <class F>
struct TempCosets {
    typedef typename TableCache<F>::template Owner<typename TableCache<F>::Cosets> Set;
    gb_ctx* ctx;
    std::map<std::tuple<u32, u32, typename F::T, int>, Set> sets;
    explicit TempCosets(gb_ctx* c) : ctx(c) {}
    TempCosets(const TempCosets&) = delete;
    ~TempCosets() {
        for (auto& kv : sets)
            for (size_t i = 0; i < kv.second.pooled_bytes.size(); i++) pool_free(ctx, kv.second.owned[i], kv.second.pooled_bytes[i]);
    }
};
template <class F>
gb_status cosets_for(gb_ctx* ctx, u32 log_n, u32 rate_bits, typename F::T shift, bool inverse,
                     const typename TableCache<F>::Cosets** out, TempCosets<F>* tmp = nullptr) {
    typedef typename F::T T;
    TableCache<F>& tc = cache<F>(ctx);
    auto key = std::make_tuple(log_n, rate_bits, shift, inverse ? 1 : 0);
    auto& sets = tmp ? tmp->sets : tc.cosets;
    auto it = sets.find(key);
    if (it != sets.end()) {
        if (!inverse)   // (released by gb_ctx_trim)
            if (gb_status sw = ensure_big_work(ctx, log_n, rate_bits, sizeof(T))) return sw;
        *out = &it->second.t;
        return GB_OK;
    }
    size_t n = (size_t)1 << log_n;
    size_t nlo = n < 4096 ? n : 4096, nhi = n > 4096 ? n / 4096 : 1;
    u32 nc = 1u << rate_bits;
    T wN = F::two_adic_generator(log_n + rate_bits);
    std::vector<T> lo(nc * nlo), hi(nc * nhi);
    for (u32 c = 0; c < nc; c++) {
        T s = F::mul(shift, F::pow(wN, bitrev32(c, rate_bits)));
        if (inverse) s = F::inv(s);
        std::vector<T> pl = powers<F>(s, nlo), ph = powers<F>(F::pow(s, 4096), nhi);
        std::memcpy(&lo[c * nlo], pl.data(), nlo * sizeof(T));
        std::memcpy(&hi[c * nhi], ph.data(), nhi * sizeof(T));
    }
    // (a TempCosets entry is filled in place: what an error leaves half built is released with the rest of it)
    typename TableCache<F>::template Owner<typename TableCache<F>::Cosets> cached_set;
    auto& set = tmp ? tmp->sets[key] : cached_set;
    std::vector<size_t>* const pooled = tmp ? &set.pooled_bytes : nullptr;
    set.t.rate_bits = rate_bits;
    gb_status s;
    // inverse tables are read as power tables only (the quotient's coset_ifft); the LDE kernels never see them
    if (const u32 K = gbk::ntt_outer_bits(log_n); K && !inverse) {   // sub-transforms of n / R rows on the shift s_c^R, R = 2^K (ntt_outer.hpp)
        if ((s = cosets_for<F>(ctx, log_n - K, rate_bits, F::pow(shift, (u64)1 << K), false, &set.t.sub, tmp))) return s;
        if ((s = ensure_big_work(ctx, log_n, rate_bits, sizeof(T)))) return s;
        DeviceBuf& wb = ctx->big_work[big_work_level(log_n)];
        set.t.work = &wb.p; set.t.work_bytes = &wb.bytes;
    }
    if constexpr (!is_goldilocks<F>)
        if (log_n == 22 && !inverse)   // BabyBear: the finer cosets of 2^20 rows (k_bb_lde_pa16x2w)
            if ((s = cosets_for<F>(ctx, 20, rate_bits + 2, shift, false, &set.t.fine, tmp))) return s;
    if ((s = upload(ctx, lo, &set.t.pow_lo, set.owned, pooled))) return s;
    if ((s = upload(ctx, hi, &set.t.pow_hi, set.owned, pooled))) return s;
    if constexpr (is_goldilocks<F>) {   // Goldilocks: the Montgomery twins the register-radix passes read (inv16_tables, lde_tables)
        if ((s = upload(ctx, times_r(lo), &set.t.pow_lo_m, set.owned, pooled))) return s;
        if ((s = upload(ctx, times_r(hi), &set.t.pow_hi_m, set.owned, pooled))) return s;
    }
    if (tmp) { *out = &set.t; return GB_OK; }
    auto res = tc.cosets.emplace(key, std::move(cached_set));
    *out = &res.first->second.t;
    return GB_OK;
}

// internal flag (not part of the C ABI): device input already in the field's device form (BabyBear: Montgomery)
static constexpr uint32_t GB_INPUT_DEVICE_FORM = 0x100;
static constexpr uint32_t GB_PUBLIC_INPUT_FLAGS = GB_INPUT_DEVICE | GB_INPUT_P3_REPR;   // what a caller may pass
// ... and what the prove entry points with a `salts` argument take besides: the salts are a seed (prover_host.inc: prove())
static constexpr uint32_t GB_PROVE_FLAGS = GB_PUBLIC_INPUT_FLAGS | GB_SALTS_FROM_SEED;
// internal flag: `salts` of commit() is a canonical device block even where `cols` is host memory (the seeded salts of prove())
static constexpr uint32_t GB_SALTS_DEVICE = 0x200;

// A matrix of input columns as the caller holds it: one contiguous [ncols][n] block (`base`), or ncols separately allocated
// columns (`ptrs`) - the reference's Vec<PolynomialValues<F>> (fri/oracle.rs:68-75) and MatrixWitness.wire_values: Vec<Vec<F>>
// (iop/witness.rs:277-279).
struct ColSrc {
    const void* base = nullptr;
    const void* const* ptrs = nullptr;
    ColSrc() {}
    ColSrc(const void* b) : base(b) {}   // NOLINT: the contiguous form converts implicitly
    static ColSrc columns(const void* const* p) { ColSrc s; s.ptrs = p; return s; }
    const char* col(size_t c, size_t col_bytes) const {
        return ptrs ? static_cast<const char*>(ptrs[c]) : static_cast<const char*>(base) + c * col_bytes;
    }
    explicit operator bool() const { return base || ptrs; }
};

// hipHostMalloc / hipHostRegister memory (gb_host_alloc, gb_host_register): the copy engine reads it directly
bool is_pinned_host(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}
bool all_pinned(const ColSrc& src, size_t ncols, size_t col_bytes) {
    if (!src.ptrs) return is_pinned_host(src.base) && is_pinned_host(static_cast<const char*>(src.base) + ncols * col_bytes - 1);
    for (size_t c = 0; c < ncols; c++)
        if (!src.ptrs[c] || !is_pinned_host(src.ptrs[c])) return false;
    return true;
}

// ---- pageable host columns ------------------------------------------------------------------------------------------------------
// hipMemcpyAsync from pageable memory is a synchronous copy that the runtime stages itself, on the calling thread.  A context
// instead owns a page-locked ring (SLOTS slots) and a few copy threads: the columns of an upload chunk are copied into a slot in
// pieces (column 0 first), and the thread that drives the commit issues the host -> device copy of every column from the ring as
// soon as its last piece has landed - while the copy engine moves the slot before and the GPU transforms and hashes the chunk
// before.  The caller's columns are read by the time the call returns; the ring is the library's.
struct Stager {
    static constexpr unsigned SLOTS = 4;
    static constexpr size_t PIECE = (size_t)1 << 20, SLOT_MIN = (size_t)64 << 20;
    struct Piece { const char* src; char* dst; size_t bytes; u32 col; };
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_work, cv_done;
    u64 generation = 0;      // guarded by m
    unsigned parked = 0;     // workers waiting for a job (guarded by m)
    bool stop = false;
    std::vector<Piece> pieces;                       // the job in flight: written only while every worker is parked
    std::atomic<size_t> next{0};
    std::unique_ptr<std::atomic<u32>[]> remaining;   // pieces left per column of the job
    size_t remaining_cap = 0;
    char* ring = nullptr;
    size_t slot_bytes = 0;
    unsigned slot = 0;
    hipEvent_t slot_done[SLOTS] = {};
    bool slot_used[SLOTS] = {};

    explicit Stager(unsigned nthreads) {
        try {   // the C ABI never unwinds: a thread the system refuses is one copy thread less (none: the calling thread copies)
            for (unsigned i = 0; i < nthreads; i++) workers.emplace_back([this] { work(); });
        } catch (...) {
        }
    }
    ~Stager() {
        { std::lock_guard<std::mutex> g(m); stop = true; }
        cv_work.notify_all();
        for (auto& t : workers) t.join();
        for (unsigned i = 0; i < SLOTS; i++)
            if (slot_done[i]) { (void)hipEventSynchronize(slot_done[i]); (void)hipEventDestroy(slot_done[i]); }
        if (ring) (void)hipHostFree(ring);
    }
    void work() {
        std::unique_lock<std::mutex> lk(m);
        u64 seen = 0;
        for (;;) {
            parked++;
            cv_done.notify_all();
            cv_work.wait(lk, [&] { return stop || generation != seen; });
            parked--;
            if (stop) return;
            seen = generation;
            lk.unlock();
            run_pieces();
            lk.lock();
        }
    }
    void run_pieces() {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= pieces.size()) return;
            const Piece& p = pieces[i];
            std::memcpy(p.dst, p.src, p.bytes);
            if (remaining[p.col].fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> g(m);
                cv_done.notify_all();
            }
        }
    }
    bool reserve(size_t need, hipStream_t copy_stream) {   // slots of at least `need` bytes
        if (slot_bytes >= need) return true;
        if (ring) {
            if (hipStreamSynchronize(copy_stream) != hipSuccess) return false;
            (void)hipHostFree(ring);
            ring = nullptr; slot_bytes = 0;
            std::fill(slot_used, slot_used + SLOTS, false);
        }
        const size_t sb = std::max(need, SLOT_MIN);
        void* p = nullptr;
        if (hipHostMalloc(&p, sb * SLOTS, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        ring = static_cast<char*>(p);
        slot_bytes = sb;
        return true;
    }
    // columns [c0, c0 + cc) of `src` -> dst (device, contiguous [cc][col_bytes]) through the ring, on `copy_stream`
    bool upload(const ColSrc& src, size_t c0, size_t cc, size_t col_bytes, char* dst, hipStream_t copy_stream) {
        if (!reserve(col_bytes, copy_stream)) return false;
        const size_t per_slot = std::max<size_t>(1, slot_bytes / col_bytes);
        for (size_t b0 = 0; b0 < cc; b0 += per_slot) {
            const size_t bc = std::min(per_slot, cc - b0);
            const unsigned s = slot;
            slot = (slot + 1) % SLOTS;
            if (slot_used[s] && hipEventSynchronize(slot_done[s]) != hipSuccess) return false;   // the copy engine has left the slot
            char* base = ring + (size_t)s * slot_bytes;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_done.wait(lk, [&] { return parked == workers.size(); });   // nobody is still inside the job before
                pieces.clear();
                if (remaining_cap < bc) { remaining.reset(new std::atomic<u32>[bc]); remaining_cap = bc; }
                for (size_t c = 0; c < bc; c++) {
                    const char* sp = src.col(c0 + b0 + c, col_bytes);
                    u32 np = 0;
                    for (size_t o = 0; o < col_bytes; o += PIECE, np++)
                        pieces.push_back(Piece{sp + o, base + c * col_bytes + o, std::min(PIECE, col_bytes - o), (u32)c});
                    remaining[c].store(np, std::memory_order_relaxed);
                }
                next.store(0, std::memory_order_relaxed);
                generation++;
            }
            cv_work.notify_all();
            if (workers.empty()) run_pieces();   // "copy_threads" = 0: the calling thread copies
            auto drain = [&] {   // an error return must not leave a worker reading the caller's columns
                std::unique_lock<std::mutex> lk(m);
                cv_done.wait(lk, [&] { return next.load(std::memory_order_relaxed) >= pieces.size() && parked == workers.size(); });
                return false;
            };
            for (size_t c = 0; c < bc;) {
                {
                    std::unique_lock<std::mutex> lk(m);
                    cv_done.wait(lk, [&] { return remaining[c].load(std::memory_order_acquire) == 0; });
                }
                size_t e = c + 1;   // every further column that is staged already goes into the same copy
                while (e < bc && remaining[e].load(std::memory_order_acquire) == 0) e++;
                if (hipMemcpyAsync(dst + (b0 + c) * col_bytes, base + c * col_bytes, (e - c) * col_bytes, hipMemcpyHostToDevice,
                                   copy_stream) != hipSuccess)
                    return drain();
                c = e;
            }
            // no event to guard the slot with: the copies out of it are in flight, so wait for them here before anybody may write
            // into the slot again (the caller falls back to plain copies for the rest)
            if (!slot_done[s] && hipEventCreateWithFlags(&slot_done[s], hipEventDisableTiming) != hipSuccess) {
                slot_done[s] = nullptr;
                (void)hipStreamSynchronize(copy_stream);
                return false;
            }
            if (hipEventRecord(slot_done[s], copy_stream) != hipSuccess) {
                (void)hipStreamSynchronize(copy_stream);
                return false;
            }
            slot_used[s] = true;
        }
        return true;
    }
};

// Host columns [c0, c0 + cc) -> dst (device, contiguous) on the context's copy stream.  Page-locked sources go straight to the copy
// engine (one copy for a contiguous block, one per column otherwise); pageable ones through the staging ring, small ones excepted.
bool upload_columns(gb_ctx* ctx, const ColSrc& src, bool pinned, size_t c0, size_t cc, size_t col_bytes, void* dst) {
    char* d = static_cast<char*>(dst);
    const bool ring = !pinned && ctx->copy_threads >= 0 && cc * col_bytes >= ((size_t)2 << 20);
    if (ring) {
        bool done = false;
        try {   // (std::bad_alloc from the piece list: thrown before any worker has been handed the job)
            if (!ctx->stager) ctx->stager = new (std::nothrow) Stager((unsigned)ctx->copy_threads);
            done = ctx->stager && ctx->stager->upload(src, c0, cc, col_bytes, d, ctx->copy_stream);
        } catch (...) {
            done = false;
        }
        if (done) return true;
        (void)hipGetLastError();   // no ring (out of page-locked memory?): the runtime's own pageable path still works
    }
    if (!src.ptrs) return hipMemcpyAsync(d, src.col(c0, col_bytes), cc * col_bytes, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess;
    for (size_t c = 0; c < cc; c++)
        if (hipMemcpyAsync(d + c * col_bytes, src.col(c0 + c, col_bytes), col_bytes, hipMemcpyHostToDevice, ctx->copy_stream) != hipSuccess)
            return false;
    return true;
}
// the same on an arbitrary stream for inputs that are not chunked (small batches, coefficients): plain copies
bool copy_columns(const ColSrc& src, size_t ncols, size_t col_bytes, void* dst, hipMemcpyKind kind, hipStream_t st) {
    char* d = static_cast<char*>(dst);
    if (!src.ptrs) return hipMemcpyAsync(d, src.base, ncols * col_bytes, kind, st) == hipSuccess;
    for (size_t c = 0; c < ncols; c++)
        if (hipMemcpyAsync(d + c * col_bytes, src.ptrs[c], col_bytes, kind, st) != hipSuccess) return false;
    return true;
}

inline size_t hout(u32 field) { return field == GB_GOLDILOCKS ? 4 : 8; }
inline size_t level_offset(u64 N, u32 k) { return (size_t)(2 * N - ((2 * N) >> k)); }

struct EventList {  // events of one enqueue sequence, destroyed together (destruction is deferred until they have completed)
    std::vector<hipEvent_t> v;
    hipEvent_t make(bool& ok) {
        hipEvent_t e = nullptr;
        if (ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) v.push_back(e);
        else ok = false;
        return e;
    }
    ~EventList() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
};

// from_values of HOST input (2^12 rows and up): the upload runs in column chunks on the context's copy stream while the inverse NTT
// and LDE of the chunk before it run on the main stream.  values_dev (optional): a device buffer [ncols][n] that receives the input
// values in the field's device form, so that the caller gets them on the device without a second transfer (prove() needs the
// routed wires there for the permutation argument).
// What a segmented host-input commit can leave behind for a caller that may have to redo its LAST column segment (the prover's
// InvZeroPermArg retry re-draws one wire of the last column): the sponge state every leaf had after columns [0, start).
struct SegKeep {
    void* state = nullptr;   // pool block; the taker returns it with pool_free(ctx, state, bytes)
    size_t bytes = 0;
    u32 start = 0;           // first column of the last segment
};
// per-field host glue: transcript hash, Merkle launchers, and what commit() does differently per field (the transforms and the
// element-wise kernels are field-generic: kernels.hpp)
template <class F>
struct Host;
template <>
struct Host<GlF> {
    typedef poseidon_gl_host::Challenger Challenger;
    typedef gbk::GlNttTables Tables;
    typedef gbk::GlCosetTables Cosets;
    static void hash_no_pad(const u64* in, size_t n, u64* out) { poseidon_gl_host::hash_no_pad(in, n, out); }
    static void merkle_leaves(const u64* lde, u64 N, u32 width, u64* levels, hipStream_t st) {
        gbk::gl_merkle_leaves(lde, N, width, N, levels, st);
    }
    static void merkle_leaves_segment(const u64* lde, u64 N, u32 c_begin, u32 c_end, u64* state, bool last, u32 next_cols, u64* levels,
                                      hipStream_t st) {
        gbk::gl_merkle_leaves_segment(lde, N, c_begin, c_end, N, state, last, next_cols, levels, st);
    }
    static void merkle_level(const u64* in, u64* out, u64 num_out, hipStream_t st) { gbk::gl_merkle_level(in, out, num_out, st); }
    static void to_device_form(const u64* src, u64* dst, size_t count, hipStream_t st) {   // canonical words ARE the device form
        if (src != dst) (void)hipMemcpyAsync(dst, src, count * sizeof(u64), hipMemcpyDeviceToDevice, st);
    }
    static u64 p3_to_canonical(u64 x) { return x >= gl::P ? x - gl::P : x; }
    static bool intt_canonical(u64*, u64*, u64*, size_t, const Tables&, hipStream_t, size_t = 0) { return false; }   // device form IS canonical
    static void from_device_form(const u64* src, u64* dst, size_t count, hipStream_t st) { to_device_form(src, dst, count, st); }
    static constexpr bool device_form_is_canonical = true;
    // commit(): columns of the first upload chunk of a host batch (4, 4, 8, then 16 columns), fewest columns staged at all, and
    // whether its scratch is reserved up front ([host input or salts | transform scratch]) or grown to what each step needs
    static constexpr size_t first_chunk = 4, min_staged_cols = 1;
    static constexpr bool scratch_up_front = false;
};
template <>
struct Host<BbF> {
    typedef poseidon2_bb_host::Challenger Challenger;
    typedef gbk::BbNttTables Tables;
    typedef gbk::BbCosetTables Cosets;
    static void hash_no_pad(const u32* in, size_t n, u32* out) { poseidon2_bb_host::hash_no_pad(in, n, out); }
    static void merkle_leaves(const u32* lde, u64 N, u32 width, u32* levels, hipStream_t st) {
        gbk::bb_merkle_leaves(lde, N, width, N, levels, st);
    }
    static void merkle_leaves_segment(const u32* lde, u64 N, u32 c_begin, u32 c_end, u32* state, bool last, u32 next_cols, u32* levels,
                                      hipStream_t st) {
        gbk::bb_merkle_leaves_segment(lde, N, c_begin, c_end, N, state, last, next_cols, levels, st);
    }
    static void merkle_level(const u32* in, u32* out, u64 num_out, hipStream_t st) { gbk::bb_merkle_level(in, out, num_out, st); }
    static void to_device_form(const u32* src, u32* dst, size_t count, hipStream_t st) { gbk::bb_to_mont(src, dst, count, st); }
    static u32 p3_to_canonical(u32 x) { return bb::from_mont(x); }
    // values -> coefficients of columns held in CANONICAL form (what commit() leaves of a host witness beyond the routed wires);
    // the first mont_cols of them are left in device form in `src`.  false: the shape is not covered, nothing was launched
    static bool intt_canonical(u32* src, u32* dst, u32* scratch, size_t ncols, const Tables& t, hipStream_t st, size_t mont_cols = 0) {
        return gbk::bb_intt_columns_canonical(src, dst, scratch, ncols, mont_cols, t, st);
    }
    static void from_device_form(const u32* src, u32* dst, size_t count, hipStream_t st) { gbk::bb_from_mont(src, dst, count, st); }
    static constexpr bool device_form_is_canonical = false;
    // 4-byte words: the same bytes per upload chunk as Goldilocks' 4, 4, 8 (8, 8, 16, then 16 columns)
    static constexpr size_t first_chunk = 8, min_staged_cols = 4;
    static constexpr bool scratch_up_front = true;
};

// GB_INPUT_P3_REPR words (the field types' in-memory words: p3-goldilocks any u64 representative, p3-monty-31 Montgomery words; the
// reduction below p is the device form) -> canonical values, in place
template <class F>
void p3_to_canonical_dev(typename F::T* p, size_t count, hipStream_t st) {
    gbk::reduce_words<F>(p, count, st);
    Host<F>::from_device_form(p, p, count, st);
}

// Upload chunks of a host batch, in columns: c, c, 2c, then 16 (c = Host<F>::first_chunk).  The GPU's per-column work (transform +
// leaf hashing) is slower than PCIe delivers columns, so after a short ramp the upload is hidden - what is not hidden is the wait for
// the FIRST columns: with 4 + 4 the first 8-column hashing segment starts after ~1.5 ms of a 2^20-row Goldilocks witness (4 + 12: ~3.5 ms).
static inline size_t upload_chunk(size_t c0, size_t c) { return c0 < 2 * c ? c : c0 < 4 * c ? 2 * c : 16; }

template <class F>
gb_status commit(gb_ctx* ctx, ColSrc cols, size_t ncols, uint32_t log_n, uint32_t rate_bits, uint32_t cap_height, const void* salts,
                 uint32_t flags, bool is_coeffs, gb_batch** out, void* values_dev = nullptr, SegKeep* keep = nullptr,
                 size_t* values_mont_cols = nullptr) {
    // values_mont_cols (BabyBear, with values_dev): in - how many leading columns of values_dev the caller reads as device-form
    // VALUES afterwards; out - how many leading columns of values_dev ARE in device (Montgomery) form, the rest being canonical as
    // uploaded (the inverse transform takes canonical input where its radix-16 kernels cover the shape; otherwise all of them)
    typedef typename F::T T;
    typedef Host<F> HF;
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!out) return fail(ctx, GB_ERR_INVALID, "null out");
    *out = nullptr;
    if (ncols == 0) return fail(ctx, GB_ERR_INVALID, "from_values/from_coeffs needs at least one polynomial (oracle.rs:101)");
    if (!cols) return fail(ctx, GB_ERR_INVALID, "null cols");
    if (cols.ptrs)
        for (size_t c = 0; c < ncols; c++)
            if (!cols.ptrs[c]) return fail(ctx, GB_ERR_INVALID, "null column pointer");
    // GB_INPUT_P3_REPR: the elements are the in-memory words of the reference's field types (p3-goldilocks: any u64 representative;
    // p3-baby-bear / p3-monty-31: x 2^32 mod p) - a host-memory convention
    const bool p3 = (flags & GB_INPUT_P3_REPR) != 0;
    if (p3 && (flags & GB_INPUT_DEVICE)) return fail(ctx, GB_ERR_INVALID, "GB_INPUT_P3_REPR describes host memory; device inputs are canonical");
    if (log_n + rate_bits > F::TWO_ADICITY)
        return fail(ctx, GB_ERR_INVALID, "LDE size exceeds the field's two-adicity (32 Goldilocks / 27 BabyBear)");
    if (cap_height > log_n + rate_bits)
        return fail(ctx, GB_ERR_INVALID, "cap_height should be at most log2(leaves.len()) (merkle_tree.rs:154-157)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const size_t n = (size_t)1 << log_n, N = n << rate_bits;
    const u32 log_N = log_n + rate_bits;
    const u32 nsalt = salts ? GB_SALT_SIZE : 0;
    const size_t width = ncols + nsalt;
    const bool dev_in = (flags & GB_INPUT_DEVICE) != 0;

    gb_batch* b = new (std::nothrow) gb_batch();
    if (!b) return fail(ctx, GB_ERR_OOM, "host allocation failed");
    b->ctx = ctx; b->field = F::TAG; b->log_n = log_n; b->rate_bits = rate_bits; b->cap_height = cap_height;
    b->nsalt = nsalt; b->ncols = ncols;
    auto cleanup = [&](gb_status s) {
        gb_batch_free(b);
        return s;
    };

    void* p = nullptr;
    const size_t in_bytes = ncols * n * sizeof(T), salt_bytes = nsalt * N * sizeof(T);
    b->coeffs_bytes = in_bytes;
    b->lde_bytes = width * N * sizeof(T);
    b->levels_bytes = 2 * N * 4 * sizeof(u64);  // 32-byte digests for both hashers
    if (pool_alloc(ctx, b->coeffs_bytes, &p) != hipSuccess) return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc coeffs"));
    b->coeffs = (u64*)p;
    if (pool_alloc(ctx, b->lde_bytes, &p) != hipSuccess) return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc lde"));
    b->lde = (u64*)p;
    if (pool_alloc(ctx, b->levels_bytes, &p) != hipSuccess) return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc digests"));
    b->levels = (u64*)p;
    T* const coeffs = (T*)b->coeffs;
    T* const lde = (T*)b->lde;
    T* const lv = (T*)b->levels;

    gb_status s;
    hipStream_t st = ctx->stream;
    // separately allocated DEVICE columns: gathered into one block, then the contiguous path
    struct GatherGuard {
        gb_ctx* ctx; void* p = nullptr; size_t bytes = 0;
        ~GatherGuard() { if (p) pool_free(ctx, p, bytes); }   // stream-ordered reuse: every reader is enqueued before the next taker
    } gather{ctx};
    if (dev_in && cols.ptrs) {
        gather.bytes = in_bytes;
        if (pool_alloc(ctx, gather.bytes, &gather.p) != hipSuccess) { gather.p = nullptr; return cleanup(fail(ctx, GB_ERR_OOM, "hipMalloc column gather")); }
        if (!copy_columns(cols, ncols, n * sizeof(T), gather.p, hipMemcpyDeviceToDevice, st)) return cleanup(fail(ctx, GB_ERR_HIP, "copy of input columns failed"));
        cols = ColSrc(gather.p);
    }
    const bool pinned = !dev_in && all_pinned(cols, ncols, n * sizeof(T));
    // Host input of a big batch: the leaf sponges run in segments of SEG columns as the columns arrive (chunked upload below), so
    // that the hashing - most of a commitment's time - overlaps the PCIe transfer instead of waiting for its end; the sponge state
    // waits in `seg_state` between segments (kernels_merkle.hip / kernels_bb.hip: k_*_merkle_leaves).
    // Segment sizes: 8, 24, 32, then 64 columns, the last segment being what is left after the last multiple of eight (at most eight
    // columns more).  The first segment is short so that the hashing starts as soon as eight columns have been transformed (~1.5 ms of
    // a 2^20-row Goldilocks witness) instead of idling until more have crossed PCIe; from then on the GPU is behind the upload, and
    // segments are long because every one of them costs a kernel's ramp and tail (~0.3 ms at 2^23 leaves: T(k absorptions) = 0.3 +
    // 2.41 k ms, measured) and a round trip of the sponge state through HBM (0.27 GB); the last one is short because it is what an
    // InvZeroPermArg retry hashes again (gb_prove_retry).  135 columns: 8, 24, 32, 64, 7 (rounds 2-3: 8, 8, 16, 32, 32, 32, 7).
    constexpr u32 SEG = 32;
    auto seg_size = [ncols](u32 done) -> u32 {
        if (done < 8) return 8u;
        if (done < 32) return 24u;
        if (done < 64) return 32u;
        const u32 left = (u32)ncols - done;                 // leave the last (ragged or whole) group of eight to the last segment
        return std::max<u32>(8u, std::min<u32>(64u, left > 1 ? 8u * ((left - 1) / 8) : 8u));
    };
    const bool segmented = !dev_in && !is_coeffs && log_N >= 19 && ncols > SEG;
    const bool keep_split = keep && dev_in && !is_coeffs && log_N >= 19 && ncols > SEG;   // same split for device input, on request
    u32 seg_done = 0;
    void* seg_state = nullptr;
    // the parked sponge state: the capacity words, plus the rate words a ragged LAST absorption leaves alone when it is a segment
    // of its own (kernels_merkle.hip / kernels_bb.hip index the rows compactly)
    u32 last_seg_start = 0;
    for (u32 sz = seg_size(0); last_seg_start + sz < ncols; sz = seg_size(last_seg_start)) last_seg_start += sz;
    const u32 kf_final = std::min<u32>(8u, (u32)(width - last_seg_start));
    const size_t seg_rows = F::H + (8 - kf_final);
    const size_t seg_state_bytes = seg_rows * N * sizeof(T);
    struct SegGuard {
        gb_ctx* ctx; void** p; size_t bytes;
        ~SegGuard() { if (*p) pool_free(ctx, *p, bytes); }
    } seg_guard{ctx, &seg_state, seg_state_bytes};
    auto hash_ready_segments = [&](size_t cols_ready) -> bool {   // every full segment that is not the last one
        for (u32 sz = seg_size(seg_done); segmented && seg_done + sz < ncols && seg_done + sz <= cols_ready; sz = seg_size(seg_done)) {
            if (!seg_state && pool_alloc(ctx, seg_state_bytes, &seg_state) != hipSuccess) { seg_state = nullptr; return false; }
            Scope sm(ctx, "build Merkle tree");
            Scope sl(ctx, "hash leaves");
            HF::merkle_leaves_segment(lde, N, seg_done, seg_done + sz, (T*)seg_state, false, (u32)(width - (seg_done + sz)), lv, st);
            seg_done += sz;
        }
        return true;
    };
    const typename HF::Tables* tabs;
    const typename HF::Cosets* cos;
    if ((s = tables_for<F>(ctx, log_n, &tabs))) return cleanup(s);
    if ((s = cosets_for<F>(ctx, log_n, rate_bits, F::generator(), false, &cos))) return cleanup(s);
    // scratch (ctx->scratch): [host input or salts | transform scratch], scr_bytes each where the field reserves it up front; else one
    // block, grown to what each step needs
    const size_t scr_bytes = HF::scratch_up_front ? std::max(in_bytes, salt_bytes) : 0;
    if ((s = ensure(ctx, ctx->scratch, 2 * scr_bytes))) return cleanup(s);
    auto scratch = [&](size_t off, size_t bytes, T** at) -> gb_status {
        if (!HF::scratch_up_front)
            if (gb_status e = ensure(ctx, ctx->scratch, bytes)) return e;
        *at = (T*)((char*)ctx->scratch.p + off);
        return GB_OK;
    };
    T* ntt_scr = nullptr;

    const bool staged = !dev_in && !is_coeffs && log_n >= 12 && ncols >= HF::min_staged_cols;
    if (staged) {
        // column chunks: H2D into values_dev / the coefficient block on the copy stream, then (main stream, behind an event) device
        // form -> inverse NTT -> LDE of the chunk -> the leaf-sponge segments that have all their columns
        T* vals = values_dev ? static_cast<T*>(values_dev) : coeffs;  // without a taker the values are transformed in place
        if ((s = scratch(scr_bytes, 16 * n * sizeof(T), &ntt_scr))) return cleanup(s);
        EventList evs;
        bool ok = true;
        hipEvent_t e0 = evs.make(ok);                               // values_dev / coeffs may be a pool block still in use on `st`
        ok = ok && hipEventRecord(e0, st) == hipSuccess && hipStreamWaitEvent(ctx->copy_stream, e0, 0) == hipSuccess;
        for (size_t c0 = 0, cc = 0; c0 < ncols && ok; c0 += cc) {
            cc = std::min(upload_chunk(c0, HF::first_chunk), ncols - c0);
            hipEvent_t copied = evs.make(ok);
            ok = ok && upload_columns(ctx, cols, pinned, c0, cc, n * sizeof(T), vals + c0 * n) &&
                 hipEventRecord(copied, ctx->copy_stream) == hipSuccess && hipStreamWaitEvent(st, copied, 0) == hipSuccess;
            if (!ok) break;
            T* const v = vals + c0 * n;
            bool direct = false;   // coefficients already: the inverse transform took the canonical values as they are
            if (p3) {   // the host's words of the field types: nothing to convert, but nothing to trust either
                gbk::reduce_words<F>(v, cc * n, st);
            } else if (!HF::device_form_is_canonical) {
                const size_t want_mont = !values_dev ? 0 : values_mont_cols ? *values_mont_cols : ncols;
                { Scope sc(ctx, "IFFT"); direct = HF::intt_canonical(v, coeffs + c0 * n, ntt_scr, cc, *tabs, st, want_mont > c0 ? want_mont - c0 : 0); }
                if (!direct) HF::to_device_form(v, v, cc * n, st);
            }
            if (!direct) {
                { Scope sc(ctx, "IFFT"); gbk::intt_columns<F>(v, coeffs + c0 * n, ntt_scr, cc, *tabs, st); }
                if (values_mont_cols) *values_mont_cols = ncols;
            }
            { Scope sc(ctx, "FFT + blinding"); gbk::lde_columns<F>(coeffs + c0 * n, lde + c0 * N, cc, *tabs, *cos, st); }
            if (!hash_ready_segments(c0 + cc)) return cleanup(fail(ctx, GB_ERR_OOM, "sponge state"));
        }
        if (!ok) return cleanup(fail(ctx, GB_ERR_HIP, "chunked upload of the input columns failed"));
    } else {
        const T* src = static_cast<const T*>(cols.base);
        if (!dev_in) {   // host input in one copy: into the coefficient block where it is in device form already, else into scratch
            T* land = coeffs;
            if (!HF::device_form_is_canonical && (s = scratch(0, in_bytes, &land))) return cleanup(s);
            if (!copy_columns(cols, ncols, n * sizeof(T), land, hipMemcpyHostToDevice, st))
                return cleanup(fail(ctx, GB_ERR_HIP, "copy of input columns failed"));
            mark_upload(ctx);
            src = land;
        }
        bool direct = false;
        if (HF::device_form_is_canonical || (flags & GB_INPUT_DEVICE_FORM) || p3) {
            // in device form already (prover-internal; a host's p3 words once reduced).  The coefficient block gets its own copy, except
            // for device values where the device form is canonical: their inverse transform reads them in place
            if (src != coeffs && (is_coeffs || !HF::device_form_is_canonical)) {
                if (hipMemcpyAsync(coeffs, src, in_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return cleanup(fail(ctx, GB_ERR_HIP, "copy of input columns failed"));
                src = coeffs;
            }
            if (p3) gbk::reduce_words<F>(coeffs, ncols * n, st);   // a host's words (the library's own device form is in range)
        } else if (!is_coeffs && log_n >= 16 && log_n <= gbk::NTT_NATIVE_LOG) {
            // canonical values on the device (a resident witness, a small host batch): the inverse transform takes them as they are
            if ((s = scratch(scr_bytes, in_bytes, &ntt_scr))) return cleanup(s);
            Scope sc(ctx, "IFFT");
            (void)HF::intt_canonical(const_cast<T*>(src), coeffs, ntt_scr, ncols, *tabs, st);
            direct = true;
        } else {
            HF::to_device_form(src, coeffs, ncols * n, st);
            src = coeffs;
        }
        if (!is_coeffs && !direct) {
            if ((s = scratch(scr_bytes, in_bytes, &ntt_scr))) return cleanup(s);
            Scope sc(ctx, "IFFT");
            gbk::intt_columns<F>(src, coeffs, ntt_scr, ncols, *tabs, st);
        }
    }
    {
        Scope sc(ctx, "FFT + blinding");
        if (!staged) gbk::lde_columns<F>(coeffs, lde, ncols, *tabs, *cos, st);
        if (nsalt) {
            // salt columns arrive in LDE-point order (like lde_values' extra columns, oracle.rs:144-148)
            // and are stored, like everything else, in leaf order: leaf j <- point bitrev(j)
            const T* sdev = static_cast<const T*>(salts);
            if (!dev_in && !(flags & GB_SALTS_DEVICE)) {
                T* sh;
                if ((s = scratch(0, salt_bytes, &sh))) return cleanup(s);
                if (hipMemcpyAsync(sh, salts, salt_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
                    return cleanup(fail(ctx, GB_ERR_HIP, "copy of salts failed"));
                mark_upload(ctx);
                if (p3) p3_to_canonical_dev<F>(sh, (size_t)nsalt * N, st);   // the salt columns are F::rand_vec words too
                sdev = sh;
            }
            gbk::bitrev_copy<F>(sdev, lde + ncols * N, log_N, nsalt, st);
        }
    }
    {
        Scope sc(ctx, "build Merkle tree");
        {
            Scope sl(ctx, "hash leaves");
            if (!seg_done && keep_split) {   // device input whose last column segment may have to be redone: hash in two segments
                if (pool_alloc(ctx, seg_state_bytes, &seg_state) != hipSuccess) { seg_state = nullptr; return cleanup(fail(ctx, GB_ERR_OOM, "sponge state")); }
                HF::merkle_leaves_segment(lde, N, 0, last_seg_start, (T*)seg_state, false, (u32)(width - last_seg_start), lv, st);
                seg_done = last_seg_start;
            }
            if (seg_done) HF::merkle_leaves_segment(lde, N, seg_done, (u32)width, (T*)seg_state, true, 0, lv, st);
            else HF::merkle_leaves(lde, N, (u32)width, lv, st);
        }
        for (u32 k = 0; k < log_N - cap_height; k++)
            HF::merkle_level(lv + F::H * level_offset(N, k), lv + F::H * level_offset(N, k + 1), N >> (k + 1), st);
    }
    if (hipGetLastError() != hipSuccess) return cleanup(fail(ctx, GB_ERR_HIP, "kernel launch failed"));
    if (keep && seg_done && seg_state) { *keep = SegKeep{seg_state, seg_state_bytes, seg_done}; seg_state = nullptr; }
    *out = b;
    return GB_OK;
}

// ---- read-backs of a batch, canonical values; each one field-generic body behind the batch's field tag
template <class F>
gb_status read_coeffs(gb_batch* b, size_t col, void* out) {
    typedef typename F::T T;
    gb_ctx* ctx = b->ctx;
    const size_t n = (size_t)1 << b->log_n;
    const T* src = (const T*)b->coeffs + col * n;
    if (!Host<F>::device_form_is_canonical) {
        gb_status s = ensure(ctx, ctx->scratch, n * sizeof(T));
        if (s) return s;
        Host<F>::from_device_form(src, (T*)ctx->scratch.p, n, ctx->stream);
        src = (const T*)ctx->scratch.p;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out, src, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
}

template <class F>
gb_status read_row(gb_batch* b, u64 leaf, u32 width, void* out) {
    typedef typename F::T T;
    gb_ctx* ctx = b->ctx;
    const u64 N = (u64)1 << (b->log_n + b->rate_bits);
    gb_status s = ensure(ctx, ctx->small, 64 * 1024);
    if (s) return s;
    if (width * sizeof(u64) > ctx->small.bytes) return fail(ctx, GB_ERR_UNSUPPORTED, "row too wide");
    gbk::gather_row<F>((const T*)b->lde, N, width, leaf, (T*)ctx->small.p, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->small.p, width * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
}
gb_status read_row(gb_batch* b, u64 leaf, u32 width, void* out) {
    return b->field == GB_BABYBEAR ? read_row<BbF>(b, leaf, width, out) : read_row<GlF>(b, leaf, width, out);
}

template <class F>
gb_status read_leaves(gb_batch* b, void* out) {
    typedef typename F::T T;
    gb_ctx* ctx = b->ctx;
    const u64 N = (u64)1 << (b->log_n + b->rate_bits);
    const u32 width = (u32)(b->ncols + b->nsalt);
    const size_t bytes = (size_t)N * width * sizeof(T);
    gb_status s = ensure(ctx, ctx->scratch, bytes);
    if (s) return s;
    gbk::transpose_to_rows<F>((const T*)b->lde, N, width, N, (T*)ctx->scratch.p, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->scratch.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
}

}  // namespace

extern "C" {

gb_status gb_ctx_create(int device, gb_ctx** out) try {
    if (!out) return fail(nullptr, GB_ERR_INVALID, "null out");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) return fail(nullptr, GB_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= count) return fail(nullptr, GB_ERR_INVALID, "device index out of range");
    gb_ctx* ctx = new (std::nothrow) gb_ctx();
    if (!ctx) return fail(nullptr, GB_ERR_OOM, "host allocation failed");
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(nullptr, GB_ERR_HIP, "hipSetDevice/hipStreamCreate failed");
    }
    *out = ctx;
    return GB_OK;
} GB_CATCH(nullptr)

gb_status gb_ctx_destroy(gb_ctx* ctx) try {
    if (!ctx) return GB_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    gb_ctx_scope_reset(ctx);
    cache<GlF>(ctx).release();
    cache<BbF>(ctx).release();
    if (ctx->scratch.p) hipFree(ctx->scratch.p);
    if (ctx->small.p) hipFree(ctx->small.p);
    for (DeviceBuf& wb : ctx->big_work) if (wb.p) hipFree(wb.p);
    if (ctx->upload_mark) hipEventDestroy(ctx->upload_mark);
    for (auto& kv : ctx->pool) hipFree(kv.second);
    if (ctx->copy_stream) hipStreamSynchronize(ctx->copy_stream);
    delete ctx->stager;   // joins the copy threads, frees the page-locked ring
    for (int s = 0; s < 2; s++) {
        if (ctx->vstage_host[s]) (void)hipHostFree(ctx->vstage_host[s]);
        if (ctx->vstage_dev[s]) (void)hipFree(ctx->vstage_dev[s]);
        if (ctx->vstage_read[s]) (void)hipEventDestroy(ctx->vstage_read[s]);
    }
    if (ctx->vkeys.p) (void)hipFree(ctx->vkeys.p);
    if (ctx->vshape.p) (void)hipFree(ctx->vshape.p);
    if (ctx->xfer_up) (void)hipHostFree(ctx->xfer_up);
    if (ctx->xfer_down) (void)hipHostFree(ctx->xfer_down);
    hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    delete ctx;
    return GB_OK;
} GB_CATCH(nullptr)   // (the object may be gone: the message goes to the thread's own slot)

const char* gb_last_error(const gb_ctx* ctx) try {
    return ctx ? ctx->err.c_str() : g_null_ctx_error.c_str();
} catch (...) {
    return "";
}

gb_status gb_ctx_synchronize(gb_ctx* ctx) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_ctx_trim(gb_ctx* ctx) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    drop_all_retry_state(ctx);
    drop_all_check_state(ctx);
    for (auto& kv : ctx->pool) (void)hipFree(kv.second);
    ctx->pool.clear();
    for (DeviceBuf& wb : ctx->big_work) {   // the coset tables hold these fields' addresses; the next lookup grows them again
        if (wb.p) (void)hipFree(wb.p);
        wb.p = nullptr; wb.bytes = 0;
    }
    if (ctx->stager) {   // the page-locked staging ring and its copy threads come back with the next pageable input
        HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
        delete ctx->stager;
        ctx->stager = nullptr;
    }
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_ctx_stream(gb_ctx* ctx, void** stream_out) try {
    if (!ctx || !stream_out) return fail(ctx, GB_ERR_INVALID, "null argument");
    *stream_out = (void*)ctx->stream;
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_ctx_set_profiling(gb_ctx* ctx, int32_t on) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    ctx->profiling = on != 0;
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_ctx_scope_ms(gb_ctx* ctx, const char* scope, double* ms_out, uint64_t* count_out) try {
    if (!ctx || !scope || !ms_out) return fail(ctx, GB_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double total = 0;
    uint64_t cnt = 0;
    auto it = ctx->scopes.find(scope);
    if (it != ctx->scopes.end()) {
        for (auto& sp : it->second.spans) {
            float ms = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, sp.first, sp.second));
            total += ms;
            cnt++;
        }
    }
    *ms_out = total;
    if (count_out) *count_out = cnt;
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_ctx_scope_reset(gb_ctx* ctx) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->scopes)
        for (auto& sp : kv.second.spans) {
            hipEventDestroy(sp.first);
            hipEventDestroy(sp.second);
        }
    ctx->scopes.clear();
    return GB_OK;
} GB_CATCH(ctx)

static gb_status commit_entry(gb_ctx* ctx, uint32_t field, ColSrc cols, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                              uint32_t cap_height, const void* salts, uint32_t flags, bool is_coeffs, gb_batch** out) {
    if (ctx && (flags & ~GB_PUBLIC_INPUT_FLAGS)) {
        if (out) *out = nullptr;
        return fail(ctx, GB_ERR_INVALID, "unknown bits in flags");
    }
    gb_status s;
    if (field == GB_GOLDILOCKS) s = commit<GlF>(ctx, cols, ncols, log_n, rate_bits, cap_height, salts, flags, is_coeffs, out);
    else if (field == GB_BABYBEAR) s = commit<BbF>(ctx, cols, ncols, log_n, rate_bits, cap_height, salts, flags, is_coeffs, out);
    else if (!ctx || !out) s = fail(ctx, GB_ERR_INVALID, ctx ? "null out" : "null ctx");
    else { *out = nullptr; s = fail(ctx, GB_ERR_INVALID, "unknown field tag"); }
    if (!(flags & GB_INPUT_DEVICE)) s = finish_host_commit(ctx, s, out);   // `cols` / `salts` are the caller's again on return
    return s;
}

gb_status gb_commit_values(gb_ctx* ctx, uint32_t field, const void* cols, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                           uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out) try {
    return commit_entry(ctx, field, cols, ncols, log_n, rate_bits, cap_height, salts, flags, false, out);
} GB_CATCH(ctx)

gb_status gb_commit_coeffs(gb_ctx* ctx, uint32_t field, const void* cols, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                           uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out) try {
    return commit_entry(ctx, field, cols, ncols, log_n, rate_bits, cap_height, salts, flags, true, out);
} GB_CATCH(ctx)

// Vec<PolynomialValues<F>> / Vec<PolynomialCoeffs<F>> as the reference holds them: ncols separately allocated columns
gb_status gb_commit_values_cols(gb_ctx* ctx, uint32_t field, const void* const* cols, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out) try {
    return commit_entry(ctx, field, ColSrc::columns(cols), ncols, log_n, rate_bits, cap_height, salts, flags, false, out);
} GB_CATCH(ctx)

gb_status gb_commit_coeffs_cols(gb_ctx* ctx, uint32_t field, const void* const* cols, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                                uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out) try {
    return commit_entry(ctx, field, ColSrc::columns(cols), ncols, log_n, rate_bits, cap_height, salts, flags, true, out);
} GB_CATCH(ctx)

// ---- page-locked host memory for a host that builds its columns where the copy engine can read them
gb_status gb_host_alloc(gb_ctx* ctx, size_t bytes, void** out) try {
    if (!ctx || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!bytes) return fail(ctx, GB_ERR_INVALID, "zero-sized allocation");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GB_ERR_OOM, "hipHostMalloc failed (page-locked memory is limited by RLIMIT_MEMLOCK and physical memory)");
    }
    *out = p;
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_host_free(gb_ctx* ctx, void* p) try {
    if (!ctx) return fail(nullptr, GB_ERR_INVALID, "null ctx");
    if (!p) return GB_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostFree(p));
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_host_register(gb_ctx* ctx, void* p, size_t bytes) try {
    if (!ctx || !p || !bytes) return fail(ctx, GB_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GB_ERR_HIP, "hipHostRegister failed (already registered, or RLIMIT_MEMLOCK)");
    }
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_host_unregister(gb_ctx* ctx, void* p) try {
    if (!ctx || !p) return fail(ctx, GB_ERR_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));   // no upload of this context is still reading it
    if (hipHostUnregister(p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GB_ERR_INVALID, "hipHostUnregister failed (not a registered range)");
    }
    return GB_OK;
} GB_CATCH(ctx)

// Tuning and debugging switches (none changes a result), all of them per context.
gb_status gb_ctx_set_option(gb_ctx* ctx, const char* key, int64_t value) try {
    if (!ctx || !key) return fail(ctx, GB_ERR_INVALID, "null argument");
    const std::string k(key);
    if (k == "copy_threads") {
        if (value < -1 || value > 64) return fail(ctx, GB_ERR_INVALID, "copy_threads must be -1 (no staging ring), 0 (calling thread) .. 64");
        if (ctx->stager && (int)value != ctx->copy_threads) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
            delete ctx->stager;
            ctx->stager = nullptr;
        }
        ctx->copy_threads = (int)value;
    } else if (k == "retry_verify") {
        ctx->retry_verify = value != 0;
    } else if (k == "check_witness") {
        ctx->check_witness = value != 0;
    } else if (k == "verify_chunk_bytes") {
        if (value < 4096 || value > ((int64_t)1 << 30)) return fail(ctx, GB_ERR_INVALID, "verify_chunk_bytes must be 4096 .. 2^30");
        ctx->verify_chunk_bytes = (size_t)value;
    } else {
        return fail(ctx, GB_ERR_INVALID, "unknown option: " + k);
    }
    return GB_OK;
} GB_CATCH(ctx)

gb_status gb_batch_free(gb_batch* b) try {
    if (!b) return GB_OK;
    if (b->ctx) {
        pool_free(b->ctx, b->coeffs, b->coeffs_bytes);
        pool_free(b->ctx, b->lde, b->lde_bytes);
        pool_free(b->ctx, b->levels, b->levels_bytes);
    }
    delete b;
    return GB_OK;
} GB_CATCH(nullptr)   // (the object may be gone: the message goes to the thread's own slot)

gb_status gb_batch_info(const gb_batch* b, uint32_t* field, size_t* ncols, uint32_t* degree_log, uint32_t* rate_bits,
                        uint32_t* cap_height, uint32_t* blinding) try {
    if (!b) return fail(nullptr, GB_ERR_INVALID, "null batch");
    if (field) *field = b->field;
    if (ncols) *ncols = b->ncols;
    if (degree_log) *degree_log = b->log_n;
    if (rate_bits) *rate_bits = b->rate_bits;
    if (cap_height) *cap_height = b->cap_height;
    if (blinding) *blinding = b->nsalt ? 1 : 0;
    return GB_OK;
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_cap(gb_batch* b, void* out) try {
    if (!b || !out) return fail(b ? b->ctx : nullptr, GB_ERR_INVALID, "null argument");
    gb_ctx* ctx = b->ctx;
    const u64 N = (u64)1 << (b->log_n + b->rate_bits);
    const u64* cap = b->levels + 4 * level_offset(N, b->log_n + b->rate_bits - b->cap_height);  // 32 B per digest
    return read_back(ctx, out, cap, ((size_t)1 << b->cap_height) * 32);
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_coeffs(gb_batch* b, size_t col, void* out) try {
    if (!b || !out) return fail(b ? b->ctx : nullptr, GB_ERR_INVALID, "null argument");
    if (col >= b->ncols) return fail(b->ctx, GB_ERR_INVALID, "polynomial index out of range");
    if (!b->coeffs) return fail(b->ctx, GB_ERR_INVALID, "a stand-alone Merkle tree holds no polynomials");
    return b->field == GB_BABYBEAR ? read_coeffs<BbF>(b, col, out) : read_coeffs<GlF>(b, col, out);
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_lde_values(gb_batch* b, uint64_t index, uint64_t step, void* out) try {
    if (!b || !out) return fail(b ? b->ctx : nullptr, GB_ERR_INVALID, "null argument");
    const u32 bits = b->log_n + b->rate_bits;
    const u64 N = (u64)1 << bits;
    u64 i = index * step;
    if (i >= N) return fail(b->ctx, GB_ERR_INVALID, "index * step out of range (oracle.rs:154-156 would index out of bounds)");
    u64 leaf = 0;
    for (u32 k = 0; k < bits; k++) leaf |= ((i >> k) & 1ull) << (bits - 1 - k);
    return read_row(b, leaf, (u32)b->ncols, out);
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_leaf(gb_batch* b, uint64_t leaf_index, void* row, void* siblings, uint32_t* nsib) try {
    if (!b) return fail(nullptr, GB_ERR_INVALID, "null batch");
    gb_ctx* ctx = b->ctx;
    const u32 bits = b->log_n + b->rate_bits;
    if (leaf_index >> bits) return fail(ctx, GB_ERR_INVALID, "leaf_index out of range (merkle_tree.rs:191)");
    if (row) {
        gb_status s = read_row(b, leaf_index, (u32)(b->ncols + b->nsalt), row);
        if (s) return s;
    }
    const u32 layers = bits - b->cap_height;
    if (nsib) *nsib = layers;
    if (siblings && layers) {
        gb_status s = ensure(ctx, ctx->small, 64 * 1024);
        if (s) return s;
        gbk::gl_gather_siblings(b->levels, bits, b->cap_height, leaf_index, (u64*)ctx->small.p, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(siblings, ctx->small.p, (size_t)layers * 32, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GB_OK;
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_digests(gb_batch* b, void* out) try {
    if (!b || !out) return fail(b ? b->ctx : nullptr, GB_ERR_INVALID, "null argument");
    gb_ctx* ctx = b->ctx;
    const u32 bits = b->log_n + b->rate_bits;
    const u64 N = (u64)1 << bits;
    const size_t total = 2 * (N - ((u64)1 << b->cap_height));
    if (!total) return GB_OK;
    const size_t bytes = total * 32;
    gb_status s = ensure(ctx, ctx->scratch, bytes);
    if (s) return s;
    gbk::gl_digests_to_reference_layout(b->levels, (u64*)ctx->scratch.p, bits, b->cap_height, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->scratch.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_leaves(gb_batch* b, void* out) try {
    if (!b || !out) return fail(b ? b->ctx : nullptr, GB_ERR_INVALID, "null argument");
    return b->field == GB_BABYBEAR ? read_leaves<BbF>(b, out) : read_leaves<GlF>(b, out);
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_batch_device_ptrs(gb_batch* b, void** coeffs, void** lde, void** digest_levels) try {
    if (!b) return fail(nullptr, GB_ERR_INVALID, "null batch");
    if (coeffs) *coeffs = b->coeffs;
    if (lde) *lde = b->lde;
    if (digest_levels) *digest_levels = b->levels;
    return GB_OK;
} GB_CATCH(b ? b->ctx : nullptr)

gb_status gb_permute(gb_ctx* ctx, uint32_t field, const void* in, void* out, uint64_t count) try {
    if (!ctx || !in || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (!count) return GB_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (field == GB_BABYBEAR) {
        const size_t bytes = count * 16 * sizeof(u32);
        gb_status s = ensure(ctx, ctx->scratch, 2 * bytes);
        if (s) return s;
        u32* din = (u32*)ctx->scratch.p;
        u32* dout = din + count * 16;
        HIP_TRY(ctx, hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, ctx->stream));
        gbk::bb_poseidon2_permute(din, dout, count, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return GB_OK;
    }
    const size_t bytes = count * 12 * sizeof(u64);
    gb_status s = ensure(ctx, ctx->scratch, 2 * bytes);
    if (s) return s;
    u64* din = (u64*)ctx->scratch.p;
    u64* dout = din + count * 12;
    HIP_TRY(ctx, hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    gbk::gl_poseidon_permute(din, dout, count, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GB_OK;
} GB_CATCH(ctx)

}  // extern "C"

// elements first_element .. first_element + count - 1 of the stream (seed, nonce) (random_stream.hpp), generated on the device
template <class F>
static gb_status random_elements_entry(gb_ctx* ctx, const gbk::rnd::Key& key, uint64_t first, uint64_t count, uint32_t flags, void* out) {
    typedef typename F::T T;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    T* dst = static_cast<T*>(out);
    const size_t bytes = count * sizeof(T);
    if (!(flags & GB_INPUT_DEVICE)) {
        if (gb_status s = ensure(ctx, ctx->scratch, bytes)) return s;
        dst = static_cast<T*>(ctx->scratch.p);
    }
    if (!gbk::random_elements<F>(key, first, count, 1, dst, 0, ctx->stream)) return fail(ctx, GB_ERR_HIP, "launch of k_random_elements failed");
    if (!(flags & GB_INPUT_DEVICE)) {
        HIP_TRY(ctx, hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return GB_OK;
}

gb_status gb_random_elements(gb_ctx* ctx, uint32_t field, const uint8_t* seed, const uint32_t* nonce, uint64_t first_element,
                             uint64_t count, uint32_t flags, void* out) try {
    if (!ctx || !seed || !nonce || !out) return fail(ctx, GB_ERR_INVALID, "null argument");
    if (field != GB_GOLDILOCKS && field != GB_BABYBEAR) return fail(ctx, GB_ERR_INVALID, "unknown field tag");
    if (flags & ~(uint32_t)GB_INPUT_DEVICE) return fail(ctx, GB_ERR_INVALID, "gb_random_elements: flags other than GB_INPUT_DEVICE");
    if (!gbk::rnd::range_ok(first_element, count))
        return fail(ctx, GB_ERR_INVALID, "gb_random_elements: the range ends past element 2^34 (the block counter has 32 bits)");
    if ((flags & GB_INPUT_DEVICE) && (reinterpret_cast<uintptr_t>(out) & 15))
        return fail(ctx, GB_ERR_INVALID, "gb_random_elements: the device destination is not 16-byte aligned");
    if (!count) return GB_OK;
    const gbk::rnd::Key key = gbk::rnd::make_key(seed, nonce);
    return field == GB_GOLDILOCKS ? random_elements_entry<GlF>(ctx, key, first_element, count, flags, out)
                                  : random_elements_entry<BbF>(ctx, key, first_element, count, flags, out);
} GB_CATCH(ctx)

#include "poly_host.inc"
#include "prover_host.inc"
#include "wiring_host.inc"
#include "verifier_host.inc"
#include "compress_host.inc"
#include "verify_batch_host.inc"
#include "constraint_host.inc"

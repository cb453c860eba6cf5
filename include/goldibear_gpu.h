/* goldibear_gpu.h - C ABI of libgoldibear_gpu.so, the MI355X (gfx950) implementation of the
 * plonky2_goldibear commitment hot path.
 *
 * The reference has no FFI: the seam is the Rust struct `PolynomialBatch` with public fields
 * (plonky2/src/fri/oracle.rs:29-40), built by `from_values` / `from_coeffs` (:68-123) and read by
 * the prover.  Each entry point below names the reference item it replaces.  INTEGRATION.md shows
 * the Rust `extern "C"` block and the `GpuPolynomialBatch` newtype that binds them.
 *
 * Conventions
 *  - every function returns a gb_status (0 = ok) and never unwinds; gb_last_error() gives text;
 *    GB_ERR_INVALID is returned where the reference would assert!/panic! on a shape violation
 *    (oracle.rs:139, merkle_tree.rs:154-157, fft.rs:174-180);
 *  - one gb_ctx per HIP device; calls on one ctx are serialised by the caller (the reference
 *    prover is single-threaded above Rayon, plonk/prover.rs:228-447); contexts are independent,
 *    which is how independent proofs shard one-per-GPU;
 *  - field elements are canonical little-endian u64 (Goldilocks) / u32 (BabyBear);
 *  - matrices are COLUMN-MAJOR [ncols][n]: the layout of Vec<PolynomialValues<F>>
 *    (iop/witness.rs:277-284) with the per-column Vecs laid end to end; the *_cols entry points take the columns where the
 *    reference has them - ncols separately allocated arrays (`const void* const* cols`, cols[i] = n elements), pageable or
 *    page-locked, no flattening copy on the host side;
 *  - gb_batch is an opaque device-resident handle; nothing large is copied back unless asked;
 *  - host input buffers (`cols`, `salts`, `witness`, `constants_sigmas`, ...) belong to the caller again as soon as the call
 *    returns (the reference moves its Vecs in): gb_commit_* wait for their uploads - not for the kernels behind them - before
 *    returning, gb_prove / gb_circuit_create end on a synchronised read-back.  Device inputs (GB_INPUT_DEVICE) are read by
 *    kernels enqueued on the context's stream and must stay valid until gb_ctx_synchronize or any read-back on that context.
 */
#ifndef GOLDIBEAR_GPU_H
#define GOLDIBEAR_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gb_ctx gb_ctx;
typedef struct gb_batch gb_batch;

typedef int32_t gb_status;
enum {
    GB_OK = 0,
    GB_ERR_INVALID = 1,     /* shape / argument violation (reference: assert!/panic!) */
    GB_ERR_HIP = 2,         /* a HIP runtime call failed */
    GB_ERR_OOM = 3,         /* device allocation failed */
    GB_ERR_UNSUPPORTED = 4  /* valid in the reference, not implemented here (e.g. log_n > 24, the lookup gates) */
};

enum { GB_GOLDILOCKS = 0, GB_BABYBEAR = 1 }; /* field tag: F = Goldilocks (Poseidon-12) | BabyBear (Poseidon2-16) */

/* `flags` of the entry points that take field-element matrices; any other bit is GB_ERR_INVALID */
enum {
    GB_INPUT_HOST = 0,   /* `cols` / `salts` / `witness` are host pointers (the drop-in case) */
    GB_INPUT_DEVICE = 1, /* they are device pointers on ctx's device (chained calls, benchmarks) */
    /* host inputs only: the elements are the reference's field types AS THEY LIE IN MEMORY (Cargo.toml:17-24 - p3-goldilocks:
     * any u64 representative of the value, not necessarily below p; p3-baby-bear / p3-monty-31: the Montgomery word
     * x * 2^32 mod p), so a Vec<F> is handed over without an as_canonical_*() pass.  Without it elements are canonical.
     * Applies to `cols` / `witness` / `salts`; results (proof bytes, accessors) are canonical either way. */
    GB_INPUT_P3_REPR = 2,
    /* gb_prove_salted*, gb_prove_partition, gb_prove_inputs only: `salts` is a HOST pointer to 32 seed bytes, whatever memory space
     * the witness is in, and the library generates the salt columns on the device (see gb_prove_salted, gb_random_elements) */
    GB_SALTS_FROM_SEED = 4
};

#define GB_SALT_SIZE 4 /* fri/oracle.rs:25 */
#define GB_SEED_SIZE 32
/* nonce[0] of the streams the library itself draws from a seed (gb_random_elements); callers' own streams use other values */
#define GB_STREAM_SALTS 1    /* (1, s, j): salt column j of commitment s (0 wires, 1 Zs / partial products, 2 quotient) */
#define GB_STREAM_BLINDING 2 /* (2, 0, 0): the values of a circuit's blinding rows, in the order the builder created their targets */

/* ---- context ------------------------------------------------------------------------------- */
/* One context = one HIP stream (+ a copy stream) and one proving thread.  Several contexts of one process prove concurrently -
 * the way to use the GPU with recursion-sized circuits, which cannot fill it alone.  They overlap only as far as the HIP runtime
 * gives their streams hardware queues of their own: it creates GPU_MAX_HW_QUEUES of them (environment, read when the runtime
 * initialises; 4 by default), so a host that keeps more than four contexts busy exports GPU_MAX_HW_QUEUES=8 before its first
 * HIP call (six 2^12-row proofs in flight: 576 proofs/s on 4 queues, 831 on 8).  The library never changes the environment. */
gb_status gb_ctx_create(int device, gb_ctx** out);
gb_status gb_ctx_destroy(gb_ctx* ctx);
const char* gb_last_error(const gb_ctx* ctx); /* valid until the next call on ctx; ctx may be NULL */
gb_status gb_ctx_synchronize(gb_ctx* ctx);
/* Freed batches keep their device blocks in a per-context pool for reuse by later commits of the
 * same shape (the reference allocates fresh Vecs per PolynomialBatch); this returns them to HIP - together with what failed
 * attempts keep for gb_prove_retry, what the first gb_check_witness prepared on each circuit (the next check builds it again),
 * the work buffers of transforms above 2^22 rows and the page-locked staging ring of pageable
 * inputs (four slots of max(64 MiB, one column): 256 MiB of host memory up to 2^23 Goldilocks rows, 512 MiB at 2^24; its copy
 * threads). */
gb_status gb_ctx_trim(gb_ctx* ctx);
/* hipStream_t all work of this ctx is enqueued on (for callers that record their own events) */
gb_status gb_ctx_stream(gb_ctx* ctx, void** stream_out);
/* Tuning and debugging switches of THIS context; none changes a result.  Unknown key / value out of range: GB_ERR_INVALID.
 *   "copy_threads"   threads of the context that stage PAGEABLE host columns into the library's page-locked ring (below):
 *                    default 4; 0 = the calling thread copies; -1 = no ring, hipMemcpyAsync straight from pageable memory
 *   "retry_verify"   1: gb_prove_retry first compares the caller's whole matrix with the copy the failed attempt kept and
 *                    returns GB_ERR_INVALID if they differ in more than witness[wire][row] (one read-back of the witness)
 *   "check_witness"  1: every gb_prove* that does the full computation checks its witness first (gb_check_witness, below) and
 *                    returns GB_ERR_UNSATISFIED instead of proof bytes that cannot verify; default 0: gb_prove* runs nothing new
 *   "verify_chunk_bytes"  gb_verify_batch: the most bytes (query rounds and per-proof records) staged and uploaded per chunk,
 *                    4096 .. 2^30; default 8388608 (8 MiB; two page-locked slots of this size).  A chunk holds at least one proof */
gb_status gb_ctx_set_option(gb_ctx* ctx, const char* key, int64_t value);

/* ---- host memory ---------------------------------------------------------------------------
 * The reference's inputs are pageable Vecs (MatrixWitness.wire_values: Vec<Vec<F>>, iop/witness.rs:277-279;
 * Vec<PolynomialValues<F>>, fri/oracle.rs:68-75).  Every host input may be pageable: big batches are staged through a
 * page-locked ring the context owns (four slots of max(64 MiB, one column), allocated at the first such call and grown when a
 * longer column arrives) by its copy threads, column by column, while
 * the columns before are transformed and hashed.  A host that can place its columns itself skips that copy: memory from
 * gb_host_alloc (hipHostMalloc) or registered with gb_host_register (hipHostRegister; unregister before freeing it) is read by
 * the copy engine directly - e.g. an allocator for the witness columns.  Registration costs about as much as one copy: it pays
 * for buffers that are reused. */
gb_status gb_host_alloc(gb_ctx* ctx, size_t bytes, void** out);
gb_status gb_host_free(gb_ctx* ctx, void* p);
gb_status gb_host_register(gb_ctx* ctx, void* p, size_t bytes);
gb_status gb_host_unregister(gb_ctx* ctx, void* p);

/* ---- timing: the reference's timed!() scopes (util/proving_process_info.rs:196-212) ---------
 * With profiling on, each commit records HIP events on ctx's stream around the scopes
 * "IFFT", "FFT + blinding", "build Merkle tree" (fri/oracle.rs:76-114; "transpose LDEs" does not
 * exist here); gb_prove adds the scopes of prove() ("compute wires commitment", ..., "fri query rounds") and two of the library's
 * own for the transforms that belong to no commitment: "quotient IFFT" (the per-coset inverse transforms of compute_quotient_polys'
 * coset_ifft) and "FRI LDE" (the layers' coset_fft, fri/prover.rs:122-125).  gb_ctx_scope_ms returns the accumulated milliseconds of
 * a scope since the last reset (*count_out: how many times it was entered) and synchronises the stream. */
gb_status gb_ctx_set_profiling(gb_ctx* ctx, int32_t on);
gb_status gb_ctx_scope_ms(gb_ctx* ctx, const char* scope, double* ms_out, uint64_t* count_out);
gb_status gb_ctx_scope_reset(gb_ctx* ctx);

/* ---- PolynomialBatch ------------------------------------------------------------------------ */
/* PolynomialBatch::from_values (fri/oracle.rs:68-90): `cols` holds ncols columns of n = 2^log_n
 * evaluations on the subgroup H_n.  Computes the coefficients, the rate-2^rate_bits LDE on the
 * coset 7*H_N, and the Merkle tree with 2^cap_height cap entries.  `salts`: NULL (blinding =
 * false) or GB_SALT_SIZE columns of N = n << rate_bits elements - the F::rand_vec columns of
 * oracle.rs:144-148, supplied by the host so that results are reproducible.
 * Errors: cap_height > log_n + rate_bits -> GB_ERR_INVALID (merkle_tree.rs:154-157). */
gb_status gb_commit_values(gb_ctx* ctx, uint32_t field, const void* cols, size_t ncols, uint32_t log_n,
                           uint32_t rate_bits, uint32_t cap_height, const void* salts, uint32_t flags,
                           gb_batch** out);
/* PolynomialBatch::from_coeffs (fri/oracle.rs:93-123): same, input already coefficients. */
gb_status gb_commit_coeffs(gb_ctx* ctx, uint32_t field, const void* cols, size_t ncols, uint32_t log_n,
                           uint32_t rate_bits, uint32_t cap_height, const void* salts, uint32_t flags,
                           gb_batch** out);
/* The same two constructors over the reference's own layout: cols[i] points to column i (n elements), each column its own
 * allocation - `values: Vec<PolynomialValues<F>>` / `polynomials: Vec<PolynomialCoeffs<F>>` (fri/oracle.rs:68-75, :93-100)
 * with cols[i] = values[i].values.as_ptr().  Host columns may be pageable (staged by the library, see "host memory") or
 * page-locked; with GB_INPUT_DEVICE they are device pointers.  `salts` stays one block of GB_SALT_SIZE columns. */
gb_status gb_commit_values_cols(gb_ctx* ctx, uint32_t field, const void* const* cols, size_t ncols, uint32_t log_n,
                                uint32_t rate_bits, uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out);
gb_status gb_commit_coeffs_cols(gb_ctx* ctx, uint32_t field, const void* const* cols, size_t ncols, uint32_t log_n,
                                uint32_t rate_bits, uint32_t cap_height, const void* salts, uint32_t flags, gb_batch** out);
gb_status gb_batch_free(gb_batch* b);

/* shape queries: .polynomials.len(), .degree_log, .rate_bits, .blinding (oracle.rs:35-39) */
gb_status gb_batch_info(const gb_batch* b, uint32_t* field, size_t* ncols, uint32_t* degree_log,
                        uint32_t* rate_bits, uint32_t* cap_height, uint32_t* blinding);

/* .merkle_tree.cap (hash/merkle_tree.rs:60-61): out[2^cap_height][H], H = 4 (GL) / 8 (BB) */
gb_status gb_batch_cap(gb_batch* b, void* out);
/* .polynomials[col].coeffs (oracle.rs:35): out[n] */
gb_status gb_batch_coeffs(gb_batch* b, size_t col, void* out);
/* get_lde_values(index, step) (oracle.rs:153-158): out[ncols] (salt columns dropped) */
gb_status gb_batch_lde_values(gb_batch* b, uint64_t index, uint64_t step, void* out);
/* MerkleTree::get(leaf_index) + MerkleTree::prove(leaf_index) (merkle_tree.rs:183-222):
 * row[ncols + salt], siblings[(log_n + rate_bits - cap_height)][H], *nsib = that count */
gb_status gb_batch_leaf(gb_batch* b, uint64_t leaf_index, void* row, void* siblings, uint32_t* nsib);
/* .merkle_tree.digests in the reference's interleaved layout (merkle_tree.rs:50-58):
 * out[2 * (N - 2^cap_height)][H].  Parity/debug aid; the device keeps level-major digests. */
gb_status gb_batch_digests(gb_batch* b, void* out);
/* .merkle_tree.leaves: out[N][ncols + salt] row-major (oracle.rs:108-109 order). Debug aid. */
gb_status gb_batch_leaves(gb_batch* b, void* out);
/* every polynomial of the batch evaluated at one extension-field point: what OpeningSet::new's eval_commitment
 * (plonk/proof.rs:359-363) computes with `p.to_extension().eval(z)`.  z: [D] canonical elements (D = 2 Goldilocks,
 * 4 BabyBear), out: [ncols][D] canonical. */
gb_status gb_batch_eval_ext(gb_batch* b, const void* z, void* out);
/* device pointers for zero-copy chaining: coeffs [ncols][n], lde [ncols+salt][N] in leaf order */
gb_status gb_batch_device_ptrs(gb_batch* b, void** coeffs, void** lde, void** digest_levels);

/* ---- circuit + prove() ------------------------------------------------------------------------
 * gb_circuit holds what CircuitBuilder::build() leaves in ProverOnlyCircuitData / CommonCircuitData
 * for the prover (plonk/circuit_builder.rs:1214-1312): the constants||sigmas commitment (committed
 * here, :1230-1239), the sigma values, k_is, and circuit_digest (:1300-1312, empty domain separator).
 * gb_circuit_create takes the gate set of the reference's dummy circuit: gates sorted by
 * (degree, id) = [NoopGate, ConstantGate{num_constants}, PublicInputGate<H>], one selector column
 * (gates/selectors.rs:142-159), evaluated inside the quotient kernel.  gb_circuit_create_gates (below) takes any gate set
 * over the eighteen built-in gate kinds GB_GATE_* with any selector grouping - every gate DefaultGateSerializer knows except
 * LookupGate / LookupTableGate, which are GB_ERR_UNSUPPORTED - and evaluates it on the GPU as well; gb_circuit_create_programs
 * adds gates of the caller's own as constraint programs (GB_GATE_PROGRAM).
 * Both of the reference's configurations are served (plonk/config.rs:119-150): GB_GOLDILOCKS = D 2, H 4,
 * Poseidon-12, 8-byte elements; GB_BABYBEAR = D 4 (x^4 - 11), H 8, Poseidon2-16, 4-byte elements.
 * Configuration range of the prover: degree_bits from 2 up to the field's two-adicity less rate_bits (32 / 27: the reference has no
 * other cap, plonk/prover.rs:228-447; 2^21 and 2^22 rows run the library's own transform passes, larger ones an outer radix step
 * around them, and what does not fit the device is GB_ERR_OOM - a 2^23-row Goldilocks proof holds ~170 GB of commitments);
 * max_quotient_degree_factor 2, 4, 8 or 16 for either field, with ceil(num_routed_wires / factor) <= 32 partial-product chunks
 * (MAX_CHUNKS); rate_bits from
 * log2 of that factor up to 8 - above it the quotient is computed on every 2^(rate_bits - log2 factor)-th point of the LDE, as
 * plonk/prover.rs:735-749 does (the reference's size-optimised recursion proofs use rate_bits 7 and 8,
 * recursion/recursive_verifier.rs:573-611); num_challenges 1 .. 16 (BabyBear from 4: circuit_builder.rs:1190-1192 demands
 * (31 - degree_bits) * c >= 100 - CircuitConfig.security_bits is fixed at the 100 of every configuration the reference defines,
 * plonk/circuit_data.rs:102-159, and is not a field of gb_circuit_config - and a count that fails that assert is GB_ERR_INVALID for
 * either field); FRI arity_bits 1 .. 8;
 * num_constants <= 4.  The quotient and gate kernels keep their per-challenge sums in registers and are compiled for 1 .. 4
 * challenges (Goldilocks) and 4 .. 10 (BabyBear) - the stock configurations; other counts run as slices of those widths. */
typedef struct gb_circuit gb_circuit;
typedef struct gb_circuit_config {
    uint32_t field;                 /* GB_GOLDILOCKS | GB_BABYBEAR */
    uint32_t degree_bits;
    uint32_t num_wires, num_routed_wires, num_constants; /* CircuitConfig (plonk/circuit_data.rs:63-93) */
    uint32_t num_challenges, max_quotient_degree_factor;
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds; /* FriConfig (fri/mod.rs:25-45) */
    uint32_t arity_bits, final_poly_bits;  /* FriReductionStrategy::ConstantArityBits.  A circuit whose strategy is Fixed(..) or
                                              MinSize(..) passes arity_bits = 0 (or any pair ConstantArityBits would panic on,
                                              fri/reduction_strategies.rs:45) and hands its list over after the create call
                                              (gb_circuit_set_fri_reduction_arity_bits); until then gb_prove* / gb_prove_openings /
                                              gb_verify* / gb_proof_* on the object answer GB_ERR_INVALID */
    uint32_t num_selectors;         /* 1 */
    uint32_t gate_constant, gate_pi;/* selector values of ConstantGate / PublicInputGate (NoopGate is the third) */
    uint32_t zero_knowledge;        /* CircuitConfig.zero_knowledge (= FriParams.hiding): the wires / Zs / quotient leaves carry
                                       SALT_SIZE salt elements (fri/oracle.rs:133-148): gb_prove_salted, gb_verify */
    uint32_t num_public_inputs;     /* CommonCircuitData.num_public_inputs (plonk/circuit_data.rs:590): gb_prove takes exactly
                                       this many; gb_verify / gb_verify_compressed / gb_proof_decompress reject a proof carrying
                                       any other count with GB_ERR_INVALID, as validate_proof_with_pis_shape does
                                       (plonk/validate_shape.rs:22-25) - hash_no_pad does not pad, so [a,b,c] and [a,b,c,0]
                                       have the same public-inputs hash and only this check tells them apart */
} gb_circuit_config;

/* constants_sigmas: [num_selectors + num_constants + num_routed_wires][2^degree_bits] VALUES on H_n
 * (selector, constants, sigma columns - circuit_builder.rs:1198-1229); k_is: [num_routed_wires].  Canonical words, or with
 * GB_INPUT_P3_REPR (host input) the field types' in-memory words - constants_sigmas and k_is alike. */
gb_status gb_circuit_create(gb_ctx* ctx, const gb_circuit_config* cfg, const void* constants_sigmas, const void* k_is,
                            uint32_t flags, gb_circuit** out);
/* the same with constants_sigmas as build() holds it (circuit_builder.rs:1198-1229: a Vec<PolynomialValues<F>>, one allocation per
 * column): constants_sigmas_cols[i] points to the 2^degree_bits canonical values of column i */
gb_status gb_circuit_create_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const void* const* constants_sigmas_cols, const void* k_is,
                                 uint32_t flags, gb_circuit** out);
gb_status gb_circuit_free(gb_circuit* c);
/* The same for a general gate set: `gates` is CommonCircuitData.gates - sorted by (degree, id) as
 * circuit_builder.rs:1194-1196 leaves them - with selectors_info flattened into each entry (gates/selectors.rs:16-26:
 * selector_indices[i], groups[selector_indices[i]]); entry i is the gate whose selector value is i.  The constraint evaluators
 * (csrc/gates.hpp) cover NoopGate, ConstantGate{param = num_consts} (gates/constant.rs), PublicInputGate<H>
 * (gates/public_input.rs), ArithmeticGate{param = num_ops} (gates/arithmetic_base.rs) and the in-circuit hash of the field's
 * configuration - PoseidonGate for Goldilocks (gates/poseidon_goldilocks.rs), Poseidon2BabyBearGate{param = num_ops} for
 * BabyBear (gates/poseidon2_babybear.rs) - which build() needs for any circuit with public inputs (circuit_builder.rs:1126-1137);
 * and the remaining gates of the recursion circuits listed below; any other kind (LookupGate, LookupTableGate) is
 * GB_ERR_UNSUPPORTED.  cfg->num_selectors = selectors_info.groups.len(),
 * cfg->num_constants = the constant columns after the selectors (max over the gates' num_constants()); cfg->gate_constant and
 * cfg->gate_pi are ignored.  constants_sigmas: [num_selectors + num_constants + num_routed_wires][2^degree_bits]. */
#define GB_GATE_NOOP 0
#define GB_GATE_CONSTANT 1
#define GB_GATE_PUBLIC_INPUT 2
#define GB_GATE_ARITHMETIC 3
#define GB_GATE_POSEIDON 4
#define GB_GATE_POSEIDON2_BABYBEAR 5
/* the rest of the recursion circuits' gate set (the gates of the reference's RECURSIVE_VERIFIER_GL fixture and
 * ExponentiationGate); D = the extension degree of the field's configuration */
#define GB_GATE_ARITHMETIC_EXTENSION 6 /* gates/arithmetic_extension.rs   param = num_ops */
#define GB_GATE_MUL_EXTENSION 7        /* gates/multiplication_extension.rs param = num_ops */
#define GB_GATE_BASE_SUM 8             /* gates/base_sum.rs               param = num_limbs, param2 = B (0 reads as 2) */
#define GB_GATE_REDUCING 9             /* gates/reducing.rs               param = num_coeffs */
#define GB_GATE_REDUCING_EXTENSION 10  /* gates/reducing_extension.rs     param = num_coeffs */
#define GB_GATE_RANDOM_ACCESS 11       /* gates/random_access.rs          param = bits, param2 = num_copies, param3 = num_extra_constants */
#define GB_GATE_POSEIDON_MDS 12        /* gates/poseidon_goldilocks_mds.rs (Goldilocks) */
#define GB_GATE_COSET_INTERPOLATION 13 /* gates/coset_interpolation.rs    param = subgroup_bits (<= 4), param2 = degree; the
                                          barycentric weights are x_i / 2^subgroup_bits and are not passed */
#define GB_GATE_EXPONENTIATION 14      /* gates/exponentiation.rs         param = num_power_bits */
#define GB_GATE_ADD_MANY 15            /* gates/add_many.rs               param = num_addends, param2 = num_ops */
#define GB_GATE_APPLY_MAT4 16          /* gates/apply_mat4.rs             param = num_ops */
#define GB_GATE_POSEIDON2_INTERNAL_PERMUTATION 17 /* gates/poseidon2_internal_permutation.rs (BabyBear) */
/* Any other gate, as data: a constraint program - the gate's eval_unfiltered (gates/gate.rs:53-272) as a straight-line program
 * of add / sub / mul over the row's wires and constants.  param = the index of the gate's program in the table handed to
 * gb_circuit_create_programs / gb_verifier_create_programs; the create functions without a table answer GB_ERR_INVALID. */
#define GB_GATE_PROGRAM 18
typedef struct gb_gate {
    uint32_t kind;            /* GB_GATE_* */
    uint32_t param;           /* ConstantGate num_consts / ArithmeticGate, Poseidon2BabyBearGate num_ops; see above; 0 otherwise */
    uint32_t selector_index;  /* which selector column carries this gate */
    uint32_t group_start, group_end; /* the gate indices sharing that column */
    uint32_t param2, param3;  /* see the gate list above; 0 otherwise */
} gb_gate;
gb_status gb_circuit_create_gates(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                  const void* constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out);
gb_status gb_circuit_create_gates_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                       const void* const* constants_sigmas_cols, const void* k_is, uint32_t flags, gb_circuit** out);
/* ---- constraint programs (GB_GATE_PROGRAM) ----
 * The programs of a circuit cross the ABI as one flat array of 64-bit words, program i being
 * program_words[program_offsets[i] .. program_offsets[i + 1]); program_offsets has num_programs + 1 ascending entries, the first 0.
 * One program:
 *   word 0   num_wires | num_constants << 32      wire columns 0 .. num_wires-1 and constants 0 .. num_constants-1 may be read
 *   word 1   num_constraints | degree << 32       Gate::num_constraints() / Gate::degree()
 *   word 2   num_regs | num_literals << 32
 *   word 3   num_instrs                           (the high half is zero)
 *   then num_literals canonical field elements, one per word (converted once at create to the device form),
 *   then num_instrs instruction words:
 *     bits 0-1    op: 0 ADD, 1 SUB, 2 MUL (reg[dst] = a OP b), 3 EMIT (the next constraint is a; dst and b are zero)
 *     bits 2-7    dst register
 *     bits 8-31   operand a: bits 8-9 its space (0 register, 1 wire column, 2 constant column after the selectors, 3 literal),
 *                 bits 10-31 its index
 *     bits 32-55  operand b, the same way
 *     bits 56-63  zero
 * EMIT yields the constraints in the order of eval_unfiltered.  At the verifier's zeta the same instructions run on extension
 * elements; a product of D-tuples of wires in F[x]/(x^D - W) is spelled out in base operations with W as a literal.
 * Limits: GB_MAX_PROGRAMS per circuit; per program GB_MAX_PROGRAM_INSTRS instructions, GB_MAX_PROGRAM_REGS registers,
 * GB_MAX_PROGRAM_LITERALS literals, GB_MAX_PROGRAM_CONSTRAINTS constraints.
 * GB_ERR_INVALID at create, the message naming the program and the instruction: a header over the limits or a length that does
 * not match it; a register read before it is written; a register, wire, constant or literal index out of range; a literal >= p;
 * a count of EMITs other than num_constraints; a gb_gate.param >= num_programs; a constraint whose degree bound (literal 0,
 * wire and constant 1, ADD / SUB the maximum, MUL the sum) exceeds `degree`; degree plus the degree of the gate's filter
 * (gates/gate.rs:391-404: one factor per other gate of its selector group, one more with several selector columns) above
 * max_quotient_degree_factor + 1 - the bound gates/selectors.rs:125-209 keeps for every gate it groups.
 * With num_programs = 0 (program_words and program_offsets may be NULL) the functions are the ones without a table.  The
 * prover evaluates program gates in a launch of their own (k_gate_programs, an interpreter with its registers in LDS); a circuit
 * without them runs exactly the kernels it ran before.  Measured cost: the interpreted gates take 5.6x
 * (Goldilocks) / 7.4x (BabyBear) the kernel time of the same gates compiled, 1.7x / 1.9x over the quotient stage at 2^14 rows. */
#define GB_MAX_PROGRAMS 16
#define GB_MAX_PROGRAM_INSTRS 4096
#define GB_MAX_PROGRAM_REGS 32
#define GB_MAX_PROGRAM_LITERALS 256
#define GB_MAX_PROGRAM_CONSTRAINTS 1024
gb_status gb_circuit_create_programs(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                     const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                     const void* constants_sigmas, const void* k_is, uint32_t flags, gb_circuit** out);
gb_status gb_circuit_create_programs_cols(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                          const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                          const void* const* constants_sigmas_cols, const void* k_is, uint32_t flags,
                                          gb_circuit** out);
/* ProverOnlyCircuitData.constants_sigmas_commitment (plonk/circuit_data.rs:532-534), the PolynomialBatch built by
 * gb_circuit_create*: a BORROWED handle - owned by the circuit, valid until gb_circuit_free, never passed to gb_batch_free.  The
 * reference's prover reads it for the opening set (plonk/proof.rs:359-377) and the query rounds. */
gb_status gb_circuit_constants_sigmas_commitment(gb_circuit* c, gb_batch** out);
/* VerifierOnlyCircuitData: constants_sigmas_cap [2^cap_height][H] and circuit_digest [H], field elements */
gb_status gb_circuit_verifier_data(gb_circuit* c, void* cap_out, void* digest_out);
/* FriParams.reduction_arity_bits (fri/mod.rs, filled by FriConfig::fri_params from FriReductionStrategy::reduction_arity_bits,
 * fri/reduction_strategies.rs:29-56).  gb_circuit_create* / gb_verifier_create derive the list of the stock strategy
 * ConstantArityBits(cfg.arity_bits, cfg.final_poly_bits); a circuit configured with Fixed(..) or MinSize(..) hands the list its
 * CommonCircuitData holds over with the setter before the first proof (prover, verifier and proof compression all read it).
 * Rejected with GB_ERR_INVALID: more than GB_MAX_FRI_LAYERS layers, an arity_bits outside [1, 8], arities that sum past degree_bits, or a layer whose tree would be lower than cap_height
 * (MerkleTree::new's assert, hash/merkle_tree.rs:154-157).  The getter writes at most GB_MAX_FRI_LAYERS entries. */
#define GB_MAX_FRI_LAYERS 32
gb_status gb_circuit_set_fri_reduction_arity_bits(gb_circuit* c, const uint32_t* arity_bits, uint32_t num_layers);
gb_status gb_circuit_fri_reduction_arity_bits(gb_circuit* c, uint32_t* arity_bits_out, uint32_t* num_layers_out);
/* prove_with_partition_witness -> internal_prove_with_partition_witness (plonk/prover.rs:160-447):
 * witness = MatrixWitness.wire_values [num_wires][n] (iop/witness.rs:277-284), already generated.
 * Writes ProofWithPublicInputs bytes (util/serialization/mod.rs:2134-2151) to proof_out; *proof_len
 * is the size needed.  The PoW witness is the MINIMUM valid nonce (the reference's find_any with one
 * thread).  GB_ERR_PERM_ARG_ZERO mirrors ProverError::InvZeroPermArg (prover.rs:512-514): the caller
 * re-randomises the random wire and retries, as prover.rs:186-226 does (in a 31-bit field about one
 * 2^20-row proof in five needs it).  public_inputs are canonical values as u64 for either field; elements of
 * `witness` and of the proof are 8 (Goldilocks) / 4 (BabyBear) bytes (hash/hash_types.rs:39-41, :73-75). */
#define GB_ERR_PERM_ARG_ZERO 16
#define GB_ERR_OPENING_IN_SUBGROUP 17
#define GB_ERR_BUFFER_TOO_SMALL 18
gb_status gb_prove(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs,
                   size_t num_public_inputs, void* proof_out, size_t proof_cap, size_t* proof_len);
/* The retry of prove_with_partition_witness (plonk/prover.rs:183-226).  When gb_prove returns GB_ERR_PERM_ARG_ZERO the reference
 * overwrites ONE wire - prover_data.random_wire (circuit_builder.rs:1073-1075: the last wire of the PublicInputGate row) - with a
 * fresh F::rand() and proves again.  gb_prove_retry(witness, wire, row) is that second call: `witness` is the matrix of the failed
 * gb_prove on this circuit with wire_values[wire][row] re-drawn and nothing else changed.  It returns exactly what
 * gb_prove(witness) returns - same bytes, same errors (another GB_ERR_PERM_ARG_ZERO included: call it again) - but where the failed
 * attempt has left its wires commitment behind (host or device witness, >= 2^19 leaves, more than 32 wires, `wire` among the columns of the
 * last leaf-sponge segment - true for the random wire of every stock configuration) only that wire's column is transformed again
 * and only the last absorption of every leaf sponge and the tree above are re-hashed: ~5 ms instead of ~40 at 2^20 BabyBear rows,
 * where one proof in five needs it.  Anything else - no failed attempt before it, another gb_prove* in between, a device attempt
 * retried with a host matrix, a zero-knowledge circuit - is simply the full computation.  The state of a failed attempt (the wires
 * commitment, the device copy of a host witness, the leaf sponges' state: ~12 GB at 2^20 Goldilocks rows) is held until the next
 * gb_prove* / gb_circuit_free on the circuit, gb_circuit_drop_retry, gb_ctx_trim - or until an allocation on the context would
 * otherwise fail.  A host retry trusts the kept device copy for every element but witness[wire][row]: a caller that changed anything
 * else must call gb_prove.  (gb_ctx_set_option(ctx, "retry_verify", 1) makes the library compare the whole matrix with the kept
 * copy first - a debugging aid, one read-back of the witness - and return GB_ERR_INVALID when they differ elsewhere.) */
gb_status gb_prove_retry(gb_circuit* c, const void* witness, uint32_t flags, uint32_t wire, uint64_t row, const uint64_t* public_inputs,
                         size_t num_public_inputs, void* proof_out, size_t proof_cap, size_t* proof_len);
/* gb_prove / gb_prove_retry / gb_prove_salted over MatrixWitness.wire_values as the reference holds it (iop/witness.rs:277-279:
 * Vec<Vec<F>>): wire_cols[w] points to the n = 2^degree_bits values of wire w, every column its own (pageable or page-locked)
 * allocation - wire_cols[w] = witness.wire_values[w].as_ptr(), no flattening copy.  Same results, same errors. */
gb_status gb_prove_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const uint64_t* public_inputs,
                        size_t num_public_inputs, void* proof_out, size_t proof_cap, size_t* proof_len);
gb_status gb_prove_retry_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, uint32_t wire, uint64_t row,
                              const uint64_t* public_inputs, size_t num_public_inputs, void* proof_out, size_t proof_cap,
                              size_t* proof_len);
/* Release what a failed attempt left behind without proving again - a caller that gives up after GB_ERR_PERM_ARG_ZERO
 * (ProverError::TooManyPermArgFailures, prover.rs:221-225).  No-op when nothing is held. */
gb_status gb_circuit_drop_retry(gb_circuit* c);
/* The same for a circuit built with cfg.zero_knowledge (prover.rs:267,334,382: `blinding` = true for the wires, Zs / partial
 * products and quotient commitments).  salts: [3][GB_SALT_SIZE][N = 2^(degree_bits + rate_bits)] canonical elements in
 * LDE-point order - the columns the reference draws with F::rand_vec (fri/oracle.rs:144-148) - for those three commitments,
 * in the same memory space as `witness` (flags); a host input for the same reason the PublicInputGate's random wires are
 * (determinism contract: same inputs, same proof bytes).
 *
 * With GB_SALTS_FROM_SEED in `flags` the randomness is a function of a seed instead: `salts` is a HOST pointer to GB_SEED_SIZE
 * bytes, whatever memory space the witness is in, and salt element [s][j][t] is element t of the stream (seed, (GB_STREAM_SALTS,
 * s, j)) of gb_random_elements - s the commitment (0 wires, 1 Zs / partial products, 2 quotient), j the salt column, t the
 * LDE-point index: the [3][GB_SALT_SIZE][N] layout above, and the proof bytes are those of the same call with that matrix.  The
 * library generates the four columns of a commitment on the device just before the commitment consumes them, into one block of
 * GB_SALT_SIZE * N elements that the three commitments share (256 MiB at 2^20 Goldilocks rows and rate 3, against the 768 MiB a
 * salt matrix occupies on the host and again on the device); nothing crosses the bus.  The contract: ONE SEED PER PROOF.  The
 * library draws no entropy of its own - the seed is the caller's, from the operating system's generator; a seed used for two
 * different witnesses gives both proofs the same salts and voids the hiding of both.  The flag on a circuit that is not
 * zero-knowledge is the error salts on such a circuit are; the flag with salts = NULL (the entry points without a salts argument
 * included) is GB_ERR_INVALID; without the flag nothing changes.  It is accepted by gb_prove_salted, gb_prove_salted_cols,
 * gb_prove_partition and gb_prove_inputs.  gb_commit_* take no seed: a caller composes gb_random_elements(.., GB_INPUT_DEVICE, buf)
 * with their device `salts` argument.
 *
 * Salting alone is not zero-knowledge: the circuit needs the blinding rows of CircuitBuilder::blind (circuit_builder.rs:879-980)
 * too - openings at zeta and g zeta and the FRI queries otherwise still leak the witness polynomials.  Those rows are the
 * builder's business and part of `witness`; the Python builder mirror adds them under a zero-knowledge config and fills them from
 * the stream (seed, (GB_STREAM_BLINDING, 0, 0)). */
gb_status gb_prove_salted(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs,
                          size_t num_public_inputs, const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len);
gb_status gb_prove_salted_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const uint64_t* public_inputs,
                               size_t num_public_inputs, const void* salts, void* proof_out, size_t proof_cap, size_t* proof_len);

/* ---- prove() from the partition witness --------------------------------------------------------------------------------------
 * prove_with_partition_witness (plonk/prover.rs:160-183) does not hold MatrixWitness.wire_values when it is called: it holds a
 * PartitionWitness (iop/witness.rs:318-372) - one value per copy class in `values` - and ProverOnlyCircuitData.representative_map
 * (plonk/circuit_data.rs:454), and its first timed step, "compute full witness", is partition_witness.full_witness()
 * (iop/witness.rs:359-371): a single-threaded loop over degree x num_wires targets, each a dependent read through the map.  The
 * functions below take those two objects as they are and build the matrix on the device, so that one value per CLASS crosses to
 * the device, not one per wire.
 *
 * gb_circuit_set_partition, once after gb_circuit_create*: representative_map[num_targets] is the reference's Vec<usize>, indexed
 * by Target::index (iop/target.rs:55-60): wire (row, column) -> row * num_wires + column, virtual target i -> degree * num_wires
 * + i; public_input_targets holds the indices of prover_data.public_inputs.  GB_ERR_INVALID: num_targets < degree * num_wires, a
 * map entry or a public-input target >= num_targets, num_public_inputs != cfg.num_public_inputs; GB_ERR_UNSUPPORTED:
 * num_targets >= 2^32.  The library keeps the representatives that wire cells actually use ("slots", ranked in ascending target
 * index) on the host and a 32-bit slot per wire cell on the device; a representative no wire cell uses - most virtual targets -
 * gets no slot.  Calling it again replaces the map. */
gb_status gb_circuit_set_partition(gb_circuit* c, const uint64_t* representative_map, uint64_t num_targets,
                                   const uint64_t* public_input_targets, size_t num_public_inputs);
/* gb_prove / gb_prove_salted from the partition witness: values[num_targets], entry i = partition_witness.values[i]
 * .unwrap_or(ZERO), canonical words or with GB_INPUT_P3_REPR the field types' in-memory words.  A HOST pointer:
 * GB_INPUT_DEVICE is GB_ERR_INVALID.  salts: NULL unless the circuit is zero-knowledge, otherwise as for gb_prove_salted (host) -
 * the [3][GB_SALT_SIZE][N] matrix or, with GB_SALTS_FROM_SEED in `flags`, the GB_SEED_SIZE seed bytes.
 * The public inputs are read from `values` through the map (get_targets, prover.rs:177).  Result, errors and proof bytes are those
 * of gb_prove / gb_prove_salted on the matrix full_witness() would build - GB_ERR_PERM_ARG_ZERO included; a value >= p in an
 * entry that a wire cell or a public input reads is GB_ERR_INVALID ("non-canonical witness element"), entries nothing reads are
 * not looked at.  Before gb_circuit_set_partition: GB_ERR_INVALID.  Timing scope: "compute full witness", the reference's name,
 * around compaction, upload and expansion (its parts: "partition compaction", "partition upload", "partition expansion"). */
gb_status gb_prove_partition(gb_circuit* c, const void* values, uint32_t flags, const void* salts, void* proof_out, size_t proof_cap,
                             size_t* proof_len);
/* The second or third attempt of prover.rs:186-226 after GB_ERR_PERM_ARG_ZERO: the caller has re-drawn
 * values[representative_map[row * num_wires + wire]] - prover_data.random_wire - and changed nothing else.  Same bytes and errors
 * as gb_prove_partition(values).  Where the failed attempt left its state behind (see gb_prove_retry) and that cell is alone in
 * its class, as the random wire is, the value goes into the device matrix the failed attempt kept, that one column is transformed
 * again and the last absorption of the leaf sponges and the tree are re-hashed; anything else is the full computation.
 * A witness that violates a copy constraint - the gb_prove tests' "broken copy class" - cannot be expressed here: every cell of a
 * class reads the same entry of `values`. */
gb_status gb_prove_partition_retry(gb_circuit* c, const void* values, uint32_t flags, uint32_t wire, uint64_t row, void* proof_out,
                                   size_t proof_cap, size_t* proof_len);
/* full_witness() on its own, for a host that keeps the prover loop: writes the canonical [num_wires][n] matrix to witness_dev_out,
 * a DEVICE buffer of the caller (16-byte aligned), on the context's stream - ready as the GB_INPUT_DEVICE input of
 * gb_commit_values and gb_zs_partial_products on the same context.  `values` is the caller's again on return. */
gb_status gb_expand_partition(gb_circuit* c, const void* values, uint32_t flags, void* witness_dev_out);

/* ---- prove() from the inputs alone: the witness generators on the device ------------------------------------------------------
 * prove() is two calls (plonk/prover.rs:136-158): generate_partial_witness, timed as "run N generators" (iop/generator.rs:25-106),
 * and prove_with_partition_witness.  gb_prove_partition starts at the second and needs a host that has run every generator and
 * hands over one word per target.  The functions below start at the first: the host hands over the generators ONCE per circuit,
 * as records, and per proof only the values it alone knows - the PartialWitness and the random values (host inputs under the
 * determinism contract) - and the generated values never leave the device.
 *
 * A record names one generator of prover_only.generators:
 *   gate generators (GB_GEN_ARITHMETIC .. GB_GEN_POSEIDON2_INTERNAL, one kind per SimpleGenerator of the built-in gates): `gate`
 *     is the index in the gate table given to gb_circuit_create_gates, `a` the row, `b` the operation (ArithmeticGate,
 *     ArithmeticExtensionGate, MulExtensionGate, AddManyGate, ApplyMat4Gate, Poseidon2BabyBearGate), the copy (RandomAccessGate)
 *     or the constant index (GB_GEN_CONSTANT: ConstantGenerator of a ConstantGate wire or of a RandomAccessGate extra constant),
 *     0 for the gates with one generator per row;
 *   GB_GEN_COPY (CopyGenerator, iop/generator.rs): `a` is the source target, `b` the destination target, `gate` is not read.
 * The host lists the generators explicitly: CircuitBuilder::build drops those of the unused operations of partly filled gates
 * (circuit_builder.rs:1252-1270), so they cannot be derived from the gate table.
 *
 * The generators of the gadgets name arbitrary targets and take several records: a HEAD record - `kind` one of
 * GB_GEN_EQUALITY .. GB_GEN_BASE_SUM, `gate` the generator's parameter (0 where it has none; NOT a gate index), `a` the number
 * of targets that follow, `b` 0 - and then ceil(a / 2) CONTINUATION records of kind GB_GEN_TARGETS whose `a` and `b` are the
 * next two targets (Target::index) in order, `gate` 0, the unused `b` of an odd count 0:
 *   kind                       gate        targets, in order                                      reference
 *   GB_GEN_EQUALITY            0           x, y, equal, inv                                       gadgets/arithmetic.rs:425-452
 *   GB_GEN_NONZERO_TEST        0           to_test, dummy                                         iop/generator.rs:400-428
 *   GB_GEN_QUOTIENT_OR_ZERO    0           numerator, denominator, quotient                       gadgets/arithmetic.rs:487-511
 *   GB_GEN_QUOTIENT_EXTENSION  0           numerator[D], denominator[D], quotient[D]              gadgets/arithmetic_extension.rs:507-532
 *   GB_GEN_SPLIT               0           integer, bits[0..64]                                   gadgets/split_join.rs:67-97
 *   GB_GEN_WIRE_SPLIT          num_limbs   integer, then the WIRE_SUM target of each gate         gadgets/split_join.rs:118-161
 *   GB_GEN_LOW_HIGH            n_log       integer, low, high                                     gadgets/range_check.rs:89-115
 *   GB_GEN_BASE_SUM            base B      the sum target, then limbs[1..]                        gadgets/split_base.rs:84-116
 * GB_GEN_WIRE_SPLIT takes the sum targets, row * num_wires + BaseSumGate::WIRE_SUM (= 0), not the rows.  Each runs its
 * run_once: Equality sets inv = (x - y)^-1 or 0 and equal = 0 / 1; NonzeroTest sets dummy = 1 for zero, else the inverse;
 * QuotientOrZero's quotient is 0 for a zero denominator; WireSplit gives each sum integer & (2^num_limbs - 1) and shifts, and with
 * num_limbs >= 64 gives the first sum the whole value and the others 0; LowHigh with n_log = 0 gives low = 0, high = integer;
 * BaseSum folds acc * B + limb from the last limb down, in field arithmetic.  A record index in an error message is the head's
 * index in the array as passed, continuation records counted.
 *
 * GENERATOR PROGRAMS: a generator of the user's own - the generators() of a program gate (GB_GATE_PROGRAM), or a SimpleGenerator
 * handed to CircuitBuilder::add_simple_generator (examples/square_root.rs) - as data, the counterpart of the constraint
 * programs above and in their word layout.  A program reads num_in dependency values and the constants of one row, and produces
 * num_out outputs in order:
 *   word 0   num_in | num_constants << 32          word 1   num_out (high half zero)
 *   word 2   num_regs | num_literals << 32         word 3   num_instrs (high half zero)
 *   then num_literals canonical words, then num_instrs instruction words.
 * An instruction word is a constraint program's: destination register in bits 2-7, operand a in bits 8-31, operand b in bits
 * 32-55, an operand its space in the low two bits and its index in the 22 above; the spaces are 0 register, 1 DEPENDENCY i (where
 * a constraint program has wire columns), 2 constant column i after the selectors, read at the record's row, 3 literal i.  The
 * opcode is (w & 3) | ((w >> 56) & 0xF) << 2 - bits 56-63 are zero in a constraint program, so no word is valid in both formats
 * with two meanings - and bits 60-63 are zero:
 *   0 ADD  1 SUB  2 MUL   reg[dst] = a op b, as in a constraint program
 *   3 OUT                 the next output is a (EMIT's twin); dst and b zero
 *   4 INV                 reg[dst] = 1 / a; a = 0 is the error "Tried to invert zero"
 *   5 INV_OR_ZERO         reg[dst] = a.try_inverse().unwrap_or(ZERO)
 *   6 IS_ZERO             reg[dst] = 1 if a = 0, else 0
 *   7 SQRT                reg[dst] = a square root of a; SQRT(0) = 0; a non-residue is an error (sqrt(x).unwrap() on None)
 *   16 IDIV               reg[dst] = floor(a / b) of the canonical representatives; b = 0 is the error "attempt to divide by zero"
 *   17 IREM               reg[dst] = a mod b of the canonical representatives; b = 0 is the same error
 *   18 SHR                reg[dst] = floor(a / 2^b); 0 when b >= 64 (the amount is a value like any other, not an immediate)
 *   19 AND                reg[dst] = a & b, bitwise on the canonical representatives
 *   20 LT                 reg[dst] = 1 if a < b as integers, else 0
 * The integer operations 16-20 read both operands as integers in [0, p); every result is <= a or is 0 or 1, a field element as
 * it stands.  With them a generator reads a target as an integer: u32 multiply-add with a carry, a borrow, a comparison,
 * range-check limbs, div_rem.  OR and XOR can leave [0, p) and are no operations.  8 .. 15 and 21 .. 63 are no opcodes.
 * The unary operations 4-7 have b zero.  With IS_ZERO and INV_OR_ZERO the generators that branch (Equality, NonzeroTest) are
 * written branch-free.  SQRT is Tonelli-Shanks step for step as examples/square_root.rs:185-219 writes it, with
 * z = two_adic_generator(TWO_ADICITY) (the example passes F::bits(), which exceeds the two-adicity).  Nothing in the reference
 * pins which of the two roots comes out: it is the one this algorithm yields.
 * Limits: GB_MAX_GENERATOR_PROGRAMS per circuit; per program GB_MAX_PROGRAM_INSTRS, GB_MAX_PROGRAM_REGS, GB_MAX_PROGRAM_LITERALS
 * as for constraint programs, and num_in + num_out <= GB_MAX_GENERATOR_PROGRAM_TARGETS.
 * A program generator's record is a gadget-style head of kind GB_GEN_PROGRAM: `gate` is the program's index, `a` the number of
 * targets (= num_in + num_out) and `b` the row whose constants the program reads (0 for a program without constants), followed
 * by ceil(a / 2) GB_GEN_TARGETS records: the num_in dependencies, then the num_out outputs.  Wire targets make it a program gate's
 * generator, virtual targets a gadget's.  It is scheduled like every other generator (levels, one storing writer per class,
 * comparing writers, unrunnable generators).
 *
 * Not built, GB_ERR_UNSUPPORTED: any other kind (17 .. 31 and 41 .. 47 are reserved), a gate generator's record that names a
 * program gate (a program gate's generators are GB_GEN_PROGRAM records), the lookup pair, the Poseidon2-Risc0 gate and
 * DummyProofGenerator; a circuit that has them stays on gb_prove_partition. */
#define GB_GEN_ARITHMETIC 0
#define GB_GEN_ARITHMETIC_EXTENSION 1
#define GB_GEN_MUL_EXTENSION 2
#define GB_GEN_CONSTANT 3
#define GB_GEN_BASE_SPLIT 4
#define GB_GEN_REDUCING 5
#define GB_GEN_REDUCING_EXTENSION 6
#define GB_GEN_RANDOM_ACCESS 7
#define GB_GEN_POSEIDON_MDS 8
#define GB_GEN_COSET_INTERPOLATION 9
#define GB_GEN_EXPONENTIATION 10
#define GB_GEN_POSEIDON 11
#define GB_GEN_POSEIDON2_BABYBEAR 12
#define GB_GEN_ADD_MANY 13
#define GB_GEN_APPLY_MAT4 14
#define GB_GEN_POSEIDON2_INTERNAL 15
#define GB_GEN_COPY 16
#define GB_GEN_EQUALITY 32
#define GB_GEN_NONZERO_TEST 33
#define GB_GEN_QUOTIENT_OR_ZERO 34
#define GB_GEN_QUOTIENT_EXTENSION 35
#define GB_GEN_SPLIT 36
#define GB_GEN_WIRE_SPLIT 37
#define GB_GEN_LOW_HIGH 38
#define GB_GEN_BASE_SUM 39
#define GB_GEN_TARGETS 40
#define GB_GEN_PROGRAM 48
#define GB_MAX_GENERATOR_PROGRAMS 256
#define GB_MAX_GENERATOR_PROGRAM_TARGETS 1024
typedef struct gb_generator {
    uint32_t kind;            /* GB_GEN_* */
    uint32_t gate;            /* a gate generator's gate index; a gadget head's parameter; a program head's program index */
    uint64_t a;
    uint64_t b;
} gb_generator;
/* After gb_circuit_set_partition (before it: GB_ERR_INVALID): generators = gb_generator[num_generators]; input_targets
 * [num_inputs] = the target indices (Target::index, as in the representative map) whose values the host supplies per proof - every
 * target of the PartialWitness and of a RandomValueGenerator; constants = the circuit's constants columns again (no read-back from
 * the device): [cfg.num_constants][degree] canonical 64-bit words for either field; flags = 0.  The library schedules the
 * generators once: a dense index over the copy classes that a wire cell, an input, a public input or a generator touches (the
 * slots of gb_circuit_set_partition first, in their order, then the classes only virtual targets use, ascending); levels
 * (inputs are level 0, a generator runs one level after the last of its dependencies is stored); for every class ONE storing
 * writer - the first in (level, record) order - while every later writer and every writer of an input class compares instead
 * (witness.rs:340-350 "set twice with different values"); a run of levels that each fit one workgroup is one kernel launch.
 * A generator with a dependency that nothing ever sets cannot run: it is left out and counted (the reference panics with
 * "{n} generators weren't run"), its outputs stay zero.  GB_ERR_INVALID: a target >= num_targets, a gate index out of range or
 * of another kind than the record's, a row, operation or constant index outside the gate's parameters, an input target listed
 * twice, unknown flags; and of the gadget records, each with the record's index: a GB_GEN_TARGETS record with no head in front of
 * it, a head whose continuation runs past the end of the array or meets another kind, a count that does not fit the kind (4, 2,
 * 3, 3 D; 1..65; >= 2; 3; >= 2), num_limbs = 0, n_log > 63, a base < 2 (`gate` is 32 bits wide: a base >= 2^32 cannot be
 * written), non-zero `gate` where no parameter is defined, non-zero `b` in a head, non-zero `gate` or padding in a continuation.
 * Of a GB_GEN_PROGRAM head, with the record's index: no programs set, a program index out of range, a != num_in + num_out, a row
 * >= degree, non-zero b for a program without constants, and the continuation errors above.
 * Nothing is read past num_generators records.  Calling it again replaces the schedule; gb_circuit_set_partition drops it. */
gb_status gb_circuit_set_generators(gb_circuit* c, const void* generators, uint64_t num_generators, const uint64_t* input_targets,
                                    uint64_t num_inputs, const uint64_t* constants, uint32_t flags);
/* The generator programs of the circuit (above), in the table layout of gb_circuit_create_programs: program_words holds the
 * programs one after another, program_offsets[num_programs + 1] their first words (program_offsets[0] = 0).  After
 * gb_circuit_set_partition and before gb_circuit_set_generators, whose GB_GEN_PROGRAM records name the programs by index.  Every
 * program is checked and copied; the tables go to device memory.  Calling it again replaces the programs and drops a schedule
 * built on the old ones; num_programs = 0 clears them; gb_circuit_set_partition drops them with the schedule.  GB_ERR_INVALID,
 * naming the program and the instruction: a header over the limits or with bits above num_out / num_instrs, a length that does
 * not match the header, more constants than the circuit has, a register read before it is written, a register, dependency,
 * constant or literal index out of range - in either operand of the binary operations 0-2 and 16-20 - a literal >= p, a count of
 * OUT other than num_out, an unknown opcode (8 .. 15, 21 .. 63), non-zero bits 60-63, a non-zero b or (for OUT) dst in OUT or a
 * unary operation 4-7.  Nothing is read past program_offsets[num_programs] words. */
gb_status gb_circuit_set_generator_programs(gb_circuit* c, const uint64_t* program_words, const uint32_t* program_offsets,
                                            uint32_t num_programs);
/* what the schedule looks like; any out pointer may be NULL */
gb_status gb_circuit_generators_info(gb_circuit* c, uint32_t* num_levels, uint32_t* num_launches, uint32_t* num_unrunnable,
                                     uint32_t* num_checks, uint32_t* num_classes);
/* class_targets_out[num_classes]: the representative target of each class of the schedule, for a host that reads
 * gb_generate_partition's values */
gb_status gb_circuit_generator_classes(gb_circuit* c, uint64_t* class_targets_out, uint64_t capacity);
/* The stage alone, for a host that keeps the prover loop: input_values[num_inputs] in the order of input_targets (host pointer;
 * canonical words of the field's width, or with GB_INPUT_P3_REPR the field types' in-memory words), values_dev_out a DEVICE
 * buffer of num_classes elements: one canonical word per class, the front part in slot order (what k_expand_partition reads),
 * classes nothing sets zero.  Returns after the generated values' error word has been read back.  GB_ERR_INVALID: an input
 * >= p ("non-canonical witness element"); two inputs, or an input and a generator, or two generators that set one class to
 * different values ("Partition containing .. was set twice with different values"); a PoseidonGate / Poseidon2BabyBearGate row
 * whose swap wire is not 0 or 1; a RandomAccessGate access index >= 2^bits; a BaseSumGate value that does not fit its limbs; a
 * QuotientGeneratorExtension with a zero denominator ("Tried to invert zero"); a generator program's IDIV or IREM by zero
 * ("attempt to divide by zero"); a BaseSumGenerator limb that is neither 0 nor 1
 * (get_bool_target: "not a bool"); a SplitGenerator / WireSplitGenerator value that does not fit its bits ("Integer too large
 * .." - the reference checks this one with debug_assert_eq!, that is in debug builds only; here it is always checked) - the
 * reference's assert!s, with the record index in gb_last_error.  Nothing faults and the circuit stays usable. */
gb_status gb_generate_partition(gb_circuit* c, const void* input_values, uint32_t flags, void* values_dev_out);
/* prove(): upload the inputs, run the generators (timing scope "run generators"), k_expand_partition straight from the generated
 * values ("compute full witness" is now the expansion alone), then the device-witness path of gb_prove unchanged.  The public
 * inputs are read from the generated values, in the same read-back as the error word.  salts as for gb_prove_partition (the
 * matrix, or the seed with GB_SALTS_FROM_SEED).  The
 * proof bytes are those of gb_prove_partition on the same values; errors are gb_generate_partition's and gb_prove's. */
gb_status gb_prove_inputs(gb_circuit* c, const void* input_values, uint32_t flags, const void* salts, void* proof_out,
                          size_t proof_cap, size_t* proof_len);
/* After GB_ERR_PERM_ARG_ZERO: the caller has re-drawn the input whose target is wire `wire` of row `row` -
 * prover_data.random_wire - and changed nothing else.  Same bytes and errors as gb_prove_inputs(input_values).  Where that input's
 * class has no generator that reads or writes it and the cell is alone in its class, as holds for random_wire, and the failed
 * attempt left its state behind, the value goes into the kept matrix as in gb_prove_partition_retry; anything else is the full
 * computation. */
gb_status gb_prove_inputs_retry(gb_circuit* c, const void* input_values, uint32_t flags, uint32_t wire, uint64_t row,
                                void* proof_out, size_t proof_cap, size_t* proof_len);

/* ---- does this witness satisfy this circuit, and if not, where does it fail? ------------------------------------------------
 * gb_prove* on a witness that breaks a gate or a copy constraint returns GB_OK and bytes that gb_verify rejects with
 * "vanishing(zeta) != Z_H(zeta) * quotient(zeta)": the reference's only guard, the trim_to_len of plonk/prover.rs:367 ("Quotient
 * has failed, the vanishing polynomial is not divisible by Z_H"), is vacuous where quotient_degree_factor is
 * max_quotient_degree_factor and a power of two, as in every configuration served here.  The check evaluates the constraints of
 * plonk/vanishing_poly.rs on H itself, where they must vanish, on the device (csrc/kernels_check.hip), and names what fails:
 *   gate violation      row r, gate g (an index into the gate table), constraint i: g is ACTIVE on r - compute_filter
 *                       (gates/gate.rs:391-404) of its selector column's value is non-zero - and constraint i of its
 *                       eval_unfiltered is the first that is not zero there.  PublicInputGate is evaluated against the hash of
 *                       the public inputs handed in, computed as gb_prove computes it; NoopGate has no constraints.
 *   selector violation  a selector value that is neither a gate index of its column's group nor UNUSED_SELECTOR (with a single
 *                       selector column, whose filters have no UNUSED factor: nor that): the circuit data is broken, not the
 *                       witness.  No gate is evaluated for that column on that row.
 *   copy violation      a wire cell whose value differs from the value of the FIRST cell of its class - the lowest
 *                       row * num_wires + column.  On a circuit with a partition (gb_circuit_set_partition) the slot map defines
 *                       the classes (copies_checked = 1); without one, the cycles of the permutation that
 *                       gb_circuit_decode_sigmas (below) has read out of the sigma columns (copies_checked = 2); with neither,
 *                       copies are not checked (copies_checked = 0) - the check never decodes sigma by itself.  Not checked
 *                       either way: lookups, and the Z / partial-product columns, which the prover computes itself.
 * A circuit made by plain gb_circuit_create is checked as the gate table {Noop, ConstantGate, PublicInputGate} it stands for: the
 * gate index is the selector value.  The first check on a circuit transforms its selector and constant columns to values on H
 * (the LDE the circuit keeps holds the coset g H, not H) and builds a row list per gate; that stays with the circuit until
 * gb_circuit_free / gb_ctx_trim.  Timing scopes: "check witness: prepare", "check witness", and inside the latter one per launch -
 * "check witness: gate kind K" (K = GB_GATE_*), "check witness: copies", "check witness: canonical words". */
#define GB_ERR_UNSATISFIED 20
#define GB_VIOLATION_GATE 1
#define GB_VIOLATION_SELECTOR 2
#define GB_VIOLATION_COPY 3
typedef struct gb_violation {   /* 48 bytes */
    uint32_t kind;         /* GB_VIOLATION_* */
    uint32_t gate;         /* GATE: index in the gate table */
    uint64_t row;          /* COPY: the cell's row */
    uint32_t index;        /* GATE: first failing constraint, eval_unfiltered order; SELECTOR: selector column; COPY: the cell's wire */
    uint32_t other_wire;   /* COPY: wire of the class's first cell */
    uint64_t other_row;    /* COPY: its row */
    uint64_t value;        /* GATE: that constraint's unfiltered value; SELECTOR: the selector value; COPY: the cell's value (canonical) */
    uint64_t other_value;  /* COPY: the first cell's value */
} gb_violation;
typedef struct gb_check_result {
    uint64_t num_gate_violations;     /* entries (row, gate) with a failing constraint, all of them, not just the listed */
    uint64_t num_selector_violations;
    uint64_t num_copy_violations;
    uint32_t copies_checked;          /* 0: not checked, 1: the partition's classes, 2: the classes decoded from sigma */
    uint32_t num_listed;
} gb_check_result;
/* witness: [num_wires][2^degree_bits] canonical values, accepted as gb_prove accepts its witness (GB_INPUT_HOST / GB_INPUT_DEVICE /
 * GB_INPUT_P3_REPR for a host's words; with GB_INPUT_DEVICE it is what gb_expand_partition wrote) - and an element that is not
 * below p is GB_ERR_INVALID ("non-canonical witness element").  violations_out: gb_violation[capacity], or NULL with capacity 0;
 * result: a gb_check_result, may be NULL (both travel as void* like the generator records of gb_circuit_set_generators).
 * GB_OK: no violation.  GB_ERR_UNSATISFIED: at least one; gb_last_error names the first (kind, row, gate index, constraint),
 * violations_out holds the first min(capacity, total) in this order - selector violations by (row, column), gate violations by
 * (row, gate), copy violations by cell index - and the counts in `result` are exact whatever the capacity.  A check keeps no retry
 * state, and for gb_prove_retry it is another call in between: what a failed attempt left on the circuit is released, and a retry
 * after a check is the full computation. */
gb_status gb_check_witness(gb_circuit* c, const void* witness, uint32_t flags, const uint64_t* public_inputs, size_t num_public_inputs,
                           void* violations_out, size_t capacity, void* result);
/* what gb_prove_partition / gb_prove_inputs run up to the device matrix - the expansion, or the generators and the expansion, with
 * the same errors, the public inputs read from the values as those functions read them - then the check */
gb_status gb_check_partition(gb_circuit* c, const void* values, uint32_t flags, void* violations_out, size_t capacity, void* result);
gb_status gb_check_inputs(gb_circuit* c, const void* input_values, uint32_t flags, void* violations_out, size_t capacity, void* result);
/* gb_ctx_set_option "check_witness" (default 0): 1 = every gb_prove*, gb_prove_partition* and gb_prove_inputs* that does the full
 * computation runs the check on its witness before the wires commitment and returns GB_ERR_UNSATISFIED instead of bytes that
 * cannot verify.  The incremental retry paths are not re-checked: only the random wire changed, and no gate constrains it. */

/* ---- the copy constraints from sigma alone -----------------------------------------------------------------------------------
 * The sigma columns ARE the copy permutation, written as field elements: sigma[col][row] = k_is[col'] w^row' sends the cell
 * (col, row) to (col', row') (plonk/permutation_argument.rs, circuit_builder.rs:1005-1040).  gb_circuit_decode_sigmas reads
 * (col', row') back out of every value on the device (csrc/kernels_sigma.hip, csrc/sigma_decode.hpp) - the coset by
 * s^n = k_is[col']^n, the row by a discrete logarithm in the group of order n = 2^degree_bits - checks that the result is a
 * permutation of the routed cells, and labels every wire cell with the lowest cell of its cycle (a cell is
 * row * num_wires + column, as in gb_violation; non-routed wires and fixed points label themselves).  The cycles are the copy
 * classes: from then on the witness check compares every cell with the first cell of its class on this circuit too, and with the
 * option "check_witness" gb_prove* refuses a broken copy with GB_ERR_UNSATISFIED.  Any gb_circuit_create* handle, either field.
 * The labels stay with the circuit until gb_circuit_free / gb_ctx_trim; a call on a circuit that has them does no device work -
 * except that, where a partition has been set since, it compares the two (below).
 * GB_ERR_INVALID, the circuit as usable as before and no labels kept:
 *   "k_is do not name distinct cosets"   two k_is[j]^n coincide (or a k_is[j] is 0)
 *   "sigma names no routed cell at row r, wire c: the value v .."   the lowest cell whose value is in none of the cosets
 *                                        k_is[j] H, j < num_routed_wires - 0, or a coset of a non-routed wire
 *   "sigma is not a permutation: row r, wire c and another cell both go to row r', wire c'"   the lowest cell whose target is shared
 *   "partition and sigma disagree at row r, wire c (partition: first cell A, sigma: first cell B)"   a partition is set and, for
 *                                        the lowest routed cell where they differ, the first cell of its class in the slot map
 *                                        is not its label: the representative_map does not describe the wiring of these sigmas
 *   flags other than 0.
 * GB_ERR_UNSUPPORTED: more than 2^32 wire cells.  Timing scopes: "decode sigmas: decode", "decode sigmas: classes", "decode
 * sigmas: compare" (the sigma values on H are resident with the circuit: there is no transform). */
typedef struct gb_sigma_info {
    uint64_t routed_cells;       /* num_routed_wires * 2^degree_bits */
    uint64_t moved_cells;        /* cells with sigma(cell) != cell */
    uint64_t num_classes;        /* cycles of length >= 2 */
    uint64_t largest_class;      /* cells in the longest cycle (1 if none) */
    uint32_t rounds;             /* doubling rounds the class pass ran */
    uint32_t compared_partition; /* 1: a partition was set and its classes were compared */
} gb_sigma_info;
gb_status gb_circuit_decode_sigmas(gb_circuit* c, uint32_t flags, void* info /* gb_sigma_info, may be NULL */);
/* first_cell_out[num_wires * 2^degree_bits] (host): the label of every wire cell.  GB_ERR_INVALID if the sigmas have not been
 * decoded. */
gb_status gb_circuit_copy_classes(gb_circuit* c, uint32_t* first_cell_out);

/* ---- copy constraints to sigma columns and representative map ------------------------------------------------------------------
 * The other direction: "generate sigma polynomials" of CircuitBuilder::build (plonk/circuit_builder.rs:1005-1040, 1220-1224;
 * plonk/permutation_argument.rs) on the device (csrc/kernels_wiring.hip, csrc/wiring.hpp), a stage of its own on a context like
 * gb_fft.  Target indices are those of gb_circuit_set_partition: wire (row, column) is row * num_wires + column, virtual target
 * i is degree * num_wires + i.  copy_constraints ([num_copies][2], the Target::index of both sides) and k_is ([num_routed_wires],
 * canonical) are host pointers.  sigmas_out is [num_routed_wires][2^degree_bits] canonical values on H: a host pointer, or with
 * GB_INPUT_DEVICE a device pointer of the caller (16-byte aligned) written on the context's stream - ready to be named by the
 * column pointers of gb_circuit_create*_cols(.., GB_INPUT_DEVICE).  The call returns when everything is written.
 * Every result but `rounds` is a function of the arguments alone, whatever the order in which the device ran its threads:
 *   classes              the connected components of the targets under the pairs
 *   representative map   representative_map_out[t] (host, [num_targets]; may be NULL) = the lowest target index of t's class: a valid
 *                        ProverOnlyCircuitData.representative_map for gb_circuit_set_partition.  It need not be the reference's,
 *                        whose roots depend on the order of its merges; nothing in a proof depends on which member it is.
 *   sigmas               within a class the routed wire cells in ascending row * num_wires + column order each point to the next,
 *                        the last to the first (the order wire_partition pushes them in, permutation_argument.rs:94-100):
 *                        sigma[col][row] = k_is[col'] w^row', w = two_adic_generator(degree_bits), and k_is[col] w^row for a cell
 *                        alone in its class - byte for byte the reference's values.  Virtual targets join classes and appear in
 *                        no sigma.
 * num_copies = 0 gives the identity sigmas and the identity map.
 * GB_ERR_INVALID, the outputs unspecified and the context as usable as before: a null argument; an unknown field tag;
 * num_routed_wires = 0 or > num_wires; num_targets < degree * num_wires; a k_is entry >= p; flag bits other than
 * GB_INPUT_DEVICE; and, checked on the device before an index is used as an address,
 *   "copy constraint i names target t, but there are N targets"   the lowest pair with an entry >= num_targets
 *   "Tried to route a wire that isn't routable: copy constraint i, target t (row r, wire c)"   the lowest pair that names a wire
 *                        cell of a column >= num_routed_wires (circuit_builder.rs:543-551)
 * GB_ERR_UNSUPPORTED: num_targets >= 2^32, or degree_bits above the field's two-adicity.  GB_ERR_OOM as elsewhere.
 * Timing scopes: "wiring: upload", "wiring: classes", "wiring: order", "wiring: sigmas". */
typedef struct gb_wiring_info {
    uint64_t routed_cells;     /* num_routed_wires * 2^degree_bits */
    uint64_t moved_cells;      /* routed cells with sigma(cell) != cell */
    uint64_t num_classes;      /* classes holding >= 2 routed wire cells */
    uint64_t largest_class;    /* routed wire cells in the largest such class (1 if none) */
    uint64_t merged_targets;   /* targets whose representative is not themselves */
    uint32_t rounds;           /* compression passes over the forest, the last one - which moved no pointer - included; a pass lets
                                  every target jump up to 4 ancestors.  A diagnostic: the shape the lock-free merges leave the
                                  forest in, and so this count, depends on the order the device ran them in */
    uint32_t reserved;
} gb_wiring_info;
gb_status gb_wiring_sigmas(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t num_wires, uint32_t num_routed_wires,
                           const void* k_is, const uint64_t* copy_constraints, uint64_t num_copies, uint64_t num_targets, uint32_t flags,
                           void* sigmas_out, uint64_t* representative_map_out, void* info /* gb_wiring_info, may be NULL */);

/* verify() of a proof produced for this circuit (plonk/verifier.rs:17-128, fri/verifier.rs:67-250,
 * plonk/get_challenges.rs:26-101), restated for the dummy gate set and run on the HOST like the reference's verifier: the
 * Fiat-Shamir replay, vanishing(zeta) == Z_H(zeta) * quotient(zeta), the proof of work, every Merkle path and the FRI
 * folding checks.  GB_OK = the proof verifies; GB_ERR_VERIFY names the failed check in gb_last_error; GB_ERR_INVALID =
 * malformed bytes. */
#define GB_ERR_VERIFY 19
gb_status gb_verify(gb_circuit* c, const void* proof, size_t proof_len);
/* gb_verify of many proofs of ONE circuit at once, with the query rounds - the Merkle paths and the folding checks, ~96 % of a
 * verification - checked on the device of `ctx`; the transcript, the vanishing identity and the proof of work stay on the host,
 * split over the context's "copy_threads".  For every i, results[i].status is what gb_verify(c, proofs[i], proof_lens[i])
 * returns and gb_verify_check_text(results[i].check) is the text it leaves in gb_last_error; of several failing checks the one
 * gb_verify reaches first is named (parse errors, the vanishing identity, the proof of work, then per query round in order: the
 * initial paths by oracle, each layer's consistency check and then its path, the final polynomial).
 *   c       any handle gb_verify accepts, either field - a gb_verifier_create* object made with a NULL context included
 *   ctx     the device; NULL, or a circuit that belongs to another context: GB_ERR_INVALID
 *   flags   0 (anything else: GB_ERR_INVALID).  Compressed proofs go to gb_verify_compressed_batch below
 *   results gb_verify_result[num_proofs], host
 * Returns GB_OK: every proof verified; GB_ERR_VERIFY: the call completed, at least one proof did not verify (results says which -
 * GB_ERR_INVALID proofs included); anything else: the call did not complete and results is unspecified.  num_proofs == 0: GB_OK.
 * A proof whose query section does not have the circuit's shape (a Merkle path length byte that differs) is checked on the host;
 * no device offset is derived from proof content.  The staged bytes per chunk are bounded by the context option
 * "verify_chunk_bytes" (gb_ctx_set_option: 4096 .. 2^30, default 8388608 = 8 MiB per staging slot, two slots); a chunk holds at
 * least one proof.  While a chunk's kernels run the host stage of the next chunk proceeds.
 * Timing scopes: "verify batch: host stage" (the span on the stream during which the host stage of a chunk ran), "verify batch:
 * upload", "verify batch: paths", "verify batch: queries". */
#define GB_VCHECK_NONE 0
#define GB_VCHECK_TRUNCATED 1          /* GB_ERR_INVALID: "proof bytes are truncated" */
#define GB_VCHECK_NON_CANONICAL 2      /* GB_ERR_INVALID: a word >= p */
#define GB_VCHECK_PI_IMPLAUSIBLE 3     /* GB_ERR_INVALID */
#define GB_VCHECK_PI_COUNT 4           /* GB_ERR_INVALID: validate_proof_with_pis_shape */
#define GB_VCHECK_TRAILING 5           /* GB_ERR_INVALID: "trailing bytes in proof" */
#define GB_VCHECK_VANISHING 6          /* GB_ERR_VERIFY from here on, but for the two path lengths */
#define GB_VCHECK_POW 7
#define GB_VCHECK_INITIAL_PATH_LEN 8   /* GB_ERR_INVALID; query_round, index = oracle */
#define GB_VCHECK_INITIAL_PATH 9       /* query_round, index = oracle */
#define GB_VCHECK_CONSISTENCY 10       /* query_round, index = layer */
#define GB_VCHECK_LAYER_PATH_LEN 11    /* GB_ERR_INVALID; query_round, index = layer */
#define GB_VCHECK_LAYER_PATH 12        /* query_round, index = layer */
#define GB_VCHECK_FINAL_POLY 13        /* query_round */
typedef struct gb_verify_result {
    uint32_t status;       /* GB_OK, GB_ERR_VERIFY or GB_ERR_INVALID: what gb_verify returns for this proof */
    uint32_t check;        /* GB_VCHECK_*: the check gb_verify would name; 0 when status == GB_OK */
    uint32_t query_round;  /* for the FRI query checks, else UINT32_MAX */
    uint32_t index;        /* oracle index (initial paths) or layer index (consistency, layer path), else UINT32_MAX */
} gb_verify_result;
gb_status gb_verify_batch(gb_ctx* ctx, gb_circuit* c, const void* const* proofs, const size_t* proof_lens, uint32_t num_proofs,
                          uint32_t flags, void* results /* gb_verify_result[num_proofs] */);
const char* gb_verify_check_text(uint32_t check); /* "" for GB_VCHECK_NONE and for a value that is no check */
/* gb_verify_batch for COMPRESSED proofs (CompressedProofWithPublicInputs bytes, below): gb_verify_compressed of many proofs of ONE
 * circuit, checked as they stand - nothing is decompressed into bytes, and a sibling hash or a coset that several query rounds
 * share is hashed once.  For every i, results[i].status is what gb_verify_compressed(c, proofs[i], proof_lens[i]) returns and
 * gb_verify_check_text(results[i].check) the text it leaves in gb_last_error; query_round and index are what gb_verify_batch
 * reports on the decompressed proof.  Of several failing checks the one gb_verify_compressed reaches first is named:
 * decompression first (parse errors, the stored query indices against the transcript's, a missing sibling), then gb_verify's
 * order on the decompressed proof (above).  ctx, c, flags, results, the return values, num_proofs == 0, "verify_chunk_bytes" and
 * the summary in gb_last_error are gb_verify_batch's.
 * The host stage (on the context's "copy_threads") parses, replays the transcript, compares the stored indices, counts from the
 * indices alone how many siblings every stored path must hold (hash/path_compression.rs:56-95), and checks the vanishing identity
 * and the proof of work.  A path with too few siblings fails as gb_verify_compressed fails it; a proof with a path that holds MORE
 * than needed (gb_verify_compressed ignores the surplus) is decompressed and verified on the host, as is every proof of a circuit
 * with more than 256 query rounds; every other proof goes to the device with a directory of its entries - offsets the host
 * computed from the indices and checked against the proof's length; the kernels read proof bytes as field words only.
 * ctx NULL is GB_ERR_INVALID as for gb_verify_batch; where the other arguments are in order the host stage has still run, on the
 * calling thread and touching no device, and results holds its verdicts - GB_ERR_INVALID with check 0 for every proof that only a
 * device could decide (tests/sanitize drives the parser and the sibling count this way).
 * Timing scopes: "verify compressed batch: host stage", "verify compressed batch: upload", "verify compressed batch: queries"
 * (fri_combine_initial, the folds with the inferred evaluations, the final polynomial), "verify compressed batch: paths" (every
 * tree's shared paths; it runs second because a layer tree's leaf is a re-inflated coset).
 * The checks only a compressed proof can fail (an enum, numbered from 16: the GB_VCHECK_ macros above are gb_verify's own): */
enum {
    GB_VCHECK_COMPRESSED_INDICES = 16,         /* GB_ERR_VERIFY: the stored query indices are not the transcript's */
    GB_VCHECK_COMPRESSED_MISSING_SIBLING = 17, /* GB_ERR_INVALID: a stored Merkle path holds fewer siblings than the indices demand */
    GB_VCHECK_COMPRESSED_TRAILING = 18         /* GB_ERR_INVALID: "trailing bytes in compressed proof" */
};
gb_status gb_verify_compressed_batch(gb_ctx* ctx, gb_circuit* c, const void* const* proofs, const size_t* proof_lens,
                                     uint32_t num_proofs, uint32_t flags, void* results /* gb_verify_result[num_proofs] */);
/* Compressed proofs, on the host like the reference's (hash/path_compression.rs, fri/proof.rs:137-384, plonk/proof.rs:96-260):
 * gb_proof_compress = ProofWithPublicInputs::compress -> CompressedProofWithPublicInputs bytes (util/serialization/mod.rs:2168-2256:
 * Merkle paths of one tree share their siblings, a repeated query index is stored once, the FRI evaluation the verifier can infer
 * is dropped); gb_proof_decompress = CompressedProofWithPublicInputs::decompress (replays the transcript, recomputes the inferred
 * evaluations, re-inflates the paths) -> the original bytes; gb_verify_compressed = CompressedProofWithPublicInputs::verify.
 * *out_len receives the size written (or needed, with GB_ERR_BUFFER_TOO_SMALL).  They need the circuit's common data only, so a
 * gb_verifier_create object serves as well. */
gb_status gb_proof_compress(gb_circuit* c, const void* proof, size_t proof_len, void* out, size_t out_cap, size_t* out_len);
gb_status gb_proof_decompress(gb_circuit* c, const void* compressed, size_t compressed_len, void* out, size_t out_cap, size_t* out_len);
gb_status gb_verify_compressed(gb_circuit* c, const void* compressed, size_t compressed_len);
/* A circuit object for gb_verify alone, from what a verifier holds: CommonCircuitData (cfg + gates, as for
 * gb_circuit_create_gates; k_is [num_routed_wires]) and VerifierOnlyCircuitData (constants_sigmas_cap [2^cap_height][H],
 * circuit_digest [H]), all host pointers to canonical elements.  Touches no device: ctx may be NULL (gb_last_error(NULL) then
 * reports).  With it gb_verify checks the reference's own serialized proofs - tests/test_abi_verify_fixture.py runs the
 * RECURSIVE_VERIFIER_GL regression proof (recursion/regression_test_data.rs) through it.  Free with gb_circuit_free. */
gb_status gb_verifier_create(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates, const void* k_is,
                             const void* constants_sigmas_cap, const void* circuit_digest, gb_circuit** out);
/* the same for a gate set with GB_GATE_PROGRAM entries (see "constraint programs" above) */
gb_status gb_verifier_create_programs(gb_ctx* ctx, const gb_circuit_config* cfg, const gb_gate* gates, uint32_t num_gates,
                                      const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                      const void* k_is, const void* constants_sigmas_cap, const void* circuit_digest,
                                      gb_circuit** out);

/* ---- the stages of prove(), one at a time ---------------------------------------------------------------------------------
 * For a host that keeps the reference's prover loop (plonk/prover.rs:228-447) and its Challenger and swaps in the heavy calls
 * one by one: wires / Zs / quotient commitments through gb_commit_values / gb_commit_coeffs, the opening set through
 * gb_batch_eval_ext, and the three functions below.  gb_prove is exactly this sequence with the transcript kept inside the
 * library (tests/test_gpu_stage_abi.py drives the stages from Python with the oracle's Challenger and gets gb_prove's bytes).
 * Challenges are canonical field elements, host pointers.  Results are canonical; `flags` (GB_INPUT_HOST / GB_INPUT_DEVICE) names
 * the memory space of the large operand AND of the result buffer. */

/* wires_permutation_partial_products_and_zs + all_wires_permutation_partial_products (plonk/prover.rs:449-546): witness =
 * wire_values [num_wires][n] (only the routed columns are read); betas, gammas: [num_challenges].  values_out:
 * [num_challenges * (1 + num_partial_products)][n] VALUES on H_n in the order prover.rs:318-329 hands them to from_values - every
 * challenge's Z first, then each challenge's partial products.  GB_ERR_PERM_ARG_ZERO = ProverError::InvZeroPermArg (:512-514). */
gb_status gb_zs_partial_products(gb_circuit* c, const void* witness, uint32_t flags, const void* betas, const void* gammas,
                                 void* values_out);
/* the same with the witness as separately allocated columns (only wire_cols[0 .. num_routed_wires) are read) */
gb_status gb_zs_partial_products_cols(gb_circuit* c, const void* const* wire_cols, uint32_t flags, const void* betas,
                                      const void* gammas, void* values_out);
/* compute_quotient_polys (plonk/prover.rs:712-926) followed by the split into degree-n chunks (:345-376).  wires and
 * zs_partial_products are the commitments of the same proof (gb_commit_values of the witness / of gb_zs_partial_products' output),
 * made on this circuit's context; public_inputs_hash: [H]; betas, gammas, alphas: [num_challenges].  chunks_out:
 * [num_challenges * quotient_degree_factor][n] COEFFICIENTS, ready for gb_commit_coeffs (:376-387). */
gb_status gb_quotient_polys(gb_circuit* c, gb_batch* wires, gb_batch* zs_partial_products, const void* public_inputs_hash,
                            const void* betas, const void* gammas, const void* alphas, uint32_t flags, void* chunks_out);
/* Challenger<F, H> (iop/challenger.rs:18-31) by value: sponge_state (SPONGE_WIDTH = 12 / 16 words used), input_buffer and
 * output_buffer (at most SPONGE_RATE = 8 each; challenges pop from the END of output_buffer, :84-94).  Canonical values as u64 for
 * either field. */
typedef struct gb_challenger_state {
    uint64_t sponge_state[16];
    uint64_t input_buffer[8];
    uint64_t output_buffer[8];
    uint32_t input_len, output_len;
} gb_challenger_state;
/* PolynomialBatch::prove_openings (fri/oracle.rs:187-246) on the PLONK instance of this circuit (get_fri_instance(zeta),
 * plonk/circuit_data.rs:438-520: constants/sigmas, wires, Zs / partial products, quotient - the Zs also at g * zeta) followed by
 * fri_proof (fri/prover.rs:29-81): commit phase, proof of work (the MINIMUM nonce), query rounds.  zeta: [D]; `challenger` is the
 * transcript after observe_openings (plonk/prover.rs:418) and is left as the reference leaves it.  fri_proof_out receives the
 * FriProof bytes (util/serialization/mod.rs:1679-1695): commit_phase_merkle_caps, query_round_proofs, final_poly, pow_witness -
 * the part of ProofWithPublicInputs between the opening set and the public inputs; *fri_proof_len is the size needed.
 * On ANY error - GB_ERR_BUFFER_TOO_SMALL of a size query included - *challenger is left exactly as it was passed in, so the
 * call can be repeated with a buffer of *fri_proof_len bytes and returns the bytes gb_prove would (the query itself runs the
 * whole stage: ask once, keep the size - it depends on the configuration only). */
gb_status gb_prove_openings(gb_circuit* c, gb_batch* wires, gb_batch* zs_partial_products, gb_batch* quotient, const void* zeta,
                            gb_challenger_state* challenger, void* fri_proof_out, size_t fri_proof_cap, size_t* fri_proof_len);

/* PolynomialBatch::prove_openings (fri/oracle.rs:187-246) on any FriInstanceInfo (fri/structure.rs), then fri_proof
 * (fri/prover.rs:29-81).  oracles[num_oracles]: commitments made on ctx.  Batch b opens batch_sizes[b] polynomials at
 * points[b] ([num_batches][D] canonical words); polynomials: [sum of batch_sizes][2] = (oracle_index, polynomial_index), batch
 * after batch, in the order of FriBatchInfo::polynomials.  degree_bits, rate_bits, cap_height and the field are the oracles' own.
 * challenger / fri_proof_out / sizes / behaviour on error: exactly as gb_prove_openings.
 * The lists may be in any order, name a polynomial in several batches or twice in one, and leave an oracle out of every batch: it
 * still contributes its row and path to every query round, as fri_proof is handed every oracle's tree.  Blinding needs no flag:
 * an oracle committed with salts opens rows of ncols + GB_SALT_SIZE words; polynomial_index counts polynomials only.
 * GB_ERR_INVALID (with a message): num_oracles, num_batches or a batch size of zero; a NULL oracle, one from another context or
 * field, or a stand-alone Merkle tree; oracles that differ in degree_bits, rate_bits or cap_height; an index out of range; a
 * reduction_arity_bits list gb_circuit_set_fri_reduction_arity_bits would refuse for this shape (the empty list is valid); a
 * coordinate >= p; proof_of_work_bits > 31.  GB_ERR_UNSUPPORTED: a point equal to zero - divide_by_linear runs here on the powers
 * of the point's INVERSE (any other point is fine, one inside the subgroup included: the reference does not check it here). */
#define GB_MAX_FRI_QUERY_ROUNDS 4096 /* num_query_rounds of the two functions below: 0 or above this is GB_ERR_INVALID */
gb_status gb_fri_prove_openings(gb_ctx* ctx, gb_batch* const* oracles, uint32_t num_oracles, const void* points,
                                const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials,
                                const uint32_t* reduction_arity_bits, uint32_t num_layers, uint32_t proof_of_work_bits,
                                uint32_t num_query_rounds, gb_challenger_state* challenger, void* fri_proof_out,
                                size_t fri_proof_cap, size_t* fri_proof_len);
/* verify_fri_proof (fri/verifier.rs:67-250) for the same description of an instance, on the host; ctx may be NULL.
 * oracle_num_polys / oracle_blinding: FriOracleInfo; hiding: FriParams.hiding; openings: [sum of batch_sizes][D] (FriOpenings);
 * initial_caps: [num_oracles][2^cap_height][H]; challenger: the transcript after the openings were observed (by value: the caller's
 * copy is not advanced).  GB_OK / GB_ERR_VERIFY (the failed check in gb_last_error) / GB_ERR_INVALID (malformed bytes or arguments). */
gb_status gb_fri_verify(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t hiding,
                        const uint32_t* oracle_num_polys, const uint32_t* oracle_blinding, uint32_t num_oracles, const void* points,
                        const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials, const void* openings,
                        const void* initial_caps, const uint32_t* reduction_arity_bits, uint32_t num_layers,
                        uint32_t proof_of_work_bits, uint32_t num_query_rounds, const gb_challenger_state* challenger,
                        const void* fri_proof, size_t fri_proof_len);
/* gb_fri_verify of `num_items` proofs that share ONE instance shape, the query rounds - every Merkle path, fri_combine_initial and
 * the folding checks - on the device of `ctx`, as gb_verify_batch runs them for the proofs of one PLONK circuit.  The shape is the
 * field, degree_bits, rate_bits, cap_height, hiding, oracle_num_polys, oracle_blinding, batch_sizes, polynomials,
 * reduction_arity_bits, proof_of_work_bits and num_query_rounds: the same flat arrays with the same meaning as gb_fri_verify.
 * Proofs of several shapes: group them by shape, one call per group.  Per item i, tables of HOST pointers / arrays:
 *   points[i]        [num_batches][D]          every proof has its own zeta
 *   openings[i]      [sum of batch_sizes][D]
 *   initial_caps[i]  [num_oracles][2^cap_height][H]; the pointers may alias (a cap all items share is passed once)
 *   challengers[i]   the transcript after the openings were observed, by value: never advanced
 *   fri_proofs[i], fri_proof_lens[i]           FriProof bytes
 *   flags   0 (anything else: GB_ERR_INVALID);  results: gb_verify_result[num_items], host
 * For every i, results[i].status is what gb_fri_verify returns for that item alone and gb_verify_check_text(results[i].check) the
 * text it leaves in gb_last_error for the checks that have a GB_VCHECK_ code (truncated, trailing, the two path lengths, the proof
 * of work, initial path, consistency, layer path, final polynomial); a word >= p in the item's points, openings, caps or proof
 * bytes is GB_ERR_INVALID with GB_VCHECK_NON_CANONICAL, a challenger state gb_fri_verify refuses GB_ERR_INVALID with check 0.
 * query_round and index follow gb_verify_batch (oracle index for initial paths, layer index for consistency and layer paths, else
 * UINT32_MAX); of several failing checks the one gb_fri_verify reaches first is named.
 * Returns GB_OK: every item verified; GB_ERR_VERIFY: the call completed and at least one item did not verify (GB_ERR_INVALID items
 * included); anything else: the call did not complete and results is unspecified.  num_items == 0: GB_OK.  An error of the shared
 * shape is no verdict: it fails the call with gb_fri_verify's status and message; a NULL table or a NULL entry is GB_ERR_INVALID.
 * The host stage (on the context's "copy_threads", in gb_fri_verify's order) checks the item's words, parses the proof, replays the
 * transcript, reduces the openings and checks the proof of work; an item whose length or whose path-length bytes are not the
 * shape's is walked on the host, every other item's query section is uploaded as it stands with a record of its challenges and
 * caps - no device offset is derived from proof content.  Chunks, the two staging slots and "verify_chunk_bytes" are
 * gb_verify_batch's.  Limits of the device path (a shape beyond them is no error: every item is walked on the host, over the copy
 * threads, with the same results): GB_FRI_VERIFY_BATCH_MAX_ORACLES oracles, GB_FRI_VERIFY_BATCH_MAX_BATCHES batches,
 * GB_FRI_VERIFY_BATCH_MAX_POLYNOMIALS entries of `polynomials`, GB_MAX_FRI_LAYERS layers, GB_MAX_FRI_QUERY_ROUNDS query rounds,
 * num_oracles + 2 * num_layers + 1 < 2^16, and a proof's query section and its record together at most
 * GB_FRI_VERIFY_BATCH_MAX_ITEM_BYTES (64 MiB: a page-locked staging slot holds at least one item, whatever "verify_chunk_bytes" says).
 * ctx NULL is GB_ERR_INVALID; where the other arguments are in order the host stage has still run, on the calling thread and
 * touching no device, and results holds its verdicts - GB_ERR_INVALID with check 0 for every item that only a device could decide.
 * Timing scopes: "fri verify batch: host stage", "fri verify batch: upload", "fri verify batch: paths", "fri verify batch: queries". */
#define GB_FRI_VERIFY_BATCH_MAX_ORACLES 64
#define GB_FRI_VERIFY_BATCH_MAX_BATCHES 64
#define GB_FRI_VERIFY_BATCH_MAX_POLYNOMIALS 65536
#define GB_FRI_VERIFY_BATCH_MAX_ITEM_BYTES 67108864
gb_status gb_fri_verify_batch(gb_ctx* ctx, uint32_t field, uint32_t degree_bits, uint32_t rate_bits, uint32_t cap_height, uint32_t hiding,
                              const uint32_t* oracle_num_polys, const uint32_t* oracle_blinding, uint32_t num_oracles,
                              const uint32_t* batch_sizes, uint32_t num_batches, const uint32_t* polynomials,
                              const uint32_t* reduction_arity_bits, uint32_t num_layers, uint32_t proof_of_work_bits,
                              uint32_t num_query_rounds, const void* const* points, const void* const* openings,
                              const void* const* initial_caps, const gb_challenger_state* challengers, const void* const* fri_proofs,
                              const size_t* fri_proof_lens, uint32_t num_items, uint32_t flags,
                              void* results /* gb_verify_result[num_items] */);
/* gb_fri_verify_batch on `ctx` since it was created: *device_items = the items whose query rounds the kernels decided,
 * *host_items = every other item of a completed call (decided by the host stage, or walked on the host: an irregular item, a shape
 * beyond the device path's limits).  How a caller - and the test suite - sees that a shape left the device path. */
gb_status gb_fri_verify_batch_counts(gb_ctx* ctx, uint64_t* device_items, uint64_t* host_items);

/* ---- constraint systems over committed oracles ---------------------------------------------------------------------------------
 * The quotient stage for a host that proves with gb_commit_* / gb_fri_prove_openings and constraints of its own - a circuit with
 * lookup terms, a STARK over this FRI: the constraints are straight-line programs over CELLS (oracle, polynomial, rows ahead) of
 * the committed oracles, numbered 0, 1, 2, ... by the EMITs of program 0, then program 1, and so on; challenge c folds them as
 * sum_i alphas[c]^i * constraint_i, and the folded sum is divided by Z_H = X^n - 1 on a coset.
 * The table is that of the constraint programs above (program_words, program_offsets, at most GB_MAX_PROGRAMS; instruction words,
 * registers, literals and their limits unchanged) with two differences:
 *   word 0   num_cells | num_inputs << 32         num_inputs = 3 + num_params
 *   after the num_literals literals come num_cells CELL words (at most GB_MAX_PROGRAM_CELLS), then the instructions:
 *     bits 0-15   oracle_index
 *     bits 16-47  polynomial_index (salt columns are not polynomials)
 *     bits 48-63  row_offset: rows ahead, modulo n (0 this row, 1 the next row, n - 1 the row before)
 *   operand space 1 indexes the program's cell table instead of a wire column;
 *   operand space 2 indexes the INPUTS: 0 is X (the point), 1 is L_first(X) = L_0, 2 is L_last(X) = L_(n-1), 3 + k is params[k] -
 *   canonical base-field words for the caller's challenges and public values (plonky2's beta, gamma, delta are base-field elements).
 * Degree bounds, in gb_circuit_create_programs' units: literal and param 0; cell, X, L_first, L_last 1; ADD / SUB the maximum, MUL
 * the sum.  A constraint's bound is at most the header's `degree`, and `degree` at most 2^quotient_degree_bits + 1, so that the
 * quotient has fewer than n * 2^quotient_degree_bits coefficients.
 *
 * gb_constraint_quotient: oracles[num_oracles] (at most GB_MAX_CONSTRAINT_ORACLES) are commitments made on ctx with one degree_bits
 * and rate_bits; the constraints are evaluated on the first 2^quotient_degree_bits coset blocks of their LDEs (every
 * 2^(rate_bits - quotient_degree_bits)-th point of g * H_N, as compute_quotient_polys does), one thread per point
 * (k_constraint_quotient, the interpreter of k_gate_programs), followed by the coset inverse transform.  params: [num_params],
 * alphas: [num_challenges], host pointers, canonical.  chunks_out: [num_challenges * 2^quotient_degree_bits][n] COEFFICIENTS,
 * canonical, ready for gb_commit_coeffs: quotient_c(X) = sum_i X^(n i) chunk_(c,i)(X).  flags (GB_INPUT_HOST / GB_INPUT_DEVICE)
 * names the memory space of chunks_out, as for gb_quotient_polys.  quotient_degree_bits 1 .. 4 and at most rate_bits;
 * num_challenges 1 .. 16 (widths 1 .. 4 are compiled, other counts run as slices); num_params at most GB_MAX_CONSTRAINT_PARAMS.
 * A trace that does not satisfy its constraints is no error: the call returns GB_OK and the chunks of a polynomial for which
 * the identity below fails.
 * GB_ERR_INVALID (the message names the program and the instruction or cell; everything is checked on the host before an index
 * is used as an address): every malformation gb_circuit_create_programs refuses; an oracle_index >= num_oracles; a
 * polynomial_index not below that oracle's polynomial count; a row_offset >= n; num_inputs != 3 + num_params; a param or alpha
 * >= p; a NULL oracle, one from another context or field, or a stand-alone Merkle tree; oracles that differ in degree_bits or
 * rate_bits; num_oracles of zero or above the limit; quotient_degree_bits or num_challenges out of range; other flag bits.
 * Timing scopes: "constraint quotient: values", "constraint quotient: IFFT".
 *
 * gb_constraint_eval: the same words over the extension field at one point - the verifier's side, host only, ctx may be NULL
 * (it only receives the error message).  cell_values: the opened values of the cells in cell-table order, program after
 * program ([total cells][D]; a cell with row_offset k is the polynomial's opening at zeta * w_n^k); X = zeta,
 * L_first(zeta) = Z_H(zeta) / (n (zeta - 1)), L_last(zeta) = L_first(zeta * w_n).  folded_out[c] = sum_i alphas[c]^i *
 * constraint_i(zeta), NOT divided by Z_H: a verifier checks folded_c == Z_H(zeta) * sum_i zeta^(n i) * chunk_(c,i)(zeta), as
 * plonk/verifier.rs:60-95 does.  oracle_index is checked against GB_MAX_CONSTRAINT_ORACLES and polynomial_index not at all (no
 * oracle is at hand; neither is read); no degree is checked.  GB_ERR_INVALID besides the table's: an unknown field,
 * degree_bits above the field's two-adicity, a coordinate of zeta or of cell_values >= p.  zeta inside the subgroup H_n, where
 * L_first has no value, is GB_ERR_OPENING_IN_SUBGROUP, as for gb_prove_openings. */
#define GB_MAX_CONSTRAINT_ORACLES 16
#define GB_MAX_PROGRAM_CELLS 4096
#define GB_MAX_CONSTRAINT_PARAMS 4096
/* quotient of the alpha-folded constraints of `programs` over the LDEs of `oracles`, as degree-n coefficient chunks */
gb_status gb_constraint_quotient(gb_ctx* ctx, gb_batch* const* oracles, uint32_t num_oracles,
                                 const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                                 const void* params, uint32_t num_params, const void* alphas, uint32_t num_challenges,
                                 uint32_t quotient_degree_bits, uint32_t flags, void* chunks_out);
/* the same constraints at one extension point, from opened values: the verifier's side; host only, ctx may be NULL */
gb_status gb_constraint_eval(gb_ctx* ctx, uint32_t field, uint32_t degree_bits,
                             const uint64_t* program_words, const uint32_t* program_offsets, uint32_t num_programs,
                             const void* cell_values /* [total cells][D] */, const void* params, uint32_t num_params,
                             const void* zeta /* [D] */, const void* alphas, uint32_t num_challenges,
                             void* folded_out /* [num_challenges][D] */);

/* fri_proof_of_work (fri/prover.rs:136-188) on its own, for a host that keeps the Challenger: sponge_state is the
 * duplex state with the pending input buffer already written over lanes 0..witness_pos-1 (`duplex_intermediate_state`,
 * :165-167; [12] u64 / [16] u32 canonical), witness_pos = input_buffer.len().  Returns the MINIMUM candidate whose
 * response `permute(state with candidate at witness_pos)[7]` has >= min_leading_zeros leading zeros as a u64
 * (min_leading_zeros = proof_of_work_bits + 64 - F::order().bits(), :147). */
gb_status gb_pow_grind(gb_ctx* ctx, uint32_t field, const void* sponge_state, uint32_t witness_pos, uint32_t min_leading_zeros,
                       uint64_t* nonce);

/* ---- polynomials and Merkle trees on their own ------------------------------------------------------------------------------
 * What PolynomialBatch and prove() are made of, for a host that uses the reference's `field` crate or its Merkle tree outside
 * prove(): PolynomialCoeffs::fft / coset_fft, PolynomialValues::ifft / coset_ifft / lde / lde_onto_coset
 * (field/src/polynomial/mod.rs) and MerkleTree::new (hash/merkle_tree.rs) - the shapes of benches/ffts.rs and benches/merkle.rs.
 *
 * Transforms.  `in` and `out` are column-major blocks [ncols][len] of canonical words in NATURAL order.  ext = 0: an element is
 * one base word; ext = 1: an element is D consecutive base words (D = 2 Goldilocks, 4 BabyBear) - the layout of
 * PolynomialCoeffs<F::Extension>, which fri/oracle.rs:226-231 transforms; any other value is GB_ERR_INVALID.  `shift` is NULL (no
 * coset: the same as a shift of 1) or a HOST pointer to one canonical base-field element (8 / 4 bytes); 0 or a value >= p is
 * GB_ERR_INVALID.  The tables of 1 and of F::generator() stay with the context; those of any other shift are built for the call
 * (which then waits for the stream once while it uploads them).  flags: GB_INPUT_DEVICE - `in` AND `out` are device pointers, the
 * work is ordered on the context's stream as gb_commit_* with GB_INPUT_DEVICE, and both blocks must stay valid until
 * gb_ctx_synchronize; GB_INPUT_P3_REPR - the host input words are the reference's field types as they lie in memory.  The output
 * is canonical either way.  With host pointers the call returns when `out` is filled; pageable memory is fine.
 * log_n >= 0; log_n + rate_bits above the field's two-adicity (32 / 27) is GB_ERR_INVALID (fft.rs:174-180); ncols == 0 is GB_OK
 * and touches nothing; out == in is allowed when both have the same length (the reference consumes `self`); a device that is too
 * small is GB_ERR_OOM.  Results are bit-identical to the reference's: its zero-tail shortcut (fft.rs:189-195) is an optimisation,
 * not a different result. */

/* PolynomialCoeffs::lde(rate_bits) then fft_with_options(Some(rate_bits)) (polynomial/mod.rs:201-203, 264-275), or with a shift
 * coset_fft_with_options(shift, Some(rate_bits)) (:277-295).  coeffs [ncols][n], values [ncols][n << rate_bits]:
 * values[i] = P(shift * w_N^i). */
gb_status gb_fft(gb_ctx* ctx, uint32_t field, const void* coeffs, void* values, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                 uint32_t ext, const void* shift, uint32_t flags);
/* PolynomialValues::ifft (:57-59) / coset_ifft(shift) (:62-72).  values, coeffs [ncols][n]. */
gb_status gb_ifft(gb_ctx* ctx, uint32_t field, const void* values, void* coeffs, size_t ncols, uint32_t log_n, uint32_t ext,
                  const void* shift, uint32_t flags);
/* PolynomialValues::lde(rate_bits) (:78-81; shift NULL) / lde_onto_coset (:84-88; shift = F::generator(), any shift accepted):
 * values on H_n -> values on shift * H_N, N = n << rate_bits.  The coefficients in between never leave the device. */
gb_status gb_lde(gb_ctx* ctx, uint32_t field, const void* values, void* out, size_t ncols, uint32_t log_n, uint32_t rate_bits,
                 uint32_t ext, const void* shift, uint32_t flags);

/* MerkleTree::new(leaves, cap_height) (hash/merkle_tree.rs:152-181).  The tree is a batch without polynomials: it keeps its leaves
 * and its level-major digests on the device as a commitment does, its blocks go back through the context's pool when it is
 * freed, and a gb_merkle_tree handle is a gb_batch handle - the functions below also read the tree of a commitment, and
 * gb_batch_cap / _leaf / _digests / _leaves / _free accept a stand-alone tree (gb_batch_coeffs, gb_batch_eval_ext and the stages
 * of prove() answer GB_ERR_INVALID for one: it has no coefficients). */
typedef struct gb_batch gb_merkle_tree;
/* leaves [2^log_leaves][leaf_len] ROW-major canonical words (the flattened Vec<Vec<F>>; every leaf as long as the first); leaf
 * digest = hash_or_noop.  flags: GB_INPUT_DEVICE / GB_INPUT_P3_REPR as above; host leaves belong to the caller again on return.
 * cap_height > log_leaves is GB_ERR_INVALID with the reference's message, "cap_height={} should be at most
 * log2(leaves.len())={}" (:154-157); leaf_len == 0 is GB_ERR_INVALID. */
gb_status gb_merkle_tree_create(gb_ctx* ctx, uint32_t field, const void* leaves, uint32_t log_leaves, uint32_t leaf_len,
                                uint32_t cap_height, uint32_t flags, gb_batch** out);
gb_status gb_merkle_tree_free(gb_batch* tree); /* NULL: GB_OK */
gb_status gb_merkle_tree_info(const gb_batch* tree, uint32_t* field, uint32_t* log_leaves, uint32_t* leaf_len, uint32_t* cap_height);
/* .cap (:60-61): out[2^cap_height][H] */
gb_status gb_merkle_tree_cap(gb_batch* tree, void* out);
/* get(i) + prove(i) (:183-222): row[leaf_len], siblings[log_leaves - cap_height][H], *nsib = that count; any of the three
 * pointers may be NULL; leaf_index >= 2^log_leaves is GB_ERR_INVALID */
gb_status gb_merkle_tree_leaf(gb_batch* tree, uint64_t leaf_index, void* row, void* siblings, uint32_t* nsib);
/* .digests in the reference's layout (:50-58): out[2 * (2^log_leaves - 2^cap_height)][H] */
gb_status gb_merkle_tree_digests(gb_batch* tree, void* out);

/* ---- field elements from a seed ---------------------------------------------------------------------------------------------
 * A stream is (seed[GB_SEED_SIZE], nonce[3]).  Element e of it, for e >> 2 < 2^32: the ChaCha20 block (RFC 8439 2.3: 20 rounds,
 * the "expand 32-byte k" constants) with words 4-11 the seed as eight little-endian words, word 12 the counter e >> 2 and words
 * 13-15 nonce[0..2]; of its 64 serialized bytes, bytes 16 (e & 3) .. 16 (e & 3) + 15 as a little-endian 128-bit integer x; the
 * element is x mod p, canonical.  Four elements per block in both fields, no rejection - position e depends on no other - and a
 * bias below 2^-64 (Goldilocks) / 2^-97 (BabyBear).  nonce[0] = GB_STREAM_SALTS and GB_STREAM_BLINDING are the library's own
 * streams (gb_prove_salted with GB_SALTS_FROM_SEED; the builder's blinding rows).
 * Writes elements first_element .. first_element + count - 1 as canonical words of the field's width (u64 / u32) to `out`: host
 * memory, or with flags = GB_INPUT_DEVICE a 16-byte-aligned device buffer of the caller, written on the context's stream - ready
 * as the device `salts` of gb_commit_*.  The elements are computed on the device either way.  GB_ERR_INVALID: seed, nonce or out
 * NULL; a range whose last block index does not fit 32 bits (first_element + count > 2^34); an unknown field; other flag bits; a
 * misaligned device destination. */
gb_status gb_random_elements(gb_ctx* ctx, uint32_t field, const uint8_t* seed, const uint32_t* nonce, uint64_t first_element,
                             uint64_t count, uint32_t flags, void* out);

/* ---- bare kernels (parity tests and microbenchmarks) ---------------------------------------- */
/* `count` Poseidon-12 (GL) / Poseidon2-16 (BB) permutations: in/out [count][width], host memory.
 * PoseidonGoldilocks::poseidon (hash/poseidon_goldilocks.rs:912-922). */
gb_status gb_permute(gb_ctx* ctx, uint32_t field, const void* in, void* out, uint64_t count);

#ifdef __cplusplus
}
#endif
#endif /* GOLDIBEAR_GPU_H */

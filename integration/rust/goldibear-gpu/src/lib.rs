//! Safe wrappers over the C ABI of `libgoldibear_gpu.so` (`include/goldibear_gpu.h`).
//!
//! This is the shim the reference crate would depend on under a `gpu-mi355x` feature.  Field elements
//! cross the boundary either as canonical little-endian words (`u64` Goldilocks, `u32` BabyBear - what
//! `as_canonical_u64()` / `as_canonical_u32()` give; `Repr::Canonical`) or exactly as the reference's field types lie
//! in memory (`Repr::P3InMemory` = `GB_INPUT_P3_REPR`: p3-goldilocks' possibly non-canonical `u64`, p3-baby-bear's
//! Montgomery `u32`), in which case a `Vec<F>` is handed over without any conversion pass.  Matrices are taken where the
//! reference has them: the `*_columns` methods bind the `*_cols` entry points, which read `Vec<Vec<F>>` /
//! `Vec<PolynomialValues<F>>` column by column from pageable memory - no flattening copy on the host.
//! Written against the header; not compiled in this repository (the build image has no Rust toolchain).
use std::ffi::{c_char, c_void, CStr};
use std::ptr;

#[repr(C)]
pub struct gb_ctx { _p: [u8; 0] }
#[repr(C)]
pub struct gb_batch { _p: [u8; 0] }
#[repr(C)]
pub struct gb_circuit { _p: [u8; 0] }

pub const GB_OK: i32 = 0;
pub const GB_ERR_INVALID: i32 = 1;
pub const GB_ERR_PERM_ARG_ZERO: i32 = 16;
pub const GB_ERR_VERIFY: i32 = 19;
pub const GB_ERR_UNSATISFIED: i32 = 20;
pub const GB_VIOLATION_GATE: u32 = 1;
pub const GB_VIOLATION_SELECTOR: u32 = 2;
pub const GB_VIOLATION_COPY: u32 = 3;
pub const GB_GOLDILOCKS: u32 = 0;
pub const GB_BABYBEAR: u32 = 1;
pub const GB_INPUT_HOST: u32 = 0;
pub const GB_INPUT_P3_REPR: u32 = 2;
pub const GB_SALTS_FROM_SEED: u32 = 4;
pub const GB_SEED_SIZE: usize = 32;
pub const GB_STREAM_SALTS: u32 = 1;
pub const GB_STREAM_BLINDING: u32 = 2;
pub const GB_MAX_FRI_LAYERS: usize = 32;
pub const GB_GEN_ARITHMETIC: u32 = 0;
pub const GB_GEN_ARITHMETIC_EXTENSION: u32 = 1;
pub const GB_GEN_MUL_EXTENSION: u32 = 2;
pub const GB_GEN_CONSTANT: u32 = 3;
pub const GB_GEN_BASE_SPLIT: u32 = 4;
pub const GB_GEN_REDUCING: u32 = 5;
pub const GB_GEN_REDUCING_EXTENSION: u32 = 6;
pub const GB_GEN_RANDOM_ACCESS: u32 = 7;
pub const GB_GEN_POSEIDON_MDS: u32 = 8;
pub const GB_GEN_COSET_INTERPOLATION: u32 = 9;
pub const GB_GEN_EXPONENTIATION: u32 = 10;
pub const GB_GEN_POSEIDON: u32 = 11;
pub const GB_GEN_POSEIDON2_BABYBEAR: u32 = 12;
pub const GB_GEN_ADD_MANY: u32 = 13;
pub const GB_GEN_APPLY_MAT4: u32 = 14;
pub const GB_GEN_POSEIDON2_INTERNAL: u32 = 15;
pub const GB_GEN_COPY: u32 = 16;
pub const GB_GEN_EQUALITY: u32 = 32;
pub const GB_GEN_NONZERO_TEST: u32 = 33;
pub const GB_GEN_QUOTIENT_OR_ZERO: u32 = 34;
pub const GB_GEN_QUOTIENT_EXTENSION: u32 = 35;
pub const GB_GEN_SPLIT: u32 = 36;
pub const GB_GEN_WIRE_SPLIT: u32 = 37;
pub const GB_GEN_LOW_HIGH: u32 = 38;
pub const GB_GEN_BASE_SUM: u32 = 39;
pub const GB_GEN_TARGETS: u32 = 40;
pub const GB_GEN_PROGRAM: u32 = 48;
pub const GB_MAX_GENERATOR_PROGRAMS: u32 = 256;
pub const GB_MAX_GENERATOR_PROGRAM_TARGETS: u32 = 1024;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct gb_circuit_config {
    pub field: u32,
    pub degree_bits: u32,
    pub num_wires: u32,
    pub num_routed_wires: u32,
    pub num_constants: u32,
    pub num_challenges: u32,
    pub max_quotient_degree_factor: u32,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub proof_of_work_bits: u32,
    pub num_query_rounds: u32,
    pub arity_bits: u32,
    pub final_poly_bits: u32,
    pub num_selectors: u32,
    pub gate_constant: u32,
    pub gate_pi: u32,
    /// CircuitConfig.zero_knowledge (= FriParams.hiding): salted wires / Zs / quotient leaves
    pub zero_knowledge: u32,
    /// CommonCircuitData.num_public_inputs: proofs carrying any other count are rejected (plonk/validate_shape.rs:22-25)
    pub num_public_inputs: u32,
}

/// One generator of prover_only.generators as a record (include/goldibear_gpu.h: gb_generator, GB_GEN_*): a gate generator by
/// (gate index, row, operation / copy / constant index), a CopyGenerator by (source target, destination target).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct gb_generator {
    pub kind: u32,
    pub gate: u32,
    pub a: u64,
    pub b: u64,
}

/// A gadget generator (GB_GEN_EQUALITY .. GB_GEN_BASE_SUM) appended to `out` as its head record - `param` is the generator's
/// parameter (num_limbs, n_log, the base; 0 where it has none), `a` the number of targets - and ceil(targets.len() / 2)
/// GB_GEN_TARGETS continuation records of two `Target::index` values each, in the order include/goldibear_gpu.h lists them for
/// the kind.  Returns the head's index, which is the record index the library's error messages name.
pub fn push_gadget_generator(out: &mut Vec<gb_generator>, kind: u32, param: u32, targets: &[usize]) -> usize {
    let head = out.len();
    out.push(gb_generator { kind, gate: param, a: targets.len() as u64, b: 0 });
    for pair in targets.chunks(2) {
        out.push(gb_generator { kind: GB_GEN_TARGETS, gate: 0, a: pair[0] as u64, b: pair.get(1).map_or(0, |&t| t as u64) });
    }
    head
}

/// One program generator (GB_GEN_PROGRAM): a head record - the index of its generator program (`set_generator_programs`), the
/// number of targets and the row whose constants the program reads (0 for a program without constants) - and the continuation
/// records: the program's `num_in` dependencies, then its `num_out` outputs, as `Target::index` values.  Returns the head's
/// index, which is the record index the library's error messages name.
pub fn push_program_generator(out: &mut Vec<gb_generator>, program: u32, row: usize, dependencies: &[usize], outputs: &[usize]) -> usize {
    let targets: Vec<usize> = dependencies.iter().chain(outputs.iter()).copied().collect();
    let head = push_gadget_generator(out, GB_GEN_PROGRAM, program, &targets);
    out[head].b = row as u64;
    head
}

/// `gb_circuit_generators_info`
#[derive(Clone, Copy, Debug, Default)]
pub struct GeneratorsInfo {
    pub num_levels: u32,
    pub num_launches: u32,
    pub num_unrunnable: u32,
    pub num_checks: u32,
    pub num_classes: u32,
}

/// One entry of CommonCircuitData.gates with selectors_info flattened in (include/goldibear_gpu.h: gb_gate, GB_GATE_*).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct gb_gate {
    pub kind: u32,
    pub param: u32,
    pub selector_index: u32,
    pub group_start: u32,
    pub group_end: u32,
    pub param2: u32,
    pub param3: u32,
}

/// One entry of the witness check's list (include/goldibear_gpu.h: gb_violation).  `kind` is GB_VIOLATION_GATE (gate, row,
/// index = first failing constraint, value), GB_VIOLATION_SELECTOR (row, index = selector column, value) or GB_VIOLATION_COPY
/// (row, index = wire, value; other_row, other_wire, other_value: the first cell of the class).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gb_violation {
    pub kind: u32,
    pub gate: u32,
    pub row: u64,
    pub index: u32,
    pub other_wire: u32,
    pub other_row: u64,
    pub value: u64,
    pub other_value: u64,
}

/// The counts of a witness check (include/goldibear_gpu.h: gb_check_result): exact whatever the list's capacity.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gb_check_result {
    pub num_gate_violations: u64,
    pub num_selector_violations: u64,
    pub num_copy_violations: u64,
    pub copies_checked: u32,
    pub num_listed: u32,
}

/// What `decode_sigmas` found (include/goldibear_gpu.h: gb_sigma_info): the copy permutation's cycles as copy classes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gb_sigma_info {
    pub routed_cells: u64,
    pub moved_cells: u64,
    pub num_classes: u64,
    pub largest_class: u64,
    pub rounds: u32,
    pub compared_partition: u32,
}

/// What `wiring_sigmas` made (include/goldibear_gpu.h: gb_wiring_info).  `rounds` is a diagnostic that depends on the device's schedule.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gb_wiring_info {
    pub routed_cells: u64,
    pub moved_cells: u64,
    pub num_classes: u64,
    pub largest_class: u64,
    pub merged_targets: u64,
    pub rounds: u32,
    pub reserved: u32,
}

/// The sigma columns ([num_routed_wires][2^degree_bits], canonical), the representative map and the counts.
#[derive(Clone, Debug, Default)]
pub struct Wiring<W> {
    pub sigmas: Vec<W>,
    pub representative_map: Vec<u64>,
    pub info: gb_wiring_info,
}

/// What a witness check found: the first `max_violations` violations in the header's order, and the counts.
#[derive(Clone, Debug, Default)]
pub struct CheckOutcome {
    pub violations: Vec<gb_violation>,
    pub result: gb_check_result,
}
impl CheckOutcome {
    pub fn satisfied(&self) -> bool {
        self.result.num_gate_violations + self.result.num_selector_violations + self.result.num_copy_violations == 0
    }
}

/// Challenger<F, H> by value (iop/challenger.rs:18-31) for `gb_prove_openings`: canonical values as u64 for either field;
/// challenges pop from the END of `output_buffer`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct gb_challenger_state {
    pub sponge_state: [u64; 16],
    pub input_buffer: [u64; 8],
    pub output_buffer: [u64; 8],
    pub input_len: u32,
    pub output_len: u32,
}

/// One proof's outcome of `gb_verify_batch`: `status` is what `gb_verify` returns for it, `check` the `GB_VCHECK_*` it names.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gb_verify_result {
    pub status: u32,
    pub check: u32,
    pub query_round: u32,
    pub index: u32,
}

impl gb_verify_result {
    /// the text `gb_verify` leaves in `gb_last_error` for this result's check ("" when the proof verified)
    pub fn text(&self) -> String {
        unsafe { CStr::from_ptr(gb_verify_check_text(self.check)) }.to_string_lossy().into_owned()
    }
}

/// How the words of a host matrix encode field elements (`flags` of the entry points that take matrices).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Repr {
    /// canonical values (`as_canonical_u64()` / `as_canonical_u32()`)
    Canonical,
    /// the reference's field types as they lie in memory (`GB_INPUT_P3_REPR`): `transmute`-compatible with `Vec<F>`
    P3InMemory,
}
impl Repr {
    fn flags(self) -> u32 {
        match self {
            Repr::Canonical => GB_INPUT_HOST,
            Repr::P3InMemory => GB_INPUT_HOST | GB_INPUT_P3_REPR,
        }
    }
}

extern "C" {
    fn gb_ctx_create(device: i32, out: *mut *mut gb_ctx) -> i32;
    fn gb_ctx_destroy(ctx: *mut gb_ctx) -> i32;
    fn gb_last_error(ctx: *const gb_ctx) -> *const c_char;
    fn gb_ctx_set_option(ctx: *mut gb_ctx, key: *const c_char, value: i64) -> i32;
    fn gb_host_alloc(ctx: *mut gb_ctx, bytes: usize, out: *mut *mut c_void) -> i32;
    fn gb_host_free(ctx: *mut gb_ctx, p: *mut c_void) -> i32;
    fn gb_host_register(ctx: *mut gb_ctx, p: *mut c_void, bytes: usize) -> i32;
    fn gb_host_unregister(ctx: *mut gb_ctx, p: *mut c_void) -> i32;
    fn gb_commit_values_cols(ctx: *mut gb_ctx, field: u32, cols: *const *const c_void, ncols: usize, log_n: u32, rate_bits: u32,
                             cap_height: u32, salts: *const c_void, flags: u32, out: *mut *mut gb_batch) -> i32;
    fn gb_commit_coeffs_cols(ctx: *mut gb_ctx, field: u32, cols: *const *const c_void, ncols: usize, log_n: u32, rate_bits: u32,
                             cap_height: u32, salts: *const c_void, flags: u32, out: *mut *mut gb_batch) -> i32;
    fn gb_prove_cols(c: *mut gb_circuit, wire_cols: *const *const c_void, flags: u32, public_inputs: *const u64,
                     num_public_inputs: usize, proof_out: *mut c_void, proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_prove_retry_cols(c: *mut gb_circuit, wire_cols: *const *const c_void, flags: u32, wire: u32, row: u64,
                           public_inputs: *const u64, num_public_inputs: usize, proof_out: *mut c_void, proof_cap: usize,
                           proof_len: *mut usize) -> i32;
    fn gb_prove_salted_cols(c: *mut gb_circuit, wire_cols: *const *const c_void, flags: u32, public_inputs: *const u64,
                            num_public_inputs: usize, salts: *const c_void, proof_out: *mut c_void, proof_cap: usize,
                            proof_len: *mut usize) -> i32;
    fn gb_zs_partial_products_cols(c: *mut gb_circuit, wire_cols: *const *const c_void, flags: u32, betas: *const c_void,
                                   gammas: *const c_void, values_out: *mut c_void) -> i32;
    fn gb_circuit_set_partition(c: *mut gb_circuit, representative_map: *const u64, num_targets: u64,
                                public_input_targets: *const u64, num_public_inputs: usize) -> i32;
    fn gb_prove_partition(c: *mut gb_circuit, values: *const c_void, flags: u32, salts: *const c_void, proof_out: *mut c_void,
                          proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_prove_partition_retry(c: *mut gb_circuit, values: *const c_void, flags: u32, wire: u32, row: u64, proof_out: *mut c_void,
                                proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_expand_partition(c: *mut gb_circuit, values: *const c_void, flags: u32, witness_dev_out: *mut c_void) -> i32;
    fn gb_circuit_set_generators(c: *mut gb_circuit, generators: *const c_void, num_generators: u64, input_targets: *const u64,
                                 num_inputs: u64, constants: *const u64, flags: u32) -> i32;
    fn gb_circuit_set_generator_programs(c: *mut gb_circuit, program_words: *const u64, program_offsets: *const u32,
                                         num_programs: u32) -> i32;
    fn gb_circuit_generators_info(c: *mut gb_circuit, num_levels: *mut u32, num_launches: *mut u32, num_unrunnable: *mut u32,
                                  num_checks: *mut u32, num_classes: *mut u32) -> i32;
    fn gb_circuit_generator_classes(c: *mut gb_circuit, class_targets_out: *mut u64, capacity: u64) -> i32;
    fn gb_generate_partition(c: *mut gb_circuit, input_values: *const c_void, flags: u32, values_dev_out: *mut c_void) -> i32;
    fn gb_prove_inputs(c: *mut gb_circuit, input_values: *const c_void, flags: u32, salts: *const c_void, proof_out: *mut c_void,
                       proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_prove_inputs_retry(c: *mut gb_circuit, input_values: *const c_void, flags: u32, wire: u32, row: u64, proof_out: *mut c_void,
                             proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_check_witness(c: *mut gb_circuit, witness: *const c_void, flags: u32, public_inputs: *const u64, num_public_inputs: usize,
                        violations_out: *mut c_void, capacity: usize, result: *mut c_void) -> i32;
    fn gb_check_partition(c: *mut gb_circuit, values: *const c_void, flags: u32, violations_out: *mut c_void, capacity: usize,
                          result: *mut c_void) -> i32;
    fn gb_check_inputs(c: *mut gb_circuit, input_values: *const c_void, flags: u32, violations_out: *mut c_void, capacity: usize,
                       result: *mut c_void) -> i32;
    fn gb_circuit_decode_sigmas(c: *mut gb_circuit, flags: u32, info: *mut c_void) -> i32;
    fn gb_circuit_copy_classes(c: *mut gb_circuit, first_cell_out: *mut u32) -> i32;
    fn gb_wiring_sigmas(ctx: *mut gb_ctx, field: u32, degree_bits: u32, num_wires: u32, num_routed_wires: u32, k_is: *const c_void,
                        copy_constraints: *const u64, num_copies: u64, num_targets: u64, flags: u32, sigmas_out: *mut c_void,
                        representative_map_out: *mut u64, info: *mut c_void) -> i32;
    fn gb_commit_values(ctx: *mut gb_ctx, field: u32, cols: *const c_void, ncols: usize, log_n: u32, rate_bits: u32,
                        cap_height: u32, salts: *const c_void, flags: u32, out: *mut *mut gb_batch) -> i32;
    fn gb_commit_coeffs(ctx: *mut gb_ctx, field: u32, cols: *const c_void, ncols: usize, log_n: u32, rate_bits: u32,
                        cap_height: u32, salts: *const c_void, flags: u32, out: *mut *mut gb_batch) -> i32;
    fn gb_batch_free(b: *mut gb_batch) -> i32;
    fn gb_batch_cap(b: *mut gb_batch, out: *mut c_void) -> i32;
    fn gb_batch_coeffs(b: *mut gb_batch, col: usize, out: *mut c_void) -> i32;
    fn gb_batch_lde_values(b: *mut gb_batch, index: u64, step: u64, out: *mut c_void) -> i32;
    fn gb_batch_leaf(b: *mut gb_batch, leaf_index: u64, row: *mut c_void, siblings: *mut c_void, nsib: *mut u32) -> i32;
    fn gb_batch_eval_ext(b: *mut gb_batch, z: *const c_void, out: *mut c_void) -> i32;
    fn gb_circuit_create(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, constants_sigmas: *const c_void, k_is: *const c_void,
                         flags: u32, out: *mut *mut gb_circuit) -> i32;
    fn gb_circuit_create_cols(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, constants_sigmas_cols: *const *const c_void,
                              k_is: *const c_void, flags: u32, out: *mut *mut gb_circuit) -> i32;
    fn gb_circuit_create_gates_cols(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32,
                                    constants_sigmas_cols: *const *const c_void, k_is: *const c_void, flags: u32,
                                    out: *mut *mut gb_circuit) -> i32;
    fn gb_circuit_create_programs(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32,
                                  program_words: *const u64, program_offsets: *const u32, num_programs: u32,
                                  constants_sigmas: *const c_void, k_is: *const c_void, flags: u32, out: *mut *mut gb_circuit) -> i32;
    fn gb_circuit_create_programs_cols(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32,
                                       program_words: *const u64, program_offsets: *const u32, num_programs: u32,
                                       constants_sigmas_cols: *const *const c_void, k_is: *const c_void, flags: u32,
                                       out: *mut *mut gb_circuit) -> i32;
    fn gb_circuit_free(c: *mut gb_circuit) -> i32;
    fn gb_circuit_verifier_data(c: *mut gb_circuit, cap_out: *mut c_void, digest_out: *mut c_void) -> i32;
    fn gb_circuit_set_fri_reduction_arity_bits(c: *mut gb_circuit, arity_bits: *const u32, num_layers: u32) -> i32;
    fn gb_circuit_fri_reduction_arity_bits(c: *mut gb_circuit, arity_bits_out: *mut u32, num_layers_out: *mut u32) -> i32;
    fn gb_prove(c: *mut gb_circuit, witness: *const c_void, flags: u32, public_inputs: *const u64, num_public_inputs: usize,
                proof_out: *mut c_void, proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_verify(c: *mut gb_circuit, proof: *const c_void, proof_len: usize) -> i32;
    fn gb_verify_batch(ctx: *mut gb_ctx, c: *mut gb_circuit, proofs: *const *const c_void, proof_lens: *const usize, num_proofs: u32,
                       flags: u32, results: *mut c_void) -> i32;
    fn gb_verify_check_text(check: u32) -> *const c_char;
    fn gb_verify_compressed_batch(ctx: *mut gb_ctx, c: *mut gb_circuit, proofs: *const *const c_void, proof_lens: *const usize,
                                  num_proofs: u32, flags: u32, results: *mut c_void) -> i32;
    fn gb_circuit_constants_sigmas_commitment(c: *mut gb_circuit, out: *mut *mut gb_batch) -> i32;
    fn gb_zs_partial_products(c: *mut gb_circuit, witness: *const c_void, flags: u32, betas: *const c_void, gammas: *const c_void,
                              values_out: *mut c_void) -> i32;
    fn gb_quotient_polys(c: *mut gb_circuit, wires: *mut gb_batch, zs_partial_products: *mut gb_batch,
                         public_inputs_hash: *const c_void, betas: *const c_void, gammas: *const c_void, alphas: *const c_void,
                         flags: u32, chunks_out: *mut c_void) -> i32;
    fn gb_prove_openings(c: *mut gb_circuit, wires: *mut gb_batch, zs_partial_products: *mut gb_batch, quotient: *mut gb_batch,
                         zeta: *const c_void, challenger: *mut gb_challenger_state, fri_proof_out: *mut c_void,
                         fri_proof_cap: usize, fri_proof_len: *mut usize) -> i32;
    fn gb_fri_prove_openings(ctx: *mut gb_ctx, oracles: *const *mut gb_batch, num_oracles: u32, points: *const c_void,
                             batch_sizes: *const u32, num_batches: u32, polynomials: *const u32, reduction_arity_bits: *const u32,
                             num_layers: u32, proof_of_work_bits: u32, num_query_rounds: u32, challenger: *mut gb_challenger_state,
                             fri_proof_out: *mut c_void, fri_proof_cap: usize, fri_proof_len: *mut usize) -> i32;
    fn gb_fri_verify(ctx: *mut gb_ctx, field: u32, degree_bits: u32, rate_bits: u32, cap_height: u32, hiding: u32,
                     oracle_num_polys: *const u32, oracle_blinding: *const u32, num_oracles: u32, points: *const c_void,
                     batch_sizes: *const u32, num_batches: u32, polynomials: *const u32, openings: *const c_void,
                     initial_caps: *const c_void, reduction_arity_bits: *const u32, num_layers: u32, proof_of_work_bits: u32,
                     num_query_rounds: u32, challenger: *const gb_challenger_state, fri_proof: *const c_void, fri_proof_len: usize) -> i32;
    fn gb_fri_verify_batch(ctx: *mut gb_ctx, field: u32, degree_bits: u32, rate_bits: u32, cap_height: u32, hiding: u32,
                           oracle_num_polys: *const u32, oracle_blinding: *const u32, num_oracles: u32, batch_sizes: *const u32,
                           num_batches: u32, polynomials: *const u32, reduction_arity_bits: *const u32, num_layers: u32,
                           proof_of_work_bits: u32, num_query_rounds: u32, points: *const *const c_void, openings: *const *const c_void,
                           initial_caps: *const *const c_void, challengers: *const gb_challenger_state,
                           fri_proofs: *const *const c_void, fri_proof_lens: *const usize, num_items: u32, flags: u32,
                           results: *mut c_void) -> i32;
    fn gb_fri_verify_batch_counts(ctx: *mut gb_ctx, device_items: *mut u64, host_items: *mut u64) -> i32;
    fn gb_constraint_quotient(ctx: *mut gb_ctx, oracles: *const *mut gb_batch, num_oracles: u32, program_words: *const u64,
                              program_offsets: *const u32, num_programs: u32, params: *const c_void, num_params: u32,
                              alphas: *const c_void, num_challenges: u32, quotient_degree_bits: u32, flags: u32,
                              chunks_out: *mut c_void) -> i32;
    fn gb_constraint_eval(ctx: *mut gb_ctx, field: u32, degree_bits: u32, program_words: *const u64, program_offsets: *const u32,
                          num_programs: u32, cell_values: *const c_void, params: *const c_void, num_params: u32,
                          zeta: *const c_void, alphas: *const c_void, num_challenges: u32, folded_out: *mut c_void) -> i32;
    fn gb_circuit_create_gates(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32,
                               constants_sigmas: *const c_void, k_is: *const c_void, flags: u32, out: *mut *mut gb_circuit) -> i32;
    fn gb_prove_retry(c: *mut gb_circuit, witness: *const c_void, flags: u32, wire: u32, row: u64, public_inputs: *const u64,
                      num_public_inputs: usize, proof_out: *mut c_void, proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_circuit_drop_retry(c: *mut gb_circuit) -> i32;
    fn gb_prove_salted(c: *mut gb_circuit, witness: *const c_void, flags: u32, public_inputs: *const u64, num_public_inputs: usize,
                       salts: *const c_void, proof_out: *mut c_void, proof_cap: usize, proof_len: *mut usize) -> i32;
    fn gb_random_elements(ctx: *mut gb_ctx, field: u32, seed: *const u8, nonce: *const u32, first_element: u64, count: u64, flags: u32,
                          out: *mut c_void) -> i32;
    fn gb_verifier_create(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32, k_is: *const c_void,
                          constants_sigmas_cap: *const c_void, circuit_digest: *const c_void, out: *mut *mut gb_circuit) -> i32;
    fn gb_verifier_create_programs(ctx: *mut gb_ctx, cfg: *const gb_circuit_config, gates: *const gb_gate, num_gates: u32,
                                   program_words: *const u64, program_offsets: *const u32, num_programs: u32, k_is: *const c_void,
                                   constants_sigmas_cap: *const c_void, circuit_digest: *const c_void, out: *mut *mut gb_circuit) -> i32;
    fn gb_verify_compressed(c: *mut gb_circuit, compressed: *const c_void, len: usize) -> i32;
    fn gb_proof_compress(c: *mut gb_circuit, proof: *const c_void, len: usize, out: *mut c_void, cap: usize, out_len: *mut usize) -> i32;
    fn gb_proof_decompress(c: *mut gb_circuit, compressed: *const c_void, len: usize, out: *mut c_void, cap: usize,
                           out_len: *mut usize) -> i32;
    fn gb_fft(ctx: *mut gb_ctx, field: u32, coeffs: *const c_void, values: *mut c_void, ncols: usize, log_n: u32, rate_bits: u32,
              ext: u32, shift: *const c_void, flags: u32) -> i32;
    fn gb_ifft(ctx: *mut gb_ctx, field: u32, values: *const c_void, coeffs: *mut c_void, ncols: usize, log_n: u32, ext: u32,
               shift: *const c_void, flags: u32) -> i32;
    fn gb_lde(ctx: *mut gb_ctx, field: u32, values: *const c_void, out: *mut c_void, ncols: usize, log_n: u32, rate_bits: u32,
              ext: u32, shift: *const c_void, flags: u32) -> i32;
    // a gb_merkle_tree is a gb_batch without polynomials (`typedef struct gb_batch gb_merkle_tree;`)
    fn gb_merkle_tree_create(ctx: *mut gb_ctx, field: u32, leaves: *const c_void, log_leaves: u32, leaf_len: u32, cap_height: u32,
                             flags: u32, out: *mut *mut gb_batch) -> i32;
    fn gb_merkle_tree_free(tree: *mut gb_batch) -> i32;
    fn gb_merkle_tree_info(tree: *const gb_batch, field: *mut u32, log_leaves: *mut u32, leaf_len: *mut u32, cap_height: *mut u32) -> i32;
    fn gb_merkle_tree_cap(tree: *mut gb_batch, out: *mut c_void) -> i32;
    fn gb_merkle_tree_leaf(tree: *mut gb_batch, leaf_index: u64, row: *mut c_void, siblings: *mut c_void, nsib: *mut u32) -> i32;
    fn gb_merkle_tree_digests(tree: *mut gb_batch, out: *mut c_void) -> i32;
}

/// Status code + the library's message.
#[derive(Debug)]
pub struct GpuError {
    pub status: i32,
    pub message: String,
}

/// The library reads fixed element counts through the raw pointers it is given: a safe wrapper checks the slice first.
fn need(what: &str, have: usize, want: usize) -> Result<(), GpuError> {
    if have == want {
        return Ok(());
    }
    Err(GpuError { status: GB_ERR_INVALID, message: format!("{what}: {have} elements, the circuit configuration needs {want}") })
}

fn check(ctx: *const gb_ctx, status: i32) -> Result<(), GpuError> {
    if status == GB_OK {
        return Ok(());
    }
    let p = unsafe { gb_last_error(ctx) };
    let message = if p.is_null() { String::new() } else { unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned() };
    Err(GpuError { status, message })
}

/// One per HIP device; calls on a context are serialised by the caller (the prover thread).
pub struct GpuContext(*mut gb_ctx);
unsafe impl Send for GpuContext {}

impl GpuContext {
    pub fn new(device: i32) -> Result<Self, GpuError> {
        let mut h = ptr::null_mut();
        check(ptr::null(), unsafe { gb_ctx_create(device, &mut h) })?;
        Ok(GpuContext(h))
    }
    /// Tuning / debugging switches (`gb_ctx_set_option`): "copy_threads", "retry_verify", ...; none changes a result.
    pub fn set_option(&self, key: &str, value: i64) -> Result<(), GpuError> {
        let k = std::ffi::CString::new(key).map_err(|_| GpuError { status: GB_ERR_INVALID, message: "key holds a NUL".into() })?;
        check(self.0, unsafe { gb_ctx_set_option(self.0, k.as_ptr(), value) })
    }
    /// Page-locked memory for `len` words (hipHostMalloc): columns built here go to the copy engine without the library's staging
    /// copy.  The natural use is an allocator for the witness columns (`MatrixWitness.wire_values`).
    pub fn host_alloc<W: Copy + Default>(&self, len: usize) -> Result<PinnedBuf<'_, W>, GpuError> {
        let mut p = ptr::null_mut();
        check(self.0, unsafe { gb_host_alloc(self.0, len * std::mem::size_of::<W>(), &mut p) })?;
        let buf = PinnedBuf { ctx: self, ptr: p as *mut W, len };
        unsafe { std::slice::from_raw_parts_mut(buf.ptr, len) }.fill(W::default());
        Ok(buf)
    }
    /// Page-lock an existing buffer in place (hipHostRegister) for as long as the guard lives; pays for buffers that are reused.
    pub fn host_register<'a, W>(&'a self, buf: &'a mut [W]) -> Result<Registered<'a, W>, GpuError> {
        check(self.0, unsafe { gb_host_register(self.0, buf.as_mut_ptr() as *mut c_void, std::mem::size_of_val(buf)) })?;
        Ok(Registered { ctx: self, buf })
    }
}
/// `len` words of page-locked host memory owned by the library's allocator (`gb_host_alloc` / `gb_host_free`).
pub struct PinnedBuf<'c, W> {
    ctx: &'c GpuContext,
    ptr: *mut W,
    len: usize,
}
impl<'c, W> std::ops::Deref for PinnedBuf<'c, W> {
    type Target = [W];
    fn deref(&self) -> &[W] {
        unsafe { std::slice::from_raw_parts(self.ptr, self.len) }
    }
}
impl<'c, W> std::ops::DerefMut for PinnedBuf<'c, W> {
    fn deref_mut(&mut self) -> &mut [W] {
        unsafe { std::slice::from_raw_parts_mut(self.ptr, self.len) }
    }
}
impl<'c, W> Drop for PinnedBuf<'c, W> {
    fn drop(&mut self) {
        unsafe { gb_host_free(self.ctx.0, self.ptr as *mut c_void) };
    }
}
/// A caller's buffer page-locked in place (`gb_host_register`); unregistered on drop.
pub struct Registered<'a, W> {
    ctx: &'a GpuContext,
    buf: &'a mut [W],
}
impl<'a, W> std::ops::Deref for Registered<'a, W> {
    type Target = [W];
    fn deref(&self) -> &[W] {
        self.buf
    }
}
impl<'a, W> std::ops::DerefMut for Registered<'a, W> {
    fn deref_mut(&mut self) -> &mut [W] {
        self.buf
    }
}
impl<'a, W> Drop for Registered<'a, W> {
    fn drop(&mut self) {
        unsafe { gb_host_unregister(self.ctx.0, self.buf.as_mut_ptr() as *mut c_void) };
    }
}

/// The pointer table of the `*_cols` entry points: one pointer per separately allocated column, every column `n` words long.
/// Nothing is copied: `columns[i]` is `values[i].values.as_slice()` / `witness.wire_values[i].as_slice()`.
fn column_table<W, C: AsRef<[W]>>(what: &str, columns: &[C], n: usize) -> Result<Vec<*const c_void>, GpuError> {
    let mut table = Vec::with_capacity(columns.len());
    for (i, c) in columns.iter().enumerate() {
        need(&format!("{what}[{i}]"), c.as_ref().len(), n)?;
        table.push(c.as_ref().as_ptr() as *const c_void);
    }
    Ok(table)
}
impl Drop for GpuContext {
    fn drop(&mut self) {
        unsafe { gb_ctx_destroy(self.0) };
    }
}

/// The reference's transforms on slices (field/src/polynomial/mod.rs): `PolynomialCoeffs::fft` / `coset_fft` (after `.lde(rate_bits)`),
/// `PolynomialValues::ifft` / `coset_ifft` / `lde` / `lde_onto_coset`.  `data` holds `num_polys` polynomials laid end to end, natural
/// order, canonical words (`W` = `u64` Goldilocks / `u32` BabyBear) or, with `Repr::P3InMemory`, the field type's own words; with
/// `ext` every element is D consecutive words (`PolynomialCoeffs<F::Extension>`).  `shift`: `None`, or a canonical base-field element.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Transform {
    Fft,
    Ifft,
    Lde,
}
impl GpuContext {
    /// Elements `first .. first + count` of the keyed stream (seed, nonce) as canonical words (`gb_random_elements`): ChaCha20
    /// blocks under `seed` with counter e >> 2 and the three nonce words, each 128-bit quarter reduced mod p; computed on the device.
    pub fn random_elements<W: Copy + Default>(&self, seed: &[u8; GB_SEED_SIZE], nonce: [u32; 3], first: u64, count: usize)
                                              -> Result<Vec<W>, GpuError> {
        let mut out = vec![W::default(); count.max(1)];
        check(self.0, unsafe {
            gb_random_elements(self.0, field_tag::<W>(), seed.as_ptr(), nonce.as_ptr(), first, count as u64, GB_INPUT_HOST,
                               out.as_mut_ptr() as *mut c_void)
        })?;
        out.truncate(count);
        Ok(out)
    }
    fn poly_shape<W>(len: usize, num_polys: usize, ext: bool) -> Result<u32, GpuError> {
        let d = if !ext { 1 } else if std::mem::size_of::<W>() == 8 { 2 } else { 4 };
        if num_polys == 0 || len % (num_polys * d) != 0 || !(len / (num_polys * d)).is_power_of_two() {
            return Err(GpuError { status: GB_ERR_INVALID, message: "polynomial length must be a power of two".into() });
        }
        Ok((len / (num_polys * d)).trailing_zeros())
    }
    /// One transform into a fresh vector of `len << rate_bits` words (`rate_bits` is ignored by `Transform::Ifft`).
    pub fn transform<W: Copy + Default>(&self, op: Transform, data: &[W], num_polys: usize, rate_bits: u32, ext: bool, shift: Option<W>,
                                        repr: Repr) -> Result<Vec<W>, GpuError> {
        let log_n = Self::poly_shape::<W>(data.len(), num_polys, ext)?;
        let rate_bits = if op == Transform::Ifft { 0 } else { rate_bits };
        let mut out = vec![W::default(); data.len() << rate_bits];
        let sp = shift.as_ref().map_or(ptr::null(), |s| s as *const W as *const c_void);
        let (src, dst, f) = (data.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void, field_tag::<W>());
        check(self.0, unsafe {
            match op {
                Transform::Fft => gb_fft(self.0, f, src, dst, num_polys, log_n, rate_bits, ext as u32, sp, repr.flags()),
                Transform::Ifft => gb_ifft(self.0, f, src, dst, num_polys, log_n, ext as u32, sp, repr.flags()),
                Transform::Lde => gb_lde(self.0, f, src, dst, num_polys, log_n, rate_bits, ext as u32, sp, repr.flags()),
            }
        })?;
        Ok(out)
    }
    /// `fft` / `coset_fft` / `ifft` / `coset_ifft` in place, as the reference consumes `self` (canonical words in, canonical out).
    pub fn transform_in_place<W: Copy + Default>(&self, op: Transform, data: &mut [W], num_polys: usize, ext: bool, shift: Option<W>)
                                                 -> Result<(), GpuError> {
        let log_n = Self::poly_shape::<W>(data.len(), num_polys, ext)?;
        let sp = shift.as_ref().map_or(ptr::null(), |s| s as *const W as *const c_void);
        let (p, f) = (data.as_mut_ptr() as *mut c_void, field_tag::<W>());
        check(self.0, unsafe {
            match op {
                Transform::Ifft => gb_ifft(self.0, f, p, p, num_polys, log_n, ext as u32, sp, GB_INPUT_HOST),
                Transform::Fft => gb_fft(self.0, f, p, p, num_polys, log_n, 0, ext as u32, sp, GB_INPUT_HOST),
                Transform::Lde => gb_lde(self.0, f, p, p, num_polys, log_n, 0, ext as u32, sp, GB_INPUT_HOST),
            }
        })
    }
}

impl GpuContext {
    /// "generate sigma polynomials" of `CircuitBuilder::build` (plonk/circuit_builder.rs:1005-1040) on the device: the copy
    /// constraints as pairs of `Target::index` -> sigma columns on H and a representative map (the lowest index of every class).
    /// `k_is`: one canonical word per routed wire; `num_targets`: `degree * num_wires + virtual targets`.
    pub fn wiring_sigmas<W: Copy + Default>(&self, degree_bits: u32, num_wires: u32, k_is: &[W], copy_constraints: &[[u64; 2]],
                                            num_targets: u64) -> Result<Wiring<W>, GpuError> {
        let routed = k_is.len() << degree_bits;
        let mut out = Wiring { sigmas: vec![W::default(); routed], representative_map: vec![0u64; num_targets as usize],
                               info: gb_wiring_info::default() };
        check(self.0, unsafe {
            gb_wiring_sigmas(self.0, field_tag::<W>(), degree_bits, num_wires, k_is.len() as u32, k_is.as_ptr() as *const c_void,
                             copy_constraints.as_ptr() as *const u64, copy_constraints.len() as u64, num_targets, GB_INPUT_HOST,
                             out.sigmas.as_mut_ptr() as *mut c_void, out.representative_map.as_mut_ptr(),
                             &mut out.info as *mut gb_wiring_info as *mut c_void)
        })?;
        Ok(out)
    }
}

/// `MerkleTree::new(leaves, cap_height)` (hash/merkle_tree.rs:152-181) with the leaves and digests resident on the GPU.
pub struct GpuMerkleTree<'c, W> {
    ctx: &'c GpuContext,
    handle: *mut gb_batch,
    pub log_leaves: u32,
    pub leaf_len: u32,
    pub cap_height: u32,
    _w: std::marker::PhantomData<W>,
}
impl<'c, W: Copy + Default> GpuMerkleTree<'c, W> {
    /// `leaves`: the rows laid end to end ([num_leaves][leaf_len], every leaf `leaf_len` words)
    pub fn new(ctx: &'c GpuContext, leaves: &[W], leaf_len: usize, cap_height: u32, repr: Repr) -> Result<Self, GpuError> {
        if leaf_len == 0 || leaves.len() % leaf_len != 0 || !(leaves.len() / leaf_len).is_power_of_two() {
            return Err(GpuError { status: GB_ERR_INVALID, message: "the number of leaves must be a power of two".into() });
        }
        let log_leaves = (leaves.len() / leaf_len).trailing_zeros();
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_merkle_tree_create(ctx.0, field_tag::<W>(), leaves.as_ptr() as *const c_void, log_leaves, leaf_len as u32, cap_height,
                                  repr.flags(), &mut h)
        })?;
        let (mut f, mut ll, mut w, mut ch) = (0u32, 0u32, 0u32, 0u32);
        let st = unsafe { gb_merkle_tree_info(h, &mut f, &mut ll, &mut w, &mut ch) };
        let t = Self { ctx, handle: h, log_leaves: ll, leaf_len: w, cap_height: ch, _w: std::marker::PhantomData };
        check(ctx.0, st)?;
        Ok(t)
    }
    fn hash_len() -> usize {
        if std::mem::size_of::<W>() == 8 { 4 } else { 8 }
    }
    /// `.cap`
    pub fn cap(&self) -> Result<Vec<W>, GpuError> {
        let mut out = vec![W::default(); Self::hash_len() << self.cap_height];
        check(self.ctx.0, unsafe { gb_merkle_tree_cap(self.handle, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
    /// `.digests` in the reference's layout (merkle_tree.rs:50-58)
    pub fn digests(&self) -> Result<Vec<W>, GpuError> {
        let count = 2 * ((1usize << self.log_leaves) - (1usize << self.cap_height));
        let mut out = vec![W::default(); count * Self::hash_len()];
        check(self.ctx.0, unsafe { gb_merkle_tree_digests(self.handle, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
    /// `get(i)` and `prove(i)` (merkle_tree.rs:183-222): (leaf, siblings)
    pub fn leaf_and_proof(&self, leaf_index: usize) -> Result<(Vec<W>, Vec<W>), GpuError> {
        let layers = (self.log_leaves - self.cap_height) as usize;
        let mut row = vec![W::default(); self.leaf_len as usize];
        let mut sib = vec![W::default(); layers.max(1) * Self::hash_len()];
        let mut nsib = 0u32;
        check(self.ctx.0, unsafe {
            gb_merkle_tree_leaf(self.handle, leaf_index as u64, row.as_mut_ptr() as *mut c_void, sib.as_mut_ptr() as *mut c_void, &mut nsib)
        })?;
        sib.truncate(nsib as usize * Self::hash_len());
        Ok((row, sib))
    }
}
impl<'c, W> Drop for GpuMerkleTree<'c, W> {
    fn drop(&mut self) {
        unsafe { gb_merkle_tree_free(self.handle) };
    }
}

/// `PolynomialBatch` with coefficients, LDE (leaf order) and Merkle digests resident on the GPU (fri/oracle.rs:29-40).
/// `W` is the canonical word type: `u64` for Goldilocks, `u32` for BabyBear.
pub struct GpuPolynomialBatch<'c, W> {
    ctx: &'c GpuContext,
    handle: *mut gb_batch,
    pub num_polys: usize,
    pub degree_log: u32,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub blinding: bool,
    _w: std::marker::PhantomData<W>,
}

fn field_tag<W>() -> u32 {
    if std::mem::size_of::<W>() == 8 { GB_GOLDILOCKS } else { GB_BABYBEAR }
}

impl<'c, W: Copy + Default> GpuPolynomialBatch<'c, W> {
    /// `PolynomialBatch::from_values` (oracle.rs:68-90): `values` = the columns laid end to end ([ncols][n]);
    /// `salts` = [4][n << rate_bits] when blinding.
    pub fn from_values(ctx: &'c GpuContext, values: &[W], num_polys: usize, rate_bits: u32, cap_height: u32,
                       salts: Option<&[W]>) -> Result<Self, GpuError> {
        Self::commit(ctx, values, num_polys, rate_bits, cap_height, salts, false)
    }
    /// `PolynomialBatch::from_coeffs` (oracle.rs:93-123)
    pub fn from_coeffs(ctx: &'c GpuContext, coeffs: &[W], num_polys: usize, rate_bits: u32, cap_height: u32,
                       salts: Option<&[W]>) -> Result<Self, GpuError> {
        Self::commit(ctx, coeffs, num_polys, rate_bits, cap_height, salts, true)
    }
    fn commit(ctx: &'c GpuContext, cols: &[W], num_polys: usize, rate_bits: u32, cap_height: u32, salts: Option<&[W]>,
              coeffs: bool) -> Result<Self, GpuError> {
        assert!(num_polys > 0 && cols.len() % num_polys == 0);
        let n = cols.len() / num_polys;
        assert!(n.is_power_of_two());
        let degree_log = n.trailing_zeros();
        let mut h = ptr::null_mut();
        let sp = salts.map_or(ptr::null(), |s| s.as_ptr() as *const c_void);
        let f = if coeffs { gb_commit_coeffs } else { gb_commit_values };
        check(ctx.0, unsafe {
            f(ctx.0, field_tag::<W>(), cols.as_ptr() as *const c_void, num_polys, degree_log, rate_bits, cap_height, sp, GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, num_polys, degree_log, rate_bits, cap_height, blinding: salts.is_some(), _w: std::marker::PhantomData })
    }
    /// `PolynomialBatch::from_values` (oracle.rs:68-90) over `values: Vec<PolynomialValues<F>>` AS IT IS: `columns[i]` =
    /// `values[i].values` - separately allocated, pageable - handed over as a pointer table (`gb_commit_values_cols`).
    pub fn from_value_columns<C: AsRef<[W]>>(ctx: &'c GpuContext, columns: &[C], rate_bits: u32, cap_height: u32, salts: Option<&[W]>,
                                             repr: Repr) -> Result<Self, GpuError> {
        Self::commit_columns(ctx, columns, rate_bits, cap_height, salts, repr, false)
    }
    /// `PolynomialBatch::from_coeffs` (oracle.rs:93-123) over `polynomials: Vec<PolynomialCoeffs<F>>` (`gb_commit_coeffs_cols`)
    pub fn from_coeff_columns<C: AsRef<[W]>>(ctx: &'c GpuContext, columns: &[C], rate_bits: u32, cap_height: u32, salts: Option<&[W]>,
                                             repr: Repr) -> Result<Self, GpuError> {
        Self::commit_columns(ctx, columns, rate_bits, cap_height, salts, repr, true)
    }
    fn commit_columns<C: AsRef<[W]>>(ctx: &'c GpuContext, columns: &[C], rate_bits: u32, cap_height: u32, salts: Option<&[W]>,
                                     repr: Repr, coeffs: bool) -> Result<Self, GpuError> {
        assert!(!columns.is_empty());   // oracle.rs:101
        let n = columns[0].as_ref().len();
        assert!(n.is_power_of_two());
        let degree_log = n.trailing_zeros();
        let table = column_table("columns", columns, n)?;
        if let Some(s) = salts {
            need("salts", s.len(), 4 * (n << rate_bits))?;
        }
        let sp = salts.map_or(ptr::null(), |s| s.as_ptr() as *const c_void);
        let f = if coeffs { gb_commit_coeffs_cols } else { gb_commit_values_cols };
        let mut h = ptr::null_mut();
        // the columns (and salts) are the caller's again when the call returns: the library has staged or uploaded them
        check(ctx.0, unsafe {
            f(ctx.0, field_tag::<W>(), table.as_ptr(), table.len(), degree_log, rate_bits, cap_height, sp, repr.flags(), &mut h)
        })?;
        Ok(Self { ctx, handle: h, num_polys: columns.len(), degree_log, rate_bits, cap_height, blinding: salts.is_some(),
                  _w: std::marker::PhantomData })
    }
    fn hash_len() -> usize {
        if std::mem::size_of::<W>() == 8 { 4 } else { 8 }
    }
    /// `merkle_tree.cap`: 2^cap_height hashes of NUM_HASH_OUT_ELTS words
    pub fn cap(&self) -> Result<Vec<W>, GpuError> {
        let mut out = vec![W::default(); Self::hash_len() << self.cap_height];
        check(self.ctx.0, unsafe { gb_batch_cap(self.handle, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
    /// `.polynomials[col]`
    pub fn polynomial(&self, col: usize) -> Result<Vec<W>, GpuError> {
        let mut out = vec![W::default(); 1usize << self.degree_log];
        check(self.ctx.0, unsafe { gb_batch_coeffs(self.handle, col, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
    /// `get_lde_values(index, step)` (oracle.rs:153-158)
    pub fn get_lde_values(&self, index: usize, step: usize) -> Result<Vec<W>, GpuError> {
        let mut out = vec![W::default(); self.num_polys];
        check(self.ctx.0, unsafe { gb_batch_lde_values(self.handle, index as u64, step as u64, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
    /// `merkle_tree.get(i)` and `merkle_tree.prove(i)` (merkle_tree.rs:183-222): (leaf row incl. salts, siblings)
    pub fn leaf_and_proof(&self, leaf_index: usize) -> Result<(Vec<W>, Vec<W>), GpuError> {
        let width = self.num_polys + if self.blinding { 4 } else { 0 };
        let layers = (self.degree_log + self.rate_bits - self.cap_height) as usize;
        let mut row = vec![W::default(); width];
        let mut sib = vec![W::default(); layers.max(1) * Self::hash_len()];
        let mut nsib = 0u32;
        check(self.ctx.0, unsafe {
            gb_batch_leaf(self.handle, leaf_index as u64, row.as_mut_ptr() as *mut c_void, sib.as_mut_ptr() as *mut c_void, &mut nsib)
        })?;
        sib.truncate(nsib as usize * Self::hash_len());
        Ok((row, sib))
    }
    /// every polynomial at the extension point `z` (D canonical words): plonk/proof.rs:359-363
    pub fn eval_ext(&self, z: &[W]) -> Result<Vec<W>, GpuError> {
        let d = z.len();
        let mut out = vec![W::default(); self.num_polys * d];
        check(self.ctx.0, unsafe { gb_batch_eval_ext(self.handle, z.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }
}
impl<'c, W> Drop for GpuPolynomialBatch<'c, W> {
    fn drop(&mut self) {
        unsafe { gb_batch_free(self.handle) };
    }
}

/// `FriInstanceInfo` (fri/structure.rs) as slices: `oracles[i]` = (`FriOracleInfo.num_polys`, `.blinding`); batch `b` opens
/// `polynomials[b]` = its `FriPolynomialInfo`s as (oracle_index, polynomial_index), in order, at `points[b * D .. (b + 1) * D]`.
pub struct FriInstance<'a, W> {
    pub oracles: &'a [(usize, bool)],
    pub points: &'a [W],
    pub polynomials: &'a [&'a [(usize, usize)]],
}
/// What `fri_proof` and `verify_fri_proof` read of `FriParams` (fri/mod.rs:71-86)
pub struct FriParams<'a> {
    pub degree_bits: u32,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub hiding: bool,
    pub proof_of_work_bits: u32,
    pub num_query_rounds: u32,
    pub reduction_arity_bits: &'a [usize],
}
impl<'a, W: Copy + Default> FriInstance<'a, W> {
    /// (batch_sizes, [sum][2] = (oracle_index, polynomial_index)) as the C ABI takes them; the point count is checked here
    fn lists(&self) -> Result<(Vec<u32>, Vec<u32>), GpuError> {
        let d = if std::mem::size_of::<W>() == 8 { 2 } else { 4 };   // extension degree D
        need("points", self.points.len(), self.polynomials.len() * d)?;
        let mut sizes = Vec::with_capacity(self.polynomials.len());
        let mut polys = Vec::new();
        for batch in self.polynomials {
            sizes.push(batch.len() as u32);
            for &(o, k) in batch.iter() {
                polys.push(o as u32);
                polys.push(k as u32);
            }
        }
        Ok((sizes, polys))
    }
}
/// `PolynomialBatch::prove_openings` (fri/oracle.rs:187-246) on any `FriInstanceInfo`, then `fri_proof`: FriProof bytes.
/// `oracles[i]` is the commitment of `instance.oracles[i]`; `challenger` (the transcript after the openings were observed) is
/// advanced as the reference's is, and left alone on an error.
pub fn fri_prove_openings<'c, W: Copy + Default>(ctx: &'c GpuContext, instance: &FriInstance<W>, oracles: &[&GpuPolynomialBatch<'c, W>],
                                                 params: &FriParams, challenger: &mut gb_challenger_state) -> Result<Vec<u8>, GpuError> {
    need("oracles", oracles.len(), instance.oracles.len())?;
    for (b, &(num_polys, blinding)) in oracles.iter().zip(instance.oracles) {
        need("FriOracleInfo.num_polys", num_polys, b.num_polys)?;
        if blinding != b.blinding {
            return Err(GpuError { status: GB_ERR_INVALID, message: "FriOracleInfo.blinding does not match the batch's salts".into() });
        }
    }
    let (sizes, polys) = instance.lists()?;
    let handles: Vec<*mut gb_batch> = oracles.iter().map(|b| b.handle).collect();
    let arity: Vec<u32> = params.reduction_arity_bits.iter().map(|&b| b as u32).collect();
    let mut buf = vec![0u8; 8 << 20];
    let mut len = 0usize;
    check(ctx.0, unsafe {
        gb_fri_prove_openings(ctx.0, handles.as_ptr(), handles.len() as u32, instance.points.as_ptr() as *const c_void, sizes.as_ptr(),
                              sizes.len() as u32, polys.as_ptr(), arity.as_ptr(), arity.len() as u32, params.proof_of_work_bits,
                              params.num_query_rounds, challenger, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
    })?;
    buf.truncate(len);
    Ok(buf)
}
/// `verify_fri_proof` (fri/verifier.rs:67-250) on the host: Ok(true), Ok(false) when a check fails, Err for malformed bytes or
/// arguments.  `openings`: every batch's values laid end to end ([sum of batch sizes][D]); `initial_caps`: every oracle's cap laid
/// end to end; `challenger`: the transcript after the openings were observed (not advanced).
pub fn fri_verify<W: Copy + Default>(instance: &FriInstance<W>, openings: &[W], initial_caps: &[W], params: &FriParams,
                                     challenger: &gb_challenger_state, fri_proof: &[u8]) -> Result<bool, GpuError> {
    let (d, h) = if std::mem::size_of::<W>() == 8 { (2, 4) } else { (4, 8) };
    let (sizes, polys) = instance.lists()?;
    need("openings", openings.len(), polys.len() / 2 * d)?;
    need("initial_caps", initial_caps.len(), instance.oracles.len() * (h << params.cap_height))?;
    let num_polys: Vec<u32> = instance.oracles.iter().map(|o| o.0 as u32).collect();
    let blinding: Vec<u32> = instance.oracles.iter().map(|o| o.1 as u32).collect();
    let arity: Vec<u32> = params.reduction_arity_bits.iter().map(|&b| b as u32).collect();
    let st = unsafe {
        gb_fri_verify(ptr::null_mut(), field_tag::<W>(), params.degree_bits, params.rate_bits, params.cap_height, params.hiding as u32,
                      num_polys.as_ptr(), blinding.as_ptr(), num_polys.len() as u32, instance.points.as_ptr() as *const c_void,
                      sizes.as_ptr(), sizes.len() as u32, polys.as_ptr(), openings.as_ptr() as *const c_void,
                      initial_caps.as_ptr() as *const c_void, arity.as_ptr(), arity.len() as u32, params.proof_of_work_bits,
                      params.num_query_rounds, challenger, fri_proof.as_ptr() as *const c_void, fri_proof.len())
    };
    if st == GB_ERR_VERIFY {
        return Ok(false);
    }
    check(ptr::null(), st)?;
    Ok(true)
}
/// One proof of `fri_verify_batch`: what `fri_verify` takes beside the shape.  `points`: [num_batches][D]; `openings` and
/// `initial_caps` laid end to end as for `fri_verify`; `challenger`: the transcript after the openings were observed (not advanced).
pub struct FriBatchItem<'a, W> {
    pub points: &'a [W],
    pub openings: &'a [W],
    pub initial_caps: &'a [W],
    pub challenger: gb_challenger_state,
    pub fri_proof: &'a [u8],
}
/// `fri_verify` of many proofs on ONE instance shape, the query rounds on the device (`gb_fri_verify_batch`): one
/// `gb_verify_result` per item (its `status` is what `fri_verify` would answer); Err only when the call itself did not complete.
/// `shape` gives the oracles and the lists (its own `points` are not read: every item brings its points); proofs of several
/// shapes are grouped by the caller, one call per shape.
pub fn fri_verify_batch<W: Copy + Default>(ctx: &GpuContext, shape: &FriInstance<W>, params: &FriParams, items: &[FriBatchItem<W>])
                                           -> Result<Vec<gb_verify_result>, GpuError> {
    let (d, h) = if std::mem::size_of::<W>() == 8 { (2, 4) } else { (4, 8) };
    let mut sizes = Vec::with_capacity(shape.polynomials.len());
    let mut polys = Vec::new();
    for batch in shape.polynomials {
        sizes.push(batch.len() as u32);
        for &(o, k) in batch.iter() {
            polys.push(o as u32);
            polys.push(k as u32);
        }
    }
    for it in items {
        need("points", it.points.len(), sizes.len() * d)?;
        need("openings", it.openings.len(), polys.len() / 2 * d)?;
        need("initial_caps", it.initial_caps.len(), shape.oracles.len() * (h << params.cap_height))?;
    }
    let num_polys: Vec<u32> = shape.oracles.iter().map(|o| o.0 as u32).collect();
    let blinding: Vec<u32> = shape.oracles.iter().map(|o| o.1 as u32).collect();
    let arity: Vec<u32> = params.reduction_arity_bits.iter().map(|&b| b as u32).collect();
    let points: Vec<*const c_void> = items.iter().map(|it| it.points.as_ptr() as *const c_void).collect();
    let openings: Vec<*const c_void> = items.iter().map(|it| it.openings.as_ptr() as *const c_void).collect();
    let caps: Vec<*const c_void> = items.iter().map(|it| it.initial_caps.as_ptr() as *const c_void).collect();
    let proofs: Vec<*const c_void> = items.iter().map(|it| it.fri_proof.as_ptr() as *const c_void).collect();
    let lens: Vec<usize> = items.iter().map(|it| it.fri_proof.len()).collect();
    let challengers: Vec<gb_challenger_state> = items.iter().map(|it| it.challenger).collect();
    let mut res = vec![gb_verify_result::default(); items.len()];
    let st = unsafe {
        gb_fri_verify_batch(ctx.0, field_tag::<W>(), params.degree_bits, params.rate_bits, params.cap_height, params.hiding as u32,
                            num_polys.as_ptr(), blinding.as_ptr(), num_polys.len() as u32, sizes.as_ptr(), sizes.len() as u32,
                            polys.as_ptr(), arity.as_ptr(), arity.len() as u32, params.proof_of_work_bits, params.num_query_rounds,
                            points.as_ptr(), openings.as_ptr(), caps.as_ptr(), challengers.as_ptr(), proofs.as_ptr(), lens.as_ptr(),
                            items.len() as u32, 0, res.as_mut_ptr() as *mut c_void)
    };
    if st != GB_ERR_VERIFY {
        check(ctx.0, st)?;
    }
    Ok(res)
}
/// (device_items, host_items) of `fri_verify_batch` on `ctx` since it was created (`gb_fri_verify_batch_counts`)
pub fn fri_verify_batch_counts(ctx: &GpuContext) -> Result<(u64, u64), GpuError> {
    let (mut dev, mut host) = (0u64, 0u64);
    check(ctx.0, unsafe { gb_fri_verify_batch_counts(ctx.0, &mut dev, &mut host) })?;
    Ok((dev, host))
}

/// What `CircuitBuilder::build()` leaves for the prover, resident on the GPU (circuit_builder.rs:1214-1312).
pub struct GpuCircuit<'c, W> {
    ctx: &'c GpuContext,
    handle: *mut gb_circuit,
    pub config: gb_circuit_config,
    /// lengths the C side reads without being told: targets of `set_partition`'s map, inputs of `set_generators`
    num_targets: std::cell::Cell<Option<usize>>,
    num_inputs: std::cell::Cell<Option<usize>>,
    _w: std::marker::PhantomData<W>,
}

pub enum ProveOutcome {
    Proof(Vec<u8>),
    /// `ProverError::InvZeroPermArg`: re-randomise the random wire and call again (plonk/prover.rs:183-226)
    PermArgZero,
}

/// The library reads program_words up to the last offset: the offsets must ascend from 0 to program_words.len().
fn program_table_len(program_words: &[u64], program_offsets: &[u32]) -> Result<u32, GpuError> {
    let ascending = program_offsets.windows(2).all(|w| w[0] <= w[1]) && program_offsets.first().map_or(true, |&o| o == 0);
    need("program_words", program_words.len(), if ascending { program_offsets.last().map_or(0, |&o| o as usize) } else { usize::MAX })?;
    Ok(program_offsets.len().saturating_sub(1) as u32)
}

impl<'c, W: Copy + Default> GpuCircuit<'c, W> {
    pub fn new(ctx: &'c GpuContext, mut config: gb_circuit_config, constants_sigmas: &[W], k_is: &[W]) -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_circuit_create(ctx.0, &config, constants_sigmas.as_ptr() as *const c_void, k_is.as_ptr() as *const c_void, GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, config, num_targets: std::cell::Cell::new(None), num_inputs: std::cell::Cell::new(None),
                  _w: std::marker::PhantomData })
    }
    /// The same for any gate set the library evaluates (`gates` = CommonCircuitData.gates with selectors_info, sorted as build()
    /// leaves them); GB_ERR_UNSUPPORTED (status 4) tells the caller to keep the CPU prover for this circuit.
    pub fn with_gates(ctx: &'c GpuContext, mut config: gb_circuit_config, gates: &[gb_gate], constants_sigmas: &[W], k_is: &[W])
                      -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_circuit_create_gates(ctx.0, &config, gates.as_ptr(), gates.len() as u32, constants_sigmas.as_ptr() as *const c_void,
                                    k_is.as_ptr() as *const c_void, GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, config, num_targets: std::cell::Cell::new(None), num_inputs: std::cell::Cell::new(None),
                  _w: std::marker::PhantomData })
    }
    /// `with_gates` for a gate set with gates of the host's own (`kind` = GB_GATE_PROGRAM, `param` = index of the gate's program):
    /// the programs lie end to end in `program_words`, program i at program_offsets[i] .. program_offsets[i + 1]; a program is the
    /// gate's eval_unfiltered as the words include/goldibear_gpu.h describes ("constraint programs"); INTEGRATION.md shows how a
    /// host records them from `eval_unfiltered_circuit`.
    pub fn with_programs(ctx: &'c GpuContext, mut config: gb_circuit_config, gates: &[gb_gate], program_words: &[u64], program_offsets: &[u32],
                         constants_sigmas: &[W], k_is: &[W]) -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        let num_programs = program_table_len(program_words, program_offsets)?;
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_circuit_create_programs(ctx.0, &config, gates.as_ptr(), gates.len() as u32, program_words.as_ptr(), program_offsets.as_ptr(),
                                       num_programs, constants_sigmas.as_ptr() as *const c_void, k_is.as_ptr() as *const c_void,
                                       GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, config, num_targets: std::cell::Cell::new(None), num_inputs: std::cell::Cell::new(None),
                  _w: std::marker::PhantomData })
    }
    /// `with_programs` over one column per `Vec` (`gb_circuit_create_programs_cols`)
    pub fn with_programs_columns<C: AsRef<[W]>>(ctx: &'c GpuContext, mut config: gb_circuit_config, gates: &[gb_gate],
                                                program_words: &[u64], program_offsets: &[u32], constants_sigmas: &[C], k_is: &[W]) -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        need("constants_sigmas", constants_sigmas.len(), (config.num_selectors + config.num_constants + config.num_routed_wires) as usize)?;
        need("k_is", k_is.len(), config.num_routed_wires as usize)?;
        let table = column_table("constants_sigmas", constants_sigmas, 1usize << config.degree_bits)?;
        let num_programs = program_table_len(program_words, program_offsets)?;
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_circuit_create_programs_cols(ctx.0, &config, gates.as_ptr(), gates.len() as u32, program_words.as_ptr(), program_offsets.as_ptr(),
                                            num_programs, table.as_ptr(), k_is.as_ptr() as *const c_void, GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, config, num_targets: std::cell::Cell::new(None), num_inputs: std::cell::Cell::new(None),
                  _w: std::marker::PhantomData })
    }
    /// `with_gates` over `constants_sigmas_vecs` as `build()` holds them (circuit_builder.rs:1198-1229): one column per `Vec`, canonical
    /// words, handed over as a pointer table (`gb_circuit_create_gates_cols`)
    pub fn with_gates_columns<C: AsRef<[W]>>(ctx: &'c GpuContext, mut config: gb_circuit_config, gates: &[gb_gate], constants_sigmas: &[C],
                                             k_is: &[W]) -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        need("constants_sigmas", constants_sigmas.len(), (config.num_selectors + config.num_constants + config.num_routed_wires) as usize)?;
        need("k_is", k_is.len(), config.num_routed_wires as usize)?;
        let table = column_table("constants_sigmas", constants_sigmas, 1usize << config.degree_bits)?;
        let mut h = ptr::null_mut();
        check(ctx.0, unsafe {
            gb_circuit_create_gates_cols(ctx.0, &config, gates.as_ptr(), gates.len() as u32, table.as_ptr(), k_is.as_ptr() as *const c_void,
                                         GB_INPUT_HOST, &mut h)
        })?;
        Ok(Self { ctx, handle: h, config, num_targets: std::cell::Cell::new(None), num_inputs: std::cell::Cell::new(None),
                  _w: std::marker::PhantomData })
    }
    /// Zero-knowledge circuits: `salts` = [3][4][N] canonical words, the F::rand_vec columns of the wires / Zs / quotient
    /// commitments (fri/oracle.rs:144-148)
    pub fn prove_salted(&self, witness: &[W], public_inputs: &[u64], salts: &[W]) -> Result<ProveOutcome, GpuError> {
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_salted(self.handle, witness.as_ptr() as *const c_void, GB_INPUT_HOST, public_inputs.as_ptr(), public_inputs.len(),
                            salts.as_ptr() as *const c_void, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(ProveOutcome::PermArgZero);
        }
        check(self.ctx.0, st)?;
        buf.truncate(len);
        Ok(ProveOutcome::Proof(buf))
    }
    /// Zero-knowledge circuits, the salts from a seed (`GB_SALTS_FROM_SEED`): the library generates the salt columns on the device
    /// from the 32 bytes - salt element [s][j][t] = element t of the stream (seed, (GB_STREAM_SALTS, s, j)) - and nothing but the
    /// seed crosses the bus.  ONE SEED PER PROOF, from the operating system's generator: the library draws no entropy, and a seed
    /// used for two different witnesses gives both proofs the same salts and voids the hiding of both.
    pub fn prove_seeded(&self, witness: &[W], public_inputs: &[u64], seed: &[u8; GB_SEED_SIZE]) -> Result<ProveOutcome, GpuError> {
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_salted(self.handle, witness.as_ptr() as *const c_void, GB_INPUT_HOST | GB_SALTS_FROM_SEED, public_inputs.as_ptr(),
                            public_inputs.len(), seed.as_ptr() as *const c_void, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(ProveOutcome::PermArgZero);
        }
        check(self.ctx.0, st)?;
        buf.truncate(len);
        Ok(ProveOutcome::Proof(buf))
    }
    /// `ProofWithPublicInputs::compress` on serialized bytes (plonk/proof.rs:111-122)
    pub fn compress(&self, proof: &[u8]) -> Result<Vec<u8>, GpuError> {
        let mut buf = vec![0u8; proof.len().max(1 << 16)];
        let mut len = 0usize;
        check(self.ctx.0, unsafe { gb_proof_compress(self.handle, proof.as_ptr() as *const c_void, proof.len(),
                                                     buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len) })?;
        buf.truncate(len);
        Ok(buf)
    }
    /// `CompressedProofWithPublicInputs::decompress` (plonk/proof.rs:221-236)
    pub fn decompress(&self, compressed: &[u8]) -> Result<Vec<u8>, GpuError> {
        let mut buf = vec![0u8; (2 * compressed.len()).max(1 << 16)];
        let mut len = 0usize;
        check(self.ctx.0, unsafe { gb_proof_decompress(self.handle, compressed.as_ptr() as *const c_void, compressed.len(),
                                                       buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len) })?;
        buf.truncate(len);
        Ok(buf)
    }
    /// `CompressedProofWithPublicInputs::verify` (plonk/proof.rs:238-265)
    pub fn verify_compressed(&self, compressed: &[u8]) -> Result<bool, GpuError> {
        let st = unsafe { gb_verify_compressed(self.handle, compressed.as_ptr() as *const c_void, compressed.len()) };
        if st == GB_ERR_VERIFY {
            return Ok(false);
        }
        check(self.ctx.0, st)?;
        Ok(true)
    }
    /// `FriParams.reduction_arity_bits` of a circuit whose `FriReductionStrategy` is `Fixed(..)` or `MinSize(..)`
    /// (fri/reduction_strategies.rs:29-56): hand over `common.fri_params.reduction_arity_bits` before the first proof.
    pub fn set_fri_reduction_arity_bits(&self, arity_bits: &[usize]) -> Result<(), GpuError> {
        let bits: Vec<u32> = arity_bits.iter().map(|&b| b as u32).collect();
        check(self.ctx.0, unsafe { gb_circuit_set_fri_reduction_arity_bits(self.handle, bits.as_ptr(), bits.len() as u32) })
    }
    /// the list in force (derived from ConstantArityBits unless set)
    pub fn fri_reduction_arity_bits(&self) -> Result<Vec<usize>, GpuError> {
        let mut bits = [0u32; GB_MAX_FRI_LAYERS];
        let mut n = 0u32;
        check(self.ctx.0, unsafe { gb_circuit_fri_reduction_arity_bits(self.handle, bits.as_mut_ptr(), &mut n) })?;
        Ok(bits[..n as usize].iter().map(|&b| b as usize).collect())
    }
    /// (constants_sigmas_cap, circuit_digest)
    pub fn verifier_data(&self) -> Result<(Vec<W>, Vec<W>), GpuError> {
        let hl = if std::mem::size_of::<W>() == 8 { 4 } else { 8 };
        let mut cap = vec![W::default(); hl << self.config.cap_height];
        let mut digest = vec![W::default(); hl];
        check(self.ctx.0, unsafe { gb_circuit_verifier_data(self.handle, cap.as_mut_ptr() as *mut c_void, digest.as_mut_ptr() as *mut c_void) })?;
        Ok((cap, digest))
    }
    /// `internal_prove_with_partition_witness` (plonk/prover.rs:228-447): `witness` = wire_values [num_wires][n]
    pub fn prove(&self, witness: &[W], public_inputs: &[u64]) -> Result<ProveOutcome, GpuError> {
        need("witness", witness.len(), (self.config.num_wires as usize) << self.config.degree_bits)?;
        need("public_inputs", public_inputs.len(), self.config.num_public_inputs as usize)?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove(self.handle, witness.as_ptr() as *const c_void, GB_INPUT_HOST, public_inputs.as_ptr(), public_inputs.len(),
                     buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(ProveOutcome::PermArgZero);
        }
        check(self.ctx.0, st)?;
        buf.truncate(len);
        Ok(ProveOutcome::Proof(buf))
    }
    /// The retry of `prove_with_partition_witness` (plonk/prover.rs:183-226): `witness` is the matrix of the `prove` call that has
    /// just returned `PermArgZero`, with `wire_values[wire][row]` (the circuit's `random_wire`) re-drawn.  Same result as `prove`.
    pub fn prove_retry(&self, witness: &[W], wire: usize, row: usize, public_inputs: &[u64]) -> Result<ProveOutcome, GpuError> {
        need("witness", witness.len(), (self.config.num_wires as usize) << self.config.degree_bits)?;
        need("public_inputs", public_inputs.len(), self.config.num_public_inputs as usize)?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_retry(self.handle, witness.as_ptr() as *const c_void, GB_INPUT_HOST, wire as u32, row as u64, public_inputs.as_ptr(),
                           public_inputs.len(), buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(ProveOutcome::PermArgZero);
        }
        check(self.ctx.0, st)?;
        buf.truncate(len);
        Ok(ProveOutcome::Proof(buf))
    }
    fn finish_proof(&self, st: i32, mut buf: Vec<u8>, len: usize) -> Result<ProveOutcome, GpuError> {
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(ProveOutcome::PermArgZero);
        }
        check(self.ctx.0, st)?;
        buf.truncate(len);
        Ok(ProveOutcome::Proof(buf))
    }
    /// `internal_prove_with_partition_witness` (plonk/prover.rs:228-447) from `MatrixWitness.wire_values` AS IT IS
    /// (iop/witness.rs:277-279: `Vec<Vec<F>>`): `wire_values[w]` = the n values of wire w, every column its own pageable
    /// allocation, handed over as a pointer table (`gb_prove_cols`) - no flattened copy of the 1 GiB witness.
    pub fn prove_columns<C: AsRef<[W]>>(&self, wire_values: &[C], public_inputs: &[u64], repr: Repr) -> Result<ProveOutcome, GpuError> {
        need("wire_values", wire_values.len(), self.config.num_wires as usize)?;
        need("public_inputs", public_inputs.len(), self.config.num_public_inputs as usize)?;
        let table = column_table("wire_values", wire_values, 1usize << self.config.degree_bits)?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_cols(self.handle, table.as_ptr(), repr.flags(), public_inputs.as_ptr(), public_inputs.len(),
                          buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// `prove_retry` over the same columns with `wire_values[wire][row]` (the circuit's `random_wire`) re-drawn
    pub fn prove_retry_columns<C: AsRef<[W]>>(&self, wire_values: &[C], wire: usize, row: usize, public_inputs: &[u64], repr: Repr)
                                              -> Result<ProveOutcome, GpuError> {
        need("wire_values", wire_values.len(), self.config.num_wires as usize)?;
        need("public_inputs", public_inputs.len(), self.config.num_public_inputs as usize)?;
        let table = column_table("wire_values", wire_values, 1usize << self.config.degree_bits)?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_retry_cols(self.handle, table.as_ptr(), repr.flags(), wire as u32, row as u64, public_inputs.as_ptr(),
                                public_inputs.len(), buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// `prove_salted` over separately allocated wire columns; `salts` = [3][4][N] words in the same representation
    pub fn prove_salted_columns<C: AsRef<[W]>>(&self, wire_values: &[C], public_inputs: &[u64], salts: &[W], repr: Repr)
                                               -> Result<ProveOutcome, GpuError> {
        need("wire_values", wire_values.len(), self.config.num_wires as usize)?;
        need("public_inputs", public_inputs.len(), self.config.num_public_inputs as usize)?;
        need("salts", salts.len(), 12usize << (self.config.degree_bits + self.config.rate_bits))?;
        let table = column_table("wire_values", wire_values, 1usize << self.config.degree_bits)?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_salted_cols(self.handle, table.as_ptr(), repr.flags(), public_inputs.as_ptr(), public_inputs.len(),
                                 salts.as_ptr() as *const c_void, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// `zs_partial_products` from the witness columns (only the routed ones are read); the result is canonical
    pub fn zs_partial_products_columns<C: AsRef<[W]>>(&self, wire_values: &[C], betas: &[W], gammas: &[W], repr: Repr)
                                                      -> Result<Option<Vec<W>>, GpuError> {
        let c = &self.config;
        need("wire_values", wire_values.len(), c.num_wires as usize)?;
        need("betas", betas.len(), c.num_challenges as usize)?;
        need("gammas", gammas.len(), c.num_challenges as usize)?;
        let table = column_table("wire_values", wire_values, 1usize << c.degree_bits)?;
        let chunks = (c.num_routed_wires + c.max_quotient_degree_factor - 1) / c.max_quotient_degree_factor;
        let mut out = vec![W::default(); (c.num_challenges * chunks) as usize << c.degree_bits];
        let st = unsafe {
            gb_zs_partial_products_cols(self.handle, table.as_ptr(), repr.flags(), betas.as_ptr() as *const c_void,
                                        gammas.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(None);
        }
        check(self.ctx.0, st)?;
        Ok(Some(out))
    }
    /// `ProverOnlyCircuitData.representative_map` (plonk/circuit_data.rs:454, a `Vec<usize>` indexed by `Target::index`) and the
    /// target indices of `prover_data.public_inputs`, once after the circuit is created: what `prove_partition` expands through.
    pub fn set_partition(&self, representative_map: &[usize], public_input_targets: &[usize]) -> Result<(), GpuError> {
        let map: Vec<u64> = representative_map.iter().map(|&t| t as u64).collect();
        let pis: Vec<u64> = public_input_targets.iter().map(|&t| t as u64).collect();
        check(self.ctx.0, unsafe { gb_circuit_set_partition(self.handle, map.as_ptr(), map.len() as u64, pis.as_ptr(), pis.len()) })?;
        self.num_targets.set(Some(map.len()));
        self.num_inputs.set(None);   // the library drops the generator schedule with the old map
        Ok(())
    }
    fn need_len(what: &str, have: usize, want: Option<usize>, setter: &str) -> Result<(), GpuError> {
        match want {
            Some(w) => need(what, have, w),
            None => Err(GpuError { status: GB_ERR_INVALID, message: format!("{setter} has not been called on this circuit") }),
        }
    }
    /// `prove_with_partition_witness` from the `PartitionWitness` itself (plonk/prover.rs:160-183): `values[i]` =
    /// `partition_witness.values[i].unwrap_or(F::ZERO)`; `full_witness()` runs on the device.  `salts`: zero-knowledge circuits only.
    pub fn prove_partition(&self, values: &[W], salts: Option<&[W]>, repr: Repr) -> Result<ProveOutcome, GpuError> {
        Self::need_len("values", values.len(), self.num_targets.get(), "set_partition")?;
        if let Some(s) = salts {
            need("salts", s.len(), 12 * (1usize << (self.config.degree_bits + self.config.rate_bits)))?;
        }
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_partition(self.handle, values.as_ptr() as *const c_void, repr.flags(),
                               salts.map_or(std::ptr::null(), |s| s.as_ptr() as *const c_void), buf.as_mut_ptr() as *mut c_void, buf.len(),
                               &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// The retry (prover.rs:186-226): `values[representative_map[row * num_wires + wire]]` - the random wire - re-drawn, nothing else.
    pub fn prove_partition_retry(&self, values: &[W], wire: usize, row: usize, repr: Repr) -> Result<ProveOutcome, GpuError> {
        Self::need_len("values", values.len(), self.num_targets.get(), "set_partition")?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_partition_retry(self.handle, values.as_ptr() as *const c_void, repr.flags(), wire as u32, row as u64,
                                     buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// `full_witness()` alone into a device buffer of the caller ([num_wires][n] canonical words), on the context's stream.
    ///
    /// # Safety
    /// `witness_dev_out` must be a device allocation of num_wires * n elements on this context's device.
    pub unsafe fn expand_partition(&self, values: &[W], repr: Repr, witness_dev_out: *mut c_void) -> Result<(), GpuError> {
        Self::need_len("values", values.len(), self.num_targets.get(), "set_partition")?;
        check(self.ctx.0, gb_expand_partition(self.handle, values.as_ptr() as *const c_void, repr.flags(), witness_dev_out))
    }
    /// The circuit's generator programs (include/goldibear_gpu.h "GENERATOR PROGRAMS"): custom witness generators - a program
    /// gate's `generators()`, a `SimpleGenerator` of `add_simple_generator` - as data, one slice of words per program.  After
    /// `set_partition` and before `set_generators`, whose GB_GEN_PROGRAM records (`push_program_generator`) name them by index.
    /// Calling it again replaces them and drops the schedule; an empty list clears them.
    pub fn set_generator_programs(&self, programs: &[&[u64]]) -> Result<(), GpuError> {
        let too_long = |what: &str| GpuError { status: GB_ERR_INVALID, message: format!("set_generator_programs: {what}") };
        if programs.len() > GB_MAX_GENERATOR_PROGRAMS as usize {
            return Err(too_long("more than GB_MAX_GENERATOR_PROGRAMS programs"));
        }
        let mut words: Vec<u64> = Vec::new();
        let mut offsets: Vec<u32> = vec![0];
        for p in programs {
            words.extend(p.iter());
            if words.len() > u32::MAX as usize {
                return Err(too_long("the program table does not fit 32-bit offsets"));
            }
            offsets.push(words.len() as u32);
        }
        check(self.ctx.0, unsafe {
            gb_circuit_set_generator_programs(self.handle, words.as_ptr(), offsets.as_ptr(), programs.len() as u32)
        })?;
        self.num_inputs.set(None);
        Ok(())
    }
    /// `prover_only.generators` as records (see INTEGRATION.md "Generators as records"), the targets whose values the host supplies
    /// per proof - the `PartialWitness` and every `RandomValueGenerator` target - and the constants columns
    /// `[num_constants][degree]` as canonical words; once, after `set_partition`.
    pub fn set_generators(&self, generators: &[gb_generator], input_targets: &[usize], constants: &[u64]) -> Result<(), GpuError> {
        need("constants", constants.len(), (self.config.num_constants as usize) << self.config.degree_bits)?;
        let inputs: Vec<u64> = input_targets.iter().map(|&t| t as u64).collect();
        check(self.ctx.0, unsafe {
            gb_circuit_set_generators(self.handle, generators.as_ptr() as *const c_void, generators.len() as u64, inputs.as_ptr(),
                                      inputs.len() as u64, constants.as_ptr(), 0)
        })?;
        self.num_inputs.set(Some(inputs.len()));
        Ok(())
    }
    /// What the schedule looks like; `num_unrunnable` is the `n` of the reference's "{n} generators weren't run".
    pub fn generators_info(&self) -> Result<GeneratorsInfo, GpuError> {
        let mut i = GeneratorsInfo::default();
        check(self.ctx.0, unsafe {
            gb_circuit_generators_info(self.handle, &mut i.num_levels, &mut i.num_launches, &mut i.num_unrunnable, &mut i.num_checks,
                                       &mut i.num_classes)
        })?;
        Ok(i)
    }
    /// The representative target of every class of the schedule, in the order of `generate_partition`'s values.
    pub fn generator_classes(&self) -> Result<Vec<u64>, GpuError> {
        let mut out = vec![0u64; self.generators_info()?.num_classes as usize];
        check(self.ctx.0, unsafe { gb_circuit_generator_classes(self.handle, out.as_mut_ptr(), out.len() as u64) })?;
        Ok(out)
    }
    /// `generate_partial_witness` (iop/generator.rs:25-106) alone, into a device buffer of the caller.
    ///
    /// # Safety
    /// `values_dev_out` must be a device allocation of `num_classes` elements on this context's device.
    pub unsafe fn generate_partition(&self, input_values: &[W], repr: Repr, values_dev_out: *mut c_void) -> Result<(), GpuError> {
        Self::need_len("input_values", input_values.len(), self.num_inputs.get(), "set_generators")?;
        check(self.ctx.0, gb_generate_partition(self.handle, input_values.as_ptr() as *const c_void, repr.flags(), values_dev_out))
    }
    /// `prove()` (plonk/prover.rs:136-158) from the inputs alone: `input_values` in the order of `set_generators`' targets; the
    /// generators, `full_witness()` and the proof run on the device.  `salts`: zero-knowledge circuits only.
    pub fn prove_inputs(&self, input_values: &[W], salts: Option<&[W]>, repr: Repr) -> Result<ProveOutcome, GpuError> {
        Self::need_len("input_values", input_values.len(), self.num_inputs.get(), "set_generators")?;
        if let Some(s) = salts {
            need("salts", s.len(), 12 * (1usize << (self.config.degree_bits + self.config.rate_bits)))?;
        }
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_inputs(self.handle, input_values.as_ptr() as *const c_void, repr.flags(),
                            salts.map_or(std::ptr::null(), |s| s.as_ptr() as *const c_void), buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// The retry (prover.rs:186-226): the input of the random wire (`wire`, `row`) re-drawn, nothing else.
    pub fn prove_inputs_retry(&self, input_values: &[W], wire: usize, row: usize, repr: Repr) -> Result<ProveOutcome, GpuError> {
        Self::need_len("input_values", input_values.len(), self.num_inputs.get(), "set_generators")?;
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        let st = unsafe {
            gb_prove_inputs_retry(self.handle, input_values.as_ptr() as *const c_void, repr.flags(), wire as u32, row as u64,
                                  buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        };
        self.finish_proof(st, buf, len)
    }
    /// GB_OK and GB_ERR_UNSATISFIED both carry a result; anything else is an error.
    fn finish_check(&self, st: i32, mut violations: Vec<gb_violation>, result: gb_check_result) -> Result<CheckOutcome, GpuError> {
        if st != GB_OK && st != GB_ERR_UNSATISFIED {
            check(self.ctx.0, st)?;
        }
        violations.truncate(result.num_listed as usize);
        Ok(CheckOutcome { violations, result })
    }
    /// Does this witness (`[num_wires][degree]`, as `prove` takes it) satisfy the circuit?  Every active gate's constraints on
    /// every row and, on a circuit with a partition, the copy constraints; at most `max_violations` are listed.
    pub fn check_witness(&self, witness: &[W], public_inputs: &[u64], max_violations: usize, repr: Repr) -> Result<CheckOutcome, GpuError> {
        let c = &self.config;
        need("witness", witness.len(), (c.num_wires as usize) << c.degree_bits)?;
        need("public_inputs", public_inputs.len(), c.num_public_inputs as usize)?;
        let mut out = vec![gb_violation::default(); max_violations.max(1)];
        let mut res = gb_check_result::default();
        let st = unsafe {
            gb_check_witness(self.handle, witness.as_ptr() as *const c_void, repr.flags(), public_inputs.as_ptr(), public_inputs.len(),
                             out.as_mut_ptr() as *mut c_void, max_violations, &mut res as *mut gb_check_result as *mut c_void)
        };
        self.finish_check(st, out, res)
    }
    /// The same from `PartitionWitness.values` (after `set_partition`): `prove_partition`'s expansion, then the check.
    pub fn check_partition(&self, values: &[W], max_violations: usize, repr: Repr) -> Result<CheckOutcome, GpuError> {
        Self::need_len("values", values.len(), self.num_targets.get(), "set_partition")?;
        let mut out = vec![gb_violation::default(); max_violations.max(1)];
        let mut res = gb_check_result::default();
        let st = unsafe {
            gb_check_partition(self.handle, values.as_ptr() as *const c_void, repr.flags(), out.as_mut_ptr() as *mut c_void, max_violations,
                               &mut res as *mut gb_check_result as *mut c_void)
        };
        self.finish_check(st, out, res)
    }
    /// The same from the inputs (after `set_generators`): the generators and the expansion on the device, then the check.
    pub fn check_inputs(&self, input_values: &[W], max_violations: usize, repr: Repr) -> Result<CheckOutcome, GpuError> {
        Self::need_len("input_values", input_values.len(), self.num_inputs.get(), "set_generators")?;
        let mut out = vec![gb_violation::default(); max_violations.max(1)];
        let mut res = gb_check_result::default();
        let st = unsafe {
            gb_check_inputs(self.handle, input_values.as_ptr() as *const c_void, repr.flags(), out.as_mut_ptr() as *mut c_void, max_violations,
                            &mut res as *mut gb_check_result as *mut c_void)
        };
        self.finish_check(st, out, res)
    }
    /// Read the copy permutation back out of the sigma columns and keep its cycles as copy classes: from then on `check_witness`
    /// - and `prove*` under the option "check_witness" - check the copy constraints of a circuit that has no partition.  With a
    /// partition set, also checks that the partition's classes are the same wiring (`InvalidInput` names the first cell where
    /// they are not).  A repeated call does no device work.
    pub fn decode_sigmas(&self) -> Result<gb_sigma_info, GpuError> {
        let mut info = gb_sigma_info::default();
        check(self.ctx.0, unsafe { gb_circuit_decode_sigmas(self.handle, 0, &mut info as *mut gb_sigma_info as *mut c_void) })?;
        Ok(info)
    }
    /// After `decode_sigmas`: per wire cell `row * num_wires + column`, the lowest cell of its copy class.
    pub fn copy_classes(&self) -> Result<Vec<u32>, GpuError> {
        let c = &self.config;
        let mut out = vec![0u32; (c.num_wires as usize) << c.degree_bits];
        check(self.ctx.0, unsafe { gb_circuit_copy_classes(self.handle, out.as_mut_ptr()) })?;
        Ok(out)
    }
    /// Give up after `PermArgZero` (`ProverError::TooManyPermArgFailures`, prover.rs:221-225): releases what the failed attempt
    /// left on the device for `prove_retry` (~12 GB at 2^20 Goldilocks rows).  No-op when nothing is held.
    pub fn drop_retry(&self) -> Result<(), GpuError> {
        check(self.ctx.0, unsafe { gb_circuit_drop_retry(self.handle) })
    }
    /// `wires_permutation_partial_products_and_zs` for every challenge (plonk/prover.rs:305-329, 449-546): the values handed to
    /// `PolynomialBatch::from_values`, Zs first.  `Ok(None)` = `ProverError::InvZeroPermArg`.
    pub fn zs_partial_products(&self, witness: &[W], betas: &[W], gammas: &[W]) -> Result<Option<Vec<W>>, GpuError> {
        let c = &self.config;
        need("witness", witness.len(), (c.num_wires as usize) << c.degree_bits)?;
        need("betas", betas.len(), c.num_challenges as usize)?;
        need("gammas", gammas.len(), c.num_challenges as usize)?;
        let chunks = (c.num_routed_wires + c.max_quotient_degree_factor - 1) / c.max_quotient_degree_factor;
        let mut out = vec![W::default(); (c.num_challenges * chunks) as usize << c.degree_bits];
        let st = unsafe {
            gb_zs_partial_products(self.handle, witness.as_ptr() as *const c_void, GB_INPUT_HOST, betas.as_ptr() as *const c_void,
                                   gammas.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void)
        };
        if st == GB_ERR_PERM_ARG_ZERO {
            return Ok(None);
        }
        check(self.ctx.0, st)?;
        Ok(Some(out))
    }
    /// `compute_quotient_polys` + the split into chunks (plonk/prover.rs:345-376): coefficients for `from_coeffs`
    pub fn quotient_polys(&self, wires: &GpuPolynomialBatch<'c, W>, zs_partial_products: &GpuPolynomialBatch<'c, W>,
                          public_inputs_hash: &[W], betas: &[W], gammas: &[W], alphas: &[W]) -> Result<Vec<W>, GpuError> {
        let c = &self.config;
        need("public_inputs_hash", public_inputs_hash.len(), if std::mem::size_of::<W>() == 8 { 4 } else { 8 })?;
        need("betas", betas.len(), c.num_challenges as usize)?;
        need("gammas", gammas.len(), c.num_challenges as usize)?;
        need("alphas", alphas.len(), c.num_challenges as usize)?;
        let mut out = vec![W::default(); (c.num_challenges * c.max_quotient_degree_factor) as usize << c.degree_bits];
        check(self.ctx.0, unsafe {
            gb_quotient_polys(self.handle, wires.handle, zs_partial_products.handle, public_inputs_hash.as_ptr() as *const c_void,
                              betas.as_ptr() as *const c_void, gammas.as_ptr() as *const c_void, alphas.as_ptr() as *const c_void,
                              GB_INPUT_HOST, out.as_mut_ptr() as *mut c_void)
        })?;
        Ok(out)
    }
    /// `PolynomialBatch::prove_openings` on this circuit's FRI instance (fri/oracle.rs:187-246): FriProof bytes; `challenger`
    /// (the transcript after observe_openings) is advanced as the reference's is.
    pub fn prove_openings(&self, wires: &GpuPolynomialBatch<'c, W>, zs_partial_products: &GpuPolynomialBatch<'c, W>,
                          quotient: &GpuPolynomialBatch<'c, W>, zeta: &[W], challenger: &mut gb_challenger_state)
                          -> Result<Vec<u8>, GpuError> {
        need("zeta", zeta.len(), if std::mem::size_of::<W>() == 8 { 2 } else { 4 })?;   // extension degree D
        let mut buf = vec![0u8; 8 << 20];
        let mut len = 0usize;
        check(self.ctx.0, unsafe {
            gb_prove_openings(self.handle, wires.handle, zs_partial_products.handle, quotient.handle, zeta.as_ptr() as *const c_void,
                              challenger, buf.as_mut_ptr() as *mut c_void, buf.len(), &mut len)
        })?;
        buf.truncate(len);
        Ok(buf)
    }
    /// `prover_data.constants_sigmas_commitment`: borrowed from the circuit, for `eval_ext` / `get_lde_values`
    pub fn constants_sigmas_commitment_handle(&self) -> Result<*mut gb_batch, GpuError> {
        let mut h = ptr::null_mut();
        check(self.ctx.0, unsafe { gb_circuit_constants_sigmas_commitment(self.handle, &mut h) })?;
        Ok(h)
    }
    /// `verify` of many proofs of this circuit at once, the query rounds on the device: one `gb_verify_result` per proof (its
    /// `status` is what `verify` would answer); Err only when the call itself did not complete
    pub fn verify_batch(&self, proofs: &[&[u8]]) -> Result<Vec<gb_verify_result>, GpuError> {
        let ptrs: Vec<*const c_void> = proofs.iter().map(|p| p.as_ptr() as *const c_void).collect();
        let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
        let mut res = vec![gb_verify_result::default(); proofs.len()];
        let st = unsafe {
            gb_verify_batch(self.ctx.0, self.handle, ptrs.as_ptr(), lens.as_ptr(), proofs.len() as u32, 0,
                            res.as_mut_ptr() as *mut c_void)
        };
        if st != GB_ERR_VERIFY {
            check(self.ctx.0, st)?;
        }
        Ok(res)
    }
    /// `verify_batch` for `CompressedProofWithPublicInputs` bytes, checked as they stand (`gb_verify_compressed_batch`): `status` is
    /// what `verify_compressed` would answer
    pub fn verify_compressed_batch(&self, proofs: &[&[u8]]) -> Result<Vec<gb_verify_result>, GpuError> {
        let ptrs: Vec<*const c_void> = proofs.iter().map(|p| p.as_ptr() as *const c_void).collect();
        let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
        let mut res = vec![gb_verify_result::default(); proofs.len()];
        let st = unsafe {
            gb_verify_compressed_batch(self.ctx.0, self.handle, ptrs.as_ptr(), lens.as_ptr(), proofs.len() as u32, 0,
                                       res.as_mut_ptr() as *mut c_void)
        };
        if st != GB_ERR_VERIFY {
            check(self.ctx.0, st)?;
        }
        Ok(res)
    }
    /// `CircuitData::verify` for the gate sets the library evaluates, on the host: Ok(true), Ok(false) when a check fails
    pub fn verify(&self, proof: &[u8]) -> Result<bool, GpuError> {
        let st = unsafe { gb_verify(self.handle, proof.as_ptr() as *const c_void, proof.len()) };
        if st == GB_ERR_VERIFY {
            return Ok(false);
        }
        check(self.ctx.0, st)?;
        Ok(true)
    }
}
impl<'c, W> Drop for GpuCircuit<'c, W> {
    fn drop(&mut self) {
        unsafe { gb_circuit_free(self.handle) };
    }
}

/// `VerifierCircuitData` (plonk/circuit_data.rs:358-380): common data + verifier-only data; touches no device.
pub struct Verifier<W> {
    handle: *mut gb_circuit,
    _w: std::marker::PhantomData<W>,
}
impl<W: Copy + Default> Verifier<W> {
    pub fn new(mut config: gb_circuit_config, gates: &[gb_gate], k_is: &[W], constants_sigmas_cap: &[W], circuit_digest: &[W])
               -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        let mut h = ptr::null_mut();
        check(ptr::null(), unsafe {
            gb_verifier_create(ptr::null_mut(), &config, gates.as_ptr(), gates.len() as u32, k_is.as_ptr() as *const c_void,
                               constants_sigmas_cap.as_ptr() as *const c_void, circuit_digest.as_ptr() as *const c_void, &mut h)
        })?;
        Ok(Self { handle: h, _w: std::marker::PhantomData })
    }
    /// `new` for a gate set with GB_GATE_PROGRAM entries (`gb_verifier_create_programs`): the program table as in
    /// `GpuCircuit::with_programs`
    pub fn with_programs(mut config: gb_circuit_config, gates: &[gb_gate], program_words: &[u64], program_offsets: &[u32], k_is: &[W],
                         constants_sigmas_cap: &[W], circuit_digest: &[W]) -> Result<Self, GpuError> {
        config.field = field_tag::<W>();
        let num_programs = program_table_len(program_words, program_offsets)?;
        let mut h = ptr::null_mut();
        check(ptr::null(), unsafe {
            gb_verifier_create_programs(ptr::null_mut(), &config, gates.as_ptr(), gates.len() as u32, program_words.as_ptr(),
                                        program_offsets.as_ptr(), num_programs, k_is.as_ptr() as *const c_void,
                                        constants_sigmas_cap.as_ptr() as *const c_void, circuit_digest.as_ptr() as *const c_void, &mut h)
        })?;
        Ok(Self { handle: h, _w: std::marker::PhantomData })
    }
    pub fn verify(&self, proof: &[u8]) -> Result<bool, GpuError> {
        let st = unsafe { gb_verify(self.handle, proof.as_ptr() as *const c_void, proof.len()) };
        if st == GB_ERR_VERIFY {
            return Ok(false);
        }
        check(ptr::null(), st)?;
        Ok(true)
    }
}
impl<W> Drop for Verifier<W> {
    fn drop(&mut self) {
        unsafe { gb_circuit_free(self.handle) };
    }
}

// Internal launch interface between the C-ABI layer (api.hip) and the gfx950 kernels.
// Every launcher enqueues on `stream` and returns immediately; no allocation, no sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "field_traits.hpp"
#include "gate_set.hpp"
#include "generator_ops.hpp"
#include "challenge_slices.hpp"
#include "constraint_system.hpp"
#include "random_stream.hpp"
#include "sigma_decode.hpp"
#include "wiring.hpp"

namespace gbk {

// ---------------------------------------------------------------- NTT / LDE tables

// Device-resident twiddle tables for one transform size n = 2^log_n (built once per ctx and size).
struct GlNttTables {
    u32 log_n;
    const u64* tw4096_fwd;   // [4096] w_4096^j
    const u64* tw4096_inv;   // [4096] w_4096^-j
    const u64* tw_lo_fwd;    // [1024] w_n^e            (e < 1024)
    const u64* tw_hi_fwd;    // [max(1, n/1024)] w_n^(1024 e)
    const u64* tw_lo_inv;    // same for w_n^-1
    const u64* tw_hi_inv;
    u64 n_inv;               // n^-1 mod p
    // the same tables times R = 2^64 mod p (Montgomery form) for the register-radix passes (ntt_passes.hpp, lde_passes.hpp, kernels_ntt16.hip), whose
    // multiplications by table values then end in the 7-instruction Montgomery fold (gl::mul_mont: mont_fold_flags) instead of fold128's 11;
    // tw4096_fwd_m is [8192]: the powers, then the same powers in k_gl_lde_pb16's stage-1 order [slot][tid]
    const u64 *tw4096_fwd_m, *tw4096_inv_m, *tw_lo_fwd_m, *tw_hi_fwd_m, *tw_lo_inv_m, *tw_hi_inv_m;
    u64 n_inv_m;
    // 2^21 and 2^22 rows run the same three + two passes as 2^20 (round 6): the inverse transform's middle pass is a radix-32 / radix-64
    // DFT with twiddles w_{2^14}^-j (tw16k_inv_m, [2^14], Montgomery form)
    const u64* tw16k_inv_m;
    // log_n > 22: one outer radix-2^outer_bits step (ntt_outer.hpp) around transforms of log_n - outer_bits rows (`sub`); else null / 0
    const GlNttTables* sub;
    u32 outer_bits;
    const u64* tw_top_fwd;   // log_n > 22: [256] w_n^(brev8(j) 2^(log_m - 8)), log_m = log_n - outer_bits - the factor of the outer
                             // step's twiddle that varies over the 256 threads of a workgroup (ntt_outer.hpp k_lde_combine), contiguous
};
static constexpr u32 NTT_NATIVE_LOG = 22;   // largest transform the passes run without an outer step
static constexpr u32 NTT_OUTER_MAX_BITS = 4;
inline u32 ntt_outer_bits(u32 log_n) { return log_n <= NTT_NATIVE_LOG ? 0 : (log_n - NTT_NATIVE_LOG < NTT_OUTER_MAX_BITS ? log_n - NTT_NATIVE_LOG : NTT_OUTER_MAX_BITS); }

// Coset tables for the LDE of rate 2^rate_bits: coset c (leaf block c) has shift
// s_c = 7 * w_N^bitrev_r(c);  pow_lo[c][l] = s_c^l (l < 4096 or n), pow_hi[c][h] = s_c^(4096 h).
struct GlCosetTables {
    u32 rate_bits;
    const u64* pow_lo;  // [2^r][min(n,4096)]
    const u64* pow_hi;  // [2^r][max(1, n/4096)]
    const u64 *pow_lo_m, *pow_hi_m;  // the same times R (Montgomery form), for the strided LDE passes (lde_passes.hpp)
    // log_n > 22 (ntt_outer.hpp): the coset tables of the sub-transforms (shift^R) and the context's work buffer of this level - the
    // ADDRESS of the context's pointer / size, read at the call: the block moves when it grows
    const GlCosetTables* sub;
    void* const* work;
    const size_t* work_bytes;
};

// BabyBear: the same tables over Montgomery words (the plain tables are the kernels' form: no _m twins)
struct BbNttTables {
    u32 log_n;
    const u32 *tw4096_fwd, *tw4096_inv, *tw_lo_fwd, *tw_hi_fwd, *tw_lo_inv, *tw_hi_inv;
    u32 n_inv;
    const u32* tw16k_inv;      // log_n 21, 22: see GlNttTables
    const BbNttTables* wide;   // log_n 22: the tables of the 2^20-row transform (k_bb_lde_pa16x2w's twiddles)
    const BbNttTables* sub;    // log_n > 22
    u32 outer_bits;
    const u32* tw_top_fwd;     // log_n > 22: see GlNttTables
};
struct BbCosetTables {
    u32 rate_bits;
    const u32 *pow_lo, *pow_hi;
    const BbCosetTables* fine;   // log_n 22: the cosets of the rate 2^(rate_bits + 2) over 2^20 rows, same shift (k_bb_lde_pa16x2w)
    const BbCosetTables* sub;    // log_n > 22
    void* const* work;
    const size_t* work_bytes;
};

template <class F>
using NttTables = std::conditional_t<std::is_same<F, GlF>::value, GlNttTables, BbNttTables>;
template <class F>
using CosetTables = std::conditional_t<std::is_same<F, GlF>::value, GlCosetTables, BbCosetTables>;

// ---------------------------------------------------------------- NTT / LDE (ntt_passes.hpp, lde_passes.hpp; instantiated in kernels_ntt16.hip, kernels_bb16.hip)
// Templated on the field traits; element pointers are in the field's device form.

// Columns per group of the inverse transform's passes from 2^18 rows up, in 8-byte words (BabyBear: twice as many columns): the
// scratch block of one group is reused by the next and never leaves the Infinity Cache - measured -8 % on the three memory-bound
// passes (HISTORY.md, round 3); the LDE passes are bound by VALU issue and run all columns per launch.
static constexpr size_t INTT_GROUP = 16;

// values on H_n (natural order) -> coefficients (natural order), in `coeffs` [ncols][n].
// `scratch` must hold ncols*n elements. src may equal coeffs.
template <class F>
void intt_columns(const typename F::T* src, typename F::T* coeffs, typename F::T* scratch, size_t ncols, const NttTables<F>& t,
                  hipStream_t stream);
// BabyBear: values -> coefficients from CANONICAL values (k_intt16_p1<BbF, true>): no conversion pass; the first mont_cols columns
// of `vals` are left in Montgomery form, the rest canonical.  false: shape not covered (2^16..2^22 rows are), nothing done.
bool bb_intt_columns_canonical(u32* vals, u32* coeffs, u32* scratch, size_t ncols, size_t mont_cols, const BbNttTables& t, hipStream_t stream);
// coefficients [ncols][n] -> LDE [ncols][N] in LEAF order: lde[c][j] = P_c(7 * w_N^bitrev_logN(j))
// (fri/oracle.rs:108-109 order, no transpose / bit-reverse pass needed afterwards).
template <class F>
void lde_columns(const typename F::T* coeffs, typename F::T* lde, size_t ncols, const NttTables<F>& t, const CosetTables<F>& ct,
                 hipStream_t stream);
// gather one row (width elements at stride col_stride) into dst[0..width), canonical
template <class F>
void gather_row(const typename F::T* cols, size_t col_stride, u32 width, u64 index, typename F::T* dst, hipStream_t stream);
// leaf-order column-major [width][N] -> row-major canonical leaves [N][width] (debug / parity export)
template <class F>
void transpose_to_rows(const typename F::T* cols, size_t col_stride, u32 width, u64 rows, typename F::T* dst, hipStream_t stream);
// canonical src -> dst in device form, dst[j] = src[bitrev_bits(j)] for `ncols` columns of 2^bits elements (salt columns -> leaf order)
template <class F>
void bitrev_copy(const typename F::T* src, typename F::T* dst, u32 bits, size_t ncols, hipStream_t stream);
// any word -> the residue below p, in place (GB_INPUT_P3_REPR: the words of the reference's field types from a host)
template <class F>
void reduce_words(typename F::T* p, size_t count, hipStream_t stream);
// the keyed element stream (kernels_random.hip, random_stream.hpp): elements first .. first + count - 1 of the num_streams streams
// (key.seed, (nonce[0], nonce[1], nonce[2] + y)), stream y to out + y * stream_stride, canonical words; false when a launch failed
template <class F>
bool random_elements(const rnd::Key& key, u64 first, u64 count, u32 num_streams, typename F::T* out, u64 stream_stride, hipStream_t stream);
// PartitionWitness::full_witness (kernels_partition.hip, partition_expand.hpp): out[col][row] = staged[slots[row][col]] - slots
// [2^log_n][num_wires] row-major, out [num_wires][2^log_n]; words are copied as they are
template <class F>
void expand_partition(const u32* slots, const typename F::T* staged, typename F::T* out, u32 log_n, u32 num_wires, hipStream_t stream);
// generate_partial_witness on the device (kernels_generators.hip, generators.hpp): the launches of a schedule
// (generator_schedule.hpp) over `values`, one canonical word per copy class - the inputs scattered, everything else zero
template <class F>
void run_generators(const gen::DeviceSchedule& d, const gen::Launch* launches, size_t num_launches, const u32* level_off_host,
                    typename F::T* values, u32* err, hipStream_t stream);
// values[cls[i]] = in[i] (cls[i] = gen::OUT_SKIP: left out)
template <class F>
void scatter_inputs(const u32* cls, const typename F::T* in, u32 count, typename F::T* values, hipStream_t stream);
// out[0 .. count) = values[pi_cls[i]], out[count .. count + gen::ERROR_WORDS) = the error word
template <class F>
void gather_public(const u32* pi_cls, u32 count, const typename F::T* values, const u32* err, u64* out, hipStream_t stream);

// ---------------------------------------------------------------- stand-alone transforms and trees (kernels_poly.hip)
// The transform passes move canonical words and convert nothing (the transforms are linear and multiply by table values only:
// canonical words in, canonical words out, for BabyBear's Montgomery tables too - kernels_poly.hip).  `ext`: an element is F::D
// consecutive words, and the transforms see its coordinates as F::D columns (column c of the caller = columns c D .. c D + D - 1).

// leaf order -> natural order: one workgroup per column up to 2^POLY_SMALL_LOG elements, 64 x 64 tiles above
static constexpr u32 POLY_SMALL_LOG = 12;
// extension elements [ncols][len][D] -> coordinate columns [ncols * D][len]
template <class F>
void ext_load(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, hipStream_t stream);
// coordinate columns, natural order -> the caller's layout (interleaved if ext), element i times pow_lo[i % 4096] pow_hi[i / 4096]
// where pow_lo is not null (split powers in plain device form, as CosetTables::pow_lo / pow_hi of one coset).  dst may equal src
// unless ext; neither ext nor pow_lo: nothing to do.
template <class F>
void poly_store(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, bool ext, const typename F::T* pow_lo,
                const typename F::T* pow_hi, hipStream_t stream);
// coordinate columns in LEAF order (lde_columns' output) -> NATURAL order in the caller's layout: dst[i] = src[bitrev(i)]
template <class F>
void poly_bitrev_store(const typename F::T* src, typename F::T* dst, size_t ncols, u32 log_len, bool ext, hipStream_t stream);
// row-major canonical leaves [num_rows][width] -> column-major device form [width][num_rows]; width <= ROWS_MAX_WIDTH
static constexpr u32 ROWS_MAX_WIDTH = 64 * 65535;
template <class F>
void rows_to_columns(const typename F::T* rows, typename F::T* cols, u64 num_rows, u32 width, hipStream_t stream);

// ---------------------------------------------------------------- Poseidon-12 Merkle (kernels_merkle.hip)

// leaf digests: out[j] = hash_or_noop(row j), row j = { cols[c*col_stride + j] : c < width }
void gl_merkle_leaves(const u64* cols, size_t col_stride, u32 width, u64 num_leaves, u64* out, hipStream_t stream);
// a column segment [c_begin, c_end) of every leaf's sponge, the state parked in `state` ([4 + 8 - keep_from][num_leaves], rows as used) between segments
void gl_merkle_leaves_segment(const u64* cols, size_t col_stride, u32 c_begin, u32 c_end, u64 num_leaves, u64* state, bool last,
                              u32 next_cols, u64* out, hipStream_t stream);
// one level: out[i] = two_to_one(in[2i], in[2i+1]), i < num_out
void gl_merkle_level(const u64* in, u64* out, u64 num_out, hipStream_t stream);
// one state per 16-lane row for small trees; false = not applicable (caller uses the lane-per-leaf kernel)
bool gl_fri_leaves_coop(const u64* vals, size_t len, u32 arity_bits, u64 num_leaves, u64* out, hipStream_t stream);
bool bb_fri_leaves_coop(const u32* vals, size_t len, u32 arity_bits, u64 num_leaves, u32* out, hipStream_t stream);
// level-major digests -> the reference's interleaved layout (hash/merkle_tree.rs:50-58)
void gl_digests_to_reference_layout(const u64* levels, u64* out, u32 log_leaves, u32 cap_height, hipStream_t stream);
// siblings of MerkleTree::prove(leaf) from level-major digests: dst[i] = level_i[(leaf >> i) ^ 1], i < layers
void gl_gather_siblings(const u64* levels, u32 log_leaves, u32 cap_height, u64 leaf, u64* dst, hipStream_t stream);
// raw permutation of `count` states (tests / microbenchmarks)
void gl_poseidon_permute(const u64* in, u64* out, u64 count, hipStream_t stream);

// ---------------------------------------------------------------- BabyBear Poseidon2-16 Merkle (kernels_bb.hip); element data in Montgomery form
void bb_merkle_leaves(const u32* cols, size_t col_stride, u32 width, u64 num_leaves, u32* out, hipStream_t stream);
void bb_merkle_leaves_segment(const u32* cols, size_t col_stride, u32 c_begin, u32 c_end, u64 num_leaves, u32* state, bool last,
                              u32 next_cols, u32* out, hipStream_t stream);  // state: [8 + 8 - keep_from][num_leaves]
void bb_merkle_level(const u32* in, u32* out, u64 num_out, hipStream_t stream);
void bb_poseidon2_permute(const u32* in, u32* out, u64 count, hipStream_t stream);  // canonical in/out
void bb_to_mont(const u32* src, u32* dst, size_t n, hipStream_t stream);
void bb_from_mont(const u32* src, u32* dst, size_t n, hipStream_t stream);

// ---------------------------------------------------------------- prover (kernels_prover.hip)
// Templated on the field traits of field_traits.hpp (GlF / BbF); element pointers are in the field's device form.

static constexpr u32 MAX_CHUNKS = 32, MAX_CHALLENGES = 16, MAX_RATE = 16;

template <class F>
struct PowTab {      // base^e = lo[e & (2^lo_bits - 1)] * hi[e >> lo_bits]
    const typename F::T* lo;
    const typename F::T* hi;
    u32 lo_bits;
};
template <class F>
struct ExtPowTab {   // same for an extension-field base
    const typename F::E* lo;
    const typename F::E* hi;
    u32 lo_bits;
};
template <class F>
struct CosetPow {    // per coset c: shift_c^t = lo[c][t % nlo] * hi[c][t / nlo]
    const typename F::T* lo;
    const typename F::T* hi;
    u32 nlo, nhi;
};
template <class F>
struct ZsParams {
    u32 log_n, num_routed, num_challenges, chunk /* quotient_degree_factor */, nchunks;
    PowTab<F> w_n;   // subgroup generator powers
    typename F::T betas[MAX_CHALLENGES], gammas[MAX_CHALLENGES];   // device form; by value: no upload between the transcript and the launch
};
template <class F>
struct QuotientParams {
    // rate_bits: log2 of the QUOTIENT domain's blow-up, quotient_degree_bits of prover.rs:735 (the first 2^rate_bits coset blocks of
    // the commitments' leaf-order LDEs ARE every step-th LDE point, step = 2^(fri rate_bits - quotient_degree_bits));
    // num_challenges: the challenges this launch computes
    u32 log_n, rate_bits, num_challenges, num_routed, num_constants /* selectors + constants */, num_selectors;
    u32 chunk, nchunks, nterms;
    u32 gate_constant, gate_pi, num_gate_consts;
    PowTab<F> w_N;   // LDE domain generator powers
    const typename F::T* l0;  // [N] L_0 on the LDE domain, leaf order (l0_table)
    u32 ext_gates;            // 1: the gate terms are already in qv (gate_constraints); 0: the dummy gate set, evaluated inline
    u32 stride_bits;          // log2 of a column's length in cs / wires / zs: log_n + the FRI rate_bits
    u32 k0, total_challenges; // a slice [k0, k0 + num_challenges) of total_challenges (sliced launches only; else 0, num_challenges)
};
template <class F>
struct GateParams {
    u32 log_n, rate_bits /* of the quotient domain, as QuotientParams */, num_challenges, nterms, t0 /* index of the first gate term */;
    gates::GateSet gs;
    u32 stride_bits;   // log2 of a column's length in cs / wires
};
// the constraint programs of a circuit's GB_GATE_PROGRAM gates for k_gate_programs: headers by value, tables on the device
template <class F>
struct ProgramParams {
    gates::ProgramSet ps;
    const u64* instrs;            // instruction words of all programs (ProgramInfo::instr_off)
    const typename F::T* lits;    // literals of all programs, device form (ProgramInfo::lit_off)
};
// the witness check (kernels_check.hip): the gate set and the number of rows; no challenges, nothing is folded
template <class F>
struct CheckParams {
    gates::GateSet gs;
    u32 n;
};
template <class F>
struct PolyGroups {
    const typename F::T* ptr[4];
    u32 ncols[4];
    u32 ngroups;
};
template <class F>
struct PowState {    // canonical sponge state before the candidate is written at `pos`
    typename F::T s[F::SPONGE_W];
    u32 pos;
};

template <class F>
void zs_partial_products(const ZsParams<F>& p, const typename F::T* witness, const typename F::T* sigma, const typename F::T* k_is,
                         typename F::T* q_tmp, typename F::T* zloc_tmp, typename F::T* totals_tmp, u32* err, typename F::T* out, hipStream_t st);
// false if (chunk, num_challenges) cannot be run (see quotient_shape_supported); challenge counts without a specialisation of
// their own run as slices of compiled widths (the uniforms are laid out for the total either way)
template <class F>
bool quotient_values(const QuotientParams<F>& p, const typename F::T* cs, const typename F::T* wires, const typename F::T* zs,
                     const typename F::T* uniforms, typename F::T* qv, hipStream_t st);
bool quotient_shape_supported(u32 field, u32 chunk, u32 num_challenges);
// what the test hooks of include/goldibear_gpu_test_hooks.h ask of gate_constraints' dispatch (host side only: no kernel reads it)
struct GateLaunchOptions {
    bool force_fallback = false;        // take the lane-per-point LIGHT_GATES launch even when a tiled plan exists
    u64* fallback_launches = nullptr;   // incremented per lane-per-point LIGHT_GATES launch, forced or not
};
// qv <- the alpha-folded gate constraints of a general gate set (kernels_gates.hip), any num_challenges <= MAX_CHALLENGES (slices)
template <class F>
bool gate_constraints(const GateParams<F>& p, const typename F::T* cs, const typename F::T* wires, const typename F::T* apow,
                      const typename F::T* pi_hash, typename F::T* qv, hipStream_t st, const ProgramParams<F>* programs = nullptr,
                      const GateLaunchOptions& opt = GateLaunchOptions());
// ---- gb_constraint_quotient (kernels_constraints.hip): the checked programs of constraint_system.hpp, headers and the oracles'
// LDE blocks by value, the flat tables on the device.  rate_bits is that of the quotient domain, stride_bits the log2 of a column's
// length in every oracle's LDE (log_n + the oracles' rate_bits).
template <class F>
struct ConstraintParams {
    u32 log_n, rate_bits, stride_bits, num_programs, nterms /* constraints of all programs: the length of one challenge's alpha powers */;
    PowTab<F> w_N;                       // powers of the quotient domain's generator
    const typename F::T* l0;             // [n 2^rate_bits] L_0 on the quotient domain, leaf order (l0_table); null when no program reads it
    const typename F::T* lde[constraints::MAX_ORACLES];   // [ncols + salt][2^stride_bits] each, leaf order
    constraints::ProgramInfo p[gates::MAX_PROGRAMS];
    u32 max_regs;
    const u64* instrs;                   // instruction words of all programs (ProgramInfo::instr_off)
    const u64* cells;                    // cell words of all programs (ProgramInfo::cell_off)
    const typename F::T* lits;           // literals of all programs, device form (ProgramInfo::lit_off)
    const typename F::T* params;         // [num_inputs - 3] device form
};
// qv[(k 2^rate_bits + coset) n + il] <- sum_i alpha_k^i constraint_i / Z_H for num_challenges <= MAX_CHALLENGES challenges (slices of
// widths 1 .. 4); apow: [num_challenges][nterms] alpha powers, zh_inv: [2^rate_bits], both device form
template <class F>
bool constraint_quotient_values(const ConstraintParams<F>& p, u32 num_challenges, const typename F::T* apow, const typename F::T* zh_inv,
                                typename F::T* qv, hipStream_t st);

// ---- the witness check (kernels_check.hip's launchers; witness_check.hpp has the row logic).  hv: the selector and constant
// columns as values on H, [num_selectors + num_constants][n], natural order, device form; wit: [num_wires][n] canonical words.
// counts[MAX_LISTS] and offsets[MAX_LISTS + 1]: rows per list (a list per gate, then the rows with a selector violation) and
// their exclusive scan
template <class F>
void check_count_rows(const gates::GateSet& gs, const typename F::T* hv, u32 n, u32* counts, u32* offsets, hipStream_t st);
// rows[offsets[l] .. offsets[l + 1]): the rows of list l, ascending
template <class F>
void check_fill_rows(const gates::GateSet& gs, const typename F::T* hv, u32 n, const u32* offsets, u32* rows, hipStream_t st);
// out[i][col]: the canonical selector values of row rows[i]
template <class F>
void check_selector_values(const typename F::T* hv, u32 n, u32 num_selectors, const u32* rows, u32 count, u64* out, hipStream_t st);
// gate g on the `count` rows of its list: fail_index[i] = the first constraint of row rows[i] that is not zero (or 0xFFFFFFFF),
// fail_value[i] its canonical value, *num_failed += the entries that have one.  pi_hash: device form
template <class F>
void check_gate_rows(const CheckParams<F>& p, u32 g, const ProgramParams<F>* programs, const u32* rows, u32 count, const typename F::T* hv,
                     const typename F::T* wit, const typename F::T* pi_hash, u32* fail_index, u64* fail_value, u32* num_failed, hipStream_t st);
// first[slot] = the lowest cell row * num_wires + column of the slot's class (slots: the map of gb_circuit_set_partition)
void check_first_cells(const u32* slots, u64 cells, u32 num_slots, u32* first, hipStream_t st);
// bit c of mask (64 cells per word) = cell c differs from the first cell of its class; *num_failed += those.  first = null: a
// slot IS its class's first cell (the labels of gb_circuit_decode_sigmas as the slot map, num_slots = the number of cells)
template <class F>
void check_copies(const u32* slots, const u32* first, u32 num_slots, const typename F::T* wit, u32 n, u32 num_wires, u64* mask,
                  u32* num_failed, hipStream_t st);
// out[i] = {value of cells[i], the first cell of its class, that cell's value}
template <class F>
void check_copy_report(const u32* slots, const u32* first, u32 num_slots, const typename F::T* wit, u32 n, u32 num_wires, const u32* cells,
                       u32 count, u64* out, hipStream_t st);
// *flag |= 1 if a word of v is not below p
template <class F>
void check_canonical(const typename F::T* v, size_t count, u32* flag, hipStream_t st);

// ---- the copy permutation out of the sigma columns (kernels_sigma.hip's launchers; sigma_decode.hpp has the arithmetic).  The
// routed cells are numbered i = col * n + row as the sigma values lie, `count` = num_routed_wires * n of them (below 2^32); a wire
// cell is row * num_wires + col.  state[i] = {next, label}: the cell sigma sends i to (sigma's numbering) and the lowest cell
// number met so far on i's cycle.
template <class F>
struct SigmaDecodeParams {
    sigma::DlogTables<F> t;                     // device pointers
    const typename F::T *k_pow_n, *k_inv;       // [num_routed], device form: k_is[j]^n and 1 / k_is[j]
    u32 num_routed, num_wires;
};
// words of the decode pass: the lowest cell whose value names no routed cell and the lowest cell whose target is shared (both
// start as all ones), and whether some target was hit twice
static constexpr u32 SIGMA_WORD_NO_CELL = 0, SIGMA_WORD_SHARED = 1, SIGMA_WORD_DOUBLE_HIT = 2, SIGMA_WORDS = 3;
// the tables of a decode launch live in LDS up to this size, in global memory above it
static constexpr size_t SIGMA_LDS_MAX_BYTES = 48 << 10;
// state[i] = {target of sigma[i] or sigma::NO_CELL, i's cell number}; seen: one bit per target, zeroed by the caller
template <class F>
void sigma_decode(const SigmaDecodeParams<F>& p, const typename F::T* sigma, u32 count, uint2* state, u32* seen, u32* words,
                  hipStream_t st);
// after a double hit: words[SIGMA_WORD_SHARED] = the lowest cell whose target another cell has too; hits: [count] scratch
void sigma_shared_target(const uint2* state, u32 count, u32* hits, u32* words, hipStream_t st);
// out[i] = {SIGMA_CLOSED, the label of i's whole cycle} where the cycle has at most SIGMA_WALK + 1 cells, else in[i]
static constexpr u32 SIGMA_WALK = 8, SIGMA_CLOSED = 0xFFFFFFFFu;
// ... and stats = {classes of two cells or more, the cells in them, the largest class (0: none)} of the closed cycles
void sigma_walk(const uint2* in, uint2* out, u32 count, u64* stats, hipStream_t st);
// one doubling round in -> out over the cells that are not closed; *changed = 1 if a label fell.  copy_closed: `out` does not
// hold the closed cells yet (the first round after the walk)
void sigma_round(const uint2* in, uint2* out, u32 count, bool copy_closed, u32* changed, hipStream_t st);
// stats += the same of the cycles the walk left open (after the rounds); sizes: [count] scratch
void sigma_class_stats(const uint2* state, u32 count, u32 lg, u32 num_wires, u32* sizes, u64* stats, hipStream_t st);
// labels[cell] of all wire cells: the lowest cell of the cell's cycle, a non-routed cell itself
void sigma_labels(const uint2* state, u64 cells, u32 lg, u32 num_wires, u32 num_routed, u32* labels, hipStream_t st);
// *lowest (starts as all ones) = the lowest routed cell whose class in the slot map starts at another cell than its label
void sigma_compare(const u32* labels, const u32* slots, const u32* first, u32 num_slots, u64 cells, u32 num_wires, u32 num_routed,
                   u32* lowest, hipStream_t st);

// ---- copy constraints -> sigma columns and representative map (kernels_wiring.hip's launchers; wiring.hpp has what a thread does).
// Targets, cells and routed cells are all below 2^32.  parent: [num_targets], the forest.
void wiring_init(u32* parent, u32 num_targets, hipStream_t st);
// one slice of `count` pairs ([count][2] target indices as the caller wrote them) that starts at pair `first`; err = {the lowest
// pair with an entry >= num_targets, the lowest pair that names a wire cell of a column >= num_routed}, all ones to start with
void wiring_union(const u64* pairs, u32 count, u64 first, u32* parent, u64 num_targets, u64 cells, u32 num_wires, u32 num_routed, u64* err,
                  hipStream_t st);
// one compression pass; *changed = 1 if a pointer moved
void wiring_jump(u32* parent, u32 num_targets, u32* changed, hipStream_t st);
// count[label]++ over the routed cells (count: [degree * num_wires], zeroed by the caller)
void wiring_count(const u32* parent, u32 routed, u32 num_routed, u32 num_wires, u32* count, hipStream_t st);
// exclusive scan of data[0 .. count) in place; sums: [wiring_scan_tiles(count)] scratch
u32 wiring_scan_tiles(u32 count);
void wiring_scan(u32* data, u32 count, u32* sums, hipStream_t st);
// the routed cells whose label counts two or more, in ascending cell order: tile_count[wiring_sort_tiles(routed)] first, then
// (after its scan) keys[pos] = label, cells[pos] = cell for the m kept ones
u32 wiring_sort_tiles(u32 count);
void wiring_keep_count(const u32* parent, const u32* count, u32 routed, u32 num_routed, u32 num_wires, u32* tile_count, hipStream_t st);
void wiring_compact(const u32* parent, const u32* count, u32 routed, u32 num_routed, u32 num_wires, const u32* tile_start, u32 m, u32* keys,
                    u32* cells, hipStream_t st);
// one stable pass of the radix sort by digit `pass` of the key; hist: [wiring::RADIX * wiring_sort_tiles(m)], sums: the scan's scratch for that many words
void wiring_sort_pass(const u32* keys, const u32* cells, u32 m, u32 pass, u32* hist, u32* sums, u32* keys_out, u32* cells_out, hipStream_t st);
// succ[col * n + row] = the cell that follows in the cell's run (succ: [routed], all ones where the caller left a cell alone);
// stats[0] += runs, stats[1] = max(stats[1], the longest run)
void wiring_successors(const u32* keys, const u32* cells, u32 m, const u32* count, u32 lg, u32 num_wires, u32 routed, u32* succ, u64* stats,
                       hipStream_t st);
// out[col * n + row] = k_is[col'] w^row' (canonical) of the successor, or of the cell itself; lo / hi: the split root tables
template <class F>
void wiring_sigmas(const typename F::T* lo, const typename F::T* hi, const typename F::T* k_is, const u32* succ, u32 routed, u32 lg,
                   u32 num_wires, typename F::T* out, hipStream_t st);
void wiring_widen(const u32* parent, u32 num_targets, u64* out, hipStream_t st);
// *merged += the targets with parent[t] != t
void wiring_merged(const u32* parent, u32 num_targets, u64* merged, hipStream_t st);

// l0[j] = Z_H(x_j) / (n (x_j - 1)), zh = device copy of the 2^rate_bits values of Z_H on the cosets
template <class F>
void l0_table(u32 log_n, u32 rate_bits, const PowTab<F>& w_N, const typename F::T* zh, typename F::T* l0, hipStream_t st);
template <class F>
void quotient_combine(u32 log_n, u32 rate_bits, u32 num_challenges, const typename F::T* a, const typename F::T* mat,
                      const CosetPow<F>& inv_shift, typename F::T* out, hipStream_t st);
// lo[e] = z^e (e < nlo), hi[h] = z^(1024 h) (h < nhi): the split tables of ExtPowTab (nlo = 1024) - or a plain list of powers
// (nhi = 0) - built on the device, up to six tables per launch (a proof needs zeta, zeta_next, their inverses and FRI's alpha at once)
template <class F>
struct ExtPowJob {
    typename F::E z;
    typename F::E *lo, *hi;
    u32 nlo, nhi;
};
static constexpr u32 EXT_POW_JOBS = 6;
template <class F>
struct ExtPowJobs {
    ExtPowJob<F> j[EXT_POW_JOBS];
};
template <class F>
void ext_powtabs(const ExtPowJobs<F>& jobs, u32 njobs, hipStream_t st);
// table_k[t] = z_k^t (t < n) from the split tables, for up to two points in one launch
template <class F>
struct ExtPowTables {
    ExtPowTab<F> z[2];
    typename F::E* table[2];
};
template <class F>
void ext_pow_tables(const ExtPowTables<F>& z, u32 count, size_t n, hipStream_t st);
// out[col] = sum_t coeffs_col[t] ztab[t] for every column of up to five batches (columns numbered through the jobs in order);
// partial_tmp: ceil(n / 4096) elements per column
template <class F>
struct EvalJob {
    const typename F::T* coeffs;   // [ncols][n]
    const typename F::E* ztab;     // the point's powers (ext_pow_tables)
    u32 ncols;
};
static constexpr u32 EVAL_JOBS = 5;
template <class F>
struct EvalJobs {
    EvalJob<F> j[EVAL_JOBS];
};
template <class F>
void eval_columns(const EvalJobs<F>& jobs, u32 njobs, size_t n, typename F::E* partial_tmp, typename F::E* out, hipStream_t st);
template <class F>
void reduce_polys(const PolyGroups<F>& g, size_t n, const typename F::E* apow, typename F::E* comp, hipStream_t st);
// reduce_polys_base for up to REDUCE_SLOTS batches of any FriInstanceInfo at once: comp[s][t] = sum_j alpha^j f_{s,j}[t].  The
// batches' polynomial lists arrive as a table of runs in DEVICE memory (written by a stream-ordered copy before the launch):
// a run is `ncols` consecutive columns base + k n of one oracle; column k has power index apow0[s] + k in slot s, or is not in
// slot s at all (REDUCE_ABSENT).  A column is read once per run, whichever slots it is in.
static constexpr u32 REDUCE_SLOTS = 4, REDUCE_ABSENT = 0xFFFFFFFFu;
template <class F>
struct ReduceRun {
    const typename F::T* base;
    u32 ncols;
    u32 apow0[REDUCE_SLOTS];
};
// apow: alpha^0 .. alpha^(longest batch - 1); comp: [nslots][n]
template <class F>
void reduce_batches(const ReduceRun<F>* runs_dev, u32 nruns, u32 nslots, size_t n, const typename F::E* apow, typename F::E* comp,
                    hipStream_t st);
template <class F>
void divide_by_linear_accumulate(const typename F::E* comp, size_t n, const ExtPowTab<F>& z, const ExtPowTab<F>& zinv,
                                 typename F::E shift, int first, typename F::E* sloc_tmp, typename F::E* totals_tmp,
                                 typename F::E* final_poly, hipStream_t st);
template <class F>
void ext_split(const typename F::E* src, size_t n, typename F::T* dst, hipStream_t st);
// vals = [D][len] coordinate columns in leaf order
template <class F>
void fri_leaves(const typename F::T* vals, size_t len, u32 arity_bits, u64 num_leaves, typename F::T* out, hipStream_t st);
template <class F>
void fri_fold(const typename F::T* in, size_t in_len, u32 arity_bits, typename F::E beta, typename F::T* out, hipStream_t st);
template <class F>
void pow_grind(const PowState<F>& s, u64 start, u64 count, u32 min_lz, u64* result, hipStream_t st);
// Query rounds (fri/prover.rs:190-255): every opened row and Merkle path of the proof in ONE launch per twelve trees and one
// device buffer (one read-back) - four oracle batches, then the FRI layers.  Job j writes its nidx rows at out + j.out (CANONICAL
// values) and the nidx paths (layers x H words each, level i = sibling of leaf >> i) behind them.
template <class F>
struct QueryJob {
    const typename F::T* vals;    // the oracle's LDE batch, column-major with `stride`; a FRI layer: [D][stride] coordinate columns, leaf order
    const typename F::T* levels;  // the tree's digest levels
    u64 stride;
    u64 out;
    u32 width;                    // base elements per opened row (FRI layer: D << arity_bits)
    u32 log_leaves, layers;       // layers = log_leaves - cap_height
    u32 shift;                    // leaf = query index >> shift
    u32 arity_bits, fri;
};
static constexpr u32 QUERY_JOBS = 12;
template <class F>
struct QueryJobs {
    QueryJob<F> j[QUERY_JOBS];
};
static constexpr u32 QUERY_IDX_INLINE = 64;   // up to this many query indices travel as a launch argument (idx_dev may be null then)
struct QueryIdx {
    u64 v[QUERY_IDX_INLINE];
};
template <class F>
void query_gather(const QueryJobs<F>& jobs, u32 njobs, const u64* idx_host, const u64* idx_dev, u32 nidx, typename F::T* out, hipStream_t st);

// ---- gb_verify_batch (kernels_verify.hip): the query rounds of a chunk of proofs of one circuit.
// `rounds` holds the proofs' query sections as they stand in the proof bytes, proof after proof, nqr rounds of round_bytes each
// (words canonical, at any byte offset); every offset below comes from the circuit's shape, none from a proof.  `records` holds
// one record of rec_bytes per proof:
//   E section: fri_alpha, red_open[2], alpha_shift[2], points[2], betas[num_layers], final_poly[final_len]   (device form)
//   at rec_x_off:    u64 x_indices[nqr]
//   at rec_caps_off: T wires_cap, zs_cap, quot_cap, layer_caps[num_layers], each H << cap_height canonical words
// A failing check writes min(key) into keys[proof], key = vq::fail_key(query round, position in the round) (verify_query.hpp).
static constexpr u32 VERIFY_ORACLES = 4, VERIFY_MAX_LAYERS = 32, VERIFY_MAX_TREES = VERIFY_ORACLES + VERIFY_MAX_LAYERS;
struct VerifyTree {
    u32 row_off, num_words;   // the opened row (or coset) inside a query round: byte offset, canonical words
    u32 path_off, path_len;   // its siblings: byte offset (behind the length byte), count
    u32 shift;                // leaf index = x_index >> shift
    u32 cap_word;             // word offset of the tree's cap in the record's caps; ~0u: the circuit's own cap
};
struct VerifyLayout {
    u32 num_proofs, nqr, lgN, num_layers, final_len, round_bytes, rec_bytes, rec_x_off, rec_caps_off;
    u32 batch_sizes[2];                  // every polynomial of the four oracles at zeta; the Zs at g zeta
    u32 widths[VERIFY_ORACLES];          // polynomials per oracle (a salted row is longer: the salts are hashed, never combined)
    u32 arity_bits[VERIFY_MAX_LAYERS];
    VerifyTree trees[VERIFY_MAX_TREES];  // the four oracles, then the layers
};
template <class F>
void verify_paths(const VerifyLayout& L, const unsigned char* rounds, const unsigned char* records, const typename F::T* circuit_cap,
                  u64* keys, hipStream_t st);
template <class F>
void verify_queries(const VerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st);

// ---- gb_fri_verify_batch (kernels_verify.hip): the same two kernels over ANY FriInstanceInfo.  What the layout above holds as
// arrays of fixed size lives in device memory here - uploaded once per call, resident for all of its chunks:
//   trees[num_oracles + num_layers]   VerifyTree as above; every tree's cap is in the item's record (cap_word is never ~0u), and an
//                                     oracle's num_words counts its salts (hiding && blinding), which are hashed and never combined
//   arity_bits[num_layers], batch_sizes[num_batches]
//   batch_base[num_batches]           the first entry of batch b in poly_off (the prefix sums of batch_sizes)
//   poly_off[sum of batch_sizes]      per entry of `polynomials`: the byte offset inside a query round of that polynomial's word -
//                                     (oracle_index, polynomial_index) resolved by the host, once
// `rounds` is as above.  An item's record:
//   E section: fri_alpha, red_open[num_batches], alpha_shift[num_batches], points[num_batches], betas[num_layers],
//              final_poly[final_len]                                                                        (device form)
//   at rec_x_off:    u64 x_indices[nqr]
//   at rec_caps_off: T initial caps [num_oracles], layer_caps[num_layers], each H << cap_height canonical words
// Keys as above, with num_oracles in the positions (verify_query.hpp): num_oracles + 2 * num_layers + 1 < 2^POS_BITS.
struct FriVerifyLayout {
    u32 num_proofs, nqr, lgN, num_oracles, num_batches, num_layers, final_len, round_bytes, rec_bytes, rec_x_off, rec_caps_off;
    const VerifyTree* trees;
    const u32 *arity_bits, *batch_sizes, *batch_base, *poly_off;
};
template <class F>
void fri_verify_paths(const FriVerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st);
template <class F>
void fri_verify_queries(const FriVerifyLayout& L, const unsigned char* rounds, const unsigned char* records, u64* keys, hipStream_t st);

// ---- gb_verify_compressed_batch (kernels_verify.hip): the same checks on COMPRESSED proofs (verify_compressed.hpp).  A proof's
// query section - per tree the entries of its distinct indices, as they stand behind the stored indices - lies at
// rounds + proof * proof_stride, and its record carries a directory behind the caps:
//   at rec_dir_off: u32 entry[VERIFY_ORACLES + num_layers][nqr]   byte offset, inside the proof's query section, of the entry of
//                   query round k in tree t: the row (a layer: the coset without its inferred element), one length byte, the
//                   stored siblings.  The host has checked every entry against the proof's length and its sibling count against
//                   what the indices demand; the kernels never read past trees[t].path_len siblings, which proof_stride pads for.
// In L, trees[t].num_words is the full leaf (a layer's re-inflated coset) and row_off / path_off are unused.
// `inferred` is scratch of num_proofs * num_layers * nqr * D words: verify_compressed_queries leaves there, per layer and query
// round, the element its coset lacks (canonical) - the layer trees' leaves of verify_compressed_paths, which therefore runs second.
// A proof's query rounds share one workgroup: nqr <= VERIFY_COMPRESSED_MAX_QUERIES.
static constexpr u32 VERIFY_COMPRESSED_MAX_QUERIES = 256;
struct VerifyCompressedLayout {
    VerifyLayout L;
    u32 proof_stride, rec_dir_off;
};
template <class F>
void verify_compressed_queries(const VerifyCompressedLayout& C, const unsigned char* rounds, const unsigned char* records,
                               typename F::T* inferred, u64* keys, hipStream_t st);
template <class F>
void verify_compressed_paths(const VerifyCompressedLayout& C, const unsigned char* rounds, const unsigned char* records,
                             const typename F::T* circuit_cap, const typename F::T* inferred, u64* keys, hipStream_t st);

}  // namespace gbk

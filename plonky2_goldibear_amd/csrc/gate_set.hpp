// The gate set of a circuit as the kernels and the host code pass it around (CommonCircuitData.gates + selectors_info).
#pragma once
#include "../../include/goldibear_gpu.h"

namespace gbk {
namespace gates {

constexpr unsigned MAX_GATES = 24;  // DefaultGateSerializer knows 20 gate types (util/serialization/gate_serialization.rs:143-165)
constexpr unsigned UNUSED_SELECTOR = 0xFFFFFFFFu;  // gates/selectors.rs:13
constexpr unsigned POSEIDON_NUM_CONSTRAINTS = 12 * 7 + 22 + 12 + 1 + 4;
constexpr unsigned POSEIDON2_BB_CONSTRAINTS_PER_OP = 1 + 8 + 16 * 7 + 13 + 16;  // 150
constexpr unsigned POSEIDON2_BB_WIRES_PER_OP = 33 + 8 + 16 * 7 + 13;           // 166

constexpr unsigned MAX_INTERPOLATION_BITS = 4;   // CosetInterpolationGate subgroup_bits (= a FRI arity_bits, <= 4 here)
constexpr unsigned MAX_RANDOM_ACCESS_BITS = 6;   // (2 + 2^bits) routed wires per copy

// Constraint programs (GB_GATE_PROGRAM, include/goldibear_gpu.h): the limits checked at create and the decoded headers.  The
// instruction words and the literals (device form) of all programs lie in two flat tables; a ProgramInfo points into them.
constexpr unsigned MAX_PROGRAMS = 16, MAX_PROGRAM_INSTRS = 4096, MAX_PROGRAM_REGS = 32, MAX_PROGRAM_LITERALS = 256,
                   MAX_PROGRAM_CONSTRAINTS = 1024;
constexpr unsigned PROGRAM_HEADER_WORDS = 4;
enum ProgramOp { PROG_ADD = 0, PROG_SUB = 1, PROG_MUL = 2, PROG_EMIT = 3 };
enum ProgramSpace { PROG_REG = 0, PROG_WIRE = 1, PROG_CONST = 2, PROG_LIT = 3 };
struct ProgramInfo {
    unsigned num_wires, num_constants, num_constraints, degree, num_regs, num_literals, num_instrs;
    unsigned lit_off, instr_off;   // first literal / first instruction word in the flat tables
};
struct ProgramSet {
    unsigned num_programs, max_regs;
    ProgramInfo p[MAX_PROGRAMS];
};

struct GateSet {
    unsigned num_gates, num_selectors;
    gb_gate g[MAX_GATES];
    // two_adic_subgroup(4) and 1 / 2^b (b = 0..4) in the field's device form (u32 values for BabyBear), for
    // CosetInterpolationGate: its domain is every (16 >> b)-th entry and its barycentric weights are x_i / 2^b
    unsigned long long subgroup16[16], inv_pow2[MAX_INTERPOLATION_BITS + 1];
};

}  // namespace gates
}  // namespace gbk

// What the generator schedule (generator_schedule.hpp, host) hands to the generator kernels (generators.hpp, device): plain words,
// no HIP and no field code, so that either side compiles without the other.
//
// An Op is one scheduled generator.  Its dependencies and outputs are class indices in `args` (the dense class index of the
// schedule: the slots of partition_map.hpp first), in the order the generator's gate lays its wires out; an output entry carries
// what the schedule resolved for it: store (plain index), check (OUT_CHECK set: compare with the stored value, do not write) or
// OUT_SKIP (written or checked by another Op of the same generator).
#ifndef GOLDIBEAR_GENERATOR_OPS_HPP
#define GOLDIBEAR_GENERATOR_OPS_HPP

#include <stdint.h>

namespace gbk {
namespace gen {

// record kinds: the values of GB_GEN_* (include/goldibear_gpu.h)
enum Kind : uint32_t {
    GEN_ARITHMETIC = 0,
    GEN_ARITHMETIC_EXTENSION = 1,
    GEN_MUL_EXTENSION = 2,
    GEN_CONSTANT = 3,
    GEN_BASE_SPLIT = 4,
    GEN_REDUCING = 5,
    GEN_REDUCING_EXTENSION = 6,
    GEN_RANDOM_ACCESS = 7,
    GEN_POSEIDON_MDS = 8,
    GEN_COSET_INTERPOLATION = 9,
    GEN_EXPONENTIATION = 10,
    GEN_POSEIDON = 11,
    GEN_POSEIDON2_BABYBEAR = 12,
    GEN_ADD_MANY = 13,
    GEN_APPLY_MAT4 = 14,
    GEN_POSEIDON2_INTERNAL = 15,
    GEN_COPY = 16,
    GEN_NUM_KINDS = 17,   // gate generators and Copy: 17 .. 31 are reserved and refused
    // gadget generators: a head record (gate = the parameter, a = the number of targets, b = 0) and ceil(a / 2) GEN_TARGETS
    // continuation records that carry two targets each, in the order given beside the kind
    GEN_EQUALITY = 32,             // x, y, equal, inv
    GEN_NONZERO_TEST = 33,         // to_test, dummy
    GEN_QUOTIENT_OR_ZERO = 34,     // numerator, denominator, quotient
    GEN_QUOTIENT_EXTENSION = 35,   // numerator[D], denominator[D], quotient[D]
    GEN_SPLIT = 36,                // integer, bits[0..64]
    GEN_WIRE_SPLIT = 37,           // integer, the WIRE_SUM target of each gate; parameter num_limbs
    GEN_LOW_HIGH = 38,             // integer, low, high; parameter n_log
    GEN_BASE_SUM = 39,             // sum, limbs[1..]; parameter B
    GEN_TARGETS = 40,              // continuation
    GEN_GADGET_FIRST = GEN_EQUALITY,
    GEN_GADGET_END = GEN_TARGETS,   // one past the last head kind of the built-in gadgets: 41 .. 47 are reserved and refused
    // a generator program (below): a head record (gate = the program's index, a = the number of targets, b = the row whose
    // constants the program reads) and its GEN_TARGETS records: the num_in dependencies, then the num_out outputs
    GEN_PROGRAM = 48
};

constexpr uint32_t GROUP = 256;   // the chain kernel's workgroup: a level up to this wide stays inside a chain launch
// the kinds generators.hpp evaluates (generator_schedule.hpp refuses the others): every gate generator, Copy and the gadget heads
constexpr bool built_kind(uint32_t kind) {
    return kind < GEN_NUM_KINDS || (kind >= GEN_GADGET_FIRST && kind < GEN_GADGET_END) || kind == GEN_PROGRAM;
}
constexpr uint32_t OUT_CHECK = 0x80000000u, OUT_SKIP = 0xFFFFFFFFu, MAX_CLASSES = 0x7FFFFFFFu;

struct Op {
    uint32_t kind;      // Kind
    uint32_t record;    // index of the gb_generator record (error reports)
    uint32_t in_off;    // args[in_off .. in_off + num_in): dependency classes
    uint32_t num_in;
    uint32_t out_off;   // args[out_off .. out_off + num_out): output classes | OUT_CHECK, or OUT_SKIP
    uint32_t num_out;
    uint32_t p0, p1;    // the gate's parameters as its evaluator reads them; a gadget generator's parameter is p0;
                        // GEN_PROGRAM: p0 the program's index, p1 the first of its row's constants in the row-constants array
    uint64_t k[2];      // the row's constants, canonical words
};

// the device error word: code (0 = none), record index, class
enum Error : uint32_t {
    ERR_NONE = 0,
    ERR_SET_TWICE = 1,        // "Partition containing ... was set twice with different values" (iop/witness.rs:340-350)
    ERR_SWAP_NOT_BOOLEAN = 2,  // PoseidonGenerator / Poseidon2BabyBearGenerator: assert!(swap == 0 || swap == 1)
    ERR_ACCESS_INDEX = 3,      // RandomAccessGenerator: index >= vec_size
    ERR_SPLIT_TOO_LARGE = 4,   // BaseSplitGenerator: "Integer too large to fit in given number of limbs"; SplitGenerator and
                               // WireSplitGenerator: the reference's debug_assert_eq!(integer_value, 0, ..)
    ERR_DIVIDE_BY_ZERO = 5,    // QuotientGeneratorExtension: num / dem with dem == 0 ("Tried to invert zero")
    ERR_NOT_BOOLEAN = 6,       // BaseSumGenerator: get_bool_target, "not a bool"
    ERR_NO_SQUARE_ROOT = 7,    // a generator program's SQRT of a non-residue (examples/square_root.rs: sqrt(x).unwrap() on None)
    ERR_NO_PROGRAM_TABLES = 8,  // a GEN_PROGRAM op met by run_op without its `programs`: the caller's mistake.  Host builds report it;
                                // for the kernels generator_schedule.hpp device_schedule() refuses such a schedule on the host
    ERR_INTEGER_DIVIDE_BY_ZERO = 9   // a generator program's IDIV or IREM by zero ("attempt to divide by zero")
};
constexpr uint32_t ERROR_WORDS = 4;   // code, record, class, 0

struct Launch {
    uint32_t first_level;   // index into level_off (level 1 of the schedule is index 0)
    uint32_t num_levels;    // chain: a run of narrow levels in one workgroup; level kernel: 1
    uint32_t chain;
};

// Generator programs (include/goldibear_gpu.h, "generator programs"): a witness generator as a straight-line program in the
// word layout of the constraint programs (gates.hpp run_program).  The opcode is (w & 3) | ((w >> 56) & 0xF) << 2: ADD, SUB and
// MUL as there, OUT in EMIT's place, and the unary operations reg[dst] = op(a) above them.  From 16 on, the integer operations:
// binary, on the canonical representatives of a and b in [0, p) - quotient, remainder, right shift by a value, bitwise and, less
// than.  8 .. 15 and everything from GP_NUM_OPCODES on are no opcodes.  generator_programs.hpp checks the words; the decoded
// headers, the instruction words and the literals of all programs lie in three flat tables.
enum ProgramOpcode : uint32_t {
    GP_ADD = 0, GP_SUB = 1, GP_MUL = 2, GP_OUT = 3, GP_INV = 4, GP_INV_OR_ZERO = 5, GP_IS_ZERO = 6, GP_SQRT = 7,
    GP_FIELD_END = 8,   // one past the field operations
    GP_IDIV = 16, GP_IREM = 17, GP_SHR = 18, GP_AND = 19, GP_LT = 20, GP_NUM_OPCODES = 21
};
constexpr bool gen_program_is_opcode(uint32_t op) { return op < GP_FIELD_END || (op >= GP_IDIV && op < GP_NUM_OPCODES); }
constexpr bool gen_program_is_binary(uint32_t op) { return op < GP_OUT || (op >= GP_IDIV && op < GP_NUM_OPCODES); }   // reads operand b
constexpr uint32_t MAX_GENERATOR_PROGRAMS = 256, MAX_PROGRAM_TARGETS = 1024;
constexpr uint32_t gen_program_opcode(uint64_t w) { return ((uint32_t)w & 3) | (((uint32_t)(w >> 56) & 0xF) << 2); }
struct ProgramHeader {
    uint32_t num_in, num_constants, num_out, num_regs, num_literals, num_instrs;
    uint32_t lit_off, instr_off;   // first literal / first instruction word in the flat tables
};

struct DeviceSchedule {   // the schedule's arrays on the device
    const Op* ops;
    const uint32_t *args, *level_off;
    // with generator programs: their tables (literals in the field's device form, one per word), the row constants of the
    // schedule's program generators (canonical) and the registers of the largest program among them (0: the schedule holds none)
    const ProgramHeader* programs = nullptr;
    const uint64_t *program_instrs = nullptr, *program_lits = nullptr, *row_constants = nullptr;
    uint32_t program_regs = 0;
};

}  // namespace gen
}  // namespace gbk
#endif

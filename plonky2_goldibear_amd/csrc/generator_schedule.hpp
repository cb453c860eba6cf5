// The schedule of gb_circuit_set_generators (include/goldibear_gpu.h): generate_partial_witness (iop/generator.rs:25-106) turned
// from a work list that is polled until nothing moves into data that is resolved once per circuit.
//
// Input: the circuit's gate table and config, the representative map of gb_circuit_set_partition with the slots that
// partition_map.hpp made of it, the constants columns, the input targets (what the host supplies per proof: PartialWitness and
// every RandomValueGenerator target) and the generator records.  Output:
//   classes   a dense index over every copy class that a wire cell, an input, a public input or a generator touches: the slots of
//             partition_map.hpp first, unchanged (k_expand_partition reads the front of the values array), then the classes that
//             only virtual targets use, in ascending order of their representative;
//   levels    inputs are level 0; a generator runs one level after the last of its dependencies is stored.  Within a level the
//             generators are sorted by kind (stable in record order), so a wave runs one kind;
//   writers   the first writer of a class in (level, record) order stores; every later writer, and every writer of an input
//             class, only compares ("check") - the reference's "Partition containing .. was set twice with different values"
//             (iop/witness.rs:340-350) - and does so at least one level after the store, so the kernels need no atomics;
//   unrunnable generators: a dependency that no input and no generator ever sets.  They are left out and counted; their outputs
//             stay zero (unwrap_or(ZERO)); the reference panics with "{n} generators weren't run";
//   launches  a maximal run of consecutive levels that are each no wider than one workgroup is ONE launch of the chain kernel;
//             any wider level is one launch of the level kernel.
//
// A gate generator is one record (gate, row, operation); CopyGenerator is one record of two targets.  The gadget generators
// (Equality, NonzeroTest, QuotientOrZero, QuotientExtension, Split, WireSplit, LowHigh, BaseSum: kinds 32..39) name arbitrary
// targets: a head record (gate = the generator's parameter, a = the number of targets, b = 0) followed by ceil(a / 2)
// GEN_TARGETS records of two targets each.  Their dependencies and outputs are those targets, taken through the representative
// map as Copy's are; an error report names the head's index.  A malformed sequence - a continuation without a head, one that
// runs past the array or meets another kind, a count or parameter that does not fit the kind, non-zero b, gate or padding, a
// target out of range - answers INVALID with the record index; nothing is read past num_records.
//
// A generator program (GEN_PROGRAM, generator_programs.hpp) is one more generator of this shape: its head names the program (gate),
// the number of targets (a = num_in + num_out of the program) and the row whose constants it reads (b; 0 for a program without
// constants); the first num_in targets are its dependencies, the rest its outputs.  With wire targets it is the generator of a
// program gate, with virtual targets a gadget's.  The schedule copies constants[j][row], j < num_constants, into row_constants;
// the Op carries the program's index (p0) and the offset of its constants there (p1).
//
// Record kinds that are not built answer UNSUPPORTED: every kind outside built_kind() (generator_ops.hpp: what generators.hpp
// evaluates; 17..31 and 41..47 are reserved), a gate generator's record that names a program gate, the lookup pair, the
// Poseidon2-Risc0 gate and DummyProofGenerator, none of which has a record kind.
//
// Host code without HIP dependencies: tests/sanitize/generator_schedule.cpp compiles it alone with the sanitizers.
#ifndef GOLDIBEAR_GENERATOR_SCHEDULE_HPP
#define GOLDIBEAR_GENERATOR_SCHEDULE_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "generator_ops.hpp"
#include "generator_programs.hpp"

namespace gbk {
namespace gen {

enum ScheduleStatus { SCHED_OK = 0, SCHED_INVALID = 1, SCHED_UNSUPPORTED = 4 };   // GB_OK / GB_ERR_INVALID / GB_ERR_UNSUPPORTED

struct Record {   // gb_generator
    uint32_t kind, gate;
    uint64_t a, b;
};
struct GateDesc {   // of gb_gate
    uint32_t kind, param, param2, param3;
};
// gb_gate.kind of the gates that have generators (include/goldibear_gpu.h GB_GATE_*)
enum : uint32_t {
    G_CONSTANT = 1, G_ARITHMETIC = 3, G_POSEIDON = 4, G_POSEIDON2_BABYBEAR = 5, G_ARITHMETIC_EXTENSION = 6, G_MUL_EXTENSION = 7,
    G_BASE_SUM = 8, G_REDUCING = 9, G_REDUCING_EXTENSION = 10, G_RANDOM_ACCESS = 11, G_POSEIDON_MDS = 12, G_COSET_INTERPOLATION = 13,
    G_EXPONENTIATION = 14, G_ADD_MANY = 15, G_APPLY_MAT4 = 16, G_POSEIDON2_INTERNAL = 17, G_PROGRAM = 18
};

struct CircuitDesc {
    const uint32_t* representative_map = nullptr;   // [num_targets], every entry below num_targets (build_slot_map checked it)
    uint64_t num_targets = 0;
    uint32_t num_wires = 0, degree_bits = 0, num_constants = 0;
    uint32_t ext_degree = 2;                        // D: 2 Goldilocks, 4 BabyBear
    uint64_t order = 0;                             // the field's order: constants must lie below it
    const uint32_t* slot_reps = nullptr;            // SlotMap::reps, ascending
    size_t num_slots = 0;
    const uint32_t* pi_reps = nullptr;              // SlotMap::pi_reps
    size_t num_public_inputs = 0;
    const GateDesc* gates = nullptr;
    uint32_t num_gates = 0;
    const uint64_t* constants = nullptr;            // [num_constants][2^degree_bits] canonical words
    const GeneratorPrograms* programs = nullptr;    // of gb_circuit_set_generator_programs; null: none set
};

struct Schedule {
    uint32_t num_classes = 0, num_slots = 0, num_levels = 0, num_unrunnable = 0, num_checks = 0;
    std::vector<uint32_t> class_reps;    // [num_classes] the representative target of each class
    std::vector<uint32_t> input_cls;     // [num_inputs]
    std::vector<uint32_t> input_first;   // [num_inputs] the first input of the same class (itself when it is the first)
    std::vector<uint8_t> input_free;     // [num_inputs] no generator reads, writes or checks the input's class
    std::vector<uint32_t> pi_cls;        // [num_public_inputs]
    std::vector<Op> ops;                 // sorted by (level, kind)
    std::vector<uint32_t> args;
    std::vector<uint32_t> level_off;     // [num_levels + 1] into ops; entry l is level l + 1
    std::vector<Launch> launches;
    std::vector<uint64_t> row_constants;   // the constants of the program generators' rows, canonical (Op::p1 points into it)
    uint32_t program_regs = 0;             // the registers of the largest program a generator of the schedule runs; 0: none does
};

// The DeviceSchedule of a Schedule whose arrays lie on the device: how the launches' callers make one.  program_regs and the
// program tables travel with the ops, never apart: the kernels of a schedule without programs (program_regs == 0) hold no code
// for a program op and would leave its outputs zero without a word.  false, with a message: a program op without registers or
// without one of the tables.
inline bool device_schedule(const Schedule& s, const Op* ops, const uint32_t* args, const uint32_t* level_off, const ProgramHeader* programs,
                            const uint64_t* program_instrs, const uint64_t* program_lits, const uint64_t* row_constants, DeviceSchedule* out,
                            std::string* msg) {
    for (const Op& op : s.ops)
        if (op.kind == GEN_PROGRAM && (!s.program_regs || !programs || !program_instrs || !program_lits || !row_constants)) {
            *msg = "generator record " + std::to_string(op.record) + ": a program generator in a schedule " +
                   (s.program_regs ? "without the program tables" : "that asks for no program registers");
            return false;
        }
    *out = DeviceSchedule{ops, args, level_off, programs, program_instrs, program_lits, row_constants, s.program_regs};
    return true;
}

namespace detail {

inline uint32_t expected_gate(uint32_t kind) {
    switch (kind) {
        case GEN_ARITHMETIC: return G_ARITHMETIC;
        case GEN_ARITHMETIC_EXTENSION: return G_ARITHMETIC_EXTENSION;
        case GEN_MUL_EXTENSION: return G_MUL_EXTENSION;
        case GEN_BASE_SPLIT: return G_BASE_SUM;
        case GEN_REDUCING: return G_REDUCING;
        case GEN_REDUCING_EXTENSION: return G_REDUCING_EXTENSION;
        case GEN_RANDOM_ACCESS: return G_RANDOM_ACCESS;
        case GEN_POSEIDON_MDS: return G_POSEIDON_MDS;
        case GEN_COSET_INTERPOLATION: return G_COSET_INTERPOLATION;
        case GEN_EXPONENTIATION: return G_EXPONENTIATION;
        case GEN_POSEIDON: return G_POSEIDON;
        case GEN_POSEIDON2_BABYBEAR: return G_POSEIDON2_BABYBEAR;
        case GEN_ADD_MANY: return G_ADD_MANY;
        case GEN_APPLY_MAT4: return G_APPLY_MAT4;
        case GEN_POSEIDON2_INTERNAL: return G_POSEIDON2_INTERNAL;
        default: return 0xFFFFFFFFu;
    }
}

// the columns a gate generator reads and writes, in the order its evaluator (generators.hpp) takes them.  false: the operation,
// copy or constant index is outside the gate's parameters
inline bool gate_columns(uint32_t kind, const GateDesc& g, uint64_t b, uint32_t D, std::vector<uint32_t>* deps, std::vector<uint32_t>* outs,
                         uint32_t* p0, uint32_t* p1, int* k_from) {
    auto run = [](std::vector<uint32_t>* v, uint32_t start, uint32_t count) {
        for (uint32_t i = 0; i < count; i++) v->push_back(start + i);
    };
    const uint32_t op = (uint32_t)b;
    k_from[0] = k_from[1] = -1;   // which constants column k[i] is read from
    *p0 = g.param;
    *p1 = g.param2;
    switch (kind) {
        case GEN_ARITHMETIC:
            if (b >= g.param) return false;
            run(deps, 4 * op, 3);
            run(outs, 4 * op + 3, 1);
            k_from[0] = 0; k_from[1] = 1;
            return true;
        case GEN_ARITHMETIC_EXTENSION:
            if (b >= g.param) return false;
            run(deps, 4 * D * op, 3 * D);
            run(outs, 4 * D * op + 3 * D, D);
            k_from[0] = 0; k_from[1] = 1;
            return true;
        case GEN_MUL_EXTENSION:
            if (b >= g.param) return false;
            run(deps, 3 * D * op, 2 * D);
            run(outs, 3 * D * op + 2 * D, D);
            k_from[0] = 0;
            return true;
        case GEN_CONSTANT:   // ConstantGate's wire i, or an extra constant of a RandomAccessGate
            if (g.kind == G_CONSTANT) {
                if (b >= g.param) return false;
                run(outs, op, 1);
            } else {
                if (b >= g.param3) return false;
                run(outs, (2 + (1u << g.param)) * g.param2 + op, 1);
            }
            k_from[0] = (int)op;
            return true;
        case GEN_BASE_SPLIT:
            if (b != 0) return false;
            run(deps, 0, 1);
            run(outs, 1, g.param);
            *p1 = g.param2 ? g.param2 : 2;
            return true;
        case GEN_REDUCING:
        case GEN_REDUCING_EXTENSION: {
            if (b != 0) return false;
            const uint32_t n = g.param, cw = kind == GEN_REDUCING ? 1 : D, start_accs = 3 * D + n * cw;
            run(deps, D, 2 * D + n * cw);
            for (uint32_t i = 0; i < n; i++) run(outs, i == n - 1 ? 0 : start_accs + D * i, D);
            return true;
        }
        case GEN_RANDOM_ACCESS: {
            if (b >= g.param2) return false;
            const uint32_t vec = 1u << g.param, routed = (2 + vec) * g.param2 + g.param3;
            run(deps, (2 + vec) * op, 1);
            run(outs, routed + op * g.param, g.param);
            return true;
        }
        case GEN_POSEIDON_MDS:
            if (b != 0) return false;
            run(deps, 0, 12 * D);
            run(outs, 12 * D, 12 * D);
            return true;
        case GEN_COSET_INTERPOLATION: {
            if (b != 0) return false;
            const uint32_t npts = 1u << g.param, nint = g.param2 > 1 ? (npts - 2) / (g.param2 - 1) : 0;
            const uint32_t start_point = 1 + npts * D, start_int = start_point + 2 * D;
            run(deps, 0, 1 + npts * D + D);
            run(outs, start_int + 2 * D * nint, D);   // the shifted evaluation point
            for (uint32_t i = 0; i < nint; i++) {
                run(outs, start_int + D * i, D);
                run(outs, start_int + D * (nint + i), D);
            }
            run(outs, start_point + D, D);
            return true;
        }
        case GEN_EXPONENTIATION:
            if (b != 0) return false;
            run(deps, 0, 1 + g.param);
            run(outs, 2 + g.param, g.param);
            run(outs, 1 + g.param, 1);
            return true;
        case GEN_POSEIDON:
            if (b != 0) return false;
            run(deps, 0, 12);
            run(deps, 24, 1);
            run(outs, 25, 110);   // the deltas and every s-box input
            run(outs, 12, 12);
            return true;
        case GEN_POSEIDON2_BABYBEAR:
            if (b >= g.param) return false;
            run(deps, 33 * op, 16);
            run(deps, 33 * op + 32, 1);
            run(outs, 33 * g.param + 133 * op, 133);
            run(outs, 33 * op + 16, 16);
            return true;
        case GEN_ADD_MANY:
            if (b >= g.param2) return false;
            run(deps, (g.param + 1) * op, g.param);
            run(outs, (g.param + 1) * op + g.param, 1);
            return true;
        case GEN_APPLY_MAT4:
            if (b >= g.param) return false;
            run(deps, 8 * D * op, 4 * D);
            run(outs, 8 * D * op + 4 * D, 4 * D);
            return true;
        case GEN_POSEIDON2_INTERNAL:
            if (b != 0) return false;
            run(deps, 0, 16 * D);
            run(outs, 16 * D, 16 * D);
            return true;
        default:
            return false;
    }
}

}  // namespace detail

// *msg names what was refused.  group_width: the chain kernel's workgroup size.
inline ScheduleStatus build_schedule(const CircuitDesc& c, const Record* records, size_t num_records, const uint64_t* input_targets,
                                     size_t num_inputs, uint32_t group_width, Schedule* out, std::string* msg) {
    std::string unused;
    if (!msg) msg = &unused;
    auto refuse = [&](ScheduleStatus s, const std::string& m) { *msg = m; return s; };
    if (!out || !c.representative_map || (num_records && !records) || (num_inputs && !input_targets) || (c.num_gates && !c.gates) ||
        (c.num_slots && !c.slot_reps) || (c.num_public_inputs && !c.pi_reps) || (c.num_constants && !c.constants))
        return refuse(SCHED_INVALID, "null argument");
    if (!group_width || c.degree_bits > 31 || (c.num_targets >> 32)) return refuse(SCHED_INVALID, "circuit description out of range");
    const uint64_t n = (uint64_t)1 << c.degree_bits, NT = c.num_targets;
    if (num_records >> 31) return refuse(SCHED_UNSUPPORTED, "2^31 generator records or more");
    const uint32_t NONE = 0xFFFFFFFFu;

    // ---- records -> targets
    struct Gen {
        uint32_t kind, record, in_off, num_in, out_off, num_out, p0, p1;
        uint64_t k[2];
    };
    std::vector<Gen> gens;
    gens.reserve(num_records);
    std::vector<uint32_t> args;   // targets first, classes after the translation below
    std::vector<uint32_t> dcols, ocols;
    std::vector<uint64_t> s_row_constants;
    uint32_t program_regs = 0;
    bool any_program = false;
    for (size_t r = 0; r < num_records; r++) {
        const Record& rec = records[r];
        const std::string name = "generator record " + std::to_string(r);
        if (rec.kind == GEN_TARGETS) return refuse(SCHED_INVALID, name + ": a continuation record without a head record in front of it");
        if (!built_kind(rec.kind)) return refuse(SCHED_UNSUPPORTED, name + ": kind " + std::to_string(rec.kind) + " is no built generator kind");
        Gen g{rec.kind, (uint32_t)r, (uint32_t)args.size(), 0, 0, 0, 0, 0, {0, 0}};
        if (rec.kind >= GEN_GADGET_FIRST) {
            // a head and its continuation: the targets, dependencies first
            const uint64_t count = rec.a, D = c.ext_degree;
            bool count_ok = false, param_ok = rec.gate == 0;
            uint64_t num_in = 1;
            const ProgramHeader* prog = nullptr;
            if (rec.kind == GEN_PROGRAM) {
                if (!c.programs || c.programs->empty()) return refuse(SCHED_INVALID, name + ": no generator programs are set");
                if (rec.gate >= c.programs->headers.size())
                    return refuse(SCHED_INVALID, name + ": program index " + std::to_string(rec.gate) + " of " + std::to_string(c.programs->headers.size()));
                prog = &c.programs->headers[rec.gate];
                if (count != (uint64_t)prog->num_in + prog->num_out)
                    return refuse(SCHED_INVALID, name + ": " + std::to_string(count) + " targets, the program has " + std::to_string(prog->num_in) +
                                  " dependencies and " + std::to_string(prog->num_out) + " outputs");
                if (prog->num_constants > c.num_constants) return refuse(SCHED_INVALID, name + ": the program reads more constants than the circuit has");
                if (prog->num_constants ? rec.b >= n : rec.b != 0)
                    return refuse(SCHED_INVALID, name + (prog->num_constants ? ": row out of range" : ": non-zero b for a program that reads no constants"));
            }
            switch (rec.kind) {
                case GEN_PROGRAM: count_ok = param_ok = true; num_in = prog->num_in; break;
                case GEN_EQUALITY: count_ok = count == 4; num_in = 2; break;
                case GEN_NONZERO_TEST: count_ok = count == 2; break;
                case GEN_QUOTIENT_OR_ZERO: count_ok = count == 3; num_in = 2; break;
                case GEN_QUOTIENT_EXTENSION: count_ok = count == 3 * D; num_in = 2 * D; break;
                case GEN_SPLIT: count_ok = count >= 1 && count <= 65; break;
                case GEN_WIRE_SPLIT: count_ok = count >= 2; param_ok = rec.gate >= 1; break;
                case GEN_LOW_HIGH: count_ok = count == 3; param_ok = rec.gate <= 63; break;
                default: count_ok = count >= 2; param_ok = rec.gate >= 2; break;   // GEN_BASE_SUM: a 32-bit base
            }
            if (!count_ok) return refuse(SCHED_INVALID, name + ": " + std::to_string(count) + " targets do not fit a generator of kind " + std::to_string(rec.kind));
            if (!param_ok) return refuse(SCHED_INVALID, name + ": parameter " + std::to_string(rec.gate) + " is out of range for kind " + std::to_string(rec.kind));
            if (rec.b && !prog) return refuse(SCHED_INVALID, name + ": non-zero b in a head record");
            const uint64_t cont = count / 2 + (count & 1);
            if (cont > num_records - r - 1) return refuse(SCHED_INVALID, name + ": the continuation records run past the end of the array");
            const size_t first = args.size();
            for (uint64_t i = 0; i < cont; i++) {
                const Record& t = records[r + 1 + i];
                if (t.kind != GEN_TARGETS) return refuse(SCHED_INVALID, name + ": the continuation meets a record of kind " + std::to_string(t.kind));
                if (t.gate) return refuse(SCHED_INVALID, name + ": non-zero gate in a continuation record");
                const bool half = 2 * i + 1 == count;   // the unused b of an odd count
                if (t.a >= NT || (!half && t.b >= NT)) return refuse(SCHED_INVALID, name + ": target out of range");
                if (half && t.b) return refuse(SCHED_INVALID, name + ": non-zero padding in the last continuation record");
                args.push_back((uint32_t)t.a);
                if (!half) args.push_back((uint32_t)t.b);
            }
            if (rec.kind == GEN_BASE_SUM) {   // listed sum first: the limbs are the dependencies
                std::rotate(args.begin() + first, args.begin() + first + 1, args.end());
                num_in = count - 1;
            }
            g.num_in = (uint32_t)num_in;
            g.num_out = (uint32_t)(count - num_in);
            g.out_off = g.in_off + g.num_in;
            g.p0 = rec.gate;
            if (prog) {
                if (s_row_constants.size() >> 31) return refuse(SCHED_UNSUPPORTED, "2^31 row constants of program generators or more");
                g.p1 = (uint32_t)s_row_constants.size();
                for (uint32_t j = 0; j < prog->num_constants; j++) {
                    const uint64_t k = c.constants[(uint64_t)j * n + rec.b];
                    if (k >= c.order) return refuse(SCHED_INVALID, name + ": non-canonical constant");
                    s_row_constants.push_back(k);
                }
                program_regs = std::max(program_regs, prog->num_regs);
                any_program = true;
            }
            r += cont;
        } else if (rec.kind == GEN_COPY) {
            if (rec.a >= NT || rec.b >= NT) return refuse(SCHED_INVALID, name + ": target out of range");
            args.push_back((uint32_t)rec.a);
            args.push_back((uint32_t)rec.b);
            g.num_in = g.num_out = 1;
            g.out_off = g.in_off + 1;
        } else {
            if (rec.gate >= c.num_gates) return refuse(SCHED_INVALID, name + ": gate index out of range");
            const GateDesc& gd = c.gates[rec.gate];
            if (gd.kind == G_PROGRAM) return refuse(SCHED_UNSUPPORTED, name + ": generators of program gates are not built");
            const bool kind_ok = rec.kind == GEN_CONSTANT ? (gd.kind == G_CONSTANT || gd.kind == G_RANDOM_ACCESS)
                                                          : gd.kind == detail::expected_gate(rec.kind);
            if (!kind_ok) return refuse(SCHED_INVALID, name + ": the gate's kind does not match the record's");
            if (rec.a >= n) return refuse(SCHED_INVALID, name + ": row out of range");
            dcols.clear();
            ocols.clear();
            int k_from[2];
            if (!detail::gate_columns(rec.kind, gd, rec.b, c.ext_degree, &dcols, &ocols, &g.p0, &g.p1, k_from))
                return refuse(SCHED_INVALID, name + ": operation, copy or constant index outside the gate's parameters");
            for (int i = 0; i < 2; i++)
                if (k_from[i] >= 0) {
                    if ((uint32_t)k_from[i] >= c.num_constants) return refuse(SCHED_INVALID, name + ": constant index outside the circuit's constants");
                    g.k[i] = c.constants[(uint64_t)k_from[i] * n + rec.a];
                    if (g.k[i] >= c.order) return refuse(SCHED_INVALID, name + ": non-canonical constant");
                }
            for (uint32_t col : dcols) {
                if (col >= c.num_wires) return refuse(SCHED_INVALID, name + ": the gate does not fit the circuit's wires");
                args.push_back((uint32_t)(rec.a * c.num_wires + col));
            }
            g.num_in = (uint32_t)dcols.size();
            g.out_off = (uint32_t)args.size();
            for (uint32_t col : ocols) {
                if (col >= c.num_wires) return refuse(SCHED_INVALID, name + ": the gate does not fit the circuit's wires");
                args.push_back((uint32_t)(rec.a * c.num_wires + col));
            }
            g.num_out = (uint32_t)ocols.size();
        }
        if (args.size() >> 31) return refuse(SCHED_UNSUPPORTED, "2^31 generator operands or more");
        gens.push_back(g);
    }
    {
        std::vector<uint64_t> sorted(input_targets, input_targets + num_inputs);
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 0; i < num_inputs; i++) {
            if (sorted[i] >= NT) return refuse(SCHED_INVALID, "input target out of range");
            if (i && sorted[i] == sorted[i - 1]) return refuse(SCHED_INVALID, "input target " + std::to_string(sorted[i]) + " is listed twice");
        }
    }

    // ---- the dense class index: slots first, then what only virtual targets use, ascending
    Schedule s;
    const uint32_t* rm = c.representative_map;
    std::vector<uint32_t> cls_of(NT, NONE);
    s.class_reps.assign(c.slot_reps, c.slot_reps + c.num_slots);
    for (size_t k = 0; k < c.num_slots; k++) {
        if (c.slot_reps[k] >= NT) return refuse(SCHED_INVALID, "slot representative out of range");
        cls_of[c.slot_reps[k]] = (uint32_t)k;
    }
    {
        std::vector<uint32_t> extra;
        auto touch = [&](uint64_t target) {
            const uint32_t rep = rm[target];
            if (cls_of[rep] == NONE) extra.push_back(rep);
        };
        for (uint32_t t : args) touch(t);
        for (size_t i = 0; i < num_inputs; i++) touch(input_targets[i]);
        for (size_t i = 0; i < c.num_public_inputs; i++) {
            if (c.pi_reps[i] >= NT) return refuse(SCHED_INVALID, "public input representative out of range");
            touch(c.pi_reps[i]);
        }
        std::sort(extra.begin(), extra.end());
        extra.erase(std::unique(extra.begin(), extra.end()), extra.end());
        for (uint32_t rep : extra) {
            if (rep >= NT) return refuse(SCHED_INVALID, "representative_map entry out of range");
            cls_of[rep] = (uint32_t)s.class_reps.size();
            s.class_reps.push_back(rep);
        }
    }
    if (s.class_reps.size() > MAX_CLASSES) return refuse(SCHED_UNSUPPORTED, "2^31 copy classes or more");
    const uint32_t NC = (uint32_t)s.class_reps.size();
    s.num_classes = NC;
    s.num_slots = (uint32_t)c.num_slots;
    for (uint32_t& a : args) a = cls_of[rm[a]];
    s.pi_cls.resize(c.num_public_inputs);
    for (size_t i = 0; i < c.num_public_inputs; i++) s.pi_cls[i] = cls_of[rm[c.pi_reps[i]]];

    // ---- levels (Kahn, a level at a time): set_level[class] = the level of its store
    std::vector<uint32_t> set_level(NC, NONE);
    s.input_cls.resize(num_inputs);
    s.input_first.resize(num_inputs);
    {
        std::vector<uint32_t> first(NC, NONE);
        for (size_t i = 0; i < num_inputs; i++) {
            const uint32_t cl = cls_of[rm[input_targets[i]]];
            s.input_cls[i] = cl;
            if (first[cl] == NONE) first[cl] = (uint32_t)i;
            s.input_first[i] = first[cl];
            set_level[cl] = 0;
        }
    }
    { std::vector<uint32_t>().swap(cls_of); }
    const size_t G = gens.size();
    std::vector<uint32_t> reader_off(NC + 1, 0), unmet(G, 0);
    std::vector<uint8_t> touched(NC, 0);
    for (const Gen& g : gens) {
        for (uint32_t i = 0; i < g.num_in; i++) {
            touched[args[g.in_off + i]] = 1;
            reader_off[args[g.in_off + i] + 1]++;
        }
        for (uint32_t i = 0; i < g.num_out; i++) touched[args[g.out_off + i]] = 1;
    }
    for (uint32_t k = 0; k < NC; k++) reader_off[k + 1] += reader_off[k];
    std::vector<uint32_t> readers(reader_off[NC]), fill(reader_off.begin(), reader_off.end() - 1);
    for (size_t gi = 0; gi < G; gi++)
        for (uint32_t i = 0; i < gens[gi].num_in; i++) {
            const uint32_t cl = args[gens[gi].in_off + i];
            readers[fill[cl]++] = (uint32_t)gi;
            if (set_level[cl] == NONE) unmet[gi]++;
        }
    s.input_free.resize(num_inputs);
    for (size_t i = 0; i < num_inputs; i++) s.input_free[i] = !touched[s.input_cls[i]];

    struct Entry {
        uint32_t level, kind, gen, deferred;
        uint32_t program;   // of a program generator: a wave runs one program where the level allows it
    };
    std::vector<Entry> entries;
    std::vector<uint32_t> glevel(G, NONE), frontier, next, newly;
    enum : uint8_t { STORE = 0, CHECK_NOW = 1, CHECK_LATER = 2 };
    std::vector<uint8_t> decision(args.size(), STORE);   // per output operand
    for (size_t gi = 0; gi < G; gi++)
        if (!unmet[gi]) frontier.push_back((uint32_t)gi);
    uint32_t level = 0, max_level = 0;
    while (!frontier.empty()) {
        level++;
        std::sort(frontier.begin(), frontier.end());   // record order decides who stores
        newly.clear();
        for (uint32_t gi : frontier) {
            const Gen& g = gens[gi];
            glevel[gi] = level;
            bool now = false, later = false;
            for (uint32_t i = 0; i < g.num_out; i++) {
                const uint32_t cl = args[g.out_off + i];
                if (set_level[cl] == NONE) {
                    set_level[cl] = level;
                    newly.push_back(cl);
                    decision[g.out_off + i] = STORE;
                    now = true;
                } else if (set_level[cl] == level) {
                    decision[g.out_off + i] = CHECK_LATER;   // stored by a generator of this very level: compare one level on
                    later = true;
                } else {
                    decision[g.out_off + i] = CHECK_NOW;
                    now = true;
                }
            }
            const uint32_t program = g.kind == GEN_PROGRAM ? g.p0 : 0;
            if (now || !g.num_out) entries.push_back(Entry{level, g.kind, gi, 0, program});
            if (later) entries.push_back(Entry{level + 1, g.kind, gi, 1, program});
            max_level = std::max(max_level, later ? level + 1 : level);
        }
        next.clear();
        for (uint32_t cl : newly)
            for (uint32_t k = reader_off[cl]; k < reader_off[cl + 1]; k++)
                if (--unmet[readers[k]] == 0) next.push_back(readers[k]);
        frontier.swap(next);
    }
    for (size_t gi = 0; gi < G; gi++) s.num_unrunnable += glevel[gi] == NONE;
    s.num_levels = max_level;

    // ---- the ops, level by level and kind by kind
    std::stable_sort(entries.begin(), entries.end(), [](const Entry& x, const Entry& y) {
        return x.level != y.level ? x.level < y.level : x.kind != y.kind ? x.kind < y.kind : x.program < y.program;
    });
    s.ops.reserve(entries.size());
    s.level_off.assign((size_t)max_level + 1, 0);
    for (const Entry& e : entries) {
        const Gen& g = gens[e.gen];
        Op op{g.kind, g.record, g.in_off, g.num_in, (uint32_t)args.size(), g.num_out, g.p0, g.p1, {g.k[0], g.k[1]}};
        for (uint32_t i = 0; i < g.num_out; i++) {
            const uint32_t cl = args[g.out_off + i], d = decision[g.out_off + i];
            uint32_t word = OUT_SKIP;
            if (e.deferred) {
                if (d == CHECK_LATER) word = cl | OUT_CHECK;
            } else if (d != CHECK_LATER) {
                word = d == STORE ? cl : cl | OUT_CHECK;
            }
            if (word != OUT_SKIP && (word & OUT_CHECK)) s.num_checks++;
            args.push_back(word);
        }
        s.level_off[e.level]++;   // counts first (index = level), offsets below
        s.ops.push_back(op);
    }
    if (args.size() >> 31) return refuse(SCHED_UNSUPPORTED, "2^31 generator operands or more");
    {   // level_off[l] = first op of level l + 1
        uint32_t run = 0;
        for (uint32_t l = 1; l <= max_level; l++) {
            const uint32_t count = s.level_off[l];
            s.level_off[l - 1] = run;
            run += count;
        }
        s.level_off[max_level] = run;
    }
    s.args = std::move(args);
    s.row_constants = std::move(s_row_constants);
    s.program_regs = any_program ? std::max(program_regs, 1u) : 0;

    // ---- launches
    for (uint32_t l = 0; l < max_level;) {
        const uint32_t width = s.level_off[l + 1] - s.level_off[l];
        if (width > group_width) {
            s.launches.push_back(Launch{l, 1, 0});
            l++;
            continue;
        }
        uint32_t e = l + 1;
        while (e < max_level && s.level_off[e + 1] - s.level_off[e] <= group_width) e++;
        s.launches.push_back(Launch{l, e - l, 1});
        l = e;
    }
    *out = std::move(s);
    *msg = "";
    return SCHED_OK;
}

}  // namespace gen
}  // namespace gbk
#endif

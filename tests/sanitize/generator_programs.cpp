// csrc/generator_programs.hpp (the validator of gb_circuit_set_generator_programs) and the GEN_PROGRAM head record of
// csrc/generator_schedule.hpp, compiled alone with AddressSanitizer and UndefinedBehaviorSanitizer - host code, no HIP:
//   * every refusal of the validator, each naming its program and instruction, and every refusal of the head record, each naming
//     its record;
//   * truncated and bit-flipped program tables and record arrays, each held in an allocation of exactly the length handed over
//     (a read past it is the sanitizer's finding): every status is OK, INVALID or UNSUPPORTED;
//   * the level order of a program generator fed by a built-in generator and feeding one;
//   * the row-constants array against the constants columns at rows other than 0, also with the columns as a circuit with two
//     selector columns holds them (the selector offset itself is the caller's: tests/test_generator_programs.py and
//     tests/test_gpu_generator_programs.py check it on a built circuit with two selector columns).
// Prints what failed and exits 1; exits 0 when everything held.
#include <cstdio>
#include <cstring>
#include <memory>

#include "generator_schedule.hpp"

using namespace gbk::gen;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("line %d: %s\n", __LINE__, #cond);                   \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ull;

static uint64_t operand(uint32_t space, uint32_t index) { return space | (index << 2); }
static uint64_t instr(uint32_t op, uint32_t dst, uint64_t a, uint64_t b = 0) {
    return (uint64_t)(op & 3) | ((uint64_t)(op >> 2) << 56) | ((uint64_t)dst << 2) | (a << 8) | (b << 32);
}
static std::vector<uint64_t> program(uint32_t num_in, uint32_t num_constants, uint32_t num_out, uint32_t num_regs, std::vector<uint64_t> lits,
                                     std::vector<uint64_t> instrs) {
    std::vector<uint64_t> w = {num_in | (uint64_t)num_constants << 32, num_out, num_regs | (uint64_t)lits.size() << 32, instrs.size()};
    w.insert(w.end(), lits.begin(), lits.end());
    w.insert(w.end(), instrs.begin(), instrs.end());
    return w;
}
// r0 = d0 * d1; r1 = r0 + k0; r1 = inv_or_zero(r1); out r1; out lit0: 2 dependencies, 1 constant, 2 outputs
static std::vector<uint64_t> good_program() {
    return program(2, 1, 2, 2, {5}, {instr(GP_MUL, 0, operand(GP_SPACE_DEP, 0), operand(GP_SPACE_DEP, 1)),
                                     instr(GP_ADD, 1, operand(GP_SPACE_REG, 0), operand(GP_SPACE_CONST, 0)),
                                     instr(GP_INV_OR_ZERO, 1, operand(GP_SPACE_REG, 1)), instr(GP_OUT, 0, operand(GP_SPACE_REG, 1)),
                                     instr(GP_OUT, 0, operand(GP_SPACE_LIT, 0))});
}

// the table in allocations of exactly its length
static bool parse(const std::vector<std::vector<uint64_t>>& programs, GeneratorPrograms* out, std::string* msg, uint32_t max_constants = 2) {
    std::vector<uint64_t> words;
    std::vector<uint32_t> offsets = {0};
    for (const auto& p : programs) {
        words.insert(words.end(), p.begin(), p.end());
        offsets.push_back((uint32_t)words.size());
    }
    std::unique_ptr<uint64_t[]> w(new uint64_t[words.size()]);
    std::unique_ptr<uint32_t[]> o(new uint32_t[offsets.size()]);
    std::copy(words.begin(), words.end(), w.get());
    std::copy(offsets.begin(), offsets.end(), o.get());
    return parse_generator_programs(w.get(), o.get(), (uint32_t)programs.size(), P, max_constants, out, msg);
}

static void refused(std::vector<uint64_t> words, const char* where, const char* what, int line) {
    GeneratorPrograms g;
    std::string msg;
    const bool ok = parse({good_program(), words}, &g, &msg);
    if (ok || msg.find(where) == std::string::npos || msg.find(what) == std::string::npos || !g.empty()) {
        std::printf("line %d: expected a refusal at \"%s\" with \"%s\", got %s \"%s\"\n", line, where, what, ok ? "OK" : "a refusal", msg.c_str());
        failures++;
    }
}
#define REFUSED(words, where, what) refused(words, where, what, __LINE__)

static void validator_refusals() {
    GeneratorPrograms g;
    std::string msg;
    CHECK(parse({good_program(), good_program()}, &g, &msg) && g.headers.size() == 2 && g.max_regs == 2 && g.headers[1].instr_off == 5 &&
          g.headers[1].lit_off == 1 && g.instrs.size() == 10 && g.lits.size() == 2);
    CHECK(parse({}, &g, &msg) && g.empty());
    const uint64_t D0 = operand(GP_SPACE_DEP, 0), R0 = operand(GP_SPACE_REG, 0);
    auto with = [&](size_t word, uint64_t value) {
        std::vector<uint64_t> w = good_program();
        w[word] = value;
        return w;
    };
    const size_t I0 = GP_HEADER_WORDS + 1;   // the first instruction of good_program
    REFUSED(with(2, 33 | (uint64_t)1 << 32), "generator program 1:", "header over the limits");                      // registers
    REFUSED(with(3, 4097), "generator program 1:", "header over the limits");                                          // instructions
    REFUSED(with(2, 2 | (uint64_t)257 << 32), "generator program 1:", "header over the limits");                      // literals
    REFUSED(with(0, 1023 | (uint64_t)1 << 32), "generator program 1:", "together at most 1024");                      // num_in + num_out
    REFUSED(with(1, 2 | (uint64_t)1 << 32), "generator program 1:", "header word 1");
    REFUSED(with(3, 5 | (uint64_t)1 << 32), "generator program 1:", "header word 3");
    REFUSED(with(3, 4), "generator program 1:", "the header describes 9 words, the table holds 10");
    REFUSED(std::vector<uint64_t>(3, 0), "generator program 1:", "3 words is no program");
    REFUSED(with(0, 2 | (uint64_t)3 << 32), "generator program 1", "reads 3 constants, the circuit has 2");
    REFUSED(with(GP_HEADER_WORDS, P), "generator program 1:", "literal 0 is not canonical");
    REFUSED(with(I0 + 1, instr(GP_ADD, 1, operand(GP_SPACE_REG, 1), D0)), "generator program 1 instruction 1:", "register 1 is read before it is written");
    REFUSED(with(I0 + 1, instr(GP_ADD, 1, operand(GP_SPACE_REG, 2), D0)), "generator program 1 instruction 1:", "register 2 of 2");
    REFUSED(with(I0 + 1, instr(GP_ADD, 2, R0, D0)), "generator program 1 instruction 1:", "register 2 of 2");          // destination
    REFUSED(with(I0, instr(GP_MUL, 0, D0, operand(GP_SPACE_DEP, 2))), "generator program 1 instruction 0:", "dependency 2 of 2");
    REFUSED(with(I0 + 1, instr(GP_ADD, 1, R0, operand(GP_SPACE_CONST, 1))), "generator program 1 instruction 1:", "constant 1 of 1");
    REFUSED(with(I0 + 4, instr(GP_OUT, 0, operand(GP_SPACE_LIT, 1))), "generator program 1 instruction 4:", "literal 1 of 1");
    REFUSED(with(I0 + 4, instr(GP_SUB, 0, R0, R0)), "generator program 1:", "1 OUTs, the header declares 2");
    REFUSED(with(I0 + 2, instr(GP_OUT, 0, R0)), "generator program 1:", "3 OUTs, the header declares 2");
    REFUSED(with(I0 + 2, instr(8, 1, R0)), "generator program 1 instruction 2:", "unknown opcode 8");
    REFUSED(with(I0 + 2, instr(63, 1, R0)), "generator program 1 instruction 2:", "unknown opcode 63");
    REFUSED(with(I0 + 2, instr(GP_SQRT, 1, R0) | (uint64_t)1 << 60), "generator program 1 instruction 2:", "bits 60-63");
    REFUSED(with(I0 + 2, instr(GP_INV, 1, R0, D0)), "generator program 1 instruction 2:", "a second operand");
    REFUSED(with(I0 + 3, instr(GP_OUT, 0, R0, D0)), "generator program 1 instruction 3:", "a second operand");
    REFUSED(with(I0 + 3, instr(GP_OUT, 1, R0)), "generator program 1 instruction 3:", "OUT with a destination");
    {   // the table itself
        std::vector<uint64_t> w = good_program();
        uint32_t off[3] = {1, 10, 20};
        CHECK(!parse_generator_programs(w.data(), off, 1, P, 2, &g, &msg) && msg.find("program_offsets[0]") != std::string::npos);
        uint32_t desc[3] = {0, 10, 5};
        w.insert(w.end(), w.begin(), w.begin() + 10);
        CHECK(!parse_generator_programs(w.data(), desc, 2, P, 2, &g, &msg) && msg.find("generator program 1: program_offsets are not ascending") != std::string::npos);
        CHECK(!parse_generator_programs(nullptr, nullptr, 1, P, 2, &g, &msg) && msg.find("null") != std::string::npos);
        std::vector<uint32_t> many(MAX_GENERATOR_PROGRAMS + 2, 0);
        CHECK(!parse_generator_programs(w.data(), many.data(), MAX_GENERATOR_PROGRAMS + 1, P, 2, &g, &msg) && msg.find("more than 256") != std::string::npos);
    }
}

// a circuit of 2 wires and 2^2 rows, two constants columns, every target its own class; virtual targets from 8 on
struct Circuit {
    std::vector<uint32_t> map;
    std::vector<uint32_t> slots;
    std::vector<uint64_t> constants = {10, 11, 12, 13, 20, 21, 22, 23};
    GateDesc arithmetic{G_ARITHMETIC, 1, 0, 0};
    GeneratorPrograms programs;
    CircuitDesc d;
    explicit Circuit(bool with_programs = true, uint32_t num_targets = 24) {
        for (uint32_t t = 0; t < num_targets; t++) map.push_back(t);
        for (uint32_t t = 0; t < 8; t++) slots.push_back(t);
        std::string msg;
        if (with_programs)   // 2 + 2 targets with a constant; 1 + 1 and 2 + 1 targets without
            parse({good_program(), program(1, 0, 1, 0, {}, {instr(GP_OUT, 0, operand(GP_SPACE_DEP, 0))}),
                   program(2, 0, 1, 0, {}, {instr(GP_OUT, 0, operand(GP_SPACE_DEP, 1))})},
                  &programs, &msg);
        d.representative_map = map.data();
        d.num_targets = num_targets;
        d.num_wires = 2;
        d.degree_bits = 2;
        d.num_constants = 2;
        d.order = P;
        d.slot_reps = slots.data();
        d.num_slots = slots.size();
        d.gates = &arithmetic;
        d.num_gates = 1;
        d.constants = constants.data();
        d.programs = with_programs ? &programs : nullptr;
    }
    // records and inputs in allocations of exactly their length
    int schedule(const std::vector<Record>& records, const std::vector<uint64_t>& inputs, Schedule* s, std::string* msg) const {
        std::unique_ptr<Record[]> r(new Record[records.size()]);
        std::unique_ptr<uint64_t[]> in(new uint64_t[inputs.size()]);
        for (size_t i = 0; i < records.size(); i++) r[i] = records[i];
        for (size_t i = 0; i < inputs.size(); i++) in[i] = inputs[i];
        return build_schedule(d, r.get(), records.size(), in.get(), inputs.size(), GROUP, s, msg);
    }
};

static void head_refused(const Circuit& c, std::vector<Record> records, int status, const char* what, int line) {
    records.insert(records.begin(), Record{GEN_COPY, 0, 8, 9});   // so that the head is record 1
    Schedule s;
    std::string msg;
    const int got = c.schedule(records, {8, 10, 11}, &s, &msg);
    if (got != status || msg.find("generator record 1:") == std::string::npos || msg.find(what) == std::string::npos) {
        std::printf("line %d: expected status %d at record 1 with \"%s\", got %d \"%s\"\n", line, status, what, got, msg.c_str());
        failures++;
    }
}
#define HEAD_REFUSED(c, status, what, ...) head_refused(c, {__VA_ARGS__}, status, what, __LINE__)

static void record_refusals() {
    const Circuit c, none(false);
    const Record head{GEN_PROGRAM, 0, 4, 3}, t01{GEN_TARGETS, 0, 10, 11}, t23{GEN_TARGETS, 0, 12, 13};
    Schedule s;
    std::string msg;
    CHECK(c.schedule({head, t01, t23}, {10, 11}, &s, &msg) == SCHED_OK);
    HEAD_REFUSED(none, SCHED_INVALID, "no generator programs are set", head, t01, t23);
    HEAD_REFUSED(c, SCHED_INVALID, "program index 3 of 3", Record{GEN_PROGRAM, 3, 4, 3}, t01, t23);
    HEAD_REFUSED(c, SCHED_INVALID, "3 targets, the program has 2 dependencies and 2 outputs", Record{GEN_PROGRAM, 0, 3, 3}, t01, Record{GEN_TARGETS, 0, 12, 0});
    HEAD_REFUSED(c, SCHED_INVALID, "row out of range", Record{GEN_PROGRAM, 0, 4, 4}, t01, t23);
    HEAD_REFUSED(c, SCHED_INVALID, "non-zero b for a program that reads no constants", Record{GEN_PROGRAM, 1, 2, 1}, t01);
    HEAD_REFUSED(c, SCHED_INVALID, "run past the end", head, t01);
    HEAD_REFUSED(c, SCHED_INVALID, "the continuation meets a record of kind 16", head, t01, Record{GEN_COPY, 0, 12, 13});
    HEAD_REFUSED(c, SCHED_INVALID, "non-zero gate in a continuation", head, t01, Record{GEN_TARGETS, 1, 12, 13});
    HEAD_REFUSED(c, SCHED_INVALID, "target out of range", head, t01, Record{GEN_TARGETS, 0, 12, 24});
    HEAD_REFUSED(c, SCHED_INVALID, "non-zero padding", Record{GEN_PROGRAM, 2, 3, 0}, t01, Record{GEN_TARGETS, 0, 12, 5});
    CHECK(c.schedule({Record{GEN_PROGRAM, 2, 3, 0}, t01, Record{GEN_TARGETS, 0, 12, 0}}, {10, 11}, &s, &msg) == SCHED_OK);
    // the kinds around the new one stay refused; an arithmetic record that names a program gate stays unsupported
    HEAD_REFUSED(c, SCHED_UNSUPPORTED, "kind 47 is no built generator kind", Record{47, 0, 4, 3}, t01, t23);
    HEAD_REFUSED(c, SCHED_UNSUPPORTED, "kind 49 is no built generator kind", Record{49, 0, 4, 3}, t01, t23);
    HEAD_REFUSED(c, SCHED_UNSUPPORTED, "kind 41 is no built generator kind", Record{41, 0, 4, 3}, t01, t23);
    Circuit pg;
    pg.arithmetic.kind = G_PROGRAM;
    HEAD_REFUSED(pg, SCHED_UNSUPPORTED, "generators of program gates are not built", Record{GEN_ARITHMETIC, 0, 0, 0});
}

static void level_order_and_row_constants() {
    const Circuit c;
    // wire (0,0..2) inputs -> ArithmeticGenerator writes wire (0,3) = target 3 -> the program reads 3 and 8, writes 14 and 15 ->
    // a Copy reads 14; a second program generator at row 2 reads the inputs alone
    const std::vector<Record> records = {{GEN_COPY, 0, 14, 16},    {GEN_PROGRAM, 0, 4, 3}, {GEN_TARGETS, 0, 3, 8}, {GEN_TARGETS, 0, 14, 15},
                                         {GEN_ARITHMETIC, 0, 0, 0}, {GEN_PROGRAM, 0, 4, 2}, {GEN_TARGETS, 0, 8, 9}, {GEN_TARGETS, 0, 17, 18},
                                         {GEN_PROGRAM, 1, 2, 0},    {GEN_TARGETS, 0, 17, 19}};
    Circuit wide;
    wide.d.num_wires = 4;   // an ArithmeticGate operation needs 4 wires
    wide.d.degree_bits = 1;
    wide.constants = {10, 11, 20, 21, 30, 31};
    wide.d.constants = wide.constants.data();
    Schedule s;
    std::string msg;
    // rows 3 and 2 do not exist with degree_bits 1
    CHECK(wide.schedule(records, {0, 1, 2, 8, 9}, &s, &msg) == SCHED_INVALID && msg.find("generator record 1: row out of range") != std::string::npos);
    std::vector<Record> r = records;
    r[1].b = 1;
    r[5].b = 0;
    CHECK(wide.schedule(r, {0, 1, 2, 8, 9}, &s, &msg) == SCHED_OK);
    CHECK(s.num_levels == 3 && s.num_unrunnable == 0 && s.ops.size() == 5 && s.program_regs == 2);
    auto level_of = [&](uint32_t record) {
        for (uint32_t l = 0; l < s.num_levels; l++)
            for (uint32_t i = s.level_off[l]; i < s.level_off[l + 1]; i++)
                if (s.ops[i].record == record) return (int)l + 1;
        return -1;
    };
    CHECK(level_of(4) == 1 && level_of(5) == 1 && level_of(1) == 2 && level_of(0) == 3 && level_of(8) == 2);
    // the row constants: constants[j][row] for j < num_constants of the program (1), at the offset the op carries
    for (const Op& op : s.ops) {
        if (op.kind != GEN_PROGRAM) continue;
        CHECK(op.p0 == (op.record == 8 ? 1u : 0u) && op.num_in == (op.record == 8 ? 1u : 2u));
        if (op.record == 1) CHECK(op.p1 < s.row_constants.size() && s.row_constants[op.p1] == 11);
        if (op.record == 5) CHECK(op.p1 < s.row_constants.size() && s.row_constants[op.p1] == 10);
    }
    CHECK(s.row_constants.size() == 2);
    // a program that reads both columns, at the last row
    Circuit both;
    both.programs = GeneratorPrograms{};
    CHECK(parse({program(1, 2, 1, 1, {}, {instr(GP_ADD, 0, operand(GP_SPACE_CONST, 0), operand(GP_SPACE_CONST, 1)), instr(GP_OUT, 0, operand(GP_SPACE_REG, 0))})},
                &both.programs, &msg));
    CHECK(both.schedule({{GEN_PROGRAM, 0, 2, 3}, {GEN_TARGETS, 0, 8, 9}, {GEN_PROGRAM, 0, 2, 1}, {GEN_TARGETS, 0, 8, 10}}, {8}, &s, &msg) == SCHED_OK);
    CHECK(s.row_constants == (std::vector<uint64_t>{13, 23, 11, 21}) && s.ops.size() == 2 && s.ops[0].p1 == 0 && s.ops[1].p1 == 2);
    {   // the columns as a circuit with two selector columns holds them, constants_sigmas = [selector 0, selector 1, constants 0,
        // constants 1, sigma 0]: the caller hands over the columns behind the selectors, and the row constants at rows 2 and 3 are
        // theirs - no word of a selector column or of a sigma column, which hold other values at every row
        const uint32_t n = 4, num_selectors = 2;
        const std::vector<uint64_t> constants_sigmas = {0, 0, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 2,
                                                        40, 41, 42, 43, 50, 51, 52, 53, 90, 91, 92, 93};
        Circuit sel;
        sel.programs = both.programs;
        sel.constants.assign(constants_sigmas.begin() + num_selectors * n, constants_sigmas.begin() + (num_selectors + 2) * n);
        sel.d.constants = sel.constants.data();   // an allocation of exactly [num_constants][n]
        CHECK(sel.schedule({{GEN_PROGRAM, 0, 2, 2}, {GEN_TARGETS, 0, 8, 9}, {GEN_PROGRAM, 0, 2, 3}, {GEN_TARGETS, 0, 8, 10}}, {8}, &s, &msg) == SCHED_OK);
        CHECK(s.row_constants == (std::vector<uint64_t>{42, 52, 43, 53}));
        for (uint32_t j = 0; j < 2; j++)
            for (uint32_t k = 0; k < 2; k++)
                CHECK(s.row_constants[2 * k + j] == constants_sigmas[(num_selectors + j) * n + 2 + k]);
    }
    both.constants[7] = P;   // a constant of the row that is no field element
    CHECK(both.schedule({{GEN_PROGRAM, 0, 2, 3}, {GEN_TARGETS, 0, 8, 9}}, {8}, &s, &msg) == SCHED_INVALID && msg.find("non-canonical constant") != std::string::npos);
    // device_schedule: the registers and the tables travel with the program ops; apart, it refuses and names the record
    {
        CHECK(both.schedule({{GEN_COPY, 0, 8, 11}, {GEN_PROGRAM, 0, 2, 1}, {GEN_TARGETS, 0, 8, 9}}, {8}, &s, &msg) == SCHED_OK && s.program_regs == 1);
        const ProgramHeader* h = both.programs.headers.data();
        const uint64_t *in = both.programs.instrs.data(), *rc = s.row_constants.data(), lits[1] = {0};
        DeviceSchedule dev{nullptr, nullptr, nullptr};
        CHECK(device_schedule(s, s.ops.data(), s.args.data(), s.level_off.data(), h, in, lits, rc, &dev, &msg) && dev.program_regs == 1 &&
              dev.ops == s.ops.data() && dev.programs == h && dev.program_instrs == in && dev.program_lits == lits && dev.row_constants == rc);
        CHECK(!device_schedule(s, s.ops.data(), s.args.data(), s.level_off.data(), h, in, lits, nullptr, &dev, &msg) &&
              msg.find("generator record 1: a program generator in a schedule without the program tables") != std::string::npos);
        CHECK(!device_schedule(s, s.ops.data(), s.args.data(), s.level_off.data(), nullptr, in, lits, rc, &dev, &msg));
        Schedule none = s;
        none.program_regs = 0;
        CHECK(!device_schedule(none, s.ops.data(), s.args.data(), s.level_off.data(), h, in, lits, rc, &dev, &msg) &&
              msg.find("generator record 1: a program generator in a schedule that asks for no program registers") != std::string::npos);
    }
    // a schedule without program generators asks for no registers, and needs no tables
    CHECK(c.schedule({{GEN_COPY, 0, 8, 9}}, {8}, &s, &msg) == SCHED_OK && s.program_regs == 0 && s.row_constants.empty());
    {
        DeviceSchedule dev{nullptr, nullptr, nullptr};
        CHECK(device_schedule(s, s.ops.data(), s.args.data(), s.level_off.data(), nullptr, nullptr, nullptr, nullptr, &dev, &msg) && dev.program_regs == 0);
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void fuzz() {
    const std::vector<uint64_t> base = good_program();
    size_t accepted = 0, refused_count = 0;
    for (int it = 0; it < 20000; it++) {
        std::vector<std::vector<uint64_t>> table = {base, base};
        std::vector<uint64_t>& w = table[rnd() & 1];
        if (it % 3 == 0) w.resize(rnd() % (w.size() + 1));            // truncated
        for (int flips = 1 + (int)(rnd() % 3); flips > 0 && !w.empty(); flips--) w[rnd() % w.size()] ^= (uint64_t)1 << (rnd() % 64);
        GeneratorPrograms g;
        std::string msg;
        const bool ok = parse(table, &g, &msg);
        CHECK(ok ? (g.headers.size() == 2 && msg.empty()) : (g.empty() && !msg.empty()));
        if (ok) {   // what gen_program relies on
            for (const ProgramHeader& h : g.headers)
                CHECK((size_t)h.instr_off + h.num_instrs <= g.instrs.size() && (size_t)h.lit_off + h.num_literals <= g.lits.size() &&
                      h.num_regs <= GP_MAX_REGS && h.num_constants <= 2);
        }
        (ok ? accepted : refused_count)++;
    }
    CHECK(accepted > 100 && refused_count > 100);
    const Circuit c;
    const std::vector<Record> records = {{GEN_PROGRAM, 0, 4, 3}, {GEN_TARGETS, 0, 3, 8}, {GEN_TARGETS, 0, 14, 15}, {GEN_COPY, 0, 14, 16},
                                         {GEN_PROGRAM, 1, 2, 0}, {GEN_TARGETS, 0, 16, 19}};
    size_t ok_count = 0;
    for (int it = 0; it < 20000; it++) {
        std::vector<Record> r = records;
        if (it % 3 == 0) r.resize(rnd() % (r.size() + 1));
        for (int flips = 1 + (int)(rnd() % 3); flips > 0 && !r.empty(); flips--) {
            Record& x = r[rnd() % r.size()];
            const uint32_t bit = (uint32_t)(rnd() % 8);   // low bits: the interesting values are small
            switch (rnd() % 4) {
                case 0: x.kind ^= 1u << bit; break;
                case 1: x.gate ^= 1u << bit; break;
                case 2: x.a ^= (uint64_t)1 << (rnd() % 2 ? bit : rnd() % 64); break;
                default: x.b ^= (uint64_t)1 << (rnd() % 2 ? bit : rnd() % 64); break;
            }
        }
        Schedule s;
        std::string msg;
        const int status = c.schedule(r, {3, 8}, &s, &msg);
        CHECK(status == SCHED_OK || status == SCHED_INVALID || status == SCHED_UNSUPPORTED);
        if (status == SCHED_OK) {
            ok_count++;
            for (const Op& op : s.ops) {
                CHECK((size_t)op.in_off + op.num_in <= s.args.size() && (size_t)op.out_off + op.num_out <= s.args.size());
                if (op.kind == GEN_PROGRAM)
                    CHECK(op.p0 < c.programs.headers.size() && (size_t)op.p1 + c.programs.headers[op.p0].num_constants <= s.row_constants.size() &&
                          op.num_in == c.programs.headers[op.p0].num_in && op.num_out == c.programs.headers[op.p0].num_out);
            }
        }
    }
    CHECK(ok_count > 100);
}

int main() {
    validator_refusals();
    record_refusals();
    level_order_and_row_constants();
    fuzz();
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("generator programs: all checks held\n");
    return failures ? 1 : 0;
}

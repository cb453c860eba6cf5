// csrc/generator_programs.hpp on the integer operations of a generator program (IDIV 16, IREM 17, SHR 18, AND 19, LT 20), compiled
// alone with AddressSanitizer and UndefinedBehaviorSanitizer - host code, no HIP:
//   * each is accepted with two operands from every space, and what the interpreter relies on holds for it as for ADD: both
//     operands are checked - an out-of-range register, dependency, constant or literal and an unwritten register in the second
//     operand are refused with their index, as in the first - and the destination counts as written afterwards;
//   * 8 .. 15 and 21 .. 63 are no opcodes; OUT and the unary operations 3 .. 7 still refuse a second operand.
// Prints what failed and exits 1; exits 0 when everything held.
#include <cstdio>
#include <memory>

#include "generator_programs.hpp"

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
// 2 dependencies, 1 constant, 1 literal, 2 registers, 1 output: r0 = d0 * d1; r1 = <the instruction under test>; out r1
static std::vector<uint64_t> program(uint64_t under_test) {
    return {2 | (uint64_t)1 << 32, 1, 2 | (uint64_t)1 << 32, 3, 5,
            instr(GP_MUL, 0, operand(GP_SPACE_DEP, 0), operand(GP_SPACE_DEP, 1)), under_test, instr(GP_OUT, 0, operand(GP_SPACE_REG, 1))};
}

// the table in allocations of exactly its length
static bool parse(const std::vector<uint64_t>& words, GeneratorPrograms* out, std::string* msg) {
    std::unique_ptr<uint64_t[]> w(new uint64_t[words.size()]);
    std::copy(words.begin(), words.end(), w.get());
    const uint32_t offsets[2] = {0, (uint32_t)words.size()};
    return parse_generator_programs(w.get(), offsets, 1, P, 2, out, msg);
}

static void refused(uint64_t under_test, const std::string& what, int line) {
    GeneratorPrograms g;
    std::string msg;
    const bool ok = parse(program(under_test), &g, &msg);
    if (ok || msg.find("generator program 0 instruction 1: " + what) == std::string::npos || !g.empty()) {
        std::printf("line %d: expected a refusal at instruction 1 with \"%s\", got %s \"%s\"\n", line, what.c_str(), ok ? "OK" : "a refusal", msg.c_str());
        failures++;
    }
}
#define REFUSED(word, what) refused(word, what, __LINE__)

int main() {
    const uint64_t D0 = operand(GP_SPACE_DEP, 0), R0 = operand(GP_SPACE_REG, 0), K0 = operand(GP_SPACE_CONST, 0), L0 = operand(GP_SPACE_LIT, 0);
    CHECK(GP_IDIV == 16 && GP_IREM == 17 && GP_SHR == 18 && GP_AND == 19 && GP_LT == 20 && GP_NUM_OPCODES == 21);
    for (uint32_t op = GP_IDIV; op <= GP_LT; op++) {
        CHECK(gen_program_opcode(instr(op, 1, D0, R0)) == op);
        for (uint64_t a : {D0, R0, K0, L0})
            for (uint64_t b : {D0, R0, K0, L0}) {
                GeneratorPrograms g;
                std::string msg;
                CHECK(parse(program(instr(op, 1, a, b)), &g, &msg) && g.headers.size() == 1 && g.instrs.size() == 3 && g.instrs[1] == instr(op, 1, a, b));
            }
        // the second operand: out of range in every space, and a register that nothing has written (r1 is written by this very
        // instruction: it is read first)
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_REG, 2)), "register 2 of 2");
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_REG, 1)), "register 1 is read before it is written");
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_DEP, 2)), "dependency 2 of 2");
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_CONST, 1)), "constant 1 of 1");
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_LIT, 1)), "literal 1 of 1");
        REFUSED(instr(op, 1, D0, operand(GP_SPACE_LIT, 0x3FFFFF)), "literal 4194303 of 1");
        // the first operand and the destination, as for every operation
        REFUSED(instr(op, 1, operand(GP_SPACE_REG, 1), D0), "register 1 is read before it is written");
        REFUSED(instr(op, 1, operand(GP_SPACE_DEP, 2), D0), "dependency 2 of 2");
        REFUSED(instr(op, 2, D0, D0), "register 2 of 2");
        REFUSED(instr(op, 1, D0, D0) | (uint64_t)1 << 60, "bits 60-63");
        {   // the destination is not written before the instruction: OUT r1 without it is refused, with it accepted (above)
            GeneratorPrograms g;
            std::string msg;
            std::vector<uint64_t> w = program(instr(op, 0, D0, D0));
            CHECK(!parse(w, &g, &msg) && msg.find("instruction 2: register 1 is read before it is written") != std::string::npos);
        }
    }
    for (uint32_t op = 8; op < 64; op++) {
        if (op >= GP_IDIV && op <= GP_LT) continue;
        REFUSED(instr(op, 1, R0), "unknown opcode " + std::to_string(op));
        REFUSED(instr(op, 1, R0, D0), "unknown opcode " + std::to_string(op));
    }
    for (uint32_t op = GP_OUT; op <= GP_SQRT; op++) {
        REFUSED(instr(op, op == GP_OUT ? 0 : 1, R0, D0), "a second operand in OUT or a unary operation");
        REFUSED(instr(op, op == GP_OUT ? 0 : 1, R0, operand(GP_SPACE_LIT, 9)), "a second operand in OUT or a unary operation");
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::printf("integer operations: all checks held\n");
    return failures ? 1 : 0;
}

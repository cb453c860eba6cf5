// The generator programs of gb_circuit_set_generator_programs (include/goldibear_gpu.h gives the words and the list of what is
// refused), decoded and checked.  This is the code that reads the untrusted words: every length is checked against the offsets
// before a word is read, and after it returns gen_program (generators.hpp) needs no check of its own - every register, dependency,
// constant and literal index is in range - of both operands of a binary operation, the integer operations among them - no
// register is read before it is written and the OUTs number num_out.
//
// Host code without HIP or field dependencies (literals stay canonical here; the caller converts them to the device form once):
// tests/sanitize/generator_programs.cpp compiles it alone with the sanitizers.
#ifndef GOLDIBEAR_GENERATOR_PROGRAMS_HPP
#define GOLDIBEAR_GENERATOR_PROGRAMS_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "generator_ops.hpp"

namespace gbk {
namespace gen {

// the limits and the word layout shared with the constraint programs (gate_set.hpp, GB_MAX_PROGRAM_*)
constexpr uint32_t GP_HEADER_WORDS = 4, GP_MAX_INSTRS = 4096, GP_MAX_REGS = 32, GP_MAX_LITERALS = 256;
enum : uint32_t { GP_SPACE_REG = 0, GP_SPACE_DEP = 1, GP_SPACE_CONST = 2, GP_SPACE_LIT = 3 };

struct GeneratorPrograms {
    std::vector<ProgramHeader> headers;
    std::vector<uint64_t> instrs, lits;   // flat; literals canonical
    uint32_t max_regs = 0;
    bool empty() const { return headers.empty(); }
};

// order: the field's order.  max_constants: the circuit's constants columns (a program may not read past them).
// false: *msg names the program and the instruction; *out is empty.  num_programs == 0 is the empty set.
inline bool parse_generator_programs(const uint64_t* words, const uint32_t* offsets, uint32_t num_programs, uint64_t order,
                                     uint32_t max_constants, GeneratorPrograms* out, std::string* msg) {
    GeneratorPrograms g;
    auto refuse = [&](const std::string& m) {
        *msg = m;
        *out = GeneratorPrograms{};
        return false;
    };
    *out = GeneratorPrograms{};
    if (num_programs == 0) return true;
    if (num_programs > MAX_GENERATOR_PROGRAMS) return refuse("more than " + std::to_string(MAX_GENERATOR_PROGRAMS) + " generator programs");
    if (!words || !offsets) return refuse("null program table");
    if (offsets[0] != 0) return refuse("program_offsets[0] is not 0");
    constexpr uint32_t MAX_WORDS = GP_HEADER_WORDS + GP_MAX_LITERALS + GP_MAX_INSTRS;
    for (uint32_t pi = 0; pi < num_programs; pi++) {
        const std::string name = "generator program " + std::to_string(pi);
        if (offsets[pi + 1] < offsets[pi]) return refuse(name + ": program_offsets are not ascending");
        const uint32_t len = offsets[pi + 1] - offsets[pi];
        if (len < GP_HEADER_WORDS || len > MAX_WORDS)
            return refuse(name + ": " + std::to_string(len) + " words is no program (header " + std::to_string(GP_HEADER_WORDS) + ", at most " +
                          std::to_string(MAX_WORDS) + ")");
        const uint64_t* w = words + offsets[pi];
        ProgramHeader h{};
        h.num_in = (uint32_t)w[0]; h.num_constants = (uint32_t)(w[0] >> 32);
        h.num_out = (uint32_t)w[1];
        h.num_regs = (uint32_t)w[2]; h.num_literals = (uint32_t)(w[2] >> 32);
        h.num_instrs = (uint32_t)w[3];
        if ((w[1] >> 32) != 0) return refuse(name + ": header word 1 has bits above num_out");
        if ((w[3] >> 32) != 0) return refuse(name + ": header word 3 has bits above num_instrs");
        if (h.num_instrs > GP_MAX_INSTRS || h.num_regs > GP_MAX_REGS || h.num_literals > GP_MAX_LITERALS)
            return refuse(name + ": header over the limits (" + std::to_string(h.num_instrs) + " instructions / " + std::to_string(h.num_regs) +
                          " registers / " + std::to_string(h.num_literals) + " literals; at most 4096 / 32 / 256)");
        if ((uint64_t)h.num_in + h.num_out > MAX_PROGRAM_TARGETS)
            return refuse(name + ": header over the limits (" + std::to_string(h.num_in) + " dependencies and " + std::to_string(h.num_out) +
                          " outputs; together at most " + std::to_string(MAX_PROGRAM_TARGETS) + ")");
        if (len != GP_HEADER_WORDS + h.num_literals + h.num_instrs)
            return refuse(name + ": the header describes " + std::to_string(GP_HEADER_WORDS + h.num_literals + h.num_instrs) +
                          " words, the table holds " + std::to_string(len));
        if (h.num_constants > max_constants)
            return refuse(name + " reads " + std::to_string(h.num_constants) + " constants, the circuit has " + std::to_string(max_constants));
        h.lit_off = (uint32_t)g.lits.size();
        h.instr_off = (uint32_t)g.instrs.size();
        for (uint32_t i = 0; i < h.num_literals; i++) {
            const uint64_t v = w[GP_HEADER_WORDS + i];
            if (v >= order) return refuse(name + ": literal " + std::to_string(i) + " is not canonical");
            g.lits.push_back(v);
        }
        bool written[GP_MAX_REGS] = {};
        uint32_t outs = 0;
        const uint64_t* ins = w + GP_HEADER_WORDS + h.num_literals;
        for (uint32_t pc = 0; pc < h.num_instrs; pc++) {
            const uint64_t iw = ins[pc];
            const std::string at = name + " instruction " + std::to_string(pc);
            if (iw >> 60) return refuse(at + ": bits 60-63 are not zero");
            const uint32_t op = gen_program_opcode(iw), dst = ((uint32_t)iw >> 2) & 63;
            if (!gen_program_is_opcode(op)) return refuse(at + ": unknown opcode " + std::to_string(op));
            const uint32_t operand[2] = {(uint32_t)(iw >> 8) & 0xFFFFFF, (uint32_t)(iw >> 32) & 0xFFFFFF};
            const bool unary = !gen_program_is_binary(op);   // OUT and the unary operations (3 .. 7) read a alone
            if (unary && operand[1] != 0) return refuse(at + ": a second operand in OUT or a unary operation");
            for (uint32_t k = 0; k < (unary ? 1u : 2u); k++) {
                const uint32_t idx = operand[k] >> 2;
                switch (operand[k] & 3) {
                    case GP_SPACE_REG:
                        if (idx >= h.num_regs) return refuse(at + ": register " + std::to_string(idx) + " of " + std::to_string(h.num_regs));
                        if (!written[idx]) return refuse(at + ": register " + std::to_string(idx) + " is read before it is written");
                        break;
                    case GP_SPACE_DEP:
                        if (idx >= h.num_in) return refuse(at + ": dependency " + std::to_string(idx) + " of " + std::to_string(h.num_in));
                        break;
                    case GP_SPACE_CONST:
                        if (idx >= h.num_constants) return refuse(at + ": constant " + std::to_string(idx) + " of " + std::to_string(h.num_constants));
                        break;
                    default:
                        if (idx >= h.num_literals) return refuse(at + ": literal " + std::to_string(idx) + " of " + std::to_string(h.num_literals));
                        break;
                }
            }
            if (op == GP_OUT) {
                if (dst != 0) return refuse(at + ": OUT with a destination");
                outs++;
            } else {
                if (dst >= h.num_regs) return refuse(at + ": register " + std::to_string(dst) + " of " + std::to_string(h.num_regs));
                written[dst] = true;
            }
            g.instrs.push_back(iw);
        }
        if (outs != h.num_out) return refuse(name + ": " + std::to_string(outs) + " OUTs, the header declares " + std::to_string(h.num_out) + " outputs");
        g.headers.push_back(h);
        g.max_regs = std::max(g.max_regs, h.num_regs);
    }
    *out = std::move(g);
    *msg = "";
    return true;
}

}  // namespace gen
}  // namespace gbk
#endif

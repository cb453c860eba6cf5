// The program table of gb_constraint_quotient / gb_constraint_eval (include/goldibear_gpu.h, "constraint systems"), decoded and
// checked.  The words are those of the GB_GATE_PROGRAM programs (gate_set.hpp; gates.hpp run_program interprets them) with two
// differences: header word 0 is num_cells | num_inputs << 32, and a cell table of num_cells words follows the literals - operand
// space 1 indexes it, operand space 2 the inputs X, L_first, L_last and the caller's params.
//
// This is the code that reads untrusted input: every length is checked against the offsets before a word is read, and every
// index - register, cell, input, literal, oracle, polynomial, row offset - before the kernel or the host interpreter uses it as
// an address.  After parse_system returns SYS_OK, run_program needs no check of its own.
//
// Host code without HIP dependencies: tests/sanitize/constraint_system.cpp compiles it alone with the sanitizers.
#ifndef GOLDIBEAR_CONSTRAINT_SYSTEM_HPP
#define GOLDIBEAR_CONSTRAINT_SYSTEM_HPP

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "gate_set.hpp"

namespace gbk {
namespace constraints {

enum SystemStatus { SYS_OK = 0, SYS_INVALID = 1 };   // the values of GB_OK / GB_ERR_INVALID

constexpr uint32_t MAX_ORACLES = GB_MAX_CONSTRAINT_ORACLES, MAX_PROGRAM_CELLS = GB_MAX_PROGRAM_CELLS, MAX_PARAMS = GB_MAX_CONSTRAINT_PARAMS;
constexpr uint32_t MAX_CONSTRAINT_CHALLENGES = 16, MAX_QUOTIENT_DEGREE_BITS = 4;
enum Input { INPUT_X = 0, INPUT_L_FIRST = 1, INPUT_L_LAST = 2, NUM_BUILTIN_INPUTS = 3 };
enum Space { SPACE_REG = 0, SPACE_CELL = 1, SPACE_INPUT = 2, SPACE_LIT = 3 };   // = gates::ProgramSpace, the names of this format

// a cell word: oracle_index in bits 0-15, polynomial_index in bits 16-47, row_offset (rows ahead, modulo n) in bits 48-63
// (constexpr: the kernel decodes with the same three functions)
constexpr uint32_t cell_oracle(uint64_t w) { return (uint32_t)(w & 0xFFFF); }
constexpr uint32_t cell_polynomial(uint64_t w) { return (uint32_t)(w >> 16); }
constexpr uint32_t cell_row_offset(uint64_t w) { return (uint32_t)(w >> 48); }

struct ProgramInfo {
    uint32_t num_cells, num_inputs, num_constraints, degree, num_regs, num_literals, num_instrs;
    uint32_t lit_off, cell_off, instr_off;   // first literal / cell word / instruction word in the flat tables
};
struct System {
    uint32_t num_programs = 0, max_regs = 0, total_cells = 0, total_constraints = 0;
    bool reads_lagrange = false;             // some instruction reads L_first or L_last
    ProgramInfo p[gates::MAX_PROGRAMS] = {};
    std::vector<uint64_t> instrs, lits, cells;   // literals as they came: canonical
};
// what the table is checked against
struct Shape {
    uint64_t order = 0;                          // the field's p: literals are below it
    uint32_t num_oracles = 0;                    // oracle_index is below it (at most MAX_ORACLES)
    const uint32_t* oracle_num_polys = nullptr;  // [num_oracles] polynomial_index is below its oracle's; null: not known (the verifier's side)
    uint64_t num_rows = 0;                       // n: row_offset is below it
    uint32_t num_params = 0;                     // num_inputs of every program is 3 + num_params
    uint32_t max_degree = 0;                     // the header's degree is at most this (2^quotient_degree_bits + 1); 0: no bound
};

inline SystemStatus parse_system(const uint64_t* words, const uint32_t* offsets, uint32_t num_programs, const Shape& sh, System* out,
                                 std::string* msg) {
    namespace G = gbk::gates;
    std::string unused;
    if (!msg) msg = &unused;
    auto bad = [&](const std::string& m) { *msg = m; return SYS_INVALID; };
    if (!out) return bad("null argument");
    *out = System{};
    if (num_programs == 0) return bad("a constraint system needs at least one program");
    if (num_programs > G::MAX_PROGRAMS) return bad("more than " + std::to_string(G::MAX_PROGRAMS) + " constraint programs");
    if (!words || !offsets) return bad("null program table");
    if (offsets[0] != 0) return bad("program_offsets[0] is not 0");
    if (sh.num_oracles > MAX_ORACLES) return bad("more than " + std::to_string(MAX_ORACLES) + " oracles");
    if (sh.num_params > MAX_PARAMS) return bad("more than " + std::to_string(MAX_PARAMS) + " params");
    // a program is at most a header, the literals, the cell table and the instructions
    constexpr uint32_t MAX_WORDS = G::PROGRAM_HEADER_WORDS + G::MAX_PROGRAM_LITERALS + MAX_PROGRAM_CELLS + G::MAX_PROGRAM_INSTRS;
    for (uint32_t pi = 0; pi < num_programs; pi++) {
        const std::string name = "program " + std::to_string(pi);
        if (offsets[pi + 1] < offsets[pi]) return bad(name + ": program_offsets are not ascending");
        const uint32_t len = offsets[pi + 1] - offsets[pi];
        if (len < G::PROGRAM_HEADER_WORDS || len > MAX_WORDS)
            return bad(name + ": " + std::to_string(len) + " words is no program (header " + std::to_string(G::PROGRAM_HEADER_WORDS) +
                       ", at most " + std::to_string(MAX_WORDS) + ")");
        const uint64_t* w = words + offsets[pi];
        ProgramInfo h{};
        h.num_cells = (uint32_t)w[0]; h.num_inputs = (uint32_t)(w[0] >> 32);
        h.num_constraints = (uint32_t)w[1]; h.degree = (uint32_t)(w[1] >> 32);
        h.num_regs = (uint32_t)w[2]; h.num_literals = (uint32_t)(w[2] >> 32);
        h.num_instrs = (uint32_t)w[3];
        if ((w[3] >> 32) != 0) return bad(name + ": header word 3 has bits above num_instrs");
        if (h.num_instrs > G::MAX_PROGRAM_INSTRS || h.num_regs > G::MAX_PROGRAM_REGS || h.num_literals > G::MAX_PROGRAM_LITERALS ||
            h.num_constraints > G::MAX_PROGRAM_CONSTRAINTS || h.num_cells > MAX_PROGRAM_CELLS)
            return bad(name + ": header over the limits (" + std::to_string(h.num_instrs) + " instructions / " + std::to_string(h.num_regs) +
                       " registers / " + std::to_string(h.num_literals) + " literals / " + std::to_string(h.num_constraints) +
                       " constraints / " + std::to_string(h.num_cells) + " cells; at most 4096 / 32 / 256 / 1024 / " +
                       std::to_string(MAX_PROGRAM_CELLS) + ")");
        const uint32_t described = G::PROGRAM_HEADER_WORDS + h.num_literals + h.num_cells + h.num_instrs;
        if (len != described)
            return bad(name + ": the header describes " + std::to_string(described) + " words, the table holds " + std::to_string(len));
        if (h.num_inputs != NUM_BUILTIN_INPUTS + sh.num_params)
            return bad(name + ": num_inputs is " + std::to_string(h.num_inputs) + ", the call has X, L_first, L_last and " +
                       std::to_string(sh.num_params) + " params = " + std::to_string(NUM_BUILTIN_INPUTS + sh.num_params));
        if (sh.max_degree && h.degree > sh.max_degree)
            return bad(name + ": degree " + std::to_string(h.degree) + " is above 2^quotient_degree_bits + 1 = " + std::to_string(sh.max_degree));
        h.lit_off = (uint32_t)out->lits.size();
        h.cell_off = (uint32_t)out->cells.size();
        h.instr_off = (uint32_t)out->instrs.size();
        for (uint32_t i = 0; i < h.num_literals; i++) {
            const uint64_t v = w[G::PROGRAM_HEADER_WORDS + i];
            if (v >= sh.order) return bad(name + ": literal " + std::to_string(i) + " is not canonical");
            out->lits.push_back(v);
        }
        const uint64_t* cw = w + G::PROGRAM_HEADER_WORDS + h.num_literals;
        for (uint32_t i = 0; i < h.num_cells; i++) {
            const std::string at = name + " cell " + std::to_string(i);
            const uint32_t o = cell_oracle(cw[i]), k = cell_polynomial(cw[i]), off = cell_row_offset(cw[i]);
            if (o >= sh.num_oracles) return bad(at + ": oracle_index " + std::to_string(o) + " of " + std::to_string(sh.num_oracles));
            if (sh.oracle_num_polys && k >= sh.oracle_num_polys[o])
                return bad(at + ": polynomial_index " + std::to_string(k) + " out of range for oracle " + std::to_string(o) + " with " +
                           std::to_string(sh.oracle_num_polys[o]) + " polynomials (salt columns are not polynomials)");
            if (off >= sh.num_rows) return bad(at + ": row_offset " + std::to_string(off) + " is not below n = " + std::to_string(sh.num_rows));
            out->cells.push_back(cw[i]);
        }
        // one pass: which registers are written, and the degree bound of what each holds
        uint32_t reg_deg[G::MAX_PROGRAM_REGS];
        bool written[G::MAX_PROGRAM_REGS] = {};
        uint32_t emits = 0;
        const uint64_t* ins = cw + h.num_cells;
        for (uint32_t pc = 0; pc < h.num_instrs; pc++) {
            const uint64_t iw = ins[pc];
            const std::string at = name + " instruction " + std::to_string(pc);
            if (iw >> 56) return bad(at + ": bits 56-63 are not zero");
            const uint32_t op = (uint32_t)iw & 3, dst = ((uint32_t)iw >> 2) & 63;
            uint32_t deg[2] = {0, 0};
            const uint32_t nops = op == G::PROG_EMIT ? 1 : 2;
            for (uint32_t k = 0; k < nops; k++) {
                const uint32_t o = (uint32_t)(iw >> (k ? 32 : 8)) & 0xFFFFFF, idx = o >> 2;
                switch (o & 3) {
                    case SPACE_REG:
                        if (idx >= h.num_regs) return bad(at + ": register " + std::to_string(idx) + " of " + std::to_string(h.num_regs));
                        if (!written[idx]) return bad(at + ": register " + std::to_string(idx) + " is read before it is written");
                        deg[k] = reg_deg[idx];
                        break;
                    case SPACE_CELL:
                        if (idx >= h.num_cells) return bad(at + ": cell " + std::to_string(idx) + " of " + std::to_string(h.num_cells));
                        deg[k] = 1;
                        break;
                    case SPACE_INPUT:
                        if (idx >= h.num_inputs) return bad(at + ": input " + std::to_string(idx) + " of " + std::to_string(h.num_inputs));
                        deg[k] = idx < NUM_BUILTIN_INPUTS ? 1 : 0;   // X, L_first, L_last: 1; a param is a constant
                        if (idx == INPUT_L_FIRST || idx == INPUT_L_LAST) out->reads_lagrange = true;
                        break;
                    default:
                        if (idx >= h.num_literals) return bad(at + ": literal " + std::to_string(idx) + " of " + std::to_string(h.num_literals));
                        break;
                }
            }
            if (op == G::PROG_EMIT) {
                if (dst != 0 || ((uint32_t)(iw >> 32) & 0xFFFFFF) != 0) return bad(at + ": EMIT with a destination or a second operand");
                if (deg[0] > h.degree)
                    return bad(at + ": constraint " + std::to_string(emits) + " has degree bound " + std::to_string(deg[0]) +
                               ", the program declares " + std::to_string(h.degree));
                emits++;
                out->instrs.push_back(iw);
                continue;
            }
            if (dst >= h.num_regs) return bad(at + ": register " + std::to_string(dst) + " of " + std::to_string(h.num_regs));
            // (a bound past any quotient degree is clamped: 4096 products of it cannot wrap a u32)
            const uint32_t d = op == G::PROG_MUL ? deg[0] + deg[1] : std::max(deg[0], deg[1]);
            reg_deg[dst] = std::min(d, 1u << 16);
            written[dst] = true;
            out->instrs.push_back(iw);
        }
        if (emits != h.num_constraints)
            return bad(name + ": " + std::to_string(emits) + " EMITs, the header declares " + std::to_string(h.num_constraints) + " constraints");
        out->p[pi] = h;
        out->max_regs = std::max(out->max_regs, h.num_regs);
        out->total_cells += h.num_cells;
        out->total_constraints += h.num_constraints;
    }
    out->num_programs = num_programs;
    return SYS_OK;
}

// the scalar arguments both entry points share
inline SystemStatus check_counts(uint32_t num_challenges, uint32_t num_params, const void* params, const void* alphas, std::string* msg) {
    if (num_challenges == 0 || num_challenges > MAX_CONSTRAINT_CHALLENGES) {
        *msg = "num_challenges " + std::to_string(num_challenges) + " outside 1 .. " + std::to_string(MAX_CONSTRAINT_CHALLENGES);
        return SYS_INVALID;
    }
    if (num_params > MAX_PARAMS) { *msg = "more than " + std::to_string(MAX_PARAMS) + " params"; return SYS_INVALID; }
    if (!alphas || (num_params && !params)) { *msg = "null argument"; return SYS_INVALID; }
    return SYS_OK;
}
// params / alphas: canonical words of `width` bytes (8 Goldilocks, 4 BabyBear)
inline SystemStatus check_canonical_words(const void* v, uint32_t count, uint32_t width, uint64_t order, const char* what, std::string* msg) {
    for (uint32_t i = 0; i < count; i++) {
        const uint64_t x = width == 8 ? static_cast<const uint64_t*>(v)[i] : static_cast<const uint32_t*>(v)[i];
        if (x >= order) { *msg = std::string(what) + " " + std::to_string(i) + " is not below p"; return SYS_INVALID; }
    }
    return SYS_OK;
}

}  // namespace constraints
}  // namespace gbk

#endif

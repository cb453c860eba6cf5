// The word file of the generator-program harnesses (tests/host_shim/generator_programs.cpp, tests/device/generator_programs.hip):
// a case of schedule_case.hpp with the table of gb_circuit_set_generator_programs in front of it.  tests/generator_program_cases.py
// writes it.
//   file:  num_cases, then per case
//   case:  num_programs, program_offsets[num_programs + 1], program_words[program_offsets[num_programs]], then the case of
//          schedule_case.hpp
#pragma once
#include "generator_programs.hpp"
#include "schedule_case.hpp"

namespace program_case {

struct Case {
    std::vector<uint32_t> offsets;
    std::vector<uint64_t> words;
    schedule_case::Case circuit;
    gbk::gen::GeneratorPrograms programs;
};

inline bool parse(const std::vector<uint64_t>& in, size_t* pos, Case* c) {
    if (*pos >= in.size()) return false;
    const uint64_t np = in[(*pos)++];
    if (np > in.size() - *pos) return false;
    if (*pos + np + 1 > in.size()) return false;
    c->offsets.resize(np + 1);
    for (uint64_t i = 0; i <= np; i++) {
        if (in[*pos + i] >> 32) return false;
        c->offsets[i] = (uint32_t)in[*pos + i];
    }
    *pos += np + 1;
    const uint64_t nw = c->offsets[np];
    if (nw > in.size() - *pos) return false;
    c->words.assign(in.begin() + *pos, in.begin() + *pos + nw);
    *pos += nw;
    return schedule_case::parse(in, pos, &c->circuit);
}

// gb_circuit_set_partition, gb_circuit_set_generator_programs, then gb_circuit_set_generators
inline int schedule(Case* pc, gbk::gen::Schedule* out, std::string* msg) {
    schedule_case::Case* c = &pc->circuit;
    const char* m = "";
    if (const int s = gbk::partition::build_slot_map(c->map.data(), c->num_targets, c->num_wires << c->degree_bits, c->pis.data(),
                                                     c->num_public_inputs, c->num_public_inputs, &c->slots, &m)) {
        *msg = m;
        return s;
    }
    if (!gbk::gen::parse_generator_programs(pc->words.data(), pc->offsets.data(), (uint32_t)pc->offsets.size() - 1, c->order,
                                            (uint32_t)c->num_constants, &pc->programs, msg))
        return gbk::gen::SCHED_INVALID;
    c->map32.assign(c->map.begin(), c->map.end());
    gbk::gen::CircuitDesc d;
    d.representative_map = c->map32.data();
    d.num_targets = c->num_targets;
    d.num_wires = (uint32_t)c->num_wires;
    d.degree_bits = (uint32_t)c->degree_bits;
    d.num_constants = (uint32_t)c->num_constants;
    d.ext_degree = (uint32_t)c->ext_degree;
    d.order = c->order;
    d.slot_reps = c->slots.reps.data();
    d.num_slots = c->slots.reps.size();
    d.pi_reps = c->slots.pi_reps.data();
    d.num_public_inputs = c->slots.pi_reps.size();
    d.gates = c->gates.data();
    d.num_gates = (uint32_t)c->gates.size();
    d.constants = c->constants.data();
    d.programs = &pc->programs;
    return gbk::gen::build_schedule(d, c->records.data(), c->records.size(), c->inputs.data(), c->inputs.size(), (uint32_t)c->group_width,
                                    out, msg);
}

// what the kernels rely on beyond schedule_case::sound: a program op names a program and its row constants lie inside the array
inline bool sound(const Case& pc, const gbk::gen::Schedule& s) {
    if (!schedule_case::sound(pc.circuit, s)) return false;
    for (const gbk::gen::Op& op : s.ops) {
        if (op.kind != gbk::gen::GEN_PROGRAM) continue;
        if (op.p0 >= pc.programs.headers.size()) return false;
        const gbk::gen::ProgramHeader& h = pc.programs.headers[op.p0];
        if ((size_t)op.p1 + h.num_constants > s.row_constants.size() || op.num_in != h.num_in || op.num_out != h.num_out ||
            h.num_regs > s.program_regs)
            return false;
    }
    return s.program_regs <= gbk::gen::GP_MAX_REGS;
}

}  // namespace program_case

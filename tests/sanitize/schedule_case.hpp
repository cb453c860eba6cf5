// The word file the two generator harnesses read (tests/sanitize/generator_schedule.cpp, tests/host_shim/generators.cpp): circuits
// described the way gb_circuit_set_partition and gb_circuit_set_generators receive them.  tests/generator_cases.py writes it.
//   file:  num_cases, then per case
//   case:  num_targets, num_wires, degree_bits, num_constants, ext_degree, order, num_public_inputs, num_gates, num_records,
//          num_inputs, group_width, has_values;  representative_map[num_targets];  public_input_targets[..];
//          gates[num_gates][4] (kind, param, param2, param3);  constants[num_constants][n];  records[num_records][4] (kind, gate,
//          a, b);  input_targets[num_inputs];  and, with has_values, input_values[num_inputs]
// A count that the file cannot hold ends the program with status 3 before anything is allocated from it.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "generator_schedule.hpp"
#include "partition_map.hpp"

namespace schedule_case {

struct Case {
    uint64_t num_targets, num_wires, degree_bits, num_constants, ext_degree, order, num_public_inputs, num_gates, num_records, num_inputs,
        group_width, has_values;
    std::vector<uint64_t> map, pis, constants, inputs, values;
    std::vector<gbk::gen::GateDesc> gates;
    std::vector<gbk::gen::Record> records;
    // what the library derives before it schedules
    gbk::partition::SlotMap slots;
    std::vector<uint32_t> map32;
};

inline bool read_words(const char* path, std::vector<uint64_t>* out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t w;
    while (std::fread(&w, 8, 1, f) == 1) out->push_back(w);
    std::fclose(f);
    return true;
}

inline bool write_words(const char* path, const std::vector<uint64_t>& words) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(words.data(), 8, words.size(), f) == words.size();
    std::fclose(f);
    return ok;
}

// -> false on a malformed file
inline bool parse(const std::vector<uint64_t>& in, size_t* pos, Case* c) {
    constexpr size_t HEAD = 12;
    if (*pos + HEAD > in.size()) return false;
    const uint64_t* h = in.data() + *pos;
    c->num_targets = h[0]; c->num_wires = h[1]; c->degree_bits = h[2]; c->num_constants = h[3]; c->ext_degree = h[4]; c->order = h[5];
    c->num_public_inputs = h[6]; c->num_gates = h[7]; c->num_records = h[8]; c->num_inputs = h[9];
    c->group_width = h[10]; c->has_values = h[11];
    *pos += HEAD;
    if (c->degree_bits > 24) return false;
    const uint64_t n = (uint64_t)1 << c->degree_bits, left = in.size() - *pos;
    for (uint64_t count : {c->num_targets, c->num_public_inputs, c->num_gates * 4, c->num_constants * n, c->num_records * 4, c->num_inputs})
        if (count > left) return false;
    auto take = [&](uint64_t count, std::vector<uint64_t>* v) {
        if (*pos + count > in.size()) return false;
        v->assign(in.begin() + *pos, in.begin() + *pos + count);
        *pos += count;
        return true;
    };
    std::vector<uint64_t> g, r;
    if (!take(c->num_targets, &c->map) || !take(c->num_public_inputs, &c->pis) || !take(c->num_gates * 4, &g) ||
        !take(c->num_constants * n, &c->constants) || !take(c->num_records * 4, &r) || !take(c->num_inputs, &c->inputs))
        return false;
    if (c->has_values && !take(c->num_inputs, &c->values)) return false;
    c->gates.resize(c->num_gates);
    for (uint64_t i = 0; i < c->num_gates; i++)
        c->gates[i] = gbk::gen::GateDesc{(uint32_t)g[4 * i], (uint32_t)g[4 * i + 1], (uint32_t)g[4 * i + 2], (uint32_t)g[4 * i + 3]};
    c->records.resize(c->num_records);
    for (uint64_t i = 0; i < c->num_records; i++)
        c->records[i] = gbk::gen::Record{(uint32_t)r[4 * i], (uint32_t)r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
    return true;
}

// gb_circuit_set_partition, then gb_circuit_set_generators
inline int schedule(Case* c, gbk::gen::Schedule* out, std::string* msg) {
    const char* m = "";
    if (const int s = gbk::partition::build_slot_map(c->map.data(), c->num_targets, c->num_wires << c->degree_bits, c->pis.data(),
                                                     c->num_public_inputs, c->num_public_inputs, &c->slots, &m)) {
        *msg = m;
        return s;
    }
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
    return gbk::gen::build_schedule(d, c->records.data(), c->records.size(), c->inputs.data(), c->inputs.size(),
                                    (uint32_t)c->group_width, out, msg);
}

// what the kernels rely on (see generator_schedule.cpp)
inline bool sound(const Case& c, const gbk::gen::Schedule& s) {
    if (s.level_off.size() != (size_t)s.num_levels + 1 || s.level_off.back() != s.ops.size() || s.level_off[0] != 0) return false;
    for (size_t l = 0; l + 1 < s.level_off.size(); l++)
        if (s.level_off[l] > s.level_off[l + 1]) return false;
    if (s.class_reps.size() != s.num_classes || s.num_slots > s.num_classes) return false;
    for (const gbk::gen::Op& op : s.ops) {
        if ((size_t)op.in_off + op.num_in > s.args.size() || (size_t)op.out_off + op.num_out > s.args.size()) return false;
        for (uint32_t i = 0; i < op.num_in; i++)
            if (s.args[op.in_off + i] >= s.num_classes) return false;
        for (uint32_t i = 0; i < op.num_out; i++) {
            const uint32_t w = s.args[op.out_off + i];
            if (w != gbk::gen::OUT_SKIP && (w & ~gbk::gen::OUT_CHECK) >= s.num_classes) return false;
        }
        if (op.record >= c.records.size()) return false;
    }
    uint32_t next = 0;
    for (const gbk::gen::Launch& l : s.launches) {
        if (l.first_level != next || !l.num_levels || l.first_level + l.num_levels > s.num_levels) return false;
        for (uint32_t k = 0; k < l.num_levels; k++) {
            const uint32_t width = s.level_off[l.first_level + k + 1] - s.level_off[l.first_level + k];
            if (l.chain ? width > c.group_width : (width <= c.group_width || l.num_levels != 1)) return false;
        }
        next = l.first_level + l.num_levels;
    }
    for (uint32_t cl : s.input_cls)
        if (cl >= s.num_classes) return false;
    for (uint32_t cl : s.pi_cls)
        if (cl >= s.num_classes) return false;
    return next == s.num_levels;
}

// status; then for an accepted case: num_classes, num_slots, num_levels, num_unrunnable, num_checks, num_launches, num_ops,
// class_reps, input_cls, input_first, input_free, pi_cls, launches (first_level, num_levels, chain), level_off [num_levels + 1],
// and per op: kind, record, p0, p1, k0, k1, num_in, the dependency classes, num_out, the output words
inline void dump(int status, const gbk::gen::Schedule& s, std::vector<uint64_t>* out) {
    out->push_back((uint64_t)status);
    if (status) return;
    for (uint64_t v : {(uint64_t)s.num_classes, (uint64_t)s.num_slots, (uint64_t)s.num_levels, (uint64_t)s.num_unrunnable, (uint64_t)s.num_checks,
                       (uint64_t)s.launches.size(), (uint64_t)s.ops.size()})
        out->push_back(v);
    out->insert(out->end(), s.class_reps.begin(), s.class_reps.end());
    out->insert(out->end(), s.input_cls.begin(), s.input_cls.end());
    out->insert(out->end(), s.input_first.begin(), s.input_first.end());
    out->insert(out->end(), s.input_free.begin(), s.input_free.end());
    out->insert(out->end(), s.pi_cls.begin(), s.pi_cls.end());
    for (const gbk::gen::Launch& l : s.launches)
        for (uint64_t v : {(uint64_t)l.first_level, (uint64_t)l.num_levels, (uint64_t)l.chain}) out->push_back(v);
    out->insert(out->end(), s.level_off.begin(), s.level_off.end());
    for (const gbk::gen::Op& op : s.ops) {
        for (uint64_t v : {(uint64_t)op.kind, (uint64_t)op.record, (uint64_t)op.p0, (uint64_t)op.p1, op.k[0], op.k[1]}) out->push_back(v);
        out->push_back(op.num_in);
        for (uint32_t i = 0; i < op.num_in; i++) out->push_back(s.args[op.in_off + i]);
        out->push_back(op.num_out);
        for (uint32_t i = 0; i < op.num_out; i++) out->push_back(s.args[op.out_off + i]);
    }
}

}  // namespace schedule_case

// gen::run_op<F> with generator programs (csrc/generators.hpp gen_program, field_sqrt) compiled for the CPU and run over the
// schedule that csrc/generator_schedule.hpp makes of a circuit with program generators, op by op in the schedule's order, the
// registers in gates::ArrayRegs.  No value is compared here: tests/test_generator_programs.py holds GeneratorProgram.evaluate.
//   generator_programs <in> <out>       (the word file of tests/sanitize/program_case.hpp, every case with input values)
// out: as tests/host_shim/generators.cpp writes it.  Exit status 3 on a malformed file, 6 on an unsound schedule,
// 8 when run_op without program tables passed over a program op instead of reporting ERR_NO_PROGRAM_TABLES.
#include "generators.hpp"
#include "program_case.hpp"

using namespace gbk;

template <class F>
static bool run(const program_case::Case& pc, const gen::Schedule& s, std::vector<uint64_t>* out) {
    typedef typename F::T T;
    const schedule_case::Case& c = pc.circuit;
    std::vector<T> values(s.num_classes ? s.num_classes : 1, 0);
    for (size_t i = 0; i < s.input_cls.size(); i++)
        if (s.input_first[i] == i) values[s.input_cls[i]] = (T)c.values[i];
    std::vector<uint64_t> lits(pc.programs.lits.size());
    for (size_t i = 0; i < lits.size(); i++) lits[i] = (uint64_t)F::enc(pc.programs.lits[i]);
    T regs[gen::GP_MAX_REGS];
    const gen::Programs<gates::ArrayRegs<T>> programs{pc.programs.headers.data(), pc.programs.instrs.data(), lits.data(), s.row_constants.data(),
                                                      gates::ArrayRegs<T>{regs}};
    u32 err[gen::ERROR_WORDS] = {0, 0, 0, 0};
    for (const gen::Op& op : s.ops) gen::run_op<F>(op, s.args.data(), values.data(), err, programs);
    // run_op without its `programs` (what a schedule with program_regs == 0 runs): a program op reports, and writes nothing
    for (const gen::Op& op : s.ops) {
        if (op.kind != gen::GEN_PROGRAM) continue;
        std::vector<T> untouched(values);
        u32 e[gen::ERROR_WORDS] = {0, 0, 0, 0};
        gen::run_op<F>(op, s.args.data(), untouched.data(), e);
        if (e[0] != gen::ERR_NO_PROGRAM_TABLES || e[1] != op.record || e[2] != gen::OUT_SKIP || untouched != values) return false;
        break;
    }
    for (uint64_t v : {(uint64_t)s.num_classes, (uint64_t)s.num_levels, (uint64_t)s.launches.size(), (uint64_t)s.num_unrunnable}) out->push_back(v);
    out->insert(out->end(), s.class_reps.begin(), s.class_reps.end());
    for (u32 k = 0; k < s.num_classes; k++) out->push_back((uint64_t)values[k]);
    for (u32 e : err) out->push_back(e);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!schedule_case::read_words(argv[1], &in) || in.empty()) return 3;
    size_t pos = 1;
    for (uint64_t k = 0; k < in[0]; k++) {
        program_case::Case c;
        if (!program_case::parse(in, &pos, &c) || !c.circuit.has_values) return 3;
        gen::Schedule s;
        std::string msg;
        const int status = program_case::schedule(&c, &s, &msg);
        out.push_back((uint64_t)status);
        if (status) {
            std::printf("case %llu: %s\n", (unsigned long long)k, msg.c_str());
            continue;
        }
        if (!program_case::sound(c, s)) return 6;
        if (!(c.circuit.ext_degree == 2 ? run<GlF>(c, s, &out) : run<BbF>(c, s, &out))) return 8;
    }
    if (pos != in.size()) return 3;
    return schedule_case::write_words(argv[2], out) ? 0 : 3;
}

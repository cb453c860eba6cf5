// gen::run_op<F> (csrc/generators.hpp: the witness-generator evaluators of the generator kernels) compiled for the CPU and run
// over the schedule that csrc/generator_schedule.hpp makes of a circuit, op by op in the schedule's order - what k_generate_level
// and k_generate_chain do a level at a time.  Nothing is compared here: tests/test_generator_records.py holds the builder
// mirror's generate_partition_witness.
//   generators <in> <out>       (the word file of tests/sanitize/schedule_case.hpp, every case with input values)
// out: per case the schedule's status; for an accepted case num_classes, num_levels, num_launches, num_unrunnable, the
//      representative target of every class, the value of every class (canonical) and the error word (code, record, class, 0).
// Exit status 3 on a malformed file.
#include "generators.hpp"
#include "schedule_case.hpp"

using namespace gbk;

template <class F>
static void run(const schedule_case::Case& c, const gen::Schedule& s, std::vector<uint64_t>* out) {
    typedef typename F::T T;
    std::vector<T> values(s.num_classes ? s.num_classes : 1, 0);
    for (size_t i = 0; i < s.input_cls.size(); i++)
        if (s.input_first[i] == i) values[s.input_cls[i]] = (T)c.values[i];
    u32 err[gen::ERROR_WORDS] = {0, 0, 0, 0};
    for (const gen::Op& op : s.ops) gen::run_op<F>(op, s.args.data(), values.data(), err);
    for (uint64_t v : {(uint64_t)s.num_classes, (uint64_t)s.num_levels, (uint64_t)s.launches.size(), (uint64_t)s.num_unrunnable}) out->push_back(v);
    out->insert(out->end(), s.class_reps.begin(), s.class_reps.end());
    for (u32 k = 0; k < s.num_classes; k++) out->push_back((uint64_t)values[k]);
    for (u32 e : err) out->push_back(e);
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!schedule_case::read_words(argv[1], &in) || in.empty()) return 3;
    size_t pos = 1;
    for (uint64_t k = 0; k < in[0]; k++) {
        schedule_case::Case c;
        if (!schedule_case::parse(in, &pos, &c) || !c.has_values) return 3;
        gen::Schedule s;
        std::string msg;
        const int status = schedule_case::schedule(&c, &s, &msg);
        out.push_back((uint64_t)status);
        if (status) {
            std::printf("case %llu: %s\n", (unsigned long long)k, msg.c_str());
            continue;
        }
        if (c.ext_degree == 2) run<GlF>(c, s, &out);
        else run<BbF>(c, s, &out);
    }
    if (pos != in.size()) return 3;
    return schedule_case::write_words(argv[2], out) ? 0 : 3;
}

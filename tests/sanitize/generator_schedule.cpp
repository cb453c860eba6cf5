// The scheduler of gb_circuit_set_generators (csrc/generator_schedule.hpp, with csrc/partition_map.hpp in front of it as in the
// library) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, its own main.
//   generator_schedule <in> <out>      (the word file of tests/sanitize/schedule_case.hpp; tests/test_generator_schedule.py)
// Every op the schedule emits is checked here against what the kernels rely on: class indices below num_classes, operand runs
// inside `args`, levels in ascending order and a chain launch's levels no wider than the workgroup.  Exit status 3: malformed
// file; 6: a schedule that breaks one of these.
#include "schedule_case.hpp"

using namespace gbk::gen;

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!schedule_case::read_words(argv[1], &in) || in.empty()) return 3;
    size_t pos = 1;
    for (uint64_t k = 0; k < in[0]; k++) {
        schedule_case::Case c;
        if (!schedule_case::parse(in, &pos, &c)) return 3;
        Schedule s;
        std::string msg;
        const int status = schedule_case::schedule(&c, &s, &msg);
        if (!status && !schedule_case::sound(c, s)) return 6;
        if (status) std::printf("case %llu: %s\n", (unsigned long long)k, msg.c_str());
        schedule_case::dump(status, s, &out);
    }
    if (pos != in.size()) return 3;
    return schedule_case::write_words(argv[2], out) ? 0 : 3;
}

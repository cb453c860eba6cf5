// csrc/constraint_system.hpp alone under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_constraint_system_sanitized.py
// builds and runs this program; nothing is loaded into Python).  Input file, u64 words: the number of cases, then per case
//   order, num_oracles, has_polys, polys[16], num_rows, num_params, max_degree, num_programs, num_offsets, offsets..., num_words, words...
// The offsets and the words are copied into heap blocks of exactly their size, so a read past either is the sanitizer's to
// report.  Output file, u64 words, per case: status, total_cells, total_constraints, max_regs, reads_lagrange, instruction words,
// cell words, literals kept.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "constraint_system.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::vector<uint64_t> in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        uint64_t w;
        while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
        std::fclose(f);
    }
    size_t at = 0;
    auto next = [&]() -> uint64_t { return at < in.size() ? in[at++] : 0; };
    std::vector<uint64_t> out;
    const uint64_t cases = next();
    for (uint64_t c = 0; c < cases; c++) {
        namespace CS = gbk::constraints;
        CS::Shape sh;
        sh.order = next();
        sh.num_oracles = (uint32_t)next();
        const bool has_polys = next() != 0;
        uint32_t polys[CS::MAX_ORACLES];
        for (uint32_t i = 0; i < CS::MAX_ORACLES; i++) polys[i] = (uint32_t)next();
        sh.oracle_num_polys = has_polys ? polys : nullptr;
        sh.num_rows = next();
        sh.num_params = (uint32_t)next();
        sh.max_degree = (uint32_t)next();
        const uint32_t num_programs = (uint32_t)next();
        const size_t num_offsets = (size_t)next();
        std::unique_ptr<uint32_t[]> offsets(new uint32_t[num_offsets ? num_offsets : 1]);
        for (size_t i = 0; i < num_offsets; i++) offsets[i] = (uint32_t)next();
        const size_t num_words = (size_t)next();
        std::unique_ptr<uint64_t[]> words(new uint64_t[num_words ? num_words : 1]);
        for (size_t i = 0; i < num_words; i++) words[i] = next();
        // the ABI's contract: offsets has num_programs + 1 entries and words offsets[num_programs]; a case that breaks it is the
        // driver's mistake, not the validator's input
        if (num_programs <= gbk::gates::MAX_PROGRAMS && num_programs && (num_offsets != num_programs + 1)) return 3;
        CS::System sys;
        std::string msg;
        const CS::SystemStatus st = CS::parse_system(num_words ? words.get() : nullptr, num_offsets ? offsets.get() : nullptr, num_programs, sh, &sys, &msg);
        if (st != CS::SYS_OK && msg.empty()) return 4;   // every refusal names what it refused
        std::fprintf(stderr, "case %llu: %s\n", (unsigned long long)c, st == CS::SYS_OK ? "ok" : msg.c_str());
        const uint64_t rec[8] = {(uint64_t)st, sys.total_cells, sys.total_constraints, sys.max_regs, sys.reads_lagrange ? 1u : 0u,
                                 sys.instrs.size(), sys.cells.size(), sys.lits.size()};
        out.insert(out.end(), rec, rec + 8);
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty() && std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}

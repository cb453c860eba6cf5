// csrc/partition_map.hpp alone, under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_partition_map.py builds and
// drives it; CPU only).
//   partition_map <in> <out>
// in:  u64 words: num_cases, then per case: num_targets, num_cells, num_public_inputs, expected_public_inputs, the map
//      map_len, the map [map_len], the public-input targets [num_public_inputs].  map_len is what is allocated, num_targets what
//      the builder is told: they differ only in the case that claims 2^32 targets, which must be refused before an entry is read
// out: u64 words per case: status; on success K, reps [K], slots [num_cells], shared [K] (0 / 1), pi_reps [num_public_inputs]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "partition_map.hpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint64_t> in;
    uint64_t w;
    while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
    std::fclose(f);
    if (in.empty()) return 3;
    std::vector<uint64_t> out;
    size_t at = 1;
    for (uint64_t c = 0; c < in[0]; c++) {
        if (at + 5 > in.size()) return 3;
        const uint64_t num_targets = in[at], cells = in[at + 1], npi = in[at + 2], want_pi = in[at + 3], map_len = in[at + 4];
        at += 5;
        if (at + map_len + npi > in.size() || (map_len < num_targets && !(num_targets >> 32))) return 3;
        // exact-size copies: a read past either array is the sanitizer's to report
        std::vector<uint64_t> map(in.begin() + at, in.begin() + at + map_len);
        at += map_len;
        std::vector<uint64_t> pis(in.begin() + at, in.begin() + at + npi);
        at += npi;
        gbk::partition::SlotMap m;
        const char* msg = nullptr;
        const int st = gbk::partition::build_slot_map(map.data(), num_targets, cells, npi ? pis.data() : nullptr, npi, want_pi, &m, &msg);
        out.push_back((uint64_t)st);
        if (!msg) return 4;
        if (st != gbk::partition::MAP_OK) {
            if (!m.reps.empty() || !m.slots.empty()) return 4;   // nothing half-built is handed out
            continue;
        }
        out.push_back(m.reps.size());
        for (uint32_t r : m.reps) out.push_back(r);
        for (uint32_t s : m.slots) out.push_back(s);
        for (size_t k = 0; k < m.reps.size(); k++) out.push_back(m.is_shared((uint32_t)k) ? 1 : 0);
        for (uint32_t r : m.pi_reps) out.push_back(r);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty() && std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}

// The shared-path logic of a compressed proof (csrc/verify_compressed.hpp: sibling_counts, sibling_source, climb_level) compiled for
// the CPU over Goldilocks and the host permutation, on a word file that tests/test_verify_compressed_host.py builds from random
// index sets.  Nothing is compared here: the test holds oracle/compression.py's answers.  Built twice - plain, and with
// AddressSanitizer + UndefinedBehaviorSanitizer (its own main).
//   verify_compressed <in> <out>
// in, u64 words: the number of cases, then per case
//   height, cap_height, num_queries, leaf_width; indices[num_queries]; per query its leaf (leaf_width canonical words);
//   per query the number of stored siblings and those siblings (4 words each)
// out, u64 words, per case:
//   counts[num_queries]                                       what sibling_counts demands of every query's own path
//   per level, per query: sibling, first (sibling_source; ~0 for none) and the 4 words of the sibling that is hashed
//   per query the 4 words of its node at the cap's level
// Exit status 3 on a malformed file, 4 where a path holds fewer siblings than the climb takes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poseidon_gl_host.hpp"
#include "verify_compressed.hpp"

using namespace gbk;

struct Hasher {   // the hasher policy: one sponge state, canonical words
    u64 s[12] = {};
    void set_canonical(int i, u64 v) { s[i] = v; }
    void permute() { poseidon_gl_host::permute(s); }
    u64 out(int i) const { return s[i]; }
};

int main(int argc, char** argv) {
    typedef GlF F;
    if (argc != 3) return 2;
    std::vector<u64> in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        u64 w;
        while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
        std::fclose(f);
    }
    size_t at = 0;
    auto take = [&](size_t n) -> const u64* {
        if (n > in.size() - at) std::exit(3);
        const u64* p = in.data() + at;
        at += n;
        return p;
    };
    const u64 cases = *take(1);
    std::vector<u64> out;
    Hasher h;
    for (u64 c = 0; c < cases; c++) {
        const u64* head = take(4);
        if (head[0] > 32 || head[1] > head[0] || head[2] < 1 || head[2] > 4096 || head[3] < 1 || head[3] > 4096) return 3;
        const u32 height = (u32)head[0], cap_height = (u32)head[1], n = (u32)head[2], width = (u32)head[3], levels = height - cap_height;
        const u64* indices = take(n);
        for (u32 k = 0; k < n; k++)
            if (indices[k] >> height) return 3;
        std::vector<u64> digests((size_t)n * 4);
        for (u32 k = 0; k < n; k++) {
            const u64* leaf = take(width);
            vq::leaf_digest<F>(h, width, [leaf](u32 i) { return leaf[i]; }, digests.data() + (size_t)k * 4);
        }
        std::vector<const u64*> paths(n);
        std::vector<u32> held(n), taken(n, 0), counts(n);
        for (u32 k = 0; k < n; k++) {
            const u64 len = *take(1);
            if (len > 64) return 3;
            held[k] = (u32)len;
            paths[k] = take((size_t)len * 4);
        }
        vc::sibling_counts(indices, n, levels, counts.data());
        for (u32 k = 0; k < n; k++) out.push_back(counts[k]);
        std::vector<u64> nodes(indices, indices + n);
        for (u32 level = 0; level < levels; level++) {
            for (u32 k = 0; k < n; k++) {
                const vc::Source s = vc::sibling_source(n, k, [&](u32 j) { return nodes[j]; });
                out.push_back(s.sibling == vc::NO_QUERY ? ~(u64)0 : s.sibling);
                out.push_back(s.first == vc::NO_QUERY ? ~(u64)0 : s.first);
                if (s.sibling == vc::NO_QUERY && taken[s.first] >= held[s.first]) return 4;
                const u64* sib = s.sibling != vc::NO_QUERY ? digests.data() + (size_t)s.sibling * 4 : paths[s.first] + (size_t)taken[s.first] * 4;
                out.insert(out.end(), sib, sib + 4);
            }
            vc::climb_level<F>(h, n, nodes.data(), digests.data(), paths.data(), taken.data());
            for (auto& x : nodes) x >>= 1;
        }
        out.insert(out.end(), digests.begin(), digests.end());
        for (u32 k = 0; k < n; k++)
            if (taken[k] != counts[k]) return 5;   // the climb and the count are two statements of one rule
    }
    if (at != in.size()) return 3;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 8, out.size(), f);
    std::fclose(f);
    return 0;
}

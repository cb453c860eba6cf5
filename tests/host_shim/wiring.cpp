// csrc/wiring.hpp compiled for the CPU: the GB_HD functions gb_wiring_sigmas' kernels are made of, probed one by one, and the
// passes of kernels_wiring.hip emulated over them one element after the other.  No value is compared here:
// tests/test_wiring_host.py holds the expected ones, from tests/wiring_cases.py and Python integers.
//   wiring <in> <out>
// in (u64 words): the field (0 Goldilocks, 1 BabyBear); the number of probes, then per probe op, a, b, c, d; the number of cases,
// then per case degree_bits, num_wires, num_routed, num_targets, num_pairs, k_is[num_routed] (canonical), pairs[num_pairs][2].
//   probe ops: 0 key_bits(a)  1 digit_passes(a)  2 digit_of(a, b)  3 successor_index(a, b, c, d)  4 hook_order(a, b) as child << 32 | under
//              5 check_pair(a, b; num_targets c, num_wires d >> 32, num_routed d & 0xffffffff, 4 rows)  6 index_of_cell(a, b, c)
//              7 cell_of_index(a, b, c)  8 routed_cell(a, b, c)
//              9 find_root of a in the chain parent[t] = t - min(t, b) of c targets, then the sum of the chain's pointers
// out: one word per probe; per case the status (0, or check_pair's) and the lowest offending pair, and for status 0 the passes,
// moved cells, classes, largest class, merged targets, the representative map [num_targets] and the sigmas [num_routed][n].
// Exit status 3 on a malformed file.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wiring.hpp"

namespace {
using gbk::u32;
using gbk::u64;
namespace W = gbk::wiring;

bool read_words(const char* path, std::vector<uint64_t>* out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t w;
    while (std::fread(&w, sizeof w, 1, f) == 1) out->push_back(w);
    std::fclose(f);
    return true;
}
bool write_words(const char* path, const std::vector<uint64_t>& words) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = words.empty() || std::fwrite(words.data(), sizeof(uint64_t), words.size(), f) == words.size();
    return std::fclose(f) == 0 && ok;
}

bool probe(const uint64_t* q, std::vector<uint64_t>* out) {
    const uint64_t op = q[0], a = q[1], b = q[2], c = q[3], d = q[4];
    switch (op) {
        case 0: out->push_back(W::key_bits(a)); return true;
        case 1: out->push_back(W::digit_passes(a)); return true;
        case 2: out->push_back(W::digit_of((u32)a, (u32)b)); return true;
        case 3: out->push_back(W::successor_index((u32)a, (u32)b, c != 0, (u32)d)); return true;
        case 4: {
            u32 child, under;
            W::hook_order((u32)a, (u32)b, &child, &under);
            out->push_back((uint64_t)child << 32 | under);
            return true;
        }
        case 5: out->push_back(W::check_pair(a, b, c, 4 * (d >> 32), (u32)(d >> 32), (u32)d)); return true;
        case 6: out->push_back(W::index_of_cell((u32)a, (u32)b, (u32)c)); return true;
        case 7: out->push_back(W::cell_of_index((u32)a, (u32)b, (u32)c)); return true;
        case 8: out->push_back(W::routed_cell((u32)a, (u32)b, (u32)c)); return true;
        case 9: {
            if (c == 0 || c > (1u << 20) || a >= c) return false;
            std::vector<u32> parent(c);
            for (u64 t = 0; t < c; t++) parent[t] = (u32)(t - (t < b ? t : b));
            uint64_t word = (uint64_t)W::find_root(parent.data(), (u32)a) << 40, sum = 0;
            for (u64 t = 0; t < c; t++) {
                if (parent[t] > t) return false;   // pointers only ever fall
                sum += parent[t];
            }
            out->push_back(word | sum);
            return true;
        }
    }
    return false;
}

template <class F>
bool run_case(const std::vector<uint64_t>& in, size_t* pos, std::vector<uint64_t>* out) {
    typedef typename F::T T;
    if (in.size() - *pos < 5) return false;
    const uint64_t lg = in[*pos], nw = in[*pos + 1], nr = in[*pos + 2], num_targets = in[*pos + 3], np = in[*pos + 4];
    *pos += 5;
    if (lg > 12 || nw == 0 || nw > 256 || nr == 0 || nr > nw || num_targets < (nw << lg) || num_targets > (1u << 22)) return false;
    if (nr > in.size() - *pos || np > (in.size() - *pos - nr) / 2) return false;
    std::vector<T> k_is(nr);
    for (u64 j = 0; j < nr; j++) k_is[j] = F::enc(in[*pos + j]);
    *pos += nr;
    const uint64_t* pairs = in.data() + *pos;
    *pos += 2 * np;
    const u64 n = (u64)1 << lg, cells = nw * n;
    const u32 routed = (u32)(nr * n), nt = (u32)num_targets;

    // classes
    std::vector<u32> parent(nt);
    for (u32 t = 0; t < nt; t++) parent[t] = t;
    uint64_t bad[3] = {0, ~(uint64_t)0, ~(uint64_t)0};
    for (u64 i = 0; i < np; i++) {
        const u32 status = W::check_pair(pairs[2 * i], pairs[2 * i + 1], num_targets, cells, (u32)nw, (u32)nr);
        if (status != W::PAIR_OK) {
            if (i < bad[status]) bad[status] = i;
            continue;
        }
        if (pairs[2 * i] != pairs[2 * i + 1]) W::unite(parent.data(), (u32)pairs[2 * i], (u32)pairs[2 * i + 1]);
    }
    for (u32 status = 1; status <= 2; status++)
        if (bad[status] != ~(uint64_t)0) {
            out->push_back(status);
            out->push_back(bad[status]);
            return true;
        }
    out->push_back(0);
    out->push_back(0);
    uint64_t passes = 0;
    for (bool moved = true; moved; passes++) {
        moved = false;
        for (u32 t = 0; t < nt; t++) moved |= W::jump(parent.data(), t);
    }
    // order: counts, the compacted list, the sort's passes, the successors
    std::vector<u32> count(cells, 0), succ(routed, W::NONE), keys, vals;
    for (u32 j = 0; j < routed; j++) count[parent[W::routed_cell(j, (u32)nr, (u32)nw)]]++;
    for (u32 j = 0; j < routed; j++) {
        const u32 cell = W::routed_cell(j, (u32)nr, (u32)nw);
        if (count[parent[cell]] >= 2) {
            keys.push_back(parent[cell]);
            vals.push_back(cell);
        }
    }
    const u32 m = (u32)keys.size();
    for (u32 pass = 0; pass < W::digit_passes(cells); pass++) {
        std::vector<u32> start(W::RADIX + 1, 0), k2(m), v2(m);
        for (u32 i = 0; i < m; i++) start[W::digit_of(keys[i], pass) + 1]++;
        for (u32 d = 0; d < W::RADIX; d++) start[d + 1] += start[d];
        for (u32 i = 0; i < m; i++) {
            const u32 at = start[W::digit_of(keys[i], pass)]++;
            k2[at] = keys[i];
            v2[at] = vals[i];
        }
        keys.swap(k2);
        vals.swap(v2);
    }
    uint64_t classes = 0, largest = 0, merged = 0;
    for (u32 i = 0; i < m; i++) {
        const u32 s = W::successor_index(i, m, i + 1 < m && keys[i + 1] == keys[i], count[keys[i]]);
        if (s >= m) return false;
        const u32 index = W::index_of_cell(vals[i], (u32)lg, (u32)nw);
        if (index >= routed) return false;
        succ[index] = vals[s];
        if (i == 0 || keys[i - 1] != keys[i]) {
            classes++;
            if (count[keys[i]] > largest) largest = count[keys[i]];
        }
    }
    for (u32 t = 0; t < nt; t++) merged += parent[t] != t;
    out->push_back(passes);
    out->push_back(m);
    out->push_back(classes);
    out->push_back(largest ? largest : 1);
    out->push_back(merged);
    for (u32 t = 0; t < nt; t++) out->push_back(parent[t]);
    // sigmas: the split root tables as the context holds them
    const T w = F::two_adic_generator((u32)lg);
    std::vector<T> lo(1024), hi(n > 1024 ? n / 1024 : 1);
    T x = F::one();
    for (u32 e = 0; e < 1024; e++, x = F::mul(x, w)) lo[e] = x;
    const T w1024 = F::pow(w, 1024);
    x = F::one();
    for (size_t h = 0; h < hi.size(); h++, x = F::mul(x, w1024)) hi[h] = x;
    for (u32 i = 0; i < routed; i++) {
        const u32 cell = succ[i] == W::NONE ? W::cell_of_index(i, (u32)lg, (u32)nw) : succ[i];
        if (cell >= cells || cell % nw >= nr) return false;
        out->push_back(W::sigma_value<F>(lo.data(), hi.data(), k_is.data(), cell, (u32)nw));
    }
    return true;
}

template <class F>
bool run(const std::vector<uint64_t>& in, std::vector<uint64_t>* out) {
    size_t pos = 1;
    if (in.size() - pos < 1) return false;
    const uint64_t probes = in[pos++];
    if (probes > (in.size() - pos) / 5) return false;
    for (uint64_t q = 0; q < probes; q++, pos += 5)
        if (!probe(in.data() + pos, out)) return false;
    if (in.size() - pos < 1) return false;
    const uint64_t cases = in[pos++];
    for (uint64_t k = 0; k < cases; k++)
        if (!run_case<F>(in, &pos, out)) return false;
    return pos == in.size();
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!read_words(argv[1], &in) || in.size() < 2 || in[0] > 1) return 3;
    if (!(in[0] == 0 ? run<gbk::GlF>(in, &out) : run<gbk::BbF>(in, &out))) return 3;
    return write_words(argv[2], out) ? 0 : 3;
}

// A single-threaded host baseline for gb_wiring_sigmas (tools/wiring_times.py builds and runs it): the same result by the plain
// route - a union-find with path compression over the targets, the class minimum as representative, the routed cells of classes
// of two or more sorted by label with std::stable_sort, each one's successor, and one field product per routed cell.
//   wiring_baseline <in> [reps]
// in (u64 words): field (0 Goldilocks, 1 BabyBear), degree_bits, num_wires, num_routed, num_targets, num_pairs, k_is[num_routed],
// pairs[num_pairs][2].  Built as the host programs of tests/host_shim are (its shim.h lets a host compiler read csrc/).
// Prints per repetition: classes ms, order ms, sigmas ms, total ms, and a checksum of map and sigmas.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "field_traits.hpp"

namespace {
using gbk::u32;
using gbk::u64;

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <class F>
int run(const std::vector<uint64_t>& in, int reps) {
    typedef typename F::T T;
    const u32 lg = (u32)in[1], nw = (u32)in[2], nr = (u32)in[3];
    const u64 nt = in[4], np = in[5], n = (u64)1 << lg, cells = n * nw, routed = n * nr;
    if (in.size() != 6 + nr + 2 * np || nt < cells || nt >> 32) return 3;
    std::vector<T> k_is(nr);
    for (u32 j = 0; j < nr; j++) k_is[j] = F::enc(in[6 + j]);
    const uint64_t* pairs = in.data() + 6 + nr;
    for (u64 i = 0; i < 2 * np; i++)
        if (pairs[i] >= nt) return 3;
    for (int rep = 0; rep < reps; rep++) {
        auto t0 = std::chrono::steady_clock::now();
        std::vector<u32> parent(nt);
        std::iota(parent.begin(), parent.end(), 0u);
        auto find = [&](u32 x) {
            u32 r = x;
            while (parent[r] != r) r = parent[r];
            while (parent[x] != r) { const u32 next = parent[x]; parent[x] = r; x = next; }
            return r;
        };
        for (u64 i = 0; i < np; i++) {
            const u32 a = find((u32)pairs[2 * i]), b = find((u32)pairs[2 * i + 1]);
            if (a != b) parent[a > b ? a : b] = a > b ? b : a;   // the lower root stays: the root is the class minimum
        }
        for (u64 t = 0; t < nt; t++) parent[t] = find((u32)t);
        const double classes_ms = ms_since(t0);
        auto t1 = std::chrono::steady_clock::now();
        std::vector<u32> count(cells, 0), moved;
        for (u64 r = 0; r < n; r++)
            for (u32 c = 0; c < nr; c++) count[parent[r * nw + c]]++;
        for (u64 r = 0; r < n; r++)
            for (u32 c = 0; c < nr; c++)
                if (count[parent[r * nw + c]] >= 2) moved.push_back((u32)(r * nw + c));
        std::stable_sort(moved.begin(), moved.end(), [&](u32 x, u32 y) { return parent[x] < parent[y]; });
        std::vector<u32> succ(routed, 0xFFFFFFFFu);
        for (size_t i = 0; i < moved.size(); i++) {
            const u32 label = parent[moved[i]];
            const size_t next = i + 1 < moved.size() && parent[moved[i + 1]] == label ? i + 1 : i + 1 - count[label];
            succ[(u64)(moved[i] % nw) * n + moved[i] / nw] = moved[next];
        }
        const double order_ms = ms_since(t1);
        auto t2 = std::chrono::steady_clock::now();
        std::vector<T> subgroup(n), sigma(routed);
        const T w = F::two_adic_generator(lg);
        T x = F::one();
        for (u64 r = 0; r < n; r++, x = F::mul(x, w)) subgroup[r] = x;
        for (u32 c = 0; c < nr; c++)
            for (u64 r = 0; r < n; r++) {
                const u32 s = succ[c * n + r];
                const u64 row = s == 0xFFFFFFFFu ? r : s / nw;
                const u32 col = s == 0xFFFFFFFFu ? c : s % nw;
                sigma[c * n + r] = (T)F::dec(F::mul(k_is[col], subgroup[row]));
            }
        const double sigmas_ms = ms_since(t2);
        uint64_t sum = 0;
        for (u64 t = 0; t < nt; t++) sum = sum * 31 + parent[t];
        for (u64 i = 0; i < routed; i++) sum = sum * 31 + (uint64_t)sigma[i];
        std::printf("%.3f %.3f %.3f %.3f %016llx\n", classes_ms, order_ms, sigmas_ms, ms_since(t0), (unsigned long long)sum);
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 3;
    std::vector<uint64_t> in;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in.resize(bytes > 0 ? (size_t)bytes / 8 : 0);
    const bool ok = in.empty() || std::fread(in.data(), 8, in.size(), f) == in.size();
    std::fclose(f);
    if (!ok || in.size() < 6 || in[0] > 1 || in[1] > 32 || in[2] == 0 || in[3] == 0 || in[3] > in[2]) return 3;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 1;
    return in[0] == 0 ? run<gbk::GlF>(in, reps) : run<gbk::BbF>(in, reps);
}

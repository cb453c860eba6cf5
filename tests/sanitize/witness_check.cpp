// csrc/witness_check.hpp - the GB_HD row logic of the witness check (gb_check_witness, csrc/kernels_check.hip) - compiled alone
// for the host with AddressSanitizer and UndefinedBehaviorSanitizer, on rows the test writes.  Nothing is compared here:
// tests/test_witness_check_abi.py holds the answers of tests/witness_check_cases.py (oracle/gates.py's compute_filter and
// eval_unfiltered).
//   witness_check <in> <out>
// in:  u64 words, canonical: field, n, num_gates, num_selectors, num_constants, num_wires, the public-input hash (8 slots); the gate
//      table, 7 words per gate (kind, param, selector_index, group_start, group_end, param2, param3); the selector columns
//      [num_selectors][n]; the constants columns [num_constants][n]; the wires [num_wires][n] - each column in an allocation of
//      exactly n words, so that a read past a column is the sanitizer's finding
// out: per row and selector column three words: check::active_gate (a gate index, NO_GATE or BAD_SELECTOR), and for a gate the
//      first failing constraint's index (NO_FAILURE: none) and canonical value through check::check_row; then the row lists of
//      check::row_lists_host, the host twin of k_check_count / k_check_scan / k_check_fill: counts [num_gates + 1], offsets
//      [num_gates + 2], rows [total].
// Exit status 3 on a malformed file, 5 when an evaluator read a wire or a constant outside the gate's own.
#include <cstdio>
#include <memory>
#include <vector>

#include "witness_check.hpp"

using namespace gbk;

static constexpr u32 HEADER_WORDS = 14, GATE_WORDS = 7;

template <class F>
static int run(const std::vector<u64>& in, const char* out_path) {
    typedef typename F::T T;
    const size_t n = in[1];
    const u32 ng = (u32)in[2], nsel = (u32)in[3], nc = (u32)in[4], nw = (u32)in[5];
    if (n == 0 || ng == 0 || ng > gates::MAX_GATES || nsel == 0) return 3;
    if (in.size() != HEADER_WORDS + (size_t)GATE_WORDS * ng + ((size_t)nsel + nc + nw) * n) return 3;
    T pi_hash[8];
    for (u32 i = 0; i < 8; i++) pi_hash[i] = F::enc(in[6 + i]);
    gates::GateSet gs{};
    gs.num_gates = ng;
    gs.num_selectors = nsel;
    for (u32 g = 0; g < ng; g++) {
        const u64* h = in.data() + HEADER_WORDS + (size_t)GATE_WORDS * g;
        gs.g[g] = gb_gate{(u32)h[0], (u32)h[1], (u32)h[2], (u32)h[3], (u32)h[4], (u32)h[5], (u32)h[6]};
        if (gs.g[g].selector_index >= nsel || gs.g[g].group_end > ng) return 3;
    }
    // every column in its own allocation of exactly n words
    std::vector<std::unique_ptr<u64[]>> cols;
    const u64* src = in.data() + HEADER_WORDS + (size_t)GATE_WORDS * ng;
    for (size_t c = 0; c < (size_t)nsel + nc + nw; c++) {
        cols.emplace_back(new u64[n]);
        std::copy(src + c * n, src + (c + 1) * n, cols.back().get());
    }
    auto sel = [&](u32 col, size_t r) { return cols[col][r]; };

    std::vector<u64> out;
    bool outside = false;
    for (size_t r = 0; r < n; r++)
        for (u32 col = 0; col < nsel; col++) {
            const u32 g = check::active_gate<F>(gs, col, sel(col, r));
            u64 index = check::NO_FAILURE, value = 0;
            if (g != check::NO_GATE && g != check::BAD_SELECTOR) {
                const gb_gate& gd = gs.g[g];
                const u32 gw = gates::num_wires<F>(gd), gc = gates::num_constants<F>(gd);
                auto wire = [&](u32 w) -> T {
                    if (w >= gw || w >= nw) { outside = true; return F::zero(); }
                    return F::enc(cols[nsel + nc + w][r]);
                };
                auto konst = [&](u32 k) -> T {
                    if (k >= gc || k >= nc) { outside = true; return F::zero(); }
                    return F::enc(cols[nsel + k][r]);
                };
                const check::FirstFail<F> ff = check::check_row<F>(gs, gd, wire, konst, pi_hash);
                if (ff.seen != gates::num_constraints<F>(gd)) return 3;
                index = ff.index;
                value = ff.failed() ? F::dec(ff.value) : 0;
            }
            out.push_back(g);
            out.push_back(index);
            out.push_back(value);
        }
    // the row lists over the selector columns as one block [num_selectors][n], in an allocation of exactly that length
    std::unique_ptr<u64[]> selectors(new u64[(size_t)nsel * n]);
    for (u32 col = 0; col < nsel; col++) std::copy(cols[col].get(), cols[col].get() + n, selectors.get() + (size_t)col * n);
    const check::RowLists lists = check::row_lists_host<F>(gs, selectors.get(), n);
    out.insert(out.end(), lists.counts.begin(), lists.counts.end());
    out.insert(out.end(), lists.offsets.begin(), lists.offsets.end());
    out.insert(out.end(), lists.rows.begin(), lists.rows.end());
    if (outside) return 5;
    FILE* f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 3;
    std::fclose(f);
    std::printf("rows=%zu gates=%u selectors=%u\n", n, ng, nsel);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<u64> in;
    u64 w;
    while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
    std::fclose(f);
    if (in.size() < HEADER_WORDS) return 3;
    return in[0] == 0 ? run<GlF>(in, argv[2]) : run<BbF>(in, argv[2]);
}

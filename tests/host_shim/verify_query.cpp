// The checks of one FRI query round (csrc/verify_query.hpp) compiled for the CPU over Goldilocks and the host permutation, on a word
// file that tests/test_verify_query_host.py derives from a serialized proof.  Nothing is compared here: the test holds the verdicts
// of oracle/verifier.py's verify_fri.  Built twice - plain, and with AddressSanitizer + UndefinedBehaviorSanitizer (its own main).
//   verify_query <in> <out>
// in, u64 words, all canonical:
//   nqr, lgN, cap_height, num_layers, final_len, batch_sizes[2], widths[4], row_widths[4], arity_bits[num_layers]
//   fri_alpha (2), red_open[2] (4), alpha_shift[2] (4), points[2] (4), betas[num_layers] (2 each), final_poly[final_len] (2 each)
//   x_indices[nqr]
//   caps: the four oracles', then the layers', each 4 << cap_height words
//   per query round: per oracle its row (row_widths words) and its path (4 (lgN - cap_height) words); per layer its coset
//   (2 << arity_bits words) and its path (4 words per level down to the cap)
// out: per query round one word - the position (verify_query.hpp pos_*) of the first check that fails, or ~0.
// Exit status 3 on a malformed file.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poseidon_gl_host.hpp"
#include "verify_query.hpp"

using namespace gbk;

struct Hasher {   // the hasher policy: one sponge state, canonical words
    u64 s[12] = {};
    void set_canonical(int i, u64 v) { s[i] = v; }
    void permute() { poseidon_gl_host::permute(s); }
    u64 out(int i) const { return s[i]; }
};

int main(int argc, char** argv) {
    typedef GlF F;
    typedef F::E E;
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
        if (at + n > in.size()) std::exit(3);
        const u64* p = in.data() + at;
        at += n;
        return p;
    };
    const u64* head = take(5);
    const u32 nqr = (u32)head[0], lgN = (u32)head[1], capH = (u32)head[2], nl = (u32)head[3], final_len = (u32)head[4];
    if (lgN > 32 || capH > lgN || nl > 32) return 3;
    u32 batch_sizes[2], widths[4], row_widths[4];
    std::vector<u32> arity(nl);
    { const u64* p = take(2); for (int i = 0; i < 2; i++) batch_sizes[i] = (u32)p[i]; }
    { const u64* p = take(4); for (int i = 0; i < 4; i++) widths[i] = (u32)p[i]; }
    { const u64* p = take(4); for (int i = 0; i < 4; i++) row_widths[i] = (u32)p[i]; }
    { const u64* p = take(nl); for (u32 i = 0; i < nl; i++) arity[i] = (u32)p[i]; }
    if (batch_sizes[0] != widths[0] + widths[1] + widths[2] + widths[3] || batch_sizes[1] > widths[2]) return 3;
    for (int o = 0; o < 4; o++)
        if (row_widths[o] < widths[o]) return 3;
    auto ext = [&]() {
        const u64* p = take(2);
        E e = F::ezero();
        F::set_coord(e, 0, p[0]);
        F::set_coord(e, 1, p[1]);
        return e;
    };
    const E alpha = ext();
    E red_open[2], alpha_shift[2], points[2];
    for (auto& e : red_open) e = ext();
    for (auto& e : alpha_shift) e = ext();
    for (auto& e : points) e = ext();
    std::vector<E> betas(nl), fin(final_len);
    for (auto& e : betas) e = ext();
    for (auto& e : fin) e = ext();
    const u64* x_indices = take(nqr);
    const size_t cap_words = (size_t)4 << capH;
    const u64* caps = take((4 + nl) * cap_words);
    std::vector<u32> layer_path(nl);
    {
        u32 h = lgN;
        for (u32 li = 0; li < nl; li++) {
            if (arity[li] < 1 || arity[li] > 8 || h < arity[li] + capH) return 3;
            h -= arity[li];
            layer_path[li] = h - capH;
        }
    }
    std::vector<u64> out;
    for (u32 qr = 0; qr < nqr; qr++) {
        const u64 x_index = x_indices[qr];
        if (x_index >> lgN) return 3;
        const unsigned char* rows[4];
        u32 pos = ~0u;
        Hasher h;
        for (u32 o = 0; o < 4; o++) {
            const u64* row = take(row_widths[o]);
            const u64* path = take((size_t)4 * (lgN - capH));
            rows[o] = reinterpret_cast<const unsigned char*>(row);
            if (pos == ~0u && !vq::merkle_path_ok<F>(h, rows[o], row_widths[o], x_index, reinterpret_cast<const unsigned char*>(path),
                                                     lgN - capH, caps + o * cap_words))
                pos = vq::pos_initial_path(o);
        }
        std::vector<const u64*> cosets(nl), paths(nl);
        for (u32 li = 0; li < nl; li++) {
            cosets[li] = take((size_t)2 << arity[li]);
            paths[li] = take((size_t)4 * layer_path[li]);
        }
        if (pos == ~0u) {
            const u64 x = vq::subgroup_x<F>(lgN, x_index);
            auto poly = [&](u32 b, u32 i) {
                u32 o = 2;
                if (b == 0) {
                    o = 0;
                    while (i >= widths[o]) { i -= widths[o]; o++; }
                }
                return vq::load_word<F>(rows[o] + (size_t)i * 8);
            };
            const E old_eval = vq::combine_initial<F>(2, batch_sizes, points, red_open, alpha_shift, alpha, x, poly);
            pos = vq::fold_checks<F>(
                4, nl, arity.data(), x_index, x, old_eval, final_len,
                [&](u32 li) { return reinterpret_cast<const unsigned char*>(cosets[li]); }, [&](u32 li) { return betas[li]; },
                [&](u32 i) { return fin[i]; },
                [&](u32 li, u64 coset_index) {
                    return vq::merkle_path_ok<F>(h, reinterpret_cast<const unsigned char*>(cosets[li]), 2u << arity[li], coset_index,
                                                 reinterpret_cast<const unsigned char*>(paths[li]), layer_path[li],
                                                 caps + (4 + li) * cap_words);
                });
        }
        out.push_back(pos == ~0u ? ~(u64)0 : pos);
    }
    if (at != in.size()) return 3;
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 8, out.size(), f);
    std::fclose(f);
    return 0;
}

// gates::eval_gate<F, A> and gates::filter<F, A> (csrc/gates.hpp) compiled for the CPU over both algebras - BaseAlg<F>, what the
// quotient kernel instantiates, and ExtAlg<F>, what gb_verify runs at zeta - on caller-supplied rows.  Nothing is compared here:
// tests/test_device_headers_on_host.py holds the answers of oracle/gates.py (tests/gate_variants.py writes the file).
//   gate_eval <in> <out>
// in:  u64 words: field, nrows, num_gates, width (1 = BaseAlg, D = ExtAlg), the public-input hash (8 slots), two_adic_subgroup(4)
//      (16), 1 / 2^b for b = 0..4 - all canonical; then per gate: kind, param, selector_index, group_start, group_end, param2,
//      param3, subset (unused here: the verifier evaluates every gate in one pass), the gate's own index, many_selectors,
//      num_wires, num_constants, num_constraints; wires [num_wires][nrows][width]; constants [num_constants][nrows][width]; the
//      selector [nrows][width]
// out: per gate: gates::num_wires / num_constraints / num_constants of the tuple; the number of constraints emitted per row
//      [nrows]; the constraints [num_constraints][nrows][width]; the filter [nrows][width] - canonical.
// Exit status 3 on a malformed file, 4 when the file's interpolation tables differ from the ones computed here the way
// build_gate_set computes them, 5 when an evaluator read a wire or a constant outside the gate's own.
#include <cstdio>
#include <vector>

#include "gates.hpp"

using namespace gbk;

static constexpr u32 HEADER_WORDS = 33, GATE_WORDS = 13;

template <class F, class A>
struct Words;
template <class F>
struct Words<F, gates::BaseAlg<F>> {
    static typename F::T load(const u64* p) { return F::enc(p[0]); }
    static void store(typename F::T v, u64* p) { p[0] = F::dec(v); }
};
template <class F>
struct Words<F, gates::ExtAlg<F>> {
    static typename F::E load(const u64* p) {
        typename F::E e = F::ezero();
        for (u32 k = 0; k < F::D; k++) F::set_coord(e, k, F::enc(p[k]));
        return e;
    }
    static void store(typename F::E v, u64* p) {
        for (u32 k = 0; k < F::D; k++) p[k] = F::dec(F::coord(v, k));
    }
};

template <class F, class A>
static int run(const std::vector<u64>& in, u32 width, const char* out_path) {
    typedef typename F::T T;
    typedef typename A::V V;
    typedef Words<F, A> IO;
    const u32 nrows = (u32)in[1], ngates = (u32)in[2];
    if (nrows == 0) return 3;
    // the tables as build_gate_set (csrc/prover_host.inc) fills them
    gates::GateSet gs{};
    gs.num_gates = 1;
    {
        const T g16 = F::two_adic_generator(gates::MAX_INTERPOLATION_BITS);
        T x = F::one();
        for (u32 i = 0; i < 16; i++) { gs.subgroup16[i] = x; x = F::mul(x, g16); }
        for (u32 b = 0; b <= gates::MAX_INTERPOLATION_BITS; b++) gs.inv_pow2[b] = F::inv(F::enc(1u << b));
    }
    for (u32 i = 0; i < 16; i++)
        if (F::dec((T)gs.subgroup16[i]) != in[12 + i]) return 4;
    for (u32 b = 0; b < 5; b++)
        if (F::dec((T)gs.inv_pow2[b]) != in[28 + b]) return 4;
    T pi_hash[8];
    for (u32 i = 0; i < 8; i++) pi_hash[i] = F::enc(in[4 + i]);

    std::vector<u64> out;
    size_t pos = HEADER_WORDS;
    bool outside = false;
    for (u32 g = 0; g < ngates; g++) {
        if (pos + GATE_WORDS > in.size()) return 3;
        const u64* h = in.data() + pos;
        const gb_gate gd{(u32)h[0], (u32)h[1], (u32)h[2], (u32)h[3], (u32)h[4], (u32)h[5], (u32)h[6]};
        const u32 own = (u32)h[8], nw = (u32)h[10], nc = (u32)h[11], ncons = (u32)h[12];
        const bool many = h[9] != 0;
        const size_t stride = (size_t)nrows * width;
        if (pos + GATE_WORDS + ((size_t)nw + nc + 1) * stride > in.size()) return 3;
        const u64* wires = h + GATE_WORDS;
        const u64* consts = wires + (size_t)nw * stride;
        const u64* sel = consts + (size_t)nc * stride;
        pos += GATE_WORDS + ((size_t)nw + nc + 1) * stride;
        gs.g[0] = gd;
        const size_t base = out.size();
        out.resize(base + 3 + nrows + ((size_t)ncons + 1) * stride, 0);
        out[base] = gates::num_wires<F>(gd);
        out[base + 1] = gates::num_constraints<F>(gd);
        out[base + 2] = gates::num_constants<F>(gd);
        u64* counts = out.data() + base + 3;
        u64* cons = counts + nrows;
        u64* filt = cons + (size_t)ncons * stride;
        for (u32 j = 0; j < nrows; j++) {
            u32 idx = 0;
            auto wire = [&](u32 col) -> V {
                if (col >= nw) { outside = true; return A::cst(F::zero()); }
                return IO::load(wires + (size_t)col * stride + (size_t)j * width);
            };
            auto konst = [&](u32 i) -> V {
                if (i >= nc) { outside = true; return A::cst(F::zero()); }
                return IO::load(consts + (size_t)i * stride + (size_t)j * width);
            };
            auto emit = [&](V c) {
                if (idx < ncons) IO::store(c, cons + (size_t)idx * stride + (size_t)j * width);
                idx++;
            };
            gates::eval_gate<F, A>(gs, gd, wire, konst, pi_hash, emit);
            counts[j] = idx;
            IO::store(gates::filter<F, A>(own, gd, IO::load(sel + (size_t)j * width), many), filt + (size_t)j * width);
        }
    }
    if (pos != in.size()) return 3;
    if (outside) return 5;
    FILE* f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 3;
    std::fclose(f);
    std::printf("gates=%u rows=%u width=%u\n", ngates, nrows, width);
    return 0;
}

template <class F>
static int run_field(const std::vector<u64>& in, const char* out_path) {
    const u32 width = (u32)in[3];
    if (width == 1) return run<F, gates::BaseAlg<F>>(in, width, out_path);
    if (width == F::D) return run<F, gates::ExtAlg<F>>(in, width, out_path);
    return 3;
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
    return in[0] == 0 ? run_field<GlF>(in, argv[2]) : run_field<BbF>(in, argv[2]);
}

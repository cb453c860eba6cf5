// gates::eval_gate<F, BaseAlg<F>, SUBSET> and gates::filter<F, BaseAlg<F>> (csrc/gates.hpp) on the GPU as the quotient kernel's
// two launches instantiate them - LIGHT_GATES for the short gates, HEAVY_GATES for PoseidonGate / Poseidon2BabyBearGate - one
// thread per row of caller-supplied wires, constants and selector values, the emitted constraints written back.  Nothing is
// compared here: tests/test_device_gate_eval.py holds the answers of oracle/gates.py (tests/gate_variants.py writes the file).
//   gate_eval <in> <out>
// in:  u64 words: field, nrows, num_gates, width (1), the public-input hash (8 slots), two_adic_subgroup(4) (16), 1 / 2^b for
//      b = 0..4 - all canonical; then per gate: kind, param, selector_index, group_start, group_end, param2, param3, subset
//      (1 heavy, 2 light), the gate's own index, many_selectors, num_wires, num_constants, num_constraints; wires
//      [num_wires][nrows]; constants [num_constants][nrows]; the selector [nrows]
// out: per gate: gates::num_wires / num_constraints / num_constants of the tuple; the number of constraints emitted per row
//      [nrows]; the constraints [num_constraints][nrows]; the filter [nrows] - canonical.  One launch per gate.
// Exit status 2 on a HIP error, 3 on a malformed file, 4 when the file's interpolation tables differ from the ones computed here
// the way build_gate_set computes them, 5 when an evaluator asked for a wire or a constant outside the gate's own (it is given
// zero instead: nothing is read or written out of bounds).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "gates.hpp"

using namespace gbk;

static constexpr u32 BLOCK = 256, HEADER_WORDS = 33, GATE_WORDS = 13;

template <class F, int SUBSET>
__global__ __launch_bounds__(BLOCK) void k_eval(gates::GateSet gs, u32 own, u32 many, u32 nw, u32 nc, u32 ncons,
                                                const typename F::T* __restrict__ pi_hash, const u64* __restrict__ wires,
                                                const u64* __restrict__ consts, const u64* __restrict__ sel, u64* __restrict__ counts,
                                                u64* __restrict__ cons, u64* __restrict__ filt, u32* __restrict__ outside, u32 nrows) {
    typedef typename F::T T;
    typedef gates::BaseAlg<F> A;
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nrows) return;
    const gb_gate& gd = gs.g[0];
    u32 idx = 0;
    bool out_of_gate = false;
    auto wire = [&](u32 col) -> T {
        if (col >= nw) { out_of_gate = true; return F::zero(); }
        return F::enc(wires[(size_t)col * nrows + j]);
    };
    auto konst = [&](u32 i) -> T {
        if (i >= nc) { out_of_gate = true; return F::zero(); }
        return F::enc(consts[(size_t)i * nrows + j]);
    };
    auto emit = [&](T c) {
        if (idx < ncons) cons[(size_t)idx * nrows + j] = F::dec(c);
        idx++;
    };
    gates::eval_gate<F, A, SUBSET>(gs, gd, wire, konst, pi_hash, emit);
    counts[j] = idx;
    filt[j] = F::dec(gates::filter<F, A>(own, gd, F::enc(sel[j]), many != 0));
    if (out_of_gate) *outside = 1;
}

#define HIP_OK(e)                                                          \
    do {                                                                   \
        if ((e) != hipSuccess) {                                           \
            std::fprintf(stderr, "HIP error at line %d\n", __LINE__);      \
            return 2;                                                      \
        }                                                                  \
    } while (0)

template <class F>
static int run(const std::vector<u64>& in, const char* out_path) {
    typedef typename F::T T;
    const u32 nrows = (u32)in[1], ngates = (u32)in[2];
    if (nrows == 0 || in[3] != 1) return 3;
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

    // one pass over the file for the sizes: the whole input and the whole output live in two device buffers
    struct Gate {
        gb_gate gd;
        u32 subset, own, many, nw, nc, ncons;
        size_t in_off, out_off;   // of the gate's wires in the file / of its figures in the output, in words
    };
    std::vector<Gate> gl(ngates);
    size_t pos = HEADER_WORDS, nout = 0;
    for (u32 g = 0; g < ngates; g++) {
        if (pos + GATE_WORDS > in.size()) return 3;
        const u64* h = in.data() + pos;
        Gate& x = gl[g];
        x.gd = gb_gate{(u32)h[0], (u32)h[1], (u32)h[2], (u32)h[3], (u32)h[4], (u32)h[5], (u32)h[6]};
        x.subset = (u32)h[7], x.own = (u32)h[8], x.many = (u32)h[9], x.nw = (u32)h[10], x.nc = (u32)h[11], x.ncons = (u32)h[12];
        if (x.subset != gates::HEAVY_GATES && x.subset != gates::LIGHT_GATES) return 3;
        x.in_off = pos + GATE_WORDS;
        x.out_off = nout;
        pos += GATE_WORDS + ((size_t)x.nw + x.nc + 1) * nrows;
        nout += 3 + (size_t)nrows + ((size_t)x.ncons + 1) * nrows;
        if (pos > in.size()) return 3;
    }
    if (pos != in.size()) return 3;

    u64 *in_d, *out_d;
    T* pi_d;
    u32* outside_d;
    HIP_OK(hipMalloc(&in_d, in.size() * 8));
    HIP_OK(hipMalloc(&out_d, (nout ? nout : 1) * 8));
    HIP_OK(hipMalloc(&pi_d, sizeof(pi_hash)));
    HIP_OK(hipMalloc(&outside_d, 4));
    HIP_OK(hipMemcpy(in_d, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(pi_d, pi_hash, sizeof(pi_hash), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(out_d, 0, (nout ? nout : 1) * 8));
    HIP_OK(hipMemset(outside_d, 0, 4));
    for (const Gate& x : gl) {
        gs.g[0] = x.gd;
        const u64* wires = in_d + x.in_off;
        const u64* consts = wires + (size_t)x.nw * nrows;
        const u64* sel = consts + (size_t)x.nc * nrows;
        u64* counts = out_d + x.out_off + 3;
        u64* cons = counts + nrows;
        u64* filt = cons + (size_t)x.ncons * nrows;
        const dim3 grid((nrows + BLOCK - 1) / BLOCK), block(BLOCK);
        if (x.subset == gates::HEAVY_GATES)
            hipLaunchKernelGGL((k_eval<F, gates::HEAVY_GATES>), grid, block, 0, 0, gs, x.own, x.many, x.nw, x.nc, x.ncons, pi_d, wires, consts,
                               sel, counts, cons, filt, outside_d, nrows);
        else
            hipLaunchKernelGGL((k_eval<F, gates::LIGHT_GATES>), grid, block, 0, 0, gs, x.own, x.many, x.nw, x.nc, x.ncons, pi_d, wires, consts,
                               sel, counts, cons, filt, outside_d, nrows);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipDeviceSynchronize());
    std::vector<u64> out(nout);
    u32 outside = 0;
    HIP_OK(hipMemcpy(out.data(), out_d, nout * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&outside, outside_d, 4, hipMemcpyDeviceToHost));
    if (outside) return 5;
    for (const Gate& x : gl) {
        out[x.out_off] = gates::num_wires<F>(x.gd);
        out[x.out_off + 1] = gates::num_constraints<F>(x.gd);
        out[x.out_off + 2] = gates::num_constants<F>(x.gd);
    }
    FILE* f = std::fopen(out_path, "wb");
    if (!f || std::fwrite(out.data(), 8, nout, f) != nout) return 3;
    std::fclose(f);
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

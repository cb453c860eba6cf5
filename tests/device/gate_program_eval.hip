// gates::run_program<F, BaseAlg<F>> (csrc/gates.hpp) on the GPU with the register file in LDS, as k_gate_programs runs it: one
// thread per row of caller-supplied wires and constants, the emitted constraints written back.  Nothing is checked here: the
// caller (tests/test_device_gate_programs.py) compares with GateProgram.evaluate.
//   gate_program_eval <in> <out>
// in:  u64 words: field, nrows, num_wires, num_constants, num_constraints, num_regs, num_literals, num_instrs; the literals; the
//      instruction words; wires [num_wires][nrows]; constants [num_constants][nrows] - canonical values
// out: u64 [num_constraints][nrows] canonical.  Exit status 2 on a HIP error, 3 on a malformed file.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "gates.hpp"

using namespace gbk;

static constexpr u32 BLOCK = 256;
template <class F>
__global__ __launch_bounds__(BLOCK) void k_eval(const u64* __restrict__ ins, u32 num_instrs, const typename F::T* __restrict__ lits,
                                                const u64* __restrict__ wires, const u64* __restrict__ consts, u64* __restrict__ out,
                                                u32 nrows) {
    typedef typename F::T T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const gates::LdsRegs<T> regs{reinterpret_cast<T*>(smem) + threadIdx.x, BLOCK};
    const u32 j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nrows) return;
    u32 idx = 0;
    auto wire = [&](u32 col) { return F::enc(wires[(size_t)col * nrows + j]); };
    auto konst = [&](u32 i) { return F::enc(consts[(size_t)i * nrows + j]); };
    auto emit = [&](T c) { out[(size_t)(idx++) * nrows + j] = F::dec(c); };
    gates::run_program<F, gates::BaseAlg<F>>(ins, num_instrs, lits, regs, wire, konst, emit);
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
    const u32 nrows = (u32)in[1], nw = (u32)in[2], nc = (u32)in[3], ncons = (u32)in[4], nregs = (u32)in[5], nlits = (u32)in[6], nins = (u32)in[7];
    if (nregs > gates::MAX_PROGRAM_REGS || nrows == 0 || in.size() != 8 + (size_t)nlits + nins + ((size_t)nw + nc) * nrows) return 3;
    std::vector<T> lits(nlits ? nlits : 1);
    for (u32 i = 0; i < nlits; i++) lits[i] = F::enc(in[8 + i]);
    const u64* ins_h = in.data() + 8 + nlits;
    const u64* wires_h = ins_h + nins;
    u64 *ins_d, *wires_d, *out_d;
    T* lits_d;
    const size_t nvals = ((size_t)nw + nc) * nrows, nout = (size_t)ncons * nrows;
    HIP_OK(hipMalloc(&ins_d, (nins ? nins : 1) * 8));
    HIP_OK(hipMalloc(&lits_d, lits.size() * sizeof(T)));
    HIP_OK(hipMalloc(&wires_d, (nvals ? nvals : 1) * 8));
    HIP_OK(hipMalloc(&out_d, (nout ? nout : 1) * 8));
    HIP_OK(hipMemcpy(ins_d, ins_h, nins * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(lits_d, lits.data(), lits.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(wires_d, wires_h, nvals * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL((k_eval<F>), dim3((nrows + BLOCK - 1) / BLOCK), dim3(BLOCK), (size_t)(nregs ? nregs : 1) * BLOCK * sizeof(T), 0, ins_d,
                       nins, lits_d, wires_d, wires_d + (size_t)nw * nrows, out_d, nrows);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<u64> out(nout);
    HIP_OK(hipMemcpy(out.data(), out_d, nout * 8, hipMemcpyDeviceToHost));
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
    if (in.size() < 8) return 3;
    return in[0] == 0 ? run<GlF>(in, argv[2]) : run<BbF>(in, argv[2]);
}

// csrc/fold_acc.hpp's FoldAcc<GlF> / FoldAcc<BbF> - the unreduced alpha-fold sums of the gate kernels - and gl::fold160 compiled for the
// CPU (ROCm clang++, -include shim.h: the portable branches of the field headers) and run on the chains of fold_acc_cases.hpp.  Prints
// the census lines, then per family "name cases=N mismatches=M (...)"; exit status 1 on a mismatch, 3 when the case generator fails its
// own checks, 4 when a census class is empty.  tests/device/fold_acc.hip runs the same chains on the GPU.
// Built and run by tests/test_fold_acc_host.py.
#include "fold_acc.hpp"
#include "gate_set.hpp"
#include "fold_acc_cases.hpp"

namespace fc = fold_acc_cases;
using gbk::BbF;
using gbk::GlF;
typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned __int128 u128;

// The term count the chains go up to is the one fold_acc.hpp states, it covers every constraint program, and it is inside what both
// forms rely on: Goldilocks l4 <= 2^31 (one carry per term at most), BabyBear a u32 hi that does not wrap.
static_assert(fc::MAX_TERMS == gbk::FOLD_ACC_MAX_TERMS, "the chains stop where fold_acc.hpp says the gates do");
static_assert(gbk::gates::MAX_PROGRAM_CONSTRAINTS <= gbk::FOLD_ACC_MAX_TERMS, "a constraint program's constraints fit a chain");
static_assert((u64)gbk::FOLD_ACC_MAX_TERMS <= (1ULL << 31), "Goldilocks: l4 <= terms <= fold160's r4 bound");
static_assert((((u128)gbk::FOLD_ACC_MAX_TERMS * (bb::P - 1) * (bb::P - 1)) >> 64) < ((u128)1 << 32), "BabyBear: hi does not wrap");
static_assert((u64)bb::R2 < bb::P, "BabyBear: hi R2 < p 2^32 for every u32 hi");

template <class F, class C>
static size_t run(const C& ch) {
    typedef typename F::T T;
    std::vector<T> out(ch.count());
    for (size_t i = 0; i < ch.count(); i++) {
        gbk::FoldAcc<F> s;
        for (u32 t = ch.off[i]; t < ch.off[i + 1]; t++) s.acc(ch.c[t], ch.a[t]);
        out[i] = s.finish();
    }
    return fc::report(ch, out);
}

int main() {
    const fc::Chains<fc::GlAcc> gl = fc::gl_chains();
    const fc::Chains<fc::BbAcc> bb = fc::bb_chains();
    const fc::Fold160Cases f160 = fc::fold160_cases(gl);
    bool census = fc::print_census("gl_fold_acc", gl.census);
    census = fc::print_census("bb_fold_acc", bb.census) && census;
    census = fc::print_census("gl_fold160", f160.census) && census;
    size_t bad = run<GlF>(gl) + run<BbF>(bb);
    {
        std::vector<u64> out(f160.count());
        for (size_t i = 0; i < f160.count(); i++) {
            const fc::U160& s = f160.in[i];
            out[i] = gl::canon(gl::fold160(s.l[0], s.l[1], s.l[2], s.l[3], s.l[4]));
        }
        bad += fc::report(f160, out);
    }
    printf("total mismatches=%zu\n", bad);
    return bad ? 1 : census ? 0 : 4;
}

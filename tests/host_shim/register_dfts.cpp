// csrc/dft_gl.hpp, csrc/dft_bb.hpp and csrc/ntt_outer.hpp's dft_r compiled for the CPU (ROCm clang++, -include shim.h: the portable
// branches of the field headers) and run on the cases of register_dft_cases.hpp, one function and direction at a time.  Prints
// "gl_edges=N", "bb_edges=N" and one line "name cases=N mismatches=M (...)" per function; exit status 1 on a mismatch, 3 when the case
// generator fails its own checks.  tests/device/register_dfts.hip runs the same cases on the GPU.
// Built and run by tests/test_register_dfts_host.py.
#include <cstddef>

// ntt_outer.hpp keeps dft_r next to its kernels and launchers: names for those to parse against (none of them is instantiated here)
#define __global__
#define __launch_bounds__(...)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static const dim3 blockIdx, threadIdx;
typedef void* hipStream_t;
enum { hipMemcpyDeviceToDevice = 3 };
inline int hipMemcpyAsync(void*, const void*, size_t, int, hipStream_t) { return 0; }
inline unsigned __brev(unsigned x) {
    unsigned r = 0;
    for (int i = 0; i < 32; i++) r |= ((x >> i) & 1u) << (31 - i);
    return r;
}
#define hipLaunchKernelGGL(...) ((void)0)

#include "dft_bb.hpp"
#include "dft_gl.hpp"
#include "ntt_outer.hpp"
#include "register_dft_cases.hpp"

namespace rc = register_dft_cases;
using gbk::BbF;
using gbk::GlF;
typedef unsigned long long u64;
typedef unsigned int u32;

// the functions under test on a case's words x[0 .. W)
template <class T, bool INV>
struct Dft16 {
    static void run(T* x, T) { gbk::dft16<INV>(*reinterpret_cast<T(*)[16]>(x)); }
};
template <class T, bool INV>
struct Dft32 {
    static void run(T* x, T) { gbk::dft32<INV>(*reinterpret_cast<T(*)[32]>(x)); }
};
template <class T, bool INV, int K>
struct DftSmall {
    static void run(T* x, T) {
        T y[16] = {};
        for (int i = 0; i < (1 << K); i++) y[i] = x[i];
        gbk::dft_small<INV, K>(y);
        for (int i = 0; i < (1 << K); i++) x[i] = y[i];
    }
};
template <class T, bool INV, int H, int O>
struct Layer64 {
    static void run(T* x, T) {
        T y[64] = {};
        for (int i = 0; i < 2 * H; i++) y[O + i] = x[i];
        gbk::layer64<INV, H, O>(y);
        for (int i = 0; i < 2 * H; i++) x[i] = y[O + i];
    }
};
template <class F, int K>
struct DftR {
    typedef typename F::T T;
    static void run(T* x, T wr) { gbk::outer::dft_r<F, (u32)K>(*reinterpret_cast<T(*)[1u << K]>(x), wr); }
};
template <int K>
struct MulPow2 {
    static void run(u64* x, u64) { x[0] = gbk::mul_pow2<K>(x[0]); }
};

static size_t total_bad = 0;
template <class Fn, class R>
static void check(const rc::Cases<R>& c) {
    std::vector<typename R::W> out = c.in;
    const size_t w = (size_t)c.width;
    for (size_t i = 0; i < c.count(); i++) Fn::run(&out[i * w], c.wr);
    total_bad += rc::report(c, out);
}

template <class R, class T, bool INV>
static void dfts(const std::string& f) {
    const std::string d = INV ? "_inv" : "_fwd";
    check<Dft16<T, INV>>(rc::dft_cases<R>(f + "_dft16" + d, 4, INV));
    check<Dft32<T, INV>>(rc::dft_cases<R>(f + "_dft32" + d, 5, INV));
    check<DftSmall<T, INV, 1>>(rc::dft_cases<R>(f + "_dft_small1" + d, 1, INV));
    check<DftSmall<T, INV, 2>>(rc::dft_cases<R>(f + "_dft_small2" + d, 2, INV));
    check<DftSmall<T, INV, 3>>(rc::dft_cases<R>(f + "_dft_small3" + d, 3, INV));
    // every (H, O) that ntt_passes.hpp's k_intt16_p2w and the two dft32 instantiate
    check<Layer64<T, INV, 32, 0>>(rc::layer_cases<R>(f + "_layer64_h32_o0" + d, 5, INV));
    check<Layer64<T, INV, 16, 0>>(rc::layer_cases<R>(f + "_layer64_h16_o0" + d, 4, INV));
    check<Layer64<T, INV, 16, 32>>(rc::layer_cases<R>(f + "_layer64_h16_o32" + d, 4, INV));
}
template <class R, class F>
static void outer_dfts(const std::string& f) {
    for (int inv = 0; inv < 2; inv++) {
        const std::string d = inv ? "_inv" : "_fwd";
        check<DftR<F, 1>>(rc::dft_r_cases<R>(f + "_dft_r1" + d, 1, inv));
        check<DftR<F, 2>>(rc::dft_r_cases<R>(f + "_dft_r2" + d, 2, inv));
        check<DftR<F, 3>>(rc::dft_r_cases<R>(f + "_dft_r3" + d, 3, inv));
        check<DftR<F, 4>>(rc::dft_r_cases<R>(f + "_dft_r4" + d, 4, inv));
    }
}
template <int K>
static void shifts() {
    if constexpr (K < 96) {
        check<MulPow2<K>>(rc::mul_pow2_cases("gl_mul_pow2_" + std::to_string(K), K));
        shifts<K + 1>();
    }
}

int main() {
    rc::check_constants();
    printf("gl_edges=%zu\nbb_edges=%zu\n", rc::Gl::edges().size(), rc::Bb::edges().size());
    shifts<0>();
    dfts<rc::Gl, u64, false>("gl");
    dfts<rc::Gl, u64, true>("gl");
    outer_dfts<rc::Gl, GlF>("gl");
    dfts<rc::Bb, u32, false>("bb");
    dfts<rc::Bb, u32, true>("bb");
    outer_dfts<rc::Bb, BbF>("bb");
    printf("total mismatches=%zu\n", total_bad);
    return total_bad ? 1 : 0;
}

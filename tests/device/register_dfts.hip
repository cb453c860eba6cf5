// The register DFTs of csrc/dft_gl.hpp and csrc/dft_bb.hpp (mul_pow2, dft16, dft32, dft_small, layer64) and csrc/ntt_outer.hpp's dft_r on
// the GPU - the code gfx950 executes, with the instruction-level branches of gl_field.hpp / bb_field.hpp that the host shim never
// compiles - on the cases of tests/host_shim/register_dft_cases.hpp: one thread per case, one launch per function and direction, one
// hipDeviceSynchronize, comparison on the host.  Prints "gl_edges=N", "bb_edges=N" and one line "name cases=N mismatches=M (...)" per
// function; exit status 1 on a mismatch, 2 on a HIP error, 3 when the case generator fails its own checks.
// Built and run by tests/test_device_register_dfts.py; tests/host_shim/register_dfts.cpp runs the same cases on the CPU.
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>

#include "dft_bb.hpp"
#include "dft_gl.hpp"
#include "ntt_outer.hpp"
#include "../host_shim/register_dft_cases.hpp"

namespace rc = register_dft_cases;
using gbk::BbF;
using gbk::GlF;
typedef unsigned long long u64;
typedef unsigned int u32;

// the functions under test on a case's words x[0 .. W)
template <class T, bool INV>
struct Dft16 {
    static __device__ void run(T* x, T) { gbk::dft16<INV>(*reinterpret_cast<T(*)[16]>(x)); }
};
template <class T, bool INV>
struct Dft32 {
    static __device__ void run(T* x, T) { gbk::dft32<INV>(*reinterpret_cast<T(*)[32]>(x)); }
};
template <class T, bool INV, int K>
struct DftSmall {
    static __device__ void run(T* x, T) {
        T y[16] = {};
        for (int i = 0; i < (1 << K); i++) y[i] = x[i];
        gbk::dft_small<INV, K>(y);
        for (int i = 0; i < (1 << K); i++) x[i] = y[i];
    }
};
template <class T, bool INV, int H, int O>
struct Layer64 {
    static __device__ void run(T* x, T) {
        T y[64] = {};
        for (int i = 0; i < 2 * H; i++) y[O + i] = x[i];
        gbk::layer64<INV, H, O>(y);
        for (int i = 0; i < 2 * H; i++) x[i] = y[O + i];
    }
};
template <class F, int K>
struct DftR {
    typedef typename F::T T;
    static __device__ void run(T* x, T wr) { gbk::outer::dft_r<F, (u32)K>(*reinterpret_cast<T(*)[1u << K]>(x), wr); }
};
template <int K>
struct MulPow2 {
    static __device__ void run(u64* x, u64) { x[0] = gbk::mul_pow2<K>(x[0]); }
};

// case i's W words, in place
template <class Fn, class T, int W>
__global__ __launch_bounds__(256) void k_run(T* data, u32 n, T wr) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T x[W];
#pragma unroll
    for (int s = 0; s < W; s++) x[s] = data[(size_t)i * W + s];
    Fn::run(x, wr);
#pragma unroll
    for (int s = 0; s < W; s++) data[(size_t)i * W + s] = x[s];
}

static int hip_failed = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        hipError_t e_ = (x);                                              \
        if (e_ != hipSuccess) {                                           \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                \
            hip_failed = 1;                                               \
        }                                                                 \
    } while (0)

static std::vector<std::function<size_t()>> pending;   // copy back, compare, report: after the one synchronisation

template <class Fn, int W, class R>
static void check(rc::Cases<R> c) {
    typedef typename R::W T;
    if (hip_failed) return;
    if (c.width != W) rc::generator_failed(c.name + ": width");
    auto cs = std::make_shared<rc::Cases<R>>(std::move(c));
    std::vector<u64>().swap(cs->canonical);
    const size_t words = cs->in.size(), n = cs->count();
    T* d = nullptr;
    CHECK(hipMalloc(&d, words * sizeof(T)));
    if (hip_failed) return;
    CHECK(hipMemcpy(d, cs->in.data(), words * sizeof(T), hipMemcpyHostToDevice));
    if (hip_failed) return;
    hipLaunchKernelGGL((k_run<Fn, T, W>), dim3((u32)((n + 255) / 256)), dim3(256), 0, 0, d, (u32)n, cs->wr);
    CHECK(hipGetLastError());
    pending.push_back([cs, d, words]() -> size_t {
        std::vector<T> out(words);
        CHECK(hipMemcpy(out.data(), d, words * sizeof(T), hipMemcpyDeviceToHost));
        CHECK(hipFree(d));
        return hip_failed ? 0 : rc::report(*cs, out);
    });
}

template <class R, class T, bool INV>
static void dfts(const std::string& f) {
    const std::string d = INV ? "_inv" : "_fwd";
    check<Dft16<T, INV>, 16>(rc::dft_cases<R>(f + "_dft16" + d, 4, INV));
    check<Dft32<T, INV>, 32>(rc::dft_cases<R>(f + "_dft32" + d, 5, INV));
    check<DftSmall<T, INV, 1>, 2>(rc::dft_cases<R>(f + "_dft_small1" + d, 1, INV));
    check<DftSmall<T, INV, 2>, 4>(rc::dft_cases<R>(f + "_dft_small2" + d, 2, INV));
    check<DftSmall<T, INV, 3>, 8>(rc::dft_cases<R>(f + "_dft_small3" + d, 3, INV));
    // every (H, O) that ntt_passes.hpp's k_intt16_p2w and the two dft32 instantiate
    check<Layer64<T, INV, 32, 0>, 64>(rc::layer_cases<R>(f + "_layer64_h32_o0" + d, 5, INV));
    check<Layer64<T, INV, 16, 0>, 32>(rc::layer_cases<R>(f + "_layer64_h16_o0" + d, 4, INV));
    check<Layer64<T, INV, 16, 32>, 32>(rc::layer_cases<R>(f + "_layer64_h16_o32" + d, 4, INV));
}
template <class R, class F, bool INV>
static void outer_dfts(const std::string& f) {
    const std::string d = INV ? "_inv" : "_fwd";
    check<DftR<F, 1>, 2>(rc::dft_r_cases<R>(f + "_dft_r1" + d, 1, INV));
    check<DftR<F, 2>, 4>(rc::dft_r_cases<R>(f + "_dft_r2" + d, 2, INV));
    check<DftR<F, 3>, 8>(rc::dft_r_cases<R>(f + "_dft_r3" + d, 3, INV));
    check<DftR<F, 4>, 16>(rc::dft_r_cases<R>(f + "_dft_r4" + d, 4, INV));
}
template <int K>
static void shifts() {
    if constexpr (K < 96) {
        check<MulPow2<K>, 1>(rc::mul_pow2_cases("gl_mul_pow2_" + std::to_string(K), K));
        shifts<K + 1>();
    }
}

int main() {
    rc::check_constants();
    printf("gl_edges=%zu\nbb_edges=%zu\n", rc::Gl::edges().size(), rc::Bb::edges().size());
    shifts<0>();
    dfts<rc::Gl, u64, false>("gl");
    dfts<rc::Gl, u64, true>("gl");
    outer_dfts<rc::Gl, GlF, false>("gl");
    outer_dfts<rc::Gl, GlF, true>("gl");
    dfts<rc::Bb, u32, false>("bb");
    dfts<rc::Bb, u32, true>("bb");
    outer_dfts<rc::Bb, BbF, false>("bb");
    outer_dfts<rc::Bb, BbF, true>("bb");
    if (!hip_failed) CHECK(hipDeviceSynchronize());
    size_t total_bad = 0;
    for (auto& p : pending) {
        if (hip_failed) break;
        total_bad += p();
    }
    if (hip_failed) {
        fflush(stdout);
        return 2;
    }
    printf("total mismatches=%zu\n", total_bad);
    return total_bad ? 1 : 0;
}

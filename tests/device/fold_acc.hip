// csrc/fold_acc.hpp's FoldAcc<GlF> / FoldAcc<BbF> - the unreduced alpha-fold sums of the gate kernels - and gl::fold160 on the GPU: the
// code gfx950 executes, with the instruction-level branches of gl_field.hpp that the host shim never compiles, on the chains of
// tests/host_shim/fold_acc_cases.hpp.  One thread per chain (`FoldAcc<F> s; for t < len: s.acc(c[t], a[t]); out = s.finish()`), one
// launch per field and one for fold160, one hipDeviceSynchronize, comparison on the host.  Prints the census lines, then per family
// "name cases=N mismatches=M (...)"; exit status 1 on a mismatch, 2 on a HIP error, 3 when the case generator fails its own checks,
// 4 when a census class is empty.  Built from the headers alone (no kernels_gates.hip) and run by tests/test_device_fold_acc.py;
// tests/host_shim/fold_acc.cpp runs the same chains on the CPU.
#include <hip/hip_runtime.h>

#include "fold_acc.hpp"
#include "../host_shim/fold_acc_cases.hpp"

namespace fc = fold_acc_cases;
using gbk::BbF;
using gbk::GlF;
typedef unsigned long long u64;
typedef unsigned int u32;

// chain i: terms [off[i], off[i + 1]) of c / a (off has n + 1 entries)
template <class F>
__global__ __launch_bounds__(256) void k_chains(const u32* __restrict__ off, const typename F::T* __restrict__ c,
                                                const typename F::T* __restrict__ a, typename F::T* __restrict__ out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gbk::FoldAcc<F> s;
    for (u32 t = off[i], end = off[i + 1]; t < end; t++) s.acc(c[t], a[t]);
    out[i] = s.finish();
}
// case i: limbs[5 i .. 5 i + 5), low limb first
__global__ __launch_bounds__(256) void k_fold160(const u32* __restrict__ limbs, u64* __restrict__ out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32* l = limbs + (size_t)i * 5;
    out[i] = gl::canon(gl::fold160(l[0], l[1], l[2], l[3], l[4]));
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

template <class T>
static T* up(const std::vector<T>& v) {
    T* d = nullptr;
    if (hip_failed) return d;
    CHECK(hipMalloc(&d, v.size() * sizeof(T) + 16));
    if (!hip_failed) CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T>
static std::vector<T> down(T* d, size_t n) {
    std::vector<T> v(n);
    if (!hip_failed) CHECK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

template <class F, class C>
static typename F::T* launch(const C& ch) {
    typedef typename F::T T;
    if (ch.off.size() != ch.count() + 1 || ch.off.back() != ch.c.size() || ch.c.size() != ch.a.size()) fc::generator_failed("chain offsets");
    const u32* off = up(ch.off);
    const T* c = up(ch.c);
    const T* a = up(ch.a);
    T* out = up(std::vector<T>(ch.count()));
    if (hip_failed) return nullptr;
    hipLaunchKernelGGL((k_chains<F>), dim3((u32)((ch.count() + 255) / 256)), dim3(256), 0, 0, off, c, a, out, (u32)ch.count());
    CHECK(hipGetLastError());
    return out;
}

int main() {
    const fc::Chains<fc::GlAcc> gl = fc::gl_chains();
    const fc::Chains<fc::BbAcc> bb = fc::bb_chains();
    const fc::Fold160Cases f160 = fc::fold160_cases(gl);
    bool census = fc::print_census("gl_fold_acc", gl.census);
    census = fc::print_census("bb_fold_acc", bb.census) && census;
    census = fc::print_census("gl_fold160", f160.census) && census;
    u64* gl_out = launch<GlF>(gl);
    u32* bb_out = launch<BbF>(bb);
    std::vector<u32> limbs;
    for (const fc::U160& s : f160.in) limbs.insert(limbs.end(), s.l, s.l + 5);
    const u32* limbs_dev = up(limbs);
    u64* f160_out = up(std::vector<u64>(f160.count()));
    if (!hip_failed) {
        hipLaunchKernelGGL(k_fold160, dim3((u32)((f160.count() + 255) / 256)), dim3(256), 0, 0, limbs_dev, f160_out, (u32)f160.count());
        CHECK(hipGetLastError());
    }
    if (!hip_failed) CHECK(hipDeviceSynchronize());
    const std::vector<u64> gl_got = down(gl_out, gl.count());
    const std::vector<u32> bb_got = down(bb_out, bb.count());
    const std::vector<u64> f160_got = down(f160_out, f160.count());
    if (hip_failed) {
        fflush(stdout);
        return 2;
    }
    const size_t bad = fc::report(gl, gl_got) + fc::report(bb, bb_got) + fc::report(f160, f160_got);
    printf("total mismatches=%zu\n", bad);
    return bad ? 1 : census ? 0 : 4;
}

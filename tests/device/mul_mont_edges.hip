// gl::mul_mont_lazy / gl::mul_mont on the GPU (the device overloads of csrc/gl_field.hpp: inline-asm carry chains with their flags
// in scalar pairs) against the host overloads and against mont_fold(mul_limbs(a, b)), word for word, both FIVE forms, on the pairs
// of tests/host_shim/mul_mont_cases.hpp plus seeded random pairs.  Built and run by tests/test_mul_mont_forms.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <vector>

#include "gl_field.hpp"
#include "../host_shim/mul_mont_cases.hpp"

typedef unsigned long long u64;
typedef unsigned int u32;

__global__ void k_products(const u64* __restrict__ a, const u64* __restrict__ b, u64* __restrict__ out4, u64* __restrict__ out5,
                           u64* __restrict__ old4, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out4[i] = gl::mul_mont_lazy<false>(a[i], b[i]);
    out5[i] = gl::mul_mont_lazy<true>(a[i], b[i]);
    u32 r0, r1, hl, hh;
    gl::mul_limbs<false>(a[i], b[i], r0, r1, hl, hh);
    old4[i] = gl::mont_fold(r0, r1, hl, hh);
}

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                             \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

int main() {
    const std::vector<u64> edge = mul_mont_cases::edge_values();
    std::mt19937_64 rng(20261016);
    std::vector<u64> a, b;
    for (u64 x : edge)
        for (u64 y : edge) { a.push_back(x); b.push_back(y); }
    for (auto& pr : mul_mont_cases::no_borrow_pairs(rng)) {
        a.push_back(pr.first); b.push_back(pr.second);
        a.push_back(pr.second); b.push_back(pr.first);
    }
    for (int t = 0; t < (1 << 16); t++) {
        u64 x = rng(), y = rng();
        if (t % 4 == 1) { x %= gl::P; y %= gl::P; }
        if (t % 16 == 2) x = edge[(size_t)(rng() % edge.size())];
        a.push_back(x); b.push_back(y);
    }
    const u32 n = (u32)a.size();
    const size_t bytes = (size_t)n * sizeof(u64);
    u64 *da, *db, *d4, *d5, *dold;
    CHECK(hipMalloc(&da, bytes)); CHECK(hipMalloc(&db, bytes)); CHECK(hipMalloc(&d4, bytes)); CHECK(hipMalloc(&d5, bytes)); CHECK(hipMalloc(&dold, bytes));
    CHECK(hipMemcpy(da, a.data(), bytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(db, b.data(), bytes, hipMemcpyHostToDevice));
    k_products<<<(n + 255) / 256, 256>>>(da, db, d4, d5, dold, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<u64> g4(n), g5(n), gold(n);
    CHECK(hipMemcpy(g4.data(), d4, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(g5.data(), d5, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(gold.data(), dold, bytes, hipMemcpyDeviceToHost));
    long bad = 0, by0 = 0, by0_nonzero_low = 0;
    for (u32 i = 0; i < n; i++) {
        u32 r0, r1, hl, hh;
        gl::mul_limbs<false>(a[i], b[i], r0, r1, hl, hh);
        const u64 want = gl::mont_fold(r0, r1, hl, hh);
        const u64 h4 = gl::mul_mont_lazy<false>(a[i], b[i]), h5 = gl::mul_mont_lazy<true>(a[i], b[i]);
        if (g4[i] != want || g5[i] != want || gold[i] != want || h4 != want || h5 != want) {
            if (++bad < 5)
                printf("mismatch: a=%016llx b=%016llx device %016llx / %016llx / old %016llx, host %016llx / %016llx / old %016llx\n", a[i], b[i],
                       g4[i], g5[i], gold[i], h4, h5, want);
        }
        if (mul_mont_cases::no_borrow(a[i], b[i])) {
            by0++;
            if (a[i] * b[i] != 0) by0_nonzero_low++;
        }
    }
    printf("pairs=%u by0=%ld by0_nonzero_low=%ld mismatches=%ld\n", n, by0, by0_nonzero_low, bad);
    hipFree(da); hipFree(db); hipFree(d4); hipFree(d5); hipFree(dold);
    return bad != 0;
}

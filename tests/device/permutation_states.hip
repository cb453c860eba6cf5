// The six permutation forms of csrc/poseidon_gl_grouped.hpp, poseidon_gl_coop.hpp, poseidon2_bb.hpp and poseidon2_bb_coop.hpp on the
// GPU, one kernel per form, on caller-supplied canonical states (tests/test_device_permutation_states.py: states pulled back from
// chosen round words, tests/permutation_states.py).  Nothing is compared here: the outputs go to a file and the test compares them
// with the oracle.
//   input file:  u64 header {field (0 Goldilocks, 1 BabyBear), count, zero_capacity (0 / 1)}, then count states - 12 u64 or 16 u32 each
//   output file: three forms, count states each, the input's word type
//     Goldilocks: permute_mont_mfma_grouped(capacity_only = false); the same with capacity_only = true (words 8..11 are produced, words
//                 0..7 are written as 0); poseidon_gl_coop::permute with gl::canon.  zero_capacity = 1 (every state's words 8..11 are
//                 0) passes the flag to the two grouped forms.
//     BabyBear:   poseidon2_bb::permute; permute_scaled + canonical_out; poseidon2_bb_coop::permute.
// MFMA, DPP and the barriers of the cooperative forms are wave- or block-wide: lanes past the end work on a clamped index and skip the
// store, none returns early.  Exit status 2 on a HIP or file error.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "poseidon_gl_grouped.hpp"
#include "poseidon_gl_coop.hpp"
#include "poseidon2_bb.hpp"
#include "poseidon2_bb_coop.hpp"

typedef unsigned long long u64;
typedef unsigned int u32;

__global__ __launch_bounds__(256, 4) void k_gl_grouped(const u64* __restrict__ in, u64* __restrict__ out, u64 count, int capacity_only, int zero_capacity) {
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i0 < count;
    const u64 i = live ? i0 : count - 1;
    const poseidon_gl::MdsOperand amat = poseidon_gl::mds_mfma_matrix();
    __shared__ poseidon_gl::v4i gops_lds[poseidon_gl::GROUP_LDS_V4];
    poseidon_gl::group_ops_init(gops_lds);
    const poseidon_gl::v4i* gops = gops_lds + (threadIdx.x & 63);
    u64 s[12];
#pragma unroll
    for (int e = 0; e < 12; e++) s[e] = poseidon_gl::to_mont(in[12 * i + e]);
    poseidon_gl::permute_mont_mfma_grouped(s, amat, gops, capacity_only != 0, zero_capacity != 0);
    if (!live) return;
    if (capacity_only) {
#pragma unroll
        for (int e = 0; e < 8; e++) out[12 * i + e] = 0;
#pragma unroll
        for (int e = 8; e < 12; e++) out[12 * i + e] = poseidon_gl::from_mont(s[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 12; e++) out[12 * i + e] = poseidon_gl::from_mont(s[e]);
    }
}

__global__ __launch_bounds__(64) void k_gl_coop(const u64* __restrict__ in, u64* __restrict__ out, u64 count) {
    __shared__ u64 sh[64];
    const u32 l = threadIdx.x & 15, row = threadIdx.x >> 4;
    const u64 st = (u64)blockIdx.x * 4 + row;
    const bool valid = st < count;
    u64 x = l < 12 ? in[12 * (valid ? st : count - 1) + l] : 0;
    x = poseidon_gl_coop::permute(x, l, sh + 16 * row);
    if (valid && l < 12) out[12 * st + l] = gl::canon(x);
}

__global__ __launch_bounds__(256) void k_bb_permute(const u32* __restrict__ in, u32* __restrict__ out, u64 count, int scaled) {
    const u64 i0 = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i0 < count;
    const u64 i = live ? i0 : count - 1;
    u32 s[16];
#pragma unroll
    for (int e = 0; e < 16; e++) s[e] = bb::to_mont(in[16 * i + e]);
    if (scaled) {
        poseidon2_bb::permute_scaled(s);
#pragma unroll
        for (int e = 0; e < 16; e++) s[e] = poseidon2_bb::canonical_out(s[e]);
    } else {
        poseidon2_bb::permute(s);
#pragma unroll
        for (int e = 0; e < 16; e++) s[e] = bb::from_mont(s[e]);
    }
    if (!live) return;
#pragma unroll
    for (int e = 0; e < 16; e++) out[16 * i + e] = s[e];
}

__global__ __launch_bounds__(64) void k_bb_coop(const u32* __restrict__ in, u32* __restrict__ out, u64 count) {
    const u32 l = threadIdx.x & 15;
    const u64 st = (u64)blockIdx.x * 4 + (threadIdx.x >> 4);
    const bool valid = st < count;
    u32 x = bb::to_mont(in[16 * (valid ? st : count - 1) + l]);
    x = poseidon2_bb_coop::permute(x, l);
    if (valid) out[16 * st + l] = bb::from_mont(x);
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

template <class T, int W>
static int run(const std::vector<unsigned char>& file, u64 count, bool zero_capacity, const char* out_path) {
    const size_t words = (size_t)count * W, bytes = words * sizeof(T);
    if (file.size() != 24 + bytes) { printf("input: %zu bytes, expected %zu\n", file.size(), 24 + bytes); return 2; }
    T *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, bytes));
    CHECK(hipMalloc(&d_out, 3 * bytes));
    if (hip_failed) return 2;
    CHECK(hipMemcpy(d_in, file.data() + 24, bytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xA5, 3 * bytes));
    if (hip_failed) return 2;
    const u32 lane_blocks = (u32)((count + 255) / 256), coop_blocks = (u32)((count + 3) / 4);
    if constexpr (W == 12) {
        k_gl_grouped<<<lane_blocks, 256>>>((const u64*)d_in, (u64*)d_out, count, 0, zero_capacity);
        k_gl_grouped<<<lane_blocks, 256>>>((const u64*)d_in, (u64*)d_out + words, count, 1, zero_capacity);
        k_gl_coop<<<coop_blocks, 64>>>((const u64*)d_in, (u64*)d_out + 2 * words, count);
    } else {
        k_bb_permute<<<lane_blocks, 256>>>((const u32*)d_in, (u32*)d_out, count, 0);
        k_bb_permute<<<lane_blocks, 256>>>((const u32*)d_in, (u32*)d_out + words, count, 1);
        k_bb_coop<<<coop_blocks, 64>>>((const u32*)d_in, (u32*)d_out + 2 * words, count);
    }
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<T> h(3 * words);
    if (!hip_failed) CHECK(hipMemcpy(h.data(), d_out, 3 * bytes, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (hip_failed) return 2;
    FILE* f = fopen(out_path, "wb");
    if (!f || fwrite(h.data(), sizeof(T), h.size(), f) != h.size()) { printf("cannot write %s\n", out_path); return 2; }
    fclose(f);
    printf("states=%llu forms=3\n", count);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { printf("usage: permutation_states <in> <out>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<unsigned char> file;
    unsigned char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
    if (file.size() < 24) { printf("input: no header\n"); return 2; }
    const u64* head = reinterpret_cast<const u64*>(file.data());
    const u64 field = head[0], count = head[1], zero_capacity = head[2];
    if (field > 1 || count == 0 || count > (1u << 22) || zero_capacity > 1) { printf("input: bad header\n"); return 2; }
    return field == 0 ? run<u64, 12>(file, count, zero_capacity != 0, argv[2]) : run<u32, 16>(file, count, false, argv[2]);
}

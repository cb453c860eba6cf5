// k_expand_partition<F> (csrc/partition_expand.hpp) on the GPU, built from the header alone: out[col][row] = staged[slots[row][col]].
// Nothing is compared here: tests/test_device_partition_expand.py holds the numpy gather.
//   partition_expand <in> <out>
// in:  u64 words: field (0 Goldilocks, 1 BabyBear), num_cases, then per case: log_n, num_wires, K, slots [2^log_n * num_wires]
//      (one per word), staged [K] (one per word)
// out: per case [num_wires][2^log_n] elements of the field's width (u64 / u32), one launch per case
// Exit status 2 on a HIP error, 3 on a malformed file - a slot >= K included: nothing is read out of bounds.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "field_traits.hpp"
#include "partition_expand.hpp"

using namespace gbk;

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
    std::vector<T> all;
    size_t at = 2;
    for (u64 c = 0; c < in[1]; c++) {
        if (at + 3 > in.size()) return 3;
        const u32 log_n = (u32)in[at], nw = (u32)in[at + 1];
        const size_t K = (size_t)in[at + 2];
        at += 3;
        if (log_n < 2 || log_n > 20 || nw == 0 || nw > 1024 || K == 0) return 3;
        const size_t cells = ((size_t)1 << log_n) * nw;
        if (at + cells + K > in.size()) return 3;
        std::vector<uint32_t> slots(cells);
        std::vector<T> staged(K);
        for (size_t i = 0; i < cells; i++) {
            if (in[at + i] >= K) return 3;
            slots[i] = (uint32_t)in[at + i];
        }
        for (size_t k = 0; k < K; k++) staged[k] = (T)in[at + cells + k];
        at += cells + K;
        uint32_t* d_slots;
        T *d_staged, *d_out;
        HIP_OK(hipMalloc(&d_slots, cells * 4));
        HIP_OK(hipMalloc(&d_staged, K * sizeof(T)));
        HIP_OK(hipMalloc(&d_out, cells * sizeof(T)));
        HIP_OK(hipMemcpy(d_slots, slots.data(), cells * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_staged, staged.data(), K * sizeof(T), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xA5, cells * sizeof(T)));
        partition::launch_expand_partition<F>(d_slots, d_staged, d_out, log_n, nw, nullptr);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        all.resize(all.size() + cells);
        HIP_OK(hipMemcpy(all.data() + all.size() - cells, d_out, cells * sizeof(T), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_slots));
        HIP_OK(hipFree(d_staged));
        HIP_OK(hipFree(d_out));
    }
    if (at != in.size()) return 3;
    std::FILE* f = std::fopen(out_path, "wb");
    if (!f) return 3;
    const bool ok = std::fwrite(all.data(), sizeof(T), all.size(), f) == all.size();
    std::fclose(f);
    return ok ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<u64> in;
    u64 w;
    while (std::fread(&w, 8, 1, f) == 1) in.push_back(w);
    std::fclose(f);
    if (in.size() < 6) return 3;
    return in[0] == 0 ? run<GlF>(in, argv[2]) : in[0] == 1 ? run<BbF>(in, argv[2]) : 3;
}

// csrc/sigma_decode.hpp built for gfx950 from the header alone: sigma::decode_value in a kernel, one thread per value, over the
// same word file and the same host-made tables as tests/host_shim/sigma_decode.cpp (tests/host_shim/sigma_decode_case.hpp has the
// format and the loop over the cases).  No value is compared here: tests/test_gpu_sigma_decode.py holds the expected cells.
//   sigma_decode <in> <out>
// Exit status 3 on a malformed file, 4 on a HIP error.
#include <hip/hip_runtime.h>

#include "sigma_decode.hpp"
#include "../host_shim/sigma_decode_case.hpp"

using namespace gbk;

constexpr u32 BLOCK = 256;

template <class F>
__global__ __launch_bounds__(BLOCK) void k_decode(sigma::DlogTables<F> t, const typename F::T* __restrict__ k_pow_n,
                                                  const typename F::T* __restrict__ k_inv, u32 num_routed,
                                                  const typename F::T* __restrict__ values, u32 count, u32* __restrict__ cells) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    u32 col, row;
    if (!sigma::decode_value<F>(t, k_pow_n, k_inv, num_routed, values[i], &col, &row)) col = sigma::NO_CELL, row = 0;
    cells[2 * i] = col;
    cells[2 * i + 1] = row;
}

struct DeviceBlocks {   // freed when the case is done
    std::vector<void*> p;
    ~DeviceBlocks() { for (void* x : p) (void)hipFree(x); }
    template <class V>
    const V* up(const std::vector<V>& host) {
        void* d = nullptr;
        if (hipMalloc(&d, (host.size() ? host.size() : 1) * sizeof(V)) != hipSuccess) return nullptr;
        p.push_back(d);
        if (!host.empty() && hipMemcpy(d, host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return static_cast<const V*>(d);
    }
};

static bool g_hip_failed = false;

template <class F>
bool on_device(const sigma_case::Case<F>& c, std::vector<u32>* cells) {
    typedef typename F::T T;
    const u32 count = (u32)c.values.size();
    if (!count) return true;
    DeviceBlocks blocks;
    sigma::DlogTables<F> t = c.tables.view();
    t.sorted = blocks.up(c.tables.sorted);
    t.inv_lo = blocks.up(c.tables.inv_lo);
    t.exps = blocks.up(c.tables.exps);
    const T* k_pow_n = blocks.up(c.k_pow_n);
    const T* k_inv = blocks.up(c.k_inv);
    const T* values = blocks.up(c.values);
    u32* out = const_cast<u32*>(blocks.up(*cells));
    if (!t.sorted || !t.inv_lo || !t.exps || !k_pow_n || !k_inv || !values || !out) return !(g_hip_failed = true);
    hipLaunchKernelGGL((k_decode<F>), dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, t, k_pow_n, k_inv, (u32)c.k_pow_n.size(), values,
                       count, out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(cells->data(), out, cells->size() * sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess)
        return !(g_hip_failed = true);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!sigma_case::read_words(argv[1], &in) || in.size() < 2) return 3;
    const bool ok = in[0] == 0 ? sigma_case::run<GlF>(in, &out, on_device<GlF>) : sigma_case::run<BbF>(in, &out, on_device<BbF>);
    if (g_hip_failed) return 4;
    if (!ok) return 3;
    return sigma_case::write_words(argv[2], out) ? 0 : 3;
}

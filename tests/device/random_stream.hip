// csrc/random_stream.hpp built for gfx950 from the header alone: the block function, the two u128 -> field reductions and the
// element rule in a kernel, one thread per record, over the same word file as tests/host_shim/random_stream.cpp
// (tests/host_shim/random_stream_case.hpp has the format; a range record runs as one element record per element here).
// No value is compared here: tests/test_device_random_stream.py holds the expected words.
//   random_stream <in> <out>
// Exit status 3 on a malformed file, 4 on a HIP error.
#include <hip/hip_runtime.h>

#include "random_stream.hpp"
#include "../host_shim/random_stream_case.hpp"

constexpr unsigned BLOCK_THREADS = 256;

__global__ __launch_bounds__(BLOCK_THREADS) void k_records(const random_case::Record* __restrict__ recs, unsigned count, uint64_t* __restrict__ out) {
    const unsigned i = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= count) return;
    random_case::run_record(recs[i], out);
}

static bool g_hip_failed = false;

static bool on_device(const std::vector<random_case::Record>& recs, std::vector<uint64_t>* out) {
    if (recs.empty()) return true;
    random_case::Record* drecs = nullptr;
    uint64_t* dout = nullptr;
    const size_t rbytes = recs.size() * sizeof(random_case::Record), obytes = out->size() * sizeof(uint64_t);
    bool ok = hipMalloc(&drecs, rbytes) == hipSuccess && hipMalloc(&dout, obytes) == hipSuccess &&
              hipMemcpy(drecs, recs.data(), rbytes, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dout, out->data(), obytes, hipMemcpyHostToDevice) == hipSuccess;   // (the range_ok words are already there)
    if (ok) {
        hipLaunchKernelGGL(k_records, dim3((unsigned)((recs.size() + BLOCK_THREADS - 1) / BLOCK_THREADS)), dim3(BLOCK_THREADS), 0, 0, drecs,
                           (unsigned)recs.size(), dout);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out->data(), dout, obytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(drecs);
    (void)hipFree(dout);
    if (!ok) g_hip_failed = true;
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!random_case::read_words(argv[1], &in)) return 3;
    const bool ok = random_case::run(in, &out, on_device, true);
    if (g_hip_failed) return 4;
    if (!ok) return 3;
    return random_case::write_words(argv[2], out) ? 0 : 3;
}

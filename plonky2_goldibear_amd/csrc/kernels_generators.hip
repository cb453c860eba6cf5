// The generator kernels (generators.hpp) for the two fields: the device half of gb_generate_partition / gb_prove_inputs.
#include "kernels.hpp"
#include "generators.hpp"

namespace gbk {

template <class F>
void run_generators(const gen::DeviceSchedule& d, const gen::Launch* launches, size_t num_launches, const u32* level_off_host,
                    typename F::T* values, u32* err, hipStream_t stream) {
    gen::launch_generators<F>(d, launches, num_launches, level_off_host, values, err, stream);
}
template void run_generators<GlF>(const gen::DeviceSchedule&, const gen::Launch*, size_t, const u32*, u64*, u32*, hipStream_t);
template void run_generators<BbF>(const gen::DeviceSchedule&, const gen::Launch*, size_t, const u32*, u32*, u32*, hipStream_t);

template <class F>
void scatter_inputs(const u32* cls, const typename F::T* in, u32 count, typename F::T* values, hipStream_t stream) {
    if (!count) return;
    hipLaunchKernelGGL(gen::k_scatter_inputs<F>, dim3((count + gen::GROUP - 1) / gen::GROUP), dim3(gen::GROUP), 0, stream, cls, in, count, values);
}
template void scatter_inputs<GlF>(const u32*, const u64*, u32, u64*, hipStream_t);
template void scatter_inputs<BbF>(const u32*, const u32*, u32, u32*, hipStream_t);

template <class F>
void gather_public(const u32* pi_cls, u32 count, const typename F::T* values, const u32* err, u64* out, hipStream_t stream) {
    const u32 threads = count > gen::ERROR_WORDS ? count : gen::ERROR_WORDS;
    hipLaunchKernelGGL(gen::k_gather_public<F>, dim3((threads + gen::GROUP - 1) / gen::GROUP), dim3(gen::GROUP), 0, stream, pi_cls, count, values,
                       err, out);
}
template void gather_public<GlF>(const u32*, u32, const u64*, const u32*, u64*, hipStream_t);
template void gather_public<BbF>(const u32*, u32, const u32*, const u32*, u64*, hipStream_t);

}  // namespace gbk

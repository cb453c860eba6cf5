// k_expand_partition (partition_expand.hpp) for the two fields: the device half of gb_prove_partition / gb_expand_partition.
#include "kernels.hpp"
#include "partition_expand.hpp"

namespace gbk {

template <class F>
void expand_partition(const u32* slots, const typename F::T* staged, typename F::T* out, u32 log_n, u32 num_wires, hipStream_t stream) {
    partition::launch_expand_partition<F>(slots, staged, out, log_n, num_wires, stream);
}
template void expand_partition<GlF>(const u32*, const u64*, u64*, u32, u32, hipStream_t);
template void expand_partition<BbF>(const u32*, const u32*, u32*, u32, u32, hipStream_t);

}  // namespace gbk

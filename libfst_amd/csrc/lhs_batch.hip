// lhs_batch.hip -- the batch-of-general-lhs instances (kLhsBatch) of the two general kernels
// (kernels/eager_bfs.hpp, kernels/lazy_wave.hpp) and their launches.  One wavefront (or one
// 256-thread workgroup) takes one lhs of the batch at a time: it reads the item's 32-B
// descriptor, forms the GraphInput the single-lhs code takes (device_common.hpp lhs_item) and
// runs that code unchanged.  DeviceEngine::run_lhs_batch (device_engine.hip) drives the tiers.
// Also the two kernels that prepare a device-resident batch for it (kernels/lhs_prepare.hpp).
#include <algorithm>

#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/eager_bfs.hpp"
#include "kernels/lazy_wave.hpp"
#include "kernels/lhs_prepare.hpp"

namespace fstamd {

namespace {
const void* lhs_eager_kernel(int tier) {
  switch (tier) {
    case kLhsTierTiny128: return (const void*)eager_bfs_kernel<64, kLhsBatch, 1>;
    case kLhsTierTiny256: return (const void*)eager_bfs_kernel<64, kLhsBatch, 2>;
    case kLhsTierWave: return (const void*)eager_bfs_kernel<64, kLhsBatch>;
    default: return (const void*)eager_bfs_kernel<kLhsWG, kLhsBatch>;
  }
}
}  // namespace

int lhs_eager_per_cu(int tier) {
  int occ = 0;
  const int wg = tier == kLhsTierWG ? kLhsWG : 64;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, lhs_eager_kernel(tier), wg, 0) !=
      hipSuccess)
    occ = 1;
  return std::max(occ, 1);
}

hipError_t launch_lhs_eager(int tier, const RhsView& rhs, const ChainInput& in,
                            const GraphInput& lhs, uint32_t n_best, unsigned int* next_item,
                            const uint32_t* items, const uint32_t* num_items_dev,
                            const BfsWs& ws, const BatchOutDev& out, uint32_t grid,
                            hipStream_t stream) {
  uint32_t num_items_host = 0;
  void* args[] = {(void*)&rhs,   (void*)&in,           (void*)&lhs,
                  (void*)&n_best, (void*)&next_item,    (void*)&items,
                  (void*)&num_items_dev, (void*)&num_items_host, (void*)&ws, (void*)&out};
  return hipLaunchKernel(lhs_eager_kernel(tier), dim3(grid),
                         dim3(tier == kLhsTierWG ? kLhsWG : 64), args, 0, stream);
}

hipError_t launch_lhs_lazy(const RhsView& rhs, const ChainInput& in, const GraphInput& lhs,
                           uint32_t n_best, unsigned int* next_item, const uint32_t* items,
                           uint32_t num_items, const LazyWs& ws, const BatchOutDev& out,
                           uint32_t grid, hipStream_t stream) {
  lazy_wave_kernel<kLhsBatch><<<grid, 64, 0, stream>>>(rhs, in, lhs, n_best, next_item, items,
                                                       num_items, ws, out);
  return hipGetLastError();
}

// The device-resident entry's preparation (kernels/lhs_prepare.hpp).
hipError_t launch_lhs_prepare(const LhsPrepIn& in, const LhsPrepOut& out, uint32_t grid,
                              hipStream_t stream) {
  lhs_prepare_kernel<<<grid, 64, 0, stream>>>(in, out);
  return hipGetLastError();
}

hipError_t launch_lhs_lists(const LhsDesc* desc, uint32_t num, uint32_t* list_nonneg,
                            uint32_t* list_replay, uint32_t* totals, hipStream_t stream) {
  lhs_lists_kernel<<<1, kLhsListsWG, 0, stream>>>(desc, num, list_nonneg, list_replay, totals);
  return hipGetLastError();
}

}  // namespace fstamd

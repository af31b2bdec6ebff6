// text_pull.hip -- the streamed text batch's instances of the two pull kernels (TEXT = true:
// byte inputs, the text emission after every batched chase; kernels/eager_pull.hpp,
// kernels/lazy_pull.hpp) and their launches.  The variant is picked exactly as for labels
// (pull_kernel_dispatch.hpp).
#include <algorithm>

#include "pull_kernel_dispatch.hpp"

namespace fstamd {

int text_pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len, bool lazy) {
  int occ = 0;
  const void* k = lazy ? lazy_pull_kernel_for<true>(rhs, max_len) : pull_kernel_for<true>(rhs, max_len);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, 64, 0) != hipSuccess) occ = 1;
  return std::max(occ, 1);
}

hipError_t launch_eager_pull_text(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                  unsigned int* next_item, const EagerLaunch& lp,
                                  const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  void* args[] = {(void*)&rhs.view, (void*)&rhs.rev, (void*)&in, (void*)&n_best,
                  (void*)&next_item, (void*)&lp, (void*)&out};
  return hipLaunchKernel(pull_kernel_for<true>(rhs, in.max_len, true), dim3(grid), dim3(64), args, 0,
                         stream);
}

hipError_t launch_lazy_pull_text(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                 unsigned int* next_item, const EagerLaunch& lp,
                                 const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  void* args[] = {(void*)&rhs.view, (void*)&rhs.rev, (void*)&in, (void*)&n_best,
                  (void*)&next_item, (void*)&lp, (void*)&out};
  return hipLaunchKernel(lazy_pull_kernel_for<true>(rhs, in.max_len, true), dim3(grid), dim3(64), args,
                         0, stream);
}

}  // namespace fstamd

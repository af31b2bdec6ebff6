// code_pull.hip -- tier P's weight-code instances (CODES = true, kernels/eager_pull.hpp) for
// the streamed label batch: the chase stores each arc's weight as the byte the record already
// holds, the copy-out sends one byte per arc to the host instead of an f64, and the host
// expands the bytes with a 256-entry table (batch_streamed.cpp).  The variant is picked
// exactly as for the f64 copy-out (pull_kernel_dispatch.hpp: pull_rk and pull_pack are the
// single decision); records with wider weights (RK 0 and 1), lazy semantics and the text
// batch have no code instance and keep the f64 copy-out.
#include <algorithm>

#include "pull_kernel_dispatch.hpp"

namespace fstamd {

namespace {
// the code instance for this launch, or null when the records' weights are wider than a byte
// (log: the launch's route lines, the same as the f64 instances')
const void* pull_codes_kernel_for(const DeviceFst& rhs, uint32_t max_len, bool log = false) {
  const int rk = pull_rk(rhs, max_len);
  if (rk < 2) return nullptr;
  route_rk("eager", rk, rhs.rev, log);
  if (rk == 3) {
    const bool pack = pull_pack(rhs, max_len);
    if (log && std::getenv("FSTAMD_ROUTE_LOG"))
      std::fprintf(stderr, "[libfst_amd route] eager pull: packed cells %s\n", pack ? "on" : "off");
    if (pack) return pull_kernel_for<6, false, true>(rhs.rev);
  }
  switch (rk) {
    case 5: return pull_kernel_for<5, false, true>(rhs.rev);
    case 4: return pull_kernel_for<4, false, true>(rhs.rev);
    case 3: return pull_kernel_for<3, false, true>(rhs.rev);
    default: return pull_kernel_for<2, false, true>(rhs.rev);
  }
}
}  // namespace

bool pull_codes_table(const DeviceFst& rhs, int semantics, uint32_t max_len, double* table) {
  if (semantics != 1 || !rhs.pull_ok || !pull_codes_kernel_for(rhs, max_len)) return false;
  const int rk = pull_rk(rhs, max_len);
  if (rk >= 4) {  // the rhs's distinct weights, as uploaded (rv_weight_table)
    if (rhs.wtab_host.size() != kPullWtMax) return false;
    std::copy(rhs.wtab_host.begin(), rhs.wtab_host.end(), table);
  } else {  // the integer kinds: what the f64 chase computes, (double)c * winv
    for (uint32_t c = 0; c < 256; ++c) table[c] = (double)c * rhs.rev.winv;
  }
  return true;
}

int code_pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len) {
  int occ = 0;
  const void* k = pull_codes_kernel_for(rhs, max_len);
  if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, 64, 0) != hipSuccess) occ = 1;
  return std::max(occ, 1);
}

hipError_t launch_eager_pull_codes(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                   unsigned int* next_item, const EagerLaunch& lp,
                                   const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  const void* k = pull_codes_kernel_for(rhs, in.max_len, true);
  if (!k) return hipErrorInvalidValue;
  void* args[] = {(void*)&rhs.view, (void*)&rhs.rev, (void*)&in, (void*)&n_best,
                  (void*)&next_item, (void*)&lp, (void*)&out};
  return hipLaunchKernel(k, dim3(grid), dim3(64), args, 0, stream);
}

}  // namespace fstamd

// lattice_posterior.hip -- the launches of the lattice posteriors (kernels/lattice_posterior.hpp):
// forward and backward log-semiring sums and the -log posterior of every arc of every item of an
// lhs batch, for fst_posterior_lhs_batch and fst_device_posterior_lhs.
// DeviceEngine::run_posterior_batch (device_engine.hip) drives them.
#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/lattice_posterior.hpp"

namespace fstamd {

hipError_t launch_posterior_lds(const LatPostDev& p, uint32_t count, uint32_t grid,
                                hipStream_t stream) {
  lattice_posterior_lds_kernel<<<grid, 64, p.nb.lds_budget, stream>>>(p, count);
  return hipGetLastError();
}

hipError_t launch_posterior_hbm(const LatPostDev& p, uint32_t grid, hipStream_t stream) {
  lattice_posterior_hbm_kernel<<<grid, kNbWG, 0, stream>>>(p);
  return hipGetLastError();
}

}  // namespace fstamd

// lattice_prune.hip -- the launches of the lattice prune (kernels/lattice_prune.hpp): the beam
// cut of every item of an lhs batch, for fst_prune_lhs_batch and fst_device_prune_lhs.
// DeviceEngine::run_prune_batch (device_engine.hip) drives them; the trim ladder
// (lattice_trim.hip) then runs on the shadow view they leave.
#include <algorithm>

#include "device_engine.hpp"
#include "kernels/lattice_prune.hpp"

namespace fstamd {

hipError_t launch_prune_wave(const LatPruneDev& p, uint32_t num, uint32_t grid,
                             hipStream_t stream) {
  lattice_prune_wave_kernel<<<grid, 64, 0, stream>>>(p, num);
  return hipGetLastError();
}

hipError_t launch_prune_frontier(const LatPruneDev& p, uint32_t grid, hipStream_t stream) {
  lattice_prune_frontier_kernel<<<grid, kPruneWG, 0, stream>>>(p);
  return hipGetLastError();
}

}  // namespace fstamd

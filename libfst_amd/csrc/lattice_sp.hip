// lattice_sp.hip -- the launches of the lattice shortest path (kernels/lattice_sp.hpp):
// fst_shortest_path of every item of an lhs batch, for fst_shortest_path_lhs_batch and
// fst_device_shortest_path_lhs.  DeviceEngine::run_sp_batch (device_engine.hip) drives them.
#include <algorithm>

#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/lattice_sp.hpp"

namespace fstamd {

hipError_t launch_sp_wave(const LatSpDev& p, const uint32_t* items, uint32_t count,
                          const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  lattice_sp_wave_kernel<<<grid, 64, 0, stream>>>(p, items, count, out);
  return hipGetLastError();
}

hipError_t launch_sp_frontier(const LatSpDev& p, const BatchOutDev& out, uint32_t grid,
                              hipStream_t stream) {
  lattice_sp_frontier_kernel<<<grid, kSpWG, 0, stream>>>(p, out);
  return hipGetLastError();
}

hipError_t launch_sp_replay(const LatSpDev& p, const uint32_t* items, uint32_t count,
                            const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  lattice_sp_replay_kernel<<<grid, 64, 0, stream>>>(p, items, count, out);
  return hipGetLastError();
}

}  // namespace fstamd

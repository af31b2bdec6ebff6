// lattice_nbest.hip -- the launches of the lattice n-best (kernels/lattice_nbest.hpp): the n best
// distinct paths of every item of an lhs batch, for fst_nbest_lhs_batch and
// fst_device_nbest_lhs, and with `unique` the n best paths of distinct output texts, for
// fst_nbest_unique_lhs_batch and fst_device_nbest_unique_lhs.  DeviceEngine::run_nbest_batch
// (device_engine.hip) drives them.
#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/lattice_nbest.hpp"

namespace fstamd {

hipError_t launch_nbest_lds(const LatNbestDev& p, bool unique, uint32_t count,
                            const BatchOutDev& out, uint32_t grid, hipStream_t stream) {
  if (unique) lattice_nbest_unique_lds_kernel<<<grid, 64, p.lds_budget, stream>>>(p, count, out);
  else lattice_nbest_lds_kernel<<<grid, 64, p.lds_budget, stream>>>(p, count, out);
  return hipGetLastError();
}

hipError_t launch_nbest_hbm(const LatNbestDev& p, bool unique, const BatchOutDev& out,
                            uint32_t grid, hipStream_t stream) {
  if (unique) lattice_nbest_unique_hbm_kernel<<<grid, kNbWG, 0, stream>>>(p, out);
  else lattice_nbest_hbm_kernel<<<grid, kNbWG, 0, stream>>>(p, out);
  return hipGetLastError();
}

}  // namespace fstamd

// lattice_trim.hip -- the launches of the lattice trim (kernels/lattice_trim.hpp): connect of
// every item of a lattice arena, for FST_LATTICE_CONNECT on the three lattice entries and for
// fst_connect_lhs_batch.  host::trim_lattices (batch_lhs.cpp) drives them.
#include <algorithm>

#include "device_engine.hpp"
#include "kernels/lattice_trim.hpp"

namespace fstamd {

hipError_t launch_trim_stage(const LhsDesc* desc, uint32_t num, LatItem* item, int32_t* status,
                             uint32_t* start, hipStream_t stream) {
  lattice_trim_stage_kernel<<<(num + 255) / 256, 256, 0, stream>>>(desc, num, item, status,
                                                                   start);
  return hipGetLastError();
}

hipError_t launch_trim_access(const LatticeOutDev& arena, const LatTrimDev& t,
                              const int32_t* status, uint32_t num, uint32_t grid,
                              hipStream_t stream) {
  lattice_trim_access_kernel<<<grid, kTrimWG, 0, stream>>>(arena, t, status, num);
  return hipGetLastError();
}

hipError_t launch_trim_sweep(const LatticeOutDev& arena, const LatTrimDev& t,
                             const int32_t* status, uint32_t num, uint32_t grid,
                             hipStream_t stream) {
  lattice_trim_sweep_kernel<<<grid, 64, 0, stream>>>(arena, t, status, num);
  return hipGetLastError();
}

hipError_t launch_trim_linear(const LatticeOutDev& arena, const LatTrimDev& t,
                              const int32_t* status, uint32_t grid, hipStream_t stream) {
  lattice_trim_linear_kernel<<<grid, kTrimWG, 0, stream>>>(arena, t, status);
  return hipGetLastError();
}

hipError_t launch_trim_finalize(const LatticeOutDev& arena, const LatTrimDev& t,
                                const int32_t* status, uint32_t num, uint32_t grid,
                                hipStream_t stream) {
  lattice_trim_finalize_kernel<<<grid, 64, 0, stream>>>(arena, t, status, num);
  return hipGetLastError();
}

hipError_t launch_trim_gather(const LatticeOutDev& arena, const LatTrimDev& t,
                              const uint64_t* arc_base, const LatticeCsrDev& csr, uint32_t num,
                              uint32_t grid, hipStream_t stream) {
  lattice_trim_gather_kernel<<<grid, 64, 0, stream>>>(arena, t, arc_base, csr, num);
  return hipGetLastError();
}

}  // namespace fstamd

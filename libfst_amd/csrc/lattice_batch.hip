// lattice_batch.hip -- the lattice batch (fst_compose_frozen_batch and its lhs and device
// forms): the emitting instances of eager_bfs_kernel (kernels/eager_bfs.hpp, kEmit: chain and
// kLhsBatch lhs at the four tier shapes of run_bfs_ladder), their launches, and
// the compaction of the arena into FstLhsBatch's layout in item order, the lattice twin of
// compact_paths.  DeviceEngine::run_lattice_batch / compact_lattices (device_engine.hip) drive
// them.
#include <algorithm>

#define FSTAMD_BFS_TEMPLATES_ONLY  // device_engine.hip holds the non-template kernels
#include "device_engine.hpp"
#include "kernels/eager_bfs.hpp"

namespace fstamd {

namespace {
template <int kGraph>
const void* lattice_kernel_of(int tier) {
  switch (tier) {
    case kLhsTierTiny128: return (const void*)eager_bfs_kernel<64, kGraph, 1, true>;
    case kLhsTierTiny256: return (const void*)eager_bfs_kernel<64, kGraph, 2, true>;
    case kLhsTierWave: return (const void*)eager_bfs_kernel<64, kGraph, 0, true>;
    default: return (const void*)eager_bfs_kernel<kLhsWG, kGraph, 0, true>;
  }
}
const void* lattice_kernel(int tier, bool chain) {
  return chain ? lattice_kernel_of<kLhsChain>(tier) : lattice_kernel_of<kLhsBatch>(tier);
}
}  // namespace

// Per item: the status the result reports and what the item owns (an item that is not OK owns
// nothing).  Entry `num` is the scans' last element: offsets[num] = the total.
__global__ void lattice_count_kernel(const int32_t* status, const LatItem* item, uint32_t num,
                                     int32_t* status_out, uint64_t* cnt_states,
                                     uint64_t* cnt_arcs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > num) return;
  if (i == num) {
    cnt_states[num] = 0;
    cnt_arcs[num] = 0;
    return;
  }
  const int32_t st = status[i];
  status_out[i] = st;
  const bool ok = st == kPathOk;
  cnt_states[i] = ok ? item[i].n : 0u;
  cnt_arcs[i] = ok ? item[i].a : 0u;
}

// One wavefront per item (grid-stride): finals, global arc offsets and the four arc arrays
// from the item's place in the arena to its place in item order, consecutive lanes to
// consecutive elements on both sides.  The result depends on state_offsets / arc_base alone,
// not on where (in which order) the items landed in the arena.  An item that would read past
// the arena or write past the capacities is not copied (an engine bug; the host compares the
// totals with the capacities before it launches this).  Block 0 closes arc_offsets.
__global__ void __launch_bounds__(64)
lattice_gather_kernel(LatticeOutDev arena, const uint64_t* arc_base, LatticeCsrDev csr,
                      uint32_t num) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && csr.state_offsets[num] <= csr.state_cap)
    csr.arc_offsets[csr.state_offsets[num]] = arc_base[num];
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    const bool ok = csr.status[i] == kPathOk;
    const uint64_t so = csr.state_offsets[i], ab = arc_base[i];
    const uint32_t N = (uint32_t)(csr.state_offsets[i + 1] - so);
    const uint32_t A = (uint32_t)(arc_base[i + 1] - ab);
    if (threadIdx.x == 0) csr.start[i] = (ok && N > 0) ? 0u : kNoState;
    if (!ok || N == 0) continue;
    const LatItem it = arena.item[i];
    if (it.n != N || it.a != A) continue;
    if (so + N > csr.state_cap || ab + A > csr.arc_cap) continue;
    if (it.spos + N > arena.state_cap || it.apos + A > arena.arc_cap) continue;
    for (uint32_t s = threadIdx.x; s < N; s += 64) {
      csr.final_w[so + s] = arena.fin[it.spos + s];
      csr.arc_offsets[so + s] = ab + arena.aoff[it.spos + s];
    }
    for (uint32_t k = threadIdx.x; k < A; k += 64) {
      csr.il[ab + k] = arena.il[it.apos + k];
      csr.ol[ab + k] = arena.ol[it.apos + k];
      csr.w[ab + k] = arena.w[it.apos + k];
      csr.next[ab + k] = arena.next[it.apos + k];
    }
  }
}

int lattice_per_cu(int tier, bool chain) {
  // asked of the runtime once per instance (a property of the code object; a concurrent first
  // call stores the same value)
  static std::atomic<int> cache[2][4] = {};
  std::atomic<int>& c = cache[chain ? 1 : 0][tier & 3];
  int occ = c.load(std::memory_order_relaxed);
  if (occ > 0) return occ;
  const int wg = tier == kLhsTierWG ? kLhsWG : 64;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, lattice_kernel(tier, chain), wg, 0) !=
      hipSuccess)
    occ = 1;
  occ = std::max(occ, 1);
  c.store(occ, std::memory_order_relaxed);
  return occ;
}

hipError_t launch_lattice(int tier, bool chain, const RhsView& rhs, const ChainInput& in,
                          const GraphInput& lhs, unsigned int* next_item, const uint32_t* items,
                          const uint32_t* num_items_dev, const BfsWs& ws, const BatchOutDev& out,
                          uint32_t grid, hipStream_t stream) {
  uint32_t n_best = 1, num_items_host = 0;
  void* args[] = {(void*)&rhs,   (void*)&in,           (void*)&lhs,
                  (void*)&n_best, (void*)&next_item,    (void*)&items,
                  (void*)&num_items_dev, (void*)&num_items_host, (void*)&ws, (void*)&out};
  return hipLaunchKernel(lattice_kernel(tier, chain), dim3(grid),
                         dim3(tier == kLhsTierWG ? kLhsWG : 64), args, 0, stream);
}

hipError_t launch_lattice_count(const int32_t* status, const LatItem* item, uint32_t num,
                                int32_t* status_out, uint64_t* cnt_states, uint64_t* cnt_arcs,
                                hipStream_t stream) {
  lattice_count_kernel<<<(num + 256) / 256, 256, 0, stream>>>(status, item, num, status_out,
                                                              cnt_states, cnt_arcs);
  return hipGetLastError();
}

hipError_t launch_lattice_gather(const LatticeOutDev& arena, const uint64_t* arc_base,
                                 const LatticeCsrDev& csr, uint32_t num, uint32_t grid,
                                 hipStream_t stream) {
  lattice_gather_kernel<<<grid, 64, 0, stream>>>(arena, arc_base, csr, num);
  return hipGetLastError();
}

}  // namespace fstamd

// lattice_sp.hpp -- fst_shortest_path (src/ops/shortest-path.zig:18-139) of every item of an
// lhs batch, on the device, with no compose.  An item is its LhsDesc over the
// batch's concatenated CSR, read in place; keys and back words live in a workspace of 16 B per
// state of the shard, indexed like the finals (state_base + s).
//
// Items without kLhsReplay (every weight >= +0, no +inf arc): dist is the least fixpoint of
// d(X) = min fl(d(s) + w) from d(start) = One (§4.1b), so any schedule of relaxations that ends
// with no arc able to lower a key computes it (§4.1e).  The wave tier reaches it by ascending
// sweeps over 64-state chunks, the frontier tier by label correcting; both then run
// bfs_shortest_path's tail (back words, best final, backtrace) on a BfsTables view of the item.
// Items with kLhsReplay take sp_replay, lane 0 replaying the reference's heap (§4.1c).
// Every loop is bounded: sweeps by the budget, a chunk's rounds by kSpChunkRounds, the frontier's
// rounds by the state count and the deadline, the replay by its deadline.
#pragma once
#include "eager_bfs.hpp"

namespace fstamd {

constexpr int kSpWG = 256;                // the frontier tier: one workgroup per item
constexpr uint32_t kSpChunkRounds = 128;  // a chunk that has not closed by then: hand the item on

// One item as the kernels read it: a BfsTables view (aoff / anext / ail / aol / aw / nfin the
// batch's own arrays, nd / nback the workspace) and the descriptor's scalars, wave-uniform.
struct SpItem {
  BfsTables T;
  uint64_t sb, ab;
  uint32_t n, a, start, flags;
};

__device__ __forceinline__ SpItem sp_item(const LatSpDev& p, uint32_t si) {
  const uint4* q = reinterpret_cast<const uint4*>(p.desc + si);
  const uint4 x = q[0], y = q[1];
  const auto sgpr = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  SpItem it;
  it.sb = ((uint64_t)sgpr(x.y) << 32) | sgpr(x.x);
  it.ab = ((uint64_t)sgpr(x.w) << 32) | sgpr(x.z);
  it.n = sgpr(y.x);
  it.start = sgpr(y.y);
  it.a = sgpr(y.z);
  it.flags = sgpr(y.w);
  BfsTables& T = it.T;
  T.hkey = nullptr;
  T.hval = nullptr;
  T.nkey = nullptr;
  T.lvl = nullptr;
  T.cslot = nullptr;
  // (item i's offset words start i words on: one closing word per earlier item)
  T.aoff = const_cast<uint32_t*>(p.state_off) + it.sb + sgpr(si);
  T.nfin = const_cast<double*>(p.final_w) + it.sb;
  T.anext = const_cast<uint32_t*>(p.arc_next) + it.ab;
  T.ail = const_cast<uint32_t*>(p.arc_il) + it.ab;
  T.aol = const_cast<uint32_t*>(p.arc_ol) + it.ab;
  T.aw = const_cast<double*>(p.arc_w) + it.ab;
  T.nd = p.key + it.sb;
  T.nback = p.back + it.sb;
  return it;
}

// The single call's tests before any traversal, in its order (shortest-path.zig:21-24), then
// the NaN flag (an item the prepare kernel refused carries it too, with no states and a harmless
// start).  True: the item is finished.  Uniform; lane 0 writes.
__device__ __forceinline__ bool sp_precheck(const SpItem& it, uint32_t n_best,
                                            const BatchOutDev& out, uint32_t si) {
  int32_t st = kPathOk;
  if (it.start == kNoState || n_best == 0) st = kPathEmpty;
  else if (n_best != 1) st = kPathErrorN;
  else if (it.flags & kLhsNaN) st = kPathUnsupported;
  else if (it.start >= it.n) st = kPathEmpty;  // (no validated item has such a start)
  if (st == kPathOk) return false;
  if (threadIdx.x == 0) write_status(out, si, st, 0, 0);
  return true;
}

// ---- wave tier: one wave per item, ascending sweeps over 64-state chunks --------------------
// Lane s of a chunk relaxes its state's out-arcs whenever its key differs from the one it last
// relaxed with (atomicMin on the target's key).  A chunk is repeated until no target inside it
// dropped; a drop in a lower chunk makes the sweep `pending`; a drop in a higher chunk is
// picked up when the sweep gets there.  After a sweep with nothing pending no arc can lower a
// key: every state relaxed with its final key.
__global__ void __launch_bounds__(64)
lattice_sp_wave_kernel(LatSpDev p, const uint32_t* items, uint32_t count, BatchOutDev out) {
  __shared__ BfsShared SH;
  const uint32_t lane = threadIdx.x;
  uint32_t settled = 0;  // (one atomic per wave, not per item)
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = items[li];
    const SpItem it = sp_item(p, si);
    if (sp_precheck(it, p.n_best, out, si)) {
      ++settled;
      continue;
    }
    const BfsTables& T = it.T;
    const uint32_t n = it.n;
    for (uint32_t s = lane; s < n; s += 64)
      T.nd[s] = s == it.start ? okey(w_one()) : okey(w_zero());
    __syncthreads();
    bool converged = false;
    for (uint32_t sweep = 0; sweep < p.sweeps && !converged; ++sweep) {
      bool pending = false, open = false;
      for (uint32_t c = 0; c < n && !open; c += 64) {
        const uint32_t s = c + lane;
        uint32_t a0 = 0, a1 = 0;
        if (s < n) {
          a0 = T.aoff[s];
          a1 = T.aoff[s + 1];
          a1 = a1 < it.a ? a1 : it.a;
        }
        unsigned long long done = okey(w_zero());  // the key the lane last relaxed with
        open = true;
        for (uint32_t round = 0; round < kSpChunkRounds; ++round) {
          bool inside = false, low = false;
          const unsigned long long k = s < n ? ld_agent(&T.nd[s]) : okey(w_zero());
          if (k != done) {
            done = k;
            const double ds = from_okey(k);
            for (uint32_t a = a0; a < a1; ++a) {
              const uint32_t x = T.anext[a];
              if (x >= n) continue;
              const unsigned long long v = okey(w_times(ds, T.aw[a]));  // shortest-path.zig:72
              if (v < atomicMin(&T.nd[x], v)) {
                if (x < c) low = true;
                else if (x < c + 64) inside = true;
              }
            }
          }
          pending |= __ballot(low) != 0;
          if (__ballot(inside) == 0) {
            open = false;
            break;
          }
        }
      }
      converged = !pending && !open;
    }
    if (!converged) {  // (uniform) the frontier tier starts the item afresh
      if (lane == 0) p.list[atomicAdd(&p.ctr[kSpCtrList], 1u)] = si;
      continue;
    }
    ++settled;
    bfs_shortest_path<64>(T, n, it.a, 1u, it.start, out, si, SH,
                          __builtin_amdgcn_s_memrealtime() + p.wd_ticks, false, true);
    __syncthreads();  // (SH is the next item's)
  }
  if (lane == 0 && settled) atomicAdd(&p.ctr[kSpCtrWave], settled);
}

// ---- frontier tier: one workgroup per listed item, label correcting ------------------------
// sp_frontier_kernel's rounds on the item's slices of the workspaces: round r relaxes the
// out-arcs of the states whose key dropped in round r - 1; a state joins the next frontier once
// per round (stamp), so a frontier never holds more than n states.  After round r every state
// whose shortest path has at most r + 1 arcs holds its final key, so weights >= 0 need at most
// n rounds; beyond that, or past the deadline, the item ends INTERNAL.
__global__ void __launch_bounds__(kSpWG)
lattice_sp_frontier_kernel(LatSpDev p, BatchOutDev out) {
  __shared__ BfsShared SH;
  __shared__ uint32_t cnt[2];
  __shared__ uint32_t stop;
  const uint32_t tid = threadIdx.x;
  const uint32_t count = p.ctr[kSpCtrList];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = p.list[li];
    const SpItem it = sp_item(p, si);
    if (it.start >= it.n) continue;  // (the wave tier lists no such item)
    const BfsTables& T = it.T;
    const uint32_t n = it.n;
    uint32_t* mark = p.mark + it.sb;
    uint32_t* cur = p.fa + it.sb;
    uint32_t* nxt = p.fb + it.sb;
    const unsigned long long deadline = __builtin_amdgcn_s_memrealtime() + p.wd_ticks;
    for (uint32_t s = tid; s < n; s += kSpWG) {
      T.nd[s] = s == it.start ? okey(w_one()) : okey(w_zero());
      mark[s] = ~0u;
    }
    if (tid == 0) {
      cur[0] = it.start;
      cnt[0] = 1;
      cnt[1] = 0;
      stop = 0;
    }
    __syncthreads();
    for (uint32_t r = 0;; ++r) {
      const uint32_t fsize = min(cnt[r & 1], n);
      const uint32_t halted = stop;
      __syncthreads();  // every thread has read the round's words before thread 0 writes them
      if (fsize == 0 || halted) break;
      if (tid == 0) {
        cnt[(r + 1) & 1] = 0;
        if (r > n || ((r & 63u) == 63u && __builtin_amdgcn_s_memrealtime() > deadline)) stop = 1;
      }
      __syncthreads();
      uint32_t* const push = &cnt[(r + 1) & 1];
      for (uint32_t q = tid; q < fsize; q += kSpWG) {
        const uint32_t s = ld_agent(&cur[q]);
        if (s >= n) continue;
        const double ds = from_okey(ld_agent(&T.nd[s]));
        const uint32_t a0 = T.aoff[s];
        uint32_t a1 = T.aoff[s + 1];
        a1 = a1 < it.a ? a1 : it.a;
        for (uint32_t a = a0; a < a1; ++a) {
          const uint32_t x = T.anext[a];
          if (x >= n) continue;
          const unsigned long long v = okey(w_times(ds, T.aw[a]));  // shortest-path.zig:72
          if (v < atomicMin(&T.nd[x], v) && atomicExch(&mark[x], r) != r) {
            const uint32_t slot = atomicAdd(push, 1u);
            if (slot < n) nxt[slot] = x;
          }
        }
      }
      __syncthreads();
      uint32_t* t = cur;
      cur = nxt;
      nxt = t;
    }
    const bool failed = stop != 0;
    __syncthreads();
    if (failed) {
      if (tid == 0) write_status(out, si, kPathInternal, n, it.a);
    } else {
      bfs_shortest_path<kSpWG>(T, n, it.a, 1u, it.start, out, si, SH, deadline, false, true);
    }
    if (tid == 0) atomicAdd(&p.ctr[kSpCtrFrontier], 1u);
    __syncthreads();  // (the shared words are the next item's)
  }
}

// ---- replay tier: one wave per kLhsReplay item, lane 0 replaying the reference's heap -------
// The item's heap is its (num_arcs + 1) entries at arc_base + item index of the heap workspace.
__global__ void __launch_bounds__(64)
lattice_sp_replay_kernel(LatSpDev p, const uint32_t* items, uint32_t count, BatchOutDev out) {
  uint32_t settled = 0;
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = items[li];
    const SpItem it = sp_item(p, si);
    ++settled;
    if (sp_precheck(it, p.n_best, out, si)) continue;
    sp_replay(it.T, it.n, it.a, it.start, p.heap + it.ab + si, (uint64_t)it.a + 1,
              p.settled + it.sb, out, si, __builtin_amdgcn_s_memrealtime() + p.wd_ticks);
    __syncthreads();  // (lanes 1.. wait for lane 0 before they initialise the next item)
  }
  if (threadIdx.x == 0 && settled) atomicAdd(&p.ctr[kSpCtrReplay], settled);
}

}  // namespace fstamd

// lattice_trim.hpp -- connect (src/ops/connect.zig:17-124) of every item of a lattice arena,
// on the device.  An item is LatItem {spos, apos, n, a} over the arena's fin /
// aoff / il / ol / w / next; the arena is only read.  The pass leaves
//   mark[spos + s]   the state's new id, or kNoState for a dropped state (before that: bit 0
//                    coaccessible, bit 1 accessible),
//   LatItem n, a     the trimmed counts (pad[0], pad[1] keep the untrimmed ones),
// and lattice_trim_gather_kernel then copies the kept states and arcs, in their order, to the
// item's place in FstLhsBatch's layout: lattice_gather_kernel with a filter.
//
// Kept = accessible and coaccessible; both are least fixed points, so every schedule that
// only ever marks a state for a marked neighbour and stops at a fixed point computes the same
// set: the result depends on the item alone.  Every loop is bounded by construction (sweeps
// by the budget, chunk closures by 64 rounds, the frontier BFS by n pops).
#pragma once
#include "device_common.hpp"

namespace fstamd {

constexpr int kTrimWG = 256;  // the linear tier and the accessibility pass: one workgroup per item
constexpr uint32_t kTrimCo = 1u, kTrimAcc = 2u, kTrimKept = 3u;

// isFinal of weight.zig: !isInf, so -inf is not final and NaN is.
__device__ __forceinline__ bool trim_is_final(double f) {
  return ((unsigned long long)__double_as_longlong(f) & 0x7FFFFFFFFFFFFFFFull) !=
         0x7FF0000000000000ull;
}

// One item as the trim kernels read it (pointers already at the item's first state / arc).
struct TrimView {
  const double* fin;
  const uint32_t* aoff;  // n local arc offsets; the closing one is a
  const uint32_t* next;
  uint32_t* mark;
  uint64_t spos, apos;
  uint32_t n, a;
};

// False: the item is not OK or does not lie inside the arena (an engine bug; such an item is
// left alone, as lattice_gather_kernel leaves it).  `trimmed`: LatItem already holds the
// trimmed counts and pad the untrimmed ones.
__device__ __forceinline__ bool trim_view(const LatticeOutDev& arena, const LatTrimDev& t,
                                          const int32_t* status, uint32_t i, bool trimmed,
                                          TrimView* v) {
  if (status[i] != kPathOk) return false;
  const LatItem it = arena.item[i];
  v->n = trimmed ? it.pad[0] : it.n;
  v->a = trimmed ? it.pad[1] : it.a;
  v->spos = it.spos;
  v->apos = it.apos;
  if (it.spos + v->n > arena.state_cap || it.apos + v->a > arena.arc_cap) return false;
  v->fin = arena.fin + it.spos;
  v->aoff = arena.aoff + it.spos + (uint64_t)t.aoff_skew * i;
  v->next = arena.next + it.apos;
  v->mark = t.mark + it.spos;
  return true;
}

// The arcs [*b, *e) of state s, clamped into the item.
__device__ __forceinline__ void trim_arc_range(const TrimView& v, uint32_t s, uint32_t* b,
                                               uint32_t* e) {
  const uint32_t hi = s + 1 < v.n ? v.aoff[s + 1] : v.a;
  *e = hi < v.a ? hi : v.a;
  const uint32_t lo = v.aoff[s];
  *b = lo < *e ? lo : *e;
}

// The start of item i (the compose entries: 0) or kNoState.
__device__ __forceinline__ uint32_t trim_start(const LatTrimDev& t, uint32_t i, uint32_t n) {
  const uint32_t st = t.start ? t.start[i] : 0u;
  return st < n ? st : kNoState;
}

// ---- the stand-alone entry's staging: LhsDesc -> LatItem, every item OK --------------------
__global__ void lattice_trim_stage_kernel(const LhsDesc* desc, uint32_t num, LatItem* item,
                                          int32_t* status, uint32_t* start) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  const LhsDesc d = desc[i];
  LatItem it;
  it.spos = d.state_base;
  it.apos = d.arc_base;
  it.n = d.num_states;
  it.a = d.num_arcs;
  it.pad[0] = d.num_states;
  it.pad[1] = d.num_arcs;
  item[i] = it;
  status[i] = kPathOk;
  start[i] = d.start;
}

// Frontier BFS of one workgroup over a CSR (off: n local offsets, the closing one is a) from
// the seeds in queue[0, sh[1]) (already marked; sh[0] = 0, sh[2] = sh[1], a barrier passed).
// A state enters the queue when its bit goes from 0 to 1, so once: at most n pops, and the
// level loop runs at most n + 1 times.
__device__ __forceinline__ void trim_bfs(const uint32_t* off, const uint32_t* nbr, uint32_t n,
                                         uint32_t a, uint32_t* mark, uint32_t bit,
                                         uint32_t* queue, uint32_t* sh) {
  for (uint32_t level = 0; level <= n; ++level) {
    const uint32_t head = sh[0], tail = sh[1];
    __syncthreads();
    if (head >= tail) break;
    for (uint32_t q = head + threadIdx.x; q < tail; q += kTrimWG) {
      const uint32_t s = queue[q];
      if (s >= n) continue;
      uint32_t e = s + 1 < n ? off[s + 1] : a;
      e = e < a ? e : a;
      for (uint32_t k = off[s]; k < e; ++k) {
        const uint32_t u = nbr[k];
        if (u >= n) continue;
        if (atomicOr(&mark[u], bit) & bit) continue;
        const uint32_t p = atomicAdd(&sh[2], 1u);
        if (p < n) queue[p] = u;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      sh[0] = tail;
      sh[1] = sh[2] < n ? sh[2] : n;
    }
    __syncthreads();
  }
}

// ---- accessibility (the stand-alone entry alone: compose output is accessible by
// construction): mark = kTrimAcc on the forward closure of the start, 0 elsewhere ------------
__global__ void __launch_bounds__(kTrimWG)
lattice_trim_access_kernel(LatticeOutDev arena, LatTrimDev t, const int32_t* status,
                           uint32_t num) {
  __shared__ uint32_t sh[3];
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    TrimView v;
    if (!trim_view(arena, t, status, i, false, &v)) continue;
    const uint32_t st = trim_start(t, i, v.n);
    for (uint32_t s = threadIdx.x; s < v.n; s += kTrimWG) v.mark[s] = s == st ? kTrimAcc : 0u;
    uint32_t* queue = t.queue + v.spos;
    if (threadIdx.x == 0) {
      sh[0] = 0;
      sh[1] = sh[2] = st != kNoState ? 1u : 0u;
      if (st != kNoState) queue[0] = st;
    }
    __syncthreads();
    trim_bfs(v.aoff, v.next, v.n, v.a, v.mark, kTrimAcc, queue, sh);
    __syncthreads();
  }
}

// ---- sweep tier: one wave per item, descending sweeps co[s] |= any co[next] ------------------
// A chunk of 64 states is closed in registers: lane s holds the mask of its targets inside
// the chunk and whether a target outside it is marked; the closure is ballots alone.  A sweep
// settles everything but arcs into a lower chunk whose target is marked later in the same
// sweep (`pending`).  The item has converged after a sweep without such a state, or after one
// that changed nothing; an item that has not within the budget goes to the linear tier by the
// device list.
__global__ void __launch_bounds__(64)
lattice_trim_sweep_kernel(LatticeOutDev arena, LatTrimDev t, const int32_t* status,
                          uint32_t num) {
  const uint32_t lane = threadIdx.x;
  uint32_t settled = 0;  // (one atomic per wave, not per item: every item adds to one word)
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    TrimView v;
    if (!trim_view(arena, t, status, i, false, &v)) continue;
    const uint32_t n = v.n;
    for (uint32_t s = lane; s < n; s += 64)
      v.mark[s] = (t.access ? (v.mark[s] & kTrimAcc) : kTrimAcc) |
                  (trim_is_final(v.fin[s]) ? kTrimCo : 0u);
    __syncthreads();
    bool converged = n == 0;
    for (uint32_t sweep = 0; sweep < t.sweeps && !converged; ++sweep) {
      bool pending = false, changed = false;
      for (uint32_t c = (n - 1) & ~63u;; c -= 64) {
        const uint32_t s = c + lane;
        const bool valid = s < n;
        const uint32_t m = valid ? v.mark[s] : kTrimCo;
        bool co = (m & kTrimCo) != 0, low = false;
        unsigned long long adj = 0;
        if (!co) {
          uint32_t b, e;
          trim_arc_range(v, s, &b, &e);
          for (uint32_t k = b; k < e && !co; ++k) {
            const uint32_t u = v.next[k];
            if (u >= n) continue;
            if (u >= c && u < c + 64) {
              adj |= 1ull << (u - c);
            } else if (v.mark[u] & kTrimCo) {
              co = true;
            } else if (u < c) {
              low = true;
            }
          }
        }
        unsigned long long cur = __ballot(co);
        for (int round = 0; round < 64; ++round) {
          const unsigned long long nw = cur | __ballot((adj & cur) != 0);
          if (nw == cur) break;
          cur = nw;
        }
        const bool now = (cur >> lane) & 1;
        const bool fresh = valid && now && !(m & kTrimCo);
        if (fresh) v.mark[s] = m | kTrimCo;
        changed |= __ballot(fresh) != 0;
        pending |= __ballot(valid && !now && low) != 0;
        __syncthreads();  // the chunk's marks are stored before a lower chunk reads them
        if (c == 0) break;
      }
      converged = !pending || !changed;
    }
    if (converged) {
      ++settled;
    } else if (lane == 0) {
      t.list[atomicAdd(&t.ctr[kTrimCtrList], 1u)] = i;
    }
  }
  if (lane == 0 && settled) atomicAdd(&t.ctr[kTrimCtrSweep], settled);
}

// ---- linear tier: one workgroup per listed item, O(states + arcs) ----------------------------
// The item's reverse CSR in the workspace (in-degrees by atomicAdd, a workgroup scan, the
// sources filled by a cursor per state: their order inside a state does not matter to a
// closure), then the frontier BFS from the finals.
__global__ void __launch_bounds__(kTrimWG)
lattice_trim_linear_kernel(LatticeOutDev arena, LatTrimDev t, const int32_t* status) {
  __shared__ uint32_t sh[3];
  __shared__ uint32_t scan_ws[kTrimWG / 64];
  const uint32_t count = t.ctr[kTrimCtrList];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t i = t.list[li];
    TrimView v;
    if (!trim_view(arena, t, status, i, false, &v)) continue;
    const uint32_t n = v.n, a = v.a;
    uint32_t* roff = t.roff + v.spos;
    uint32_t* rcur = t.rcur + v.spos;
    uint32_t* rsrc = t.rsrc + v.apos;
    uint32_t* queue = t.queue + v.spos;
    for (uint32_t s = threadIdx.x; s < n; s += kTrimWG) roff[s] = 0;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < a; k += kTrimWG) {
      const uint32_t u = v.next[k];
      if (u < n) atomicAdd(&roff[u], 1u);
    }
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t c = 0; c < n; c += kTrimWG) {
      const uint32_t s = c + threadIdx.x;
      // (an atomic load: the counts were made by atomics, which a plain load may not see)
      const uint32_t d =
          s < n ? __hip_atomic_load(&roff[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      uint32_t tot = 0;
      const uint32_t ex = block_excl_scan<kTrimWG>(d, scan_ws, tot);
      if (s < n) {
        roff[s] = base + ex;
        rcur[s] = base + ex;
      }
      base += tot;
    }
    const uint32_t ra = base < a ? base : a;  // arcs with a target inside the item
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < n; s += kTrimWG) {
      uint32_t b, e;
      trim_arc_range(v, s, &b, &e);
      for (uint32_t k = b; k < e; ++k) {
        const uint32_t u = v.next[k];
        if (u >= n) continue;
        const uint32_t p = atomicAdd(&rcur[u], 1u);
        if (p < ra) rsrc[p] = s;
      }
    }
    if (threadIdx.x == 0) sh[0] = sh[1] = 0;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < n; s += kTrimWG) {
      uint32_t m = v.mark[s] & ~kTrimCo;
      if (trim_is_final(v.fin[s])) {
        m |= kTrimCo;
        const uint32_t p = atomicAdd(&sh[1], 1u);
        if (p < n) queue[p] = s;
      }
      v.mark[s] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) sh[2] = sh[1];
    __syncthreads();
    trim_bfs(roff, rsrc, n, ra, v.mark, kTrimCo, queue, sh);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&t.ctr[kTrimCtrLinear], 1u);
  }
}

// One wave over the arcs of an item, in arc order, a chunk of 64 source states at a time: arc k
// is kept when its source (found among the chunk's 64 offsets by shuffles) and its target are.
// Counts the kept arcs; kWrite: also copies them to csr at ab + rank with the target
// renumbered, and the chunk's kept states' finals and arc offsets (deg: 64 LDS words).
template <bool kWrite>
__device__ __forceinline__ uint32_t trim_arc_pass(const TrimView& v, const LatticeOutDev& arena,
                                                  const LatticeCsrDev& csr, uint64_t so,
                                                  uint64_t ab, uint32_t N, uint32_t A,
                                                  uint32_t* deg) {
  const uint32_t lane = threadIdx.x, n = v.n, a = v.a;
  uint32_t run = 0;
  for (uint32_t c = 0; c < n; c += 64) {
    const uint32_t s = c + lane;
    const bool valid = s < n;
    const uint32_t m = valid ? v.mark[s] : kNoState;
    const uint32_t kept = m != kNoState ? 1u : 0u;
    uint32_t b = a, e = a;
    if (valid) trim_arc_range(v, s, &b, &e);
    const uint32_t lo = __shfl(b, 0, 64);
    uint32_t hi = a;
    if (c + 64 < n) hi = v.aoff[c + 64] < a ? v.aoff[c + 64] : a;
    if (kWrite) {
      deg[lane] = 0;
      __syncthreads();
    }
    const uint32_t run0 = run;
    for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool av = k < hi;
      uint32_t j = 0;  // the last lane whose first arc is at or before k: the arc's source
#pragma unroll
      for (uint32_t step = 32; step; step >>= 1) {
        const uint32_t bt = __shfl(b, (int)(j + step), 64);
        if (bt <= k) j += step;
      }
      const uint32_t src_kept = __shfl(kept, (int)j, 64);
      uint32_t mm = kNoState;
      if (av && src_kept) {
        const uint32_t u = v.next[k];
        if (u < n) mm = v.mark[u];
      }
      const bool keep = mm != kNoState;
      const unsigned long long bal = __ballot(keep);
      const uint32_t pos = run + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      if (kWrite && keep && pos < A && mm < N) {
        const uint64_t q = ab + pos, g = v.apos + k;
        csr.il[q] = arena.il[g];
        csr.ol[q] = arena.ol[g];
        csr.w[q] = arena.w[g];
        csr.next[q] = mm;
        atomicAdd(&deg[j], 1u);
      }
      run += (uint32_t)__popcll(bal);
    }
    if (kWrite) {
      __syncthreads();
      const uint32_t d = deg[lane];
      const uint32_t ex = wave_incl_scan(d) - d;
      if (kept && m < N) {
        const double f = v.fin[s];
        csr.final_w[so + m] = trim_is_final(f) ? f : __longlong_as_double(0x7FF0000000000000ll);
        csr.arc_offsets[so + m] = ab + run0 + ex;
      }
      __syncthreads();
    }
  }
  return run;
}

// ---- the old -> new map and the trimmed counts: one wave per item ---------------------------
__global__ void __launch_bounds__(64)
lattice_trim_finalize_kernel(LatticeOutDev arena, LatTrimDev t, const int32_t* status,
                             uint32_t num) {
  const uint32_t lane = threadIdx.x;
  unsigned long long tot[4] = {0, 0, 0, 0};  // (added once per wave: the route log's totals)
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    TrimView v;
    if (!trim_view(arena, t, status, i, false, &v)) continue;
    const uint32_t n = v.n;
    uint32_t kept_n = 0;
    for (uint32_t c = 0; c < n; c += 64) {
      const uint32_t s = c + lane;
      const bool kept = s < n && (v.mark[s] & kTrimKept) == kTrimKept;
      const unsigned long long bal = __ballot(kept);
      if (s < n)
        v.mark[s] = kept ? kept_n + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)) : kNoState;
      kept_n += (uint32_t)__popcll(bal);
    }
    __syncthreads();
    const uint32_t st = trim_start(t, i, n);
    uint32_t kept_a = 0;
    if (st == kNoState || v.mark[st] == kNoState) {
      kept_n = 0;  // the start is not kept: the empty FST
    } else {
      kept_a = trim_arc_pass<false>(v, arena, LatticeCsrDev{}, 0, 0, 0, 0, nullptr);
    }
    if (lane == 0) {
      LatItem* it = arena.item + i;
      it->pad[0] = v.n;
      it->pad[1] = v.a;
      it->n = kept_n;
      it->a = kept_a;
    }
    tot[0] += v.n;
    tot[1] += kept_n;
    tot[2] += v.a;
    tot[3] += kept_a;
  }
  if (lane == 0 && tot[0] + tot[2])
    for (int k = 0; k < 4; ++k) atomicAdd(&t.tot[k], tot[k]);
}

// ---- lattice_gather_kernel with the filter: one wave per item --------------------------------
// The same contract: the result depends on state_offsets / arc_base and the item alone; an item
// whose counts disagree with the scans, or that would write past a capacity, is not copied.
__global__ void __launch_bounds__(64)
lattice_trim_gather_kernel(LatticeOutDev arena, LatTrimDev t, const uint64_t* arc_base,
                           LatticeCsrDev csr, uint32_t num) {
  __shared__ uint32_t deg[64];
  if (blockIdx.x == 0 && threadIdx.x == 0 && csr.state_offsets[num] <= csr.state_cap)
    csr.arc_offsets[csr.state_offsets[num]] = arc_base[num];
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    const uint64_t so = csr.state_offsets[i], ab = arc_base[i];
    const uint32_t N = (uint32_t)(csr.state_offsets[i + 1] - so);
    const uint32_t A = (uint32_t)(arc_base[i + 1] - ab);
    TrimView v;
    const bool ok = N > 0 && trim_view(arena, t, csr.status, i, true, &v);
    const uint32_t st = ok ? trim_start(t, i, v.n) : kNoState;
    if (threadIdx.x == 0) csr.start[i] = st != kNoState ? v.mark[st] : kNoState;
    if (!ok) continue;
    const LatItem it = arena.item[i];
    if (it.n != N || it.a != A) continue;
    if (so + N > csr.state_cap || ab + A > csr.arc_cap) continue;
    trim_arc_pass<true>(v, arena, csr, so, ab, N, A, deg);
  }
}

}  // namespace fstamd

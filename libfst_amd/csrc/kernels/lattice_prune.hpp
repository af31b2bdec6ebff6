// lattice_prune.hpp -- beam pruning of every item of an lhs batch, on the device (DESIGN.md
// §7k; the definition: fst_prune_lhs_batch, include/fst_batch.h).  An item is its LhsDesc over
// the batch's concatenated CSR, read in place.  Per item the kernels compute
//   F(s)  the least left-fold distance from the start,
//   B(s)  the least right-fold distance to a final state (the final weight included),
// and the mark pass then writes the cut as a shadow of the item's `next` (a dropped arc points
// to kNoState) and of its finals (a dropped final weight is +inf), its LatItem, status and
// start.  The trim ladder (kernels/lattice_trim.hpp) runs on that shadow view and the filtering
// gather copies what it keeps: the item's own arrays are never written.
//
// Every arc weight is >= 0 (or the item is UNSUPPORTED), so fl(x + w) >= x and both distances
// are the fixpoints every relaxation order reaches from +inf (§4.1e); B is the same problem on
// the reversed arcs with every final state a source.  Keys are pkey(), a total order on the
// non-NaN doubles (final weights, and with them B, may be negative); every test of the cut is on
// the f64 values, so the place of -0.0 below +0.0 among the keys never shows.
// Every loop is bounded: sweeps by the budget, a chunk's rounds by kPruneChunkRounds, the
// frontier's rounds by the state count and the deadline.
#pragma once
#include "device_common.hpp"

namespace fstamd {

constexpr int kPruneWG = 256;                // the frontier tier: one workgroup per item
constexpr uint32_t kPruneChunkRounds = 128;  // a chunk that has not closed by then: hand on

// Order-preserving u64 key of a non-NaN double, and back.
__device__ __forceinline__ unsigned long long pkey(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double from_pkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}
// connect's rule (trim_is_final, kernels/lattice_trim.hpp): final = the weight is not +-inf.
__device__ __forceinline__ bool prune_is_final(double f) {
  return ((unsigned long long)__double_as_longlong(f) & 0x7FFFFFFFFFFFFFFFull) !=
         0x7FF0000000000000ull;
}
__device__ __forceinline__ double prune_inf() {
  return __longlong_as_double(0x7FF0000000000000ll);
}
// (keys another lane of the wave, or another wave of the workgroup, may just have written)
template <class T>
__device__ __forceinline__ T prune_ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void prune_st(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One item as the kernels read it (pointers at the item's first state / arc), wave-uniform.
struct PruneItem {
  const uint32_t* aoff;  // n + 1 local arc offsets
  const double* fin;
  const uint32_t* next;
  const double* w;
  uint64_t sb, ab;
  uint32_t n, a, start, flags;
};

__device__ __forceinline__ PruneItem prune_item(const LatPruneDev& p, uint32_t si) {
  const uint4* q = reinterpret_cast<const uint4*>(p.desc + si);
  const uint4 x = q[0], y = q[1];
  const auto sgpr = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  PruneItem it;
  it.sb = ((uint64_t)sgpr(x.y) << 32) | sgpr(x.x);
  it.ab = ((uint64_t)sgpr(x.w) << 32) | sgpr(x.z);
  it.n = sgpr(y.x);
  it.start = sgpr(y.y);
  it.a = sgpr(y.z);
  it.flags = sgpr(y.w);
  // (item i's offset words start i words on: one closing word per earlier item)
  it.aoff = p.state_off + it.sb + sgpr(si);
  it.fin = p.final_w + it.sb;
  it.next = p.arc_next + it.ab;
  it.w = p.arc_w + it.ab;
  return it;
}

// The arcs [*a0, *a1) of state s < n, clamped into the item.
__device__ __forceinline__ void prune_arc_range(const PruneItem& it, uint32_t s, uint32_t* a0,
                                                uint32_t* a1) {
  const uint32_t hi = it.aoff[s + 1];
  *a1 = hi < it.a ? hi : it.a;
  const uint32_t lo = it.aoff[s];
  *a0 = lo < *a1 ? lo : *a1;
}

// An item with no result of its own: the empty FST under `st`.  Thread 0 writes.
__device__ __forceinline__ void prune_write_empty(const LatPruneDev& p, const PruneItem& it,
                                                  uint32_t si, int32_t st) {
  if (threadIdx.x != 0) return;
  LatItem e;
  e.spos = it.sb;
  e.apos = it.ab;
  e.n = e.a = 0;
  e.pad[0] = e.pad[1] = 0;
  p.item[si] = e;
  p.status[si] = st;
  p.start[si] = kNoState;
}

// The statuses that need no traversal, in the definition's order (an item the prepare kernel
// refused has no states and a harmless start, so its flag is looked at first).  True: the item
// is finished.  One wave, uniform.
__device__ __forceinline__ bool prune_precheck(const LatPruneDev& p, const PruneItem& it,
                                               uint32_t si) {
  int32_t st = -1;
  if (it.flags & kLhsInvalid) {
    st = kPathUnsupported;
  } else if (it.start >= it.n) {  // no start (kNoState), or no states
    st = kPathOk;
  } else if (it.flags & kLhsNaN) {
    st = kPathUnsupported;
  } else if (it.flags & kLhsReplay) {  // a sign bit or an infinity somewhere: is an arc < 0?
    bool neg = false;
    for (uint32_t k = threadIdx.x; k < it.a; k += 64) neg |= it.w[k] < 0.0;
    if (__ballot(neg) != 0) st = kPathUnsupported;
  }
  if (st < 0) return false;
  prune_write_empty(p, it, si, st);
  return true;
}

// ---- wave tier, forward: lattice_sp_wave_kernel's ascending sweeps -------------------------
// Lane s of a chunk relaxes its out-arcs whenever its key differs from the one it last relaxed
// with (atomicMin on the target's key); a chunk is repeated until no target inside it dropped;
// a drop in a lower chunk makes the sweep pending.  True: no arc can lower a key any more.
__device__ __forceinline__ bool prune_wave_forward(const PruneItem& it, unsigned long long* kf,
                                                   uint32_t sweeps) {
  const uint32_t lane = threadIdx.x, n = it.n;
  const unsigned long long kinf = pkey(prune_inf());
  for (uint32_t s = lane; s < n; s += 64) prune_st(&kf[s], s == it.start ? pkey(0.0) : kinf);
  __syncthreads();
  bool converged = false;
  for (uint32_t sweep = 0; sweep < sweeps && !converged; ++sweep) {
    bool pending = false, open = false;
    for (uint32_t c = 0; c < n && !open; c += 64) {
      const uint32_t s = c + lane;
      uint32_t a0 = 0, a1 = 0;
      if (s < n) prune_arc_range(it, s, &a0, &a1);
      unsigned long long done = kinf;  // the key the lane last relaxed with
      open = true;
      for (uint32_t round = 0; round < kPruneChunkRounds; ++round) {
        bool inside = false, low = false;
        const unsigned long long k = s < n ? prune_ld(&kf[s]) : kinf;
        if (k != done) {
          done = k;
          const double ds = from_pkey(k);
          for (uint32_t a = a0; a < a1; ++a) {
            const uint32_t x = it.next[a];
            if (x >= n) continue;
            const unsigned long long v = pkey(ds + it.w[a]);
            if (v < atomicMin(&kf[x], v)) {
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
  return converged;
}

// ---- wave tier, backward: descending sweeps as a pull ---------------------------------------
// Lane s of a chunk takes the minimum of its final weight and fl(w + B(target)) over its
// out-arcs and lowers only its own key: no atomics, no reverse CSR.  Inside a chunk a lane
// recomputes when a target of its own in the chunk was lowered in the round before (`adj`, the
// mask of those targets); a chunk is closed when a round lowers nothing.  A sweep settles
// everything but states with an arc into a lower chunk, whose target is settled later in the
// same sweep (`pending`): the item has converged after a sweep without such a state, or after
// one that lowered nothing.
__device__ __forceinline__ bool prune_wave_backward(const PruneItem& it, unsigned long long* kb,
                                                    uint32_t sweeps) {
  const uint32_t lane = threadIdx.x, n = it.n;
  const unsigned long long kinf = pkey(prune_inf());
  for (uint32_t s = lane; s < n; s += 64) {
    const double f = it.fin[s];
    prune_st(&kb[s], prune_is_final(f) ? pkey(f) : kinf);
  }
  __syncthreads();
  bool converged = false;
  for (uint32_t sweep = 0; sweep < sweeps && !converged; ++sweep) {
    bool pending = false, changed = false, open = false;
    for (uint32_t c = (n - 1) & ~63u; !open; c -= 64) {
      const uint32_t s = c + lane;
      const bool valid = s < n;
      uint32_t a0 = 0, a1 = 0;
      if (valid) prune_arc_range(it, s, &a0, &a1);
      unsigned long long adj = 0, chg = ~0ull;  // (round 0: every lane computes)
      bool low = false;
      open = true;
      for (uint32_t round = 0; round < kPruneChunkRounds; ++round) {
        bool lowered = false;
        if (valid && (round == 0 || (adj & chg) != 0)) {
          const unsigned long long cur = prune_ld(&kb[s]);
          unsigned long long best = cur;
          for (uint32_t a = a0; a < a1; ++a) {
            const uint32_t u = it.next[a];
            if (u >= n) continue;
            if (u < c) low = true;
            else if (u < c + 64) adj |= 1ull << (u - c);
            const unsigned long long v = pkey(it.w[a] + from_pkey(prune_ld(&kb[u])));
            best = v < best ? v : best;
          }
          lowered = best < cur;
          if (lowered) prune_st(&kb[s], best);
        }
        chg = __ballot(lowered);
        if (chg == 0) {
          open = false;
          break;
        }
        changed = true;
      }
      pending |= __ballot(low) != 0;
      __syncthreads();  // the chunk's keys are stored before a lower chunk reads them
      if (c == 0) break;
    }
    converged = !open && (!pending || !changed);
  }
  return converged;
}

// ---- the mark pass: best, limit, the per-arc and the per-final tests -------------------------
// WG threads on one item whose keys are final; sh_best: one shared word.  Writes the shadow
// finals and targets of the item, its LatItem, status and start.
template <int WG>
__device__ __forceinline__ void prune_mark(const LatPruneDev& p, const PruneItem& it, uint32_t si,
                                           const unsigned long long* kf,
                                           const unsigned long long* kb,
                                           unsigned long long* sh_best) {
  const uint32_t tid = threadIdx.x, n = it.n;
  const double inf = prune_inf();
  const unsigned long long kinf = pkey(inf);
  if (tid == 0) *sh_best = kinf;
  __syncthreads();
  unsigned long long mine = kinf;
  for (uint32_t s = tid; s < n; s += WG) {
    const double f = it.fin[s];
    if (!prune_is_final(f)) continue;
    const unsigned long long k = pkey(from_pkey(prune_ld(&kf[s])) + f);
    mine = k < mine ? k : mine;
  }
  if (mine != kinf) atomicMin(sh_best, mine);
  __syncthreads();
  const double best = from_pkey(*sh_best);
  const bool alive = best != inf;  // (uniform) else: no complete path, everything goes
  const double limit = best + p.beam;
  double* sfin = p.sfin + it.sb;
  uint32_t* snext = p.snext + it.ab;
  for (uint32_t s = tid; s < n; s += WG) {
    const double f = it.fin[s], fs = from_pkey(prune_ld(&kf[s]));
    const double tot = fs + f;
    sfin[s] = alive && prune_is_final(f) && tot != inf && tot <= limit ? f : inf;
    uint32_t a0, a1;
    prune_arc_range(it, s, &a0, &a1);
    for (uint32_t a = a0; a < a1; ++a) {
      const uint32_t u = it.next[a];
      bool keep = false;
      if (alive && u < n) {
        const double t = (fs + it.w[a]) + from_pkey(prune_ld(&kb[u]));
        keep = t != inf && t <= limit;
      }
      snext[a] = keep ? u : kNoState;
    }
  }
  if (tid == 0) {
    LatItem e;
    e.spos = it.sb;
    e.apos = it.ab;
    e.n = e.pad[0] = n;
    e.a = e.pad[1] = it.a;
    p.item[si] = e;
    p.status[si] = kPathOk;
    p.start[si] = it.start;
  }
  __syncthreads();  // (sh_best is the next item's)
}

// ---- wave tier: one wave per item; both key arrays in LDS up to kPruneLdsStates states, in
// the workspace (16 B per state, the item's slice at twice its first state) past that --------
__global__ void __launch_bounds__(64) lattice_prune_wave_kernel(LatPruneDev p, uint32_t num) {
  __shared__ unsigned long long lds_key[2 * kPruneLdsStates];
  __shared__ unsigned long long sh_best;
  uint32_t settled = 0;  // (one atomic per wave, not per item)
  for (uint32_t si = blockIdx.x; si < num; si += gridDim.x) {
    const PruneItem it = prune_item(p, si);
    if (prune_precheck(p, it, si)) {
      ++settled;
      continue;
    }
    unsigned long long* kf = it.n <= kPruneLdsStates ? lds_key : p.key + 2 * it.sb;
    unsigned long long* kb = kf + it.n;
    const bool converged =
        prune_wave_forward(it, kf, p.sweeps) && prune_wave_backward(it, kb, p.sweeps);
    if (!converged) {  // (uniform) the frontier tier starts the item afresh
      if (threadIdx.x == 0) p.list[atomicAdd(&p.ctr[kPrCtrList], 1u)] = si;
      continue;
    }
    ++settled;
    prune_mark<64>(p, it, si, kf, kb, &sh_best);
  }
  if (threadIdx.x == 0 && settled) atomicAdd(&p.ctr[kPrCtrWave], settled);
}

// Label correcting of one workgroup over a CSR (off: n local offsets, the closing one is a) from
// the frontier cur[0, cnt[0]) (keys set, mark all ones, cnt[1] = 0, *stop = 0, a barrier
// passed): round r relaxes the arcs of the states whose key dropped in round r - 1; a state
// joins the next frontier once per round (stamp).  widx: arc k's weight is w[widx[k]] (the
// reverse CSR), or w[k].  Weights >= 0 need at most n rounds; false: beyond that, or past the
// deadline.
__device__ __forceinline__ bool prune_frontier(const uint32_t* off, const uint32_t* nbr,
                                               const uint32_t* widx, const double* w, uint32_t n,
                                               uint32_t a, unsigned long long* key, uint32_t* mark,
                                               uint32_t* cur, uint32_t* nxt, uint32_t* cnt,
                                               uint32_t* stop, unsigned long long deadline) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t r = 0;; ++r) {
    const uint32_t fsize = min(cnt[r & 1], n);
    const uint32_t halted = *stop;
    __syncthreads();  // every thread has read the round's words before thread 0 writes them
    if (fsize == 0 || halted) break;
    if (tid == 0) {
      cnt[(r + 1) & 1] = 0;
      if (r > n || ((r & 63u) == 63u && __builtin_amdgcn_s_memrealtime() > deadline)) *stop = 1;
    }
    __syncthreads();
    uint32_t* const push = &cnt[(r + 1) & 1];
    for (uint32_t q = tid; q < fsize; q += kPruneWG) {
      const uint32_t s = prune_ld(&cur[q]);
      if (s >= n) continue;
      const double ds = from_pkey(prune_ld(&key[s]));
      uint32_t e = s + 1 < n ? off[s + 1] : a;
      e = e < a ? e : a;
      for (uint32_t k = off[s]; k < e; ++k) {
        const uint32_t x = nbr[k];
        if (x >= n) continue;
        const uint32_t wk = widx ? widx[k] : k;
        const unsigned long long v = pkey(ds + w[wk]);
        if (v < atomicMin(&key[x], v) && atomicExch(&mark[x], r) != r) {
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
  const bool ok = *stop == 0;
  __syncthreads();
  return ok;
}

// ---- frontier tier: one workgroup per listed item, label correcting in both directions ------
// Forward from the start on the item's own CSR; then the item's reverse CSR in the workspace
// (lattice_trim_linear_kernel's: in-degrees by atomicAdd, a workgroup scan, sources and arc
// indices filled by a cursor per state) and backward from every final state on it.  An item
// past its bounds ends INTERNAL with the empty FST.
__global__ void __launch_bounds__(kPruneWG) lattice_prune_frontier_kernel(LatPruneDev p) {
  __shared__ uint32_t cnt[2];
  __shared__ uint32_t stop;
  __shared__ uint32_t scan_ws[kPruneWG / 64];
  __shared__ unsigned long long sh_best;
  const uint32_t tid = threadIdx.x;
  const uint32_t count = p.ctr[kPrCtrList];
  const unsigned long long kinf = pkey(prune_inf());
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = p.list[li];
    const PruneItem it = prune_item(p, si);
    if (it.start >= it.n) continue;  // (the wave tier lists no such item)
    const uint32_t n = it.n, a = it.a;
    unsigned long long* kf = p.key + 2 * it.sb;
    unsigned long long* kb = kf + n;
    uint32_t* mark = p.mark + it.sb;
    uint32_t* fa = p.fa + it.sb;
    uint32_t* fb = p.fb + it.sb;
    uint32_t* roff = p.roff + it.sb;
    uint32_t* rcur = p.rcur + it.sb;
    uint32_t* rsrc = p.rsrc + it.ab;
    uint32_t* rarc = p.rarc + it.ab;
    const unsigned long long deadline = __builtin_amdgcn_s_memrealtime() + p.wd_ticks;
    // forward
    for (uint32_t s = tid; s < n; s += kPruneWG) {
      kf[s] = s == it.start ? pkey(0.0) : kinf;
      mark[s] = ~0u;
      roff[s] = 0;
    }
    if (tid == 0) {
      fa[0] = it.start;
      cnt[0] = 1;
      cnt[1] = 0;
      stop = 0;
    }
    __syncthreads();
    bool ok = prune_frontier(it.aoff, it.next, nullptr, it.w, n, a, kf, mark, fa, fb, cnt, &stop,
                             deadline);
    // the reverse CSR
    for (uint32_t k = tid; k < a; k += kPruneWG) {
      const uint32_t u = it.next[k];
      if (u < n) atomicAdd(&roff[u], 1u);
    }
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t c = 0; c < n; c += kPruneWG) {
      const uint32_t s = c + tid;
      // (an atomic load: the counts were made by atomics, which a plain load may not see)
      const uint32_t d = s < n ? prune_ld(&roff[s]) : 0u;
      uint32_t tot = 0;
      const uint32_t ex = block_excl_scan<kPruneWG>(d, scan_ws, tot);
      if (s < n) {
        roff[s] = base + ex;
        rcur[s] = base + ex;
      }
      base += tot;
    }
    const uint32_t ra = base < a ? base : a;  // arcs with a target inside the item
    __syncthreads();
    for (uint32_t s = tid; s < n; s += kPruneWG) {
      uint32_t a0, a1;
      prune_arc_range(it, s, &a0, &a1);
      for (uint32_t k = a0; k < a1; ++k) {
        const uint32_t u = it.next[k];
        if (u >= n) continue;
        const uint32_t q = atomicAdd(&rcur[u], 1u);
        if (q < ra) {
          rsrc[q] = s;
          rarc[q] = k;
        }
      }
    }
    // backward: every final state is a source
    if (tid == 0) {
      cnt[0] = cnt[1] = 0;
      stop = 0;
    }
    __syncthreads();
    for (uint32_t s = tid; s < n; s += kPruneWG) {
      const double f = it.fin[s];
      const bool fin = prune_is_final(f);
      kb[s] = fin ? pkey(f) : kinf;
      mark[s] = ~0u;
      if (fin) {
        const uint32_t q = atomicAdd(&cnt[0], 1u);
        if (q < n) fa[q] = s;
      }
    }
    __syncthreads();
    ok = prune_frontier(roff, rsrc, rarc, it.w, n, ra, kb, mark, fa, fb, cnt, &stop, deadline) &&
         ok;
    if (ok) {
      prune_mark<kPruneWG>(p, it, si, kf, kb, &sh_best);
    } else {
      prune_write_empty(p, it, si, kPathInternal);
    }
    if (tid == 0) atomicAdd(&p.ctr[kPrCtrFrontier], 1u);
    __syncthreads();  // (the shared words are the next item's)
  }
}

}  // namespace fstamd

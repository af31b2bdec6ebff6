// lattice_posterior.hpp -- arc posteriors of every item of an lhs batch, on the device
// (fst_posterior_lhs_batch / fst_device_posterior_lhs; the definition is the entry's comment in
// include/fst_batch.h, the argument in DESIGN.md §7l).  Forward and backward sums in the log
// semiring (weight.zig's LogWeight.plus), the total mass, and per arc the share of it that runs
// through the arc, as -log.  An item is its LhsDesc over the batch's concatenated CSR, read in
// place; the helpers that are the n-best's (nb_item, nb_scan, nb_sync, nb_ld) are used from
// lattice_nbest.hpp as they stand.  Per item, one code for both tiers (post_item):
//   0 weights   a NaN or -inf arc or final weight anywhere in the item: UNSUPPORTED.
//   1 depth     as the n-best's: depth(t) = max depth(s) + 1 by relaxation; a depth that would
//               reach the state count is a cycle: UNSUPPORTED.
//   2 reverse   in-arcs of the reached states (count, scan, fill) and the reached states in
//               order of depth, as the n-best's.
//   3 sort      the fill's atomics leave a segment in the order the hardware gave; the forward
//               fold is defined in increasing arc index, so every in-arc segment is sorted: by
//               its state's lane up to kPostLaneSort arcs (insertion; a fill is nearly in
//               order), by the whole wave or workgroup above (a bitonic network in place, so a
//               state of hundreds of in-arcs costs no lane a quadratic loop).
//   4 forward   level by level, one lane per state: alpha(t) folds logadd over the sorted
//               in-arcs.
//   5 backward  by descending level, one lane per state: beta(s) folds logadd from final(s)
//               over the CSR out-arcs.
//   6 write     one lane per arc: arc_cost; lanes over states: alpha and beta (when asked for).
// The tables (32 B per state: alpha and beta as f64, depth, in-arc offset, level offset, order;
// 8 B per arc: in-arc index, source) sit in LDS for the items they fit (one wave per item) and
// in a workspace indexed by the item's bases otherwise (one workgroup per item).  Words another
// thread wrote are read after a barrier, in the workspace with ld_agent (nb_ld, nb_sync).
// Every loop is bounded: the depth rounds and the levels by the state count and the deadline,
// the sorts by the segment's length.  Every index read from a table is checked before use.
// The fold order is fixed, so both tiers give the same bytes.
#pragma once
#define FSTAMD_NBEST_NO_KERNELS  // (its helpers alone)
#include "lattice_nbest.hpp"

namespace fstamd {

constexpr uint32_t kPostLaneSort = 32;  // in-arc segments up to here are sorted by one lane
constexpr unsigned long long kPostInfBits = 0x7FF0000000000000ull;

// One item's tables: slices of LDS or of the workspace.
struct PostTables {
  unsigned long long* alpha;  // [S] the bits of the f64
  unsigned long long* beta;   // [S]
  uint32_t* depth;            // [S] depth + 1; 0: not reached
  uint32_t* roff;             // [S] in-arc counts, then offsets, after the fill the ends
  uint32_t* lvl;              // [S] the same three for the states of each depth
  uint32_t* order;            // [S] reached states by depth
  uint32_t* rarc;             // [A] in-arcs by target, after the sort by arc index
  uint32_t* asrc;             // [A] the source of an arc of a reached state, else kNoState
};

struct PostShared : NbShared {
  unsigned long long mask[kNbWG / 64];  // per wave: the states of a chunk with a wide segment
  uint32_t bad;                         // a weight, or a sum, that makes the item UNSUPPORTED
};

__device__ __forceinline__ double post_f64(unsigned long long b) {
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ unsigned long long post_bits(double v) {
  return (unsigned long long)__double_as_longlong(v);
}
// NaN or -inf
__device__ __forceinline__ bool post_bad(double v) { return !(v > -__builtin_huge_val()); }

// LogWeight.plus with isZero's shortcut (weight.zig:67-91), in the entry comment's words.
__device__ __forceinline__ double post_logadd(double x, double y) {
  if (nb_is_zero(x)) return y;
  if (nb_is_zero(y)) return x;
  const double m = x < y ? x : y, M = x < y ? y : x;
  return m - log1p(exp(-(M - m)));
}

// A non-OK item: +inf in every entry of its ranges (a refused item has none), its status.
template <int WG>
__device__ __forceinline__ void post_fail(const LatPostDev& p, const NbItem& it, uint32_t si,
                                          int32_t st) {
  const double inf = __builtin_huge_val();
  for (uint32_t s = threadIdx.x; s < it.S; s += WG) {
    if (p.alpha) p.alpha[it.sb + s] = inf;
    if (p.beta) p.beta[it.sb + s] = inf;
  }
  for (uint32_t a = threadIdx.x; a < it.A; a += WG) p.arc_cost[it.ab + a] = inf;
  if (threadIdx.x == 0) {
    p.total[si] = inf;
    p.status[si] = st;
  }
}

// The statuses that need no traversal, as nb_precheck (an item the prepare kernel refused has no
// states, a harmless start and the NaN flag: only its status and total are written).
template <int WG>
__device__ __forceinline__ bool post_precheck(const LatPostDev& p, const NbItem& it,
                                              uint32_t si) {
  int32_t st = kPathOk;
  if (it.start == kNoState) st = kPathEmpty;
  else if (it.flags & kLhsNaN) st = kPathUnsupported;
  else if (it.start >= it.S) st = kPathEmpty;  // (no validated item has such a start)
  if (st == kPathOk) return false;
  post_fail<WG>(p, it, si, st);
  return true;
}

// seg[0 .. n) into increasing order by one lane.  The words are the fill's (other lanes', read
// behind the barrier) until the lane has moved them; in the workspace the lane's own stores of
// one pass are waited for before the next pass reads them back.
template <bool kLds>
__device__ __forceinline__ void post_lane_sort(uint32_t* seg, uint32_t n) {
  for (uint32_t i = 1; i < n; ++i) {
    const uint32_t x = nb_ld<kLds>(&seg[i]);
    uint32_t j = i;
    while (j > 0) {
      const uint32_t y = nb_ld<kLds>(&seg[j - 1]);
      if (y <= x) break;
      seg[j] = y;
      --j;
    }
    if (j != i) {
      seg[j] = x;
      if constexpr (!kLds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
}

// seg[0 .. n) into increasing order by the whole workgroup (every thread calls, n uniform): a
// bitonic network over the next power of two in place.  Every compare puts the smaller word at
// the lower index, so the padding (index >= n, read as above every word) never moves and a pair
// that reaches into it is skipped.  A step touches every word from one thread only.
template <int WG, bool kLds>
__device__ __forceinline__ void post_wide_sort(uint32_t* seg, uint32_t n) {
  unsigned long long P = 1;
  while (P < n) P <<= 1;
  const uint32_t half = (uint32_t)(P >> 1);
  for (unsigned long long k = 2; k <= P; k <<= 1) {
    for (uint32_t j = (uint32_t)(k >> 1); j > 0; j >>= 1) {
      const bool flip = j == (uint32_t)(k >> 1);  // the first step of a merge mirrors the block
      for (uint32_t idx = threadIdx.x; idx < half; idx += WG) {
        const uint32_t off = idx & (j - 1);
        const unsigned long long lo = 2ull * (idx - off) + off;
        const unsigned long long hi = flip ? 2ull * (idx - off) + (2ull * j - 1 - off) : lo + j;
        if (hi >= n) continue;
        const uint32_t x = nb_ld<kLds>(&seg[lo]), y = nb_ld<kLds>(&seg[hi]);
        if (x > y) {
          seg[lo] = y;
          seg[hi] = x;
        }
      }
      nb_sync<kLds>();
    }
  }
}

// One item, by the whole workgroup (every thread calls; SH and T are the item's).
template <int WG, bool kLds>
__device__ __forceinline__ void post_item(const LatPostDev& p, const NbItem& it,
                                          const PostTables& T, uint32_t si, PostShared& SH,
                                          unsigned long long deadline) {
  const uint32_t tid = threadIdx.x, S = it.S, A = it.A;
  const double inf = __builtin_huge_val();
  // ---- 0: the tables' first words; the weights ---------------------------------------------
  uint32_t bad = 0;
  for (uint32_t s = tid; s < S; s += WG) {
    T.alpha[s] = kPostInfBits;
    T.beta[s] = kPostInfBits;
    T.depth[s] = s == it.start ? 1u : 0u;
    T.roff[s] = 0;
    T.lvl[s] = 0;
    if (post_bad(it.fin[s])) bad = 1;
  }
  for (uint32_t a = tid; a < A; a += WG) {
    T.asrc[a] = kNoState;
    if (post_bad(it.aw[a])) bad = 1;
  }
  if (tid == 0) {
    SH.flag[0] = 0;
    SH.flag[1] = 0;
    SH.stop = 0;
    SH.bad = 0;
  }
  nb_sync<kLds>();
  if (bad) atomicOr(&SH.bad, 1u);
  nb_sync<kLds>();
  if (SH.bad) return post_fail<WG>(p, it, si, kPathUnsupported);
  bad = 0;
  // ---- 1: depth (the n-best's rounds) -------------------------------------------------------
  for (uint32_t round = 0;; ++round) {
    // (the other word: its readers left it before the last barrier of the round before)
    if (tid == 0) SH.flag[(round + 1) & 1] = 0;
    uint32_t f = 0;
    for (uint32_t s = tid; s < S; s += WG) {
      const uint32_t d = nb_ld<kLds>(&T.depth[s]);
      if (!d) continue;
      const uint32_t a0 = it.aoff[s];
      uint32_t a1 = it.aoff[s + 1];
      a1 = a1 < A ? a1 : A;
      for (uint32_t a = a0; a < a1; ++a) {
        const uint32_t x = it.anext[a];
        if (x >= S) continue;
        if (d >= S) f |= 2u;  // a path of S arcs from the start: a cycle
        else if (atomicMax(&T.depth[x], d + 1) < d + 1) f |= 1u;
      }
    }
    if (tid == 0 && (round > S || ((round & 15u) == 15u &&
                                   __builtin_amdgcn_s_memrealtime() > deadline)))
      f |= 4u;
    if (f) atomicOr(&SH.flag[round & 1], f);
    nb_sync<kLds>();
    f = SH.flag[round & 1];
    nb_sync<kLds>();  // every thread has read the word before thread 0 clears it again
    if (f & 2u) return post_fail<WG>(p, it, si, kPathUnsupported);
    if (f & 4u) return post_fail<WG>(p, it, si, kPathInternal);
    if (!(f & 1u)) break;
  }
  // ---- 2: in-arcs by target, reached states by depth ----------------------------------------
  for (uint32_t s = tid; s < S; s += WG) {
    const uint32_t d = nb_ld<kLds>(&T.depth[s]);
    if (!d || d > S) continue;
    atomicAdd(&T.lvl[d - 1], 1u);
    const uint32_t a0 = it.aoff[s];
    uint32_t a1 = it.aoff[s + 1];
    a1 = a1 < A ? a1 : A;
    for (uint32_t a = a0; a < a1; ++a) {
      const uint32_t x = it.anext[a];
      if (x >= S) continue;
      T.asrc[a] = s;
      atomicAdd(&T.roff[x], 1u);
    }
  }
  nb_sync<kLds>();
  nb_scan<WG, kLds>(T.roff, S, SH);
  nb_scan<WG, kLds>(T.lvl, S, SH);
  nb_sync<kLds>();
  for (uint32_t s = tid; s < S; s += WG) {
    const uint32_t d = nb_ld<kLds>(&T.depth[s]);
    if (!d || d > S) continue;
    const uint32_t o = atomicAdd(&T.lvl[d - 1], 1u);
    if (o < S) T.order[o] = s;
    const uint32_t a0 = it.aoff[s];
    uint32_t a1 = it.aoff[s + 1];
    a1 = a1 < A ? a1 : A;
    for (uint32_t a = a0; a < a1; ++a) {
      const uint32_t x = it.anext[a];
      if (x >= S) continue;
      const uint32_t q = atomicAdd(&T.roff[x], 1u);
      if (q < A) T.rarc[q] = a;
    }
  }
  nb_sync<kLds>();
  // ---- 3: every in-arc segment by arc index (roff[t] is now the end of t's segment) ---------
  for (uint32_t base = 0; base < S; base += WG) {
    const uint32_t t = base + tid;
    uint32_t q0 = 0, q1 = 0;
    if (t < S) {
      q0 = t ? nb_ld<kLds>(&T.roff[t - 1]) : 0u;
      q1 = nb_ld<kLds>(&T.roff[t]);
      q1 = q1 < A ? q1 : A;
    }
    const uint32_t n = q1 > q0 ? q1 - q0 : 0u;
    if (n > 1 && n <= kPostLaneSort) post_lane_sort<kLds>(T.rarc + q0, n);
    const unsigned long long wide = __ballot(n > kPostLaneSort);
    if ((tid & 63u) == 0) SH.mask[tid >> 6] = wide;
    __syncthreads();
    for (uint32_t w = 0; w < WG / 64; ++w) {
      const unsigned long long m = SH.mask[w];
      // (the same word in every thread)
      unsigned long long mm =
          ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32))
           << 32) |
          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
      while (mm) {
        const uint32_t tw = base + w * 64 + (uint32_t)__builtin_ctzll(mm);
        mm &= mm - 1;
        const uint32_t w0 = tw ? nb_ld<kLds>(&T.roff[tw - 1]) : 0u;
        uint32_t w1 = nb_ld<kLds>(&T.roff[tw]);
        w1 = w1 < A ? w1 : A;
        if (w1 > w0) post_wide_sort<WG, kLds>(T.rarc + w0, w1 - w0);
      }
    }
    __syncthreads();  // (the masks are the next chunk's)
  }
  nb_sync<kLds>();
  // ---- 4: forward, level by level (lvl[d] is now the end of level d) ------------------------
  uint32_t levels = 0;
  for (uint32_t d = 0; d < S; ++d) {
    const uint32_t lo = d ? nb_ld<kLds>(&T.lvl[d - 1]) : 0u;
    uint32_t hi = nb_ld<kLds>(&T.lvl[d]);
    hi = hi < S ? hi : S;
    if (hi <= lo) break;  // (the same words in every thread: levels are contiguous)
    if ((d & 63u) == 63u) {
      if (tid == 0 && __builtin_amdgcn_s_memrealtime() > deadline) SH.stop = 1;
      nb_sync<kLds>();
      if (SH.stop) return post_fail<WG>(p, it, si, kPathInternal);
    }
    for (uint32_t i = lo + tid; i < hi; i += WG) {
      const uint32_t t = nb_ld<kLds>(&T.order[i]);
      if (t >= S) continue;
      double acc = 0.0;
      if (t != it.start) {
        acc = inf;
        const uint32_t q0 = t ? nb_ld<kLds>(&T.roff[t - 1]) : 0u;
        uint32_t q1 = nb_ld<kLds>(&T.roff[t]);
        q1 = q1 < A ? q1 : A;
        for (uint32_t q = q0; q < q1; ++q) {
          const uint32_t a = nb_ld<kLds>(&T.rarc[q]);
          if (a >= A) continue;
          const uint32_t s = nb_ld<kLds>(&T.asrc[a]);
          if (s >= S) continue;
          acc = post_logadd(acc, post_f64(nb_ld<kLds>(&T.alpha[s])) + it.aw[a]);
        }
      }
      if (post_bad(acc)) bad = 1;  // (a term of -inf leaves the sum -inf or NaN)
      T.alpha[t] = post_bits(acc);
    }
    nb_sync<kLds>();
    levels = d + 1;
  }
  // ---- 5: backward, by descending level ------------------------------------------------------
  for (uint32_t d = levels; d-- > 0;) {
    const uint32_t lo = d ? nb_ld<kLds>(&T.lvl[d - 1]) : 0u;
    uint32_t hi = nb_ld<kLds>(&T.lvl[d]);
    hi = hi < S ? hi : S;
    if ((d & 63u) == 63u) {
      if (tid == 0 && __builtin_amdgcn_s_memrealtime() > deadline) SH.stop = 1;
      nb_sync<kLds>();
      if (SH.stop) return post_fail<WG>(p, it, si, kPathInternal);
    }
    for (uint32_t i = lo + tid; i < hi; i += WG) {
      const uint32_t s = nb_ld<kLds>(&T.order[i]);
      if (s >= S) continue;
      double acc = it.fin[s];
      const uint32_t a0 = it.aoff[s];
      uint32_t a1 = it.aoff[s + 1];
      a1 = a1 < A ? a1 : A;
      for (uint32_t a = a0; a < a1; ++a) {
        const uint32_t x = it.anext[a];
        if (x >= S) continue;
        acc = post_logadd(acc, it.aw[a] + post_f64(nb_ld<kLds>(&T.beta[x])));
      }
      if (post_bad(acc)) bad = 1;
      T.beta[s] = post_bits(acc);
    }
    nb_sync<kLds>();
  }
  if (bad) atomicOr(&SH.bad, 1u);
  nb_sync<kLds>();
  if (SH.bad) return post_fail<WG>(p, it, si, kPathUnsupported);
  // ---- 6: the total, the arcs, the states -----------------------------------------------------
  const double total = post_f64(nb_ld<kLds>(&T.beta[it.start]));
  if (nb_is_zero(total)) return post_fail<WG>(p, it, si, kPathEmpty);
  for (uint32_t a = tid; a < A; a += WG) {
    const uint32_t s = nb_ld<kLds>(&T.asrc[a]), x = it.anext[a];
    double c = inf;
    if (s < S && x < S)
      c = ((post_f64(nb_ld<kLds>(&T.alpha[s])) + it.aw[a]) + post_f64(nb_ld<kLds>(&T.beta[x]))) -
          total;
    p.arc_cost[it.ab + a] = c;
  }
  if (p.alpha)  // (uniform)
    for (uint32_t s = tid; s < S; s += WG) p.alpha[it.sb + s] = post_f64(nb_ld<kLds>(&T.alpha[s]));
  if (p.beta)
    for (uint32_t s = tid; s < S; s += WG) p.beta[it.sb + s] = post_f64(nb_ld<kLds>(&T.beta[s]));
  if (tid == 0) {
    p.total[si] = total;
    p.status[si] = kPathOk;
  }
}

// The LDS an item's tables take: 32 B per state, 8 B per arc.
__host__ __device__ __forceinline__ unsigned long long post_lds_need(uint32_t S, uint32_t A) {
  return 32ull * S + 8ull * A;
}

// ---- wave tier: one wave per item, the tables in dynamic LDS of p.nb.lds_budget bytes -------
// An item whose tables do not fit is handed to the workgroup tier through p.nb.list.
__global__ void __launch_bounds__(64) lattice_posterior_lds_kernel(LatPostDev p, uint32_t count) {
  extern __shared__ __align__(16) unsigned char post_lds[];
  __shared__ PostShared SH;
  uint32_t done = 0;  // (one atomic per wave, not per item)
  for (uint32_t si = blockIdx.x; si < count; si += gridDim.x) {
    const NbItem it = nb_item(p.nb, si);
    if (post_precheck<64>(p, it, si)) {
      ++done;
      continue;
    }
    if (post_lds_need(it.S, it.A) > p.nb.lds_budget) {  // (uniform)
      if (threadIdx.x == 0) p.nb.list[atomicAdd(&p.nb.ctr[kNbCtrList], 1u)] = si;
      continue;
    }
    PostTables T;
    T.alpha = reinterpret_cast<unsigned long long*>(post_lds);
    T.beta = T.alpha + it.S;
    T.depth = reinterpret_cast<uint32_t*>(T.beta + it.S);
    T.roff = T.depth + it.S;
    T.lvl = T.roff + it.S;
    T.order = T.lvl + it.S;
    T.rarc = T.order + it.S;
    T.asrc = T.rarc + it.A;
    ++done;
    post_item<64, true>(p, it, T, si, SH, __builtin_amdgcn_s_memrealtime() + p.nb.wd_ticks);
    __syncthreads();  // (SH and the tables are the next item's)
  }
  if (threadIdx.x == 0 && done) atomicAdd(&p.nb.ctr[kNbCtrLds], done);
}

// ---- workgroup tier: one workgroup per listed item, the tables in the workspace --------------
// The item's slices: state words at state_base, arc words at arc_base.
__global__ void __launch_bounds__(kNbWG) lattice_posterior_hbm_kernel(LatPostDev p) {
  __shared__ PostShared SH;
  const uint32_t count = p.nb.ctr[kNbCtrList];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = p.nb.list[li];
    const NbItem it = nb_item(p.nb, si);
    if (it.start >= it.S) continue;  // (the wave tier lists no such item)
    PostTables T;
    T.alpha = p.nb.eg + it.sb;
    T.beta = p.nb.ear + it.sb;
    T.depth = p.nb.depth + it.sb;
    T.roff = p.nb.roff + it.sb;
    T.lvl = p.nb.lvl + it.sb;
    T.order = p.nb.order + it.sb;
    T.rarc = p.nb.rarc + it.ab;
    T.asrc = p.nb.asrc + it.ab;
    post_item<kNbWG, false>(p, it, T, si, SH, __builtin_amdgcn_s_memrealtime() + p.nb.wd_ticks);
    if (threadIdx.x == 0) atomicAdd(&p.nb.ctr[kNbCtrHbm], 1u);
    __syncthreads();  // (SH is the next item's)
  }
}

}  // namespace fstamd

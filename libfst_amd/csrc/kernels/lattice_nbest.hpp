// lattice_nbest.hpp -- the n best distinct paths of every item of an lhs batch, on the device
// (fst_nbest_lhs_batch / fst_device_nbest_lhs; the contract is in include/fst_batch.h, the
// argument in DESIGN.md §7i).  An item is its LhsDesc over the batch's concatenated CSR, read in
// place, as in lattice_sp.hpp.  Per item, one code for both tiers (nbest_item):
//   1 depth     depth(start) = 0, depth(t) = max depth(s) + 1 over every arc from a reached
//               state, by relaxation (atomicMax) until nothing changes.  A depth that would
//               reach the state count is a cycle: UNSUPPORTED.  That bounds the rounds too.
//   2 reverse   in-arcs of the reached states (count, scan, fill) and the reached states in
//               order of depth (the same three steps on the depth histogram).
//   3 lists     level by level, one lane per state: E(t) = the n smallest (g, a, r) over the
//               in-arcs a and the ranks r of E(src(a)), kept sorted by bounded insertion.  A
//               source list rises in (g, a, r), so an arc is left at its first candidate that
//               does not make the list (or that overflowed to +inf).
//   4 select    n rounds, each the least (total, t, r) above the round before; then lanes
//               0 .. n-1 of the first wave walk their path back through (a, r), the item's
//               arena space is reserved with one atomic, and the arcs are written forward.
// The tables (16 B per list entry, five words per state, two per arc) sit in LDS for the items
// they fit (one wave per item) and in a workspace indexed by the item's bases otherwise (one
// workgroup per item).  Words another thread wrote are read after a barrier, in the workspace
// with ld_agent as the frontier tier of lattice_sp.hpp reads its own.
// Every loop is bounded: the depth rounds by the state count, the levels likewise, both by the
// deadline; walks by the state count.  Every index read from a table is checked before use.
//
// kUnique (fst_nbest_unique_lhs_batch / fst_device_nbest_unique_lhs): the n best
// paths with pairwise different OUTPUT TEXTS (the non-epsilon olabels).  A third word per list
// entry, eh, holds a 64-bit hash of the prefix's text; a list keeps per text only its least
// prefix (nb_pull), the selection passes over a winner whose text was chosen before.  Different
// hashes mean different texts; equal hashes are confirmed label by label (nb_same_text), so the
// result does not depend on the hash (FSTAMD_NBEST_HASH_MASK).  The tables are then 24 B per
// list entry.  The plain instances hold none of this.
#pragma once
#include "eager_bfs.hpp"

namespace fstamd {

constexpr int kNbWG = 256;              // the HBM tier: one workgroup per item
constexpr uint32_t kNbNoArc = ~0u;      // the empty prefix has no last arc

struct NbItem {
  const uint32_t* aoff;
  const double* fin;
  const uint32_t* anext;
  const uint32_t* ail;
  const uint32_t* aol;
  const double* aw;
  uint64_t sb, ab;
  uint32_t S, A, start, flags;
};

__device__ __forceinline__ NbItem nb_item(const LatNbestDev& p, uint32_t si) {
  const uint4* q = reinterpret_cast<const uint4*>(p.desc + si);
  const uint4 x = q[0], y = q[1];
  const auto sgpr = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  NbItem it;
  it.sb = ((uint64_t)sgpr(x.y) << 32) | sgpr(x.x);
  it.ab = ((uint64_t)sgpr(x.w) << 32) | sgpr(x.z);
  it.S = sgpr(y.x);
  it.start = sgpr(y.y);
  it.A = sgpr(y.z);
  it.flags = sgpr(y.w);
  // (item i's offset words start i words on: one closing word per earlier item)
  it.aoff = p.state_off + it.sb + sgpr(si);
  it.fin = p.final_w + it.sb;
  it.anext = p.arc_next + it.ab;
  it.ail = p.arc_il + it.ab;
  it.aol = p.arc_ol + it.ab;
  it.aw = p.arc_w + it.ab;
  return it;
}

// One item's tables: slices of LDS or of the workspace.
struct NbTables {
  unsigned long long* eg;   // [S * n] the cost of list entry r of state t at t * n + r
  unsigned long long* ear;  // [S * n] (last arc << 32) | rank of the rest in E(src)
  unsigned long long* eh;   // [S * n] kUnique: the hash of the prefix's output text
  uint32_t* depth;          // [S] depth + 1; 0: not reached
  uint32_t* roff;           // [S] in-arc counts, then offsets, after the fill the ends
  uint32_t* cnt;            // [S] entries in E(t)
  uint32_t* lvl;            // [S] the same three for the states of each depth
  uint32_t* order;          // [S] reached states by depth
  uint32_t* rarc;           // [A] in-arcs by target
  uint32_t* asrc;           // [A] the source of an arc of a reached state
};

struct NbShared {
  uint32_t flag[2];
  uint32_t stop;
  uint32_t scan[kNbWG / 64];
  unsigned long long red[kNbWG / 64];
  unsigned long long sel[kNbestMax];
};
// kUnique: the hashes of the texts chosen so far, beside their (t, r) in sel.
struct NbSharedUnique : NbShared {
  unsigned long long selh[kNbestMax];
};

template <bool kLds, class T>
__device__ __forceinline__ T nb_ld(const T* p) {
  if constexpr (kLds) return *p;
  else return ld_agent(p);
}

// The barrier between two phases of an item.  The workspace's words are read by the other waves
// of the workgroup with agent-scope loads, which go to the L2 the workgroup's own stores were
// written through to: the stores before the barrier are waited for first (a workgroup-scope
// barrier alone does not wait for them; an agent-scope release fence does, but with its L2
// write-back the 65,536 tagger lattices took 20.0 ms at n = 8 against 7.1 ms with the wait
// alone, profiles/lattice_nbest).
template <bool kLds>
__device__ __forceinline__ void nb_sync() {
  if constexpr (!kLds) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Order-preserving u64 of any non-NaN double, -0.0 with +0.0.
__device__ __forceinline__ unsigned long long nb_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ bool nb_is_zero(double v) { return v == __builtin_huge_val(); }

template <int WG>
__device__ __forceinline__ unsigned long long nb_block_min(unsigned long long v, NbShared& SH) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(v, o, 64);
    v = y < v ? y : v;
  }
  if constexpr (WG == 64) {
    return v;
  } else {
    if ((threadIdx.x & 63) == 0) SH.red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = SH.red[0];
#pragma unroll
    for (int i = 1; i < WG / 64; ++i) m = SH.red[i] < m ? SH.red[i] : m;
    __syncthreads();
    return m;
  }
}

// Exclusive scan of p[0 .. S) in place, in chunks of the workgroup.
template <int WG, bool kLds>
__device__ __forceinline__ void nb_scan(uint32_t* p, uint32_t S, NbShared& SH) {
  uint32_t run = 0;
  for (uint32_t base = 0; base < S; base += WG) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < S ? nb_ld<kLds>(&p[i]) : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan<WG>(v, SH.scan, tot);
    if (i < S) p[i] = run + ex;
    run += tot;
  }
}

// The same status for the item's n strings.
template <int WG>
__device__ __forceinline__ void nb_status(const BatchOutDev& out, uint32_t si, uint32_t n,
                                          int32_t st, const NbItem& it) {
  for (uint32_t k = threadIdx.x; k < n; k += WG) write_status(out, si * n + k, st, it.S, it.A);
}

// The statuses that need no traversal, in the contract's order (an item the prepare kernel
// refused has no states, a harmless start and the NaN flag).  True: the item is finished.
template <int WG>
__device__ __forceinline__ bool nb_precheck(const NbItem& it, uint32_t n, const BatchOutDev& out,
                                            uint32_t si) {
  int32_t st = kPathOk;
  if (it.start == kNoState) st = kPathEmpty;
  else if (it.flags & kLhsNaN) st = kPathUnsupported;
  else if (it.start >= it.S) st = kPathEmpty;  // (no validated item has such a start)
  if (st == kPathOk) return false;
  nb_status<WG>(out, si, n, st, it);
  return true;
}

// (g, ar) before (pg, par): the order of two list entries
__device__ __forceinline__ bool nb_less(double g, unsigned long long ar, double pg,
                                        unsigned long long par) {
  return g < pg || (g == pg && ar < par);
}

// ---- kUnique: the output text of a prefix ---------------------------------------------------
constexpr unsigned long long kNbHashSeed = 0x9E3779B97F4A7C15ull;  // the empty text

// The hash of a text with one more label (the result never depends on it: nb_same_text).
__device__ __forceinline__ unsigned long long nb_mix(unsigned long long h, uint32_t label,
                                                     unsigned long long mask) {
  h = (h ^ label) * 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  return (h ^ (h >> 29)) & mask;
}

// One step of a walk back through a prefix: from list entry (s, r) to the entry of its rest,
// over every arc of an epsilon olabel.  Returns the next label of the text, read backwards, or
// 0 at the empty prefix ((s, r) is then the start's entry).  steps counts the arcs taken: a
// prefix has fewer than the item has states.
template <bool kLds>
__device__ __forceinline__ uint32_t nb_text_back(const NbItem& it, const NbTables& T, uint32_t n,
                                                 uint32_t& s, uint32_t& r, uint32_t& steps,
                                                 bool& bad) {
  for (;;) {
    const unsigned long long ar = nb_ld<kLds>(&T.ear[(size_t)s * n + r]);
    const uint32_t a = (uint32_t)(ar >> 32);
    if (a == kNbNoArc) return 0;
    r = (uint32_t)ar;
    if (a >= it.A || r >= n || ++steps >= it.S) break;
    s = nb_ld<kLds>(&T.asrc[a]);
    if (s >= it.S) break;
    const uint32_t l = it.aol[a];
    if (l) return l;
  }
  bad = true;
  return 0;
}

// Whether two prefixes print the same text.  A prefix is a list entry (s, r) with s < S and
// r < n, plus one pending label in front of it (0: none), which is how a candidate that is in no
// list yet is given: its last arc's olabel and its source entry.  The texts are compared from
// their ends; they are equal if both walks reach the empty prefix together, or meet in one
// entry with nothing pending.  `bad`: a walk broke its bound or read a bad index.
template <bool kLds>
__device__ __forceinline__ bool nb_same_text(const NbItem& it, const NbTables& T, uint32_t n,
                                             uint32_t la, uint32_t sa, uint32_t ra, uint32_t lb,
                                             uint32_t sb, uint32_t rb, bool& bad) {
  uint32_t na = 0, nb = 0;
  for (;;) {
    if (!la && !lb && sa == sb && ra == rb) return true;
    if (!la) la = nb_text_back<kLds>(it, T, n, sa, ra, na, bad);
    if (!lb) lb = nb_text_back<kLds>(it, T, n, sb, rb, nb, bad);
    if (bad || la != lb) return false;
    if (!la) return true;  // both at the empty prefix
    la = lb = 0;
  }
}

// E(t) of one state, by one lane: see the file comment.  kUnique: Eu(t), the at most n least
// prefixes with pairwise different texts; a candidate whose text the list holds takes that
// entry's place if it comes before it and is passed over otherwise.  False: a walk broke.
template <bool kLds, bool kUnique>
__device__ __forceinline__ bool nb_pull(const NbItem& it, const NbTables& T, uint32_t n,
                                        uint32_t t, unsigned long long hmask) {
  const size_t eb = (size_t)t * n;
  uint32_t c = 0;
  bool bad = false;
  if (t == it.start) {
    T.eg[eb] = (unsigned long long)__double_as_longlong(0.0);
    T.ear[eb] = (unsigned long long)kNbNoArc << 32;
    if constexpr (kUnique) T.eh[eb] = kNbHashSeed & hmask;
    c = 1;
  } else {
    const uint32_t q0 = t ? nb_ld<kLds>(&T.roff[t - 1]) : 0u;
    uint32_t q1 = nb_ld<kLds>(&T.roff[t]);
    q1 = q1 < it.A ? q1 : it.A;
    for (uint32_t q = q0; q < q1; ++q) {
      const uint32_t a = nb_ld<kLds>(&T.rarc[q]);
      if (a >= it.A) continue;
      const double w = it.aw[a];
      if (nb_is_zero(w)) continue;  // an arc of +inf is never part of a path
      const uint32_t s = nb_ld<kLds>(&T.asrc[a]);
      if (s >= it.S) continue;
      uint32_t cs = nb_ld<kLds>(&T.cnt[s]);
      cs = cs < n ? cs : n;
      const size_t sbs = (size_t)s * n;
      uint32_t ol = 0;
      if constexpr (kUnique) ol = it.aol[a];
      for (uint32_t r = 0; r < cs; ++r) {
        const double g = __longlong_as_double((long long)nb_ld<kLds>(&T.eg[sbs + r])) + w;
        if (nb_is_zero(g)) break;  // (the rest of the source list costs no less)
        const unsigned long long ar = ((unsigned long long)a << 32) | r;
        [[maybe_unused]] const bool full = c == n;
        uint32_t pos;
        if (c == n) {  // full: the candidate replaces the last entry or the arc is done
          pos = n - 1;
          if (!nb_less(g, ar, __longlong_as_double((long long)T.eg[eb + pos]), T.ear[eb + pos]))
            break;
        } else {
          pos = c++;
        }
        [[maybe_unused]] unsigned long long h = 0;
        if constexpr (kUnique) {
          h = nb_ld<kLds>(&T.eh[sbs + r]);
          if (ol) h = nb_mix(h, ol, hmask);
          // the entry of the same text, if the list holds one (entries 0 .. have - 1)
          const uint32_t have = full ? n : pos;
          uint32_t twin = have;
          for (uint32_t j = 0; j < have && !bad; ++j) {
            if (T.eh[eb + j] != h) continue;
            if (nb_same_text<kLds>(it, T, n, ol, s, r, 0u, t, j, bad)) {
              twin = j;
              break;
            }
          }
          if (bad) {
            if (!full) --c;
            break;
          }
          if (twin < have) {
            if (!full) --c;  // (the list does not grow)
            if (!nb_less(g, ar, __longlong_as_double((long long)T.eg[eb + twin]),
                         T.ear[eb + twin]))
              continue;  // the twin is before the candidate: on to the next rank
            pos = twin;  // the candidate takes its place
          }
        }
        // (the lane's own list: its own stores, read back in program order)
        while (pos > 0) {
          const unsigned long long pg = T.eg[eb + pos - 1], par = T.ear[eb + pos - 1];
          if (!nb_less(g, ar, __longlong_as_double((long long)pg), par)) break;
          T.eg[eb + pos] = pg;
          T.ear[eb + pos] = par;
          if constexpr (kUnique) T.eh[eb + pos] = T.eh[eb + pos - 1];
          --pos;
        }
        T.eg[eb + pos] = (unsigned long long)__double_as_longlong(g);
        T.ear[eb + pos] = ar;
        if constexpr (kUnique) T.eh[eb + pos] = h;
      }
      if (bad) break;
    }
  }
  T.cnt[t] = c;
  return !bad;
}

// One item, by the whole workgroup (every thread calls; SH and T are the item's).
// SH is an NbShared, for kUnique an NbSharedUnique; hmask: FSTAMD_NBEST_HASH_MASK (kUnique).
template <int WG, bool kLds, bool kUnique, class Shared>
__device__ __forceinline__ void nbest_item(const NbItem& it, const NbTables& T, uint32_t n,
                                           const BatchOutDev& out, uint32_t si, Shared& SH,
                                           unsigned long long deadline,
                                           unsigned long long hmask) {
  const uint32_t tid = threadIdx.x, S = it.S, A = it.A;
  // ---- 1: depth -----------------------------------------------------------------------
  for (uint32_t s = tid; s < S; s += WG) {
    T.depth[s] = s == it.start ? 1u : 0u;
    T.roff[s] = 0;
    T.lvl[s] = 0;
    T.cnt[s] = 0;
  }
  if (tid == 0) {
    SH.flag[0] = 0;
    SH.flag[1] = 0;
    SH.stop = 0;
  }
  nb_sync<kLds>();
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
    if (f & 2u) return nb_status<WG>(out, si, n, kPathUnsupported, it);
    if (f & 4u) return nb_status<WG>(out, si, n, kPathInternal, it);
    if (!(f & 1u)) break;
  }
  // ---- 2: in-arcs by target, reached states by depth -----------------------------------
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
    const uint32_t p = atomicAdd(&T.lvl[d - 1], 1u);
    if (p < S) T.order[p] = s;
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
  // ---- 3: the lists, level by level (lvl[d] is now the end of level d) -------------------
  for (uint32_t d = 0; d < S; ++d) {
    const uint32_t lo = d ? nb_ld<kLds>(&T.lvl[d - 1]) : 0u;
    uint32_t hi = nb_ld<kLds>(&T.lvl[d]);
    hi = hi < S ? hi : S;
    if (hi <= lo) break;  // (the same words in every thread: levels are contiguous)
    if ((d & 63u) == 63u) {
      if (tid == 0 && __builtin_amdgcn_s_memrealtime() > deadline) SH.stop = 1;
      nb_sync<kLds>();
      if (SH.stop) return nb_status<WG>(out, si, n, kPathInternal, it);
    }
    for (uint32_t i = lo + tid; i < hi; i += WG) {
      const uint32_t t = nb_ld<kLds>(&T.order[i]);
      if (t < S && !nb_pull<kLds, kUnique>(it, T, n, t, hmask)) SH.stop = 1;
    }
    nb_sync<kLds>();
  }
  if constexpr (kUnique) {  // (a text walk that broke its bound; read after the level's barrier)
    if (SH.stop) return nb_status<WG>(out, si, n, kPathInternal, it);
  }
  // ---- 4: the n best complete paths, by (total, final state, rank) -----------------------
  uint32_t m = 0;
  unsigned long long last_k = 0, last_t = 0;
  // One round: the least (total, t, r) above the round before, ~0 if there is none (uniform).
  const auto round_min = [&](bool k, unsigned long long& mk) {
    unsigned long long bk = ~0ull, bt = ~0ull;
    for (uint32_t t = tid; t < S; t += WG) {
      if (!nb_ld<kLds>(&T.depth[t])) continue;
      const double fw = it.fin[t];
      if (nb_is_zero(fw)) continue;
      uint32_t c = nb_ld<kLds>(&T.cnt[t]);
      c = c < n ? c : n;
      for (uint32_t r = 0; r < c; ++r) {
        const double tot =
            __longlong_as_double((long long)nb_ld<kLds>(&T.eg[(size_t)t * n + r])) + fw;
        if (nb_is_zero(tot)) break;
        const unsigned long long ck = nb_key(tot), ct = ((unsigned long long)t << 32) | r;
        if (k && !(ck > last_k || (ck == last_k && ct > last_t))) continue;
        // (keys rise with r: the first one above the last choice is this state's least)
        if (ck < bk || (ck == bk && ct < bt)) {
          bk = ck;
          bt = ct;
        }
        break;
      }
    }
    mk = nb_block_min<WG>(bk, SH);
    return nb_block_min<WG>(bk == mk ? bt : ~0ull, SH);
  };
  if constexpr (!kUnique) {
    for (uint32_t k = 0; k < n; ++k) {
      unsigned long long mk;
      const unsigned long long mt = round_min(k != 0, mk);
      if (mt == ~0ull) break;  // (uniform) fewer than n complete paths
      if (tid == 0) SH.sel[k] = mt;
      last_k = mk;
      last_t = mt;
      ++m;
    }
  } else {
    // The same rounds; a winner whose text was chosen before advances (last_k, last_t) without
    // taking a slot.  Every wave compares the winner with the chosen paths for itself, lane j
    // with path j, so the verdict is uniform without a word of LDS.  A round passes one (final
    // state, rank) entry: there are at most S * n.
    const unsigned long long rounds = (unsigned long long)S * n;
    for (unsigned long long round = 0; m < n && round < rounds; ++round) {
      if ((round & 15u) == 15u) {
        if (tid == 0 && __builtin_amdgcn_s_memrealtime() > deadline) SH.stop = 1;
        nb_sync<kLds>();
        if (SH.stop) return nb_status<WG>(out, si, n, kPathInternal, it);
      }
      unsigned long long mk;
      const unsigned long long mt = round_min(round != 0, mk);
      if (mt == ~0ull) break;  // (uniform) fewer than n distinct texts
      last_k = mk;
      last_t = mt;
      const uint32_t wt = (uint32_t)(mt >> 32), wr = (uint32_t)mt;  // (wt < S, wr < n: as scanned)
      const unsigned long long wh = nb_ld<kLds>(&T.eh[(size_t)wt * n + wr]);
      const uint32_t j = tid & 63u;
      bool bad = false, twin = false;
      if (j < m && SH.selh[j] == wh) {
        const unsigned long long e = SH.sel[j];
        twin = nb_same_text<kLds>(it, T, n, 0u, wt, wr, 0u, (uint32_t)(e >> 32), (uint32_t)e, bad);
      }
      if (__ballot(bad)) return nb_status<WG>(out, si, n, kPathInternal, it);
      if (__ballot(twin)) continue;
      if (tid == 0) {
        SH.sel[m] = mt;
        SH.selh[m] = wh;
      }
      ++m;  // (the other waves read sel and selh behind the next round's barriers)
    }
  }
  nb_sync<kLds>();
  if (tid >= 64) return;
  // the first wave: lane k walks path k back for its length ...
  uint32_t len = 0, end_t = 0, end_r = 0;
  bool bad = false;
  if (tid < m) {
    const unsigned long long e = SH.sel[tid];
    end_t = (uint32_t)(e >> 32);
    end_r = (uint32_t)e;
    uint32_t ct = end_t, cr = end_r;
    for (;;) {
      const unsigned long long ar = nb_ld<kLds>(&T.ear[(size_t)ct * n + cr]);
      const uint32_t a = (uint32_t)(ar >> 32);
      if (a == kNbNoArc) break;
      cr = (uint32_t)ar;
      if (a >= A || cr >= n || ++len >= S) {  // (a path has fewer arcs than the item states)
        bad = true;
        break;
      }
      ct = nb_ld<kLds>(&T.asrc[a]);
      if (ct >= S) {
        bad = true;
        break;
      }
    }
    if (bad) len = 0;
  }
  // ... the item reserves the sum with one atomic ...
  const uint32_t incl = wave_incl_scan(len);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  unsigned long long o = 0;
  if (tid == 0 && total) o = atomicAdd(out.cursor, (unsigned long long)total);
  const uint32_t o_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o >> 32));
  o = ((unsigned long long)o_hi << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o);
  o += incl - len;
  if (tid >= n) return;
  // ... and lane k writes string si * n + k, the arcs forward
  const uint32_t str = si * n + tid;
  if (tid >= m) return write_status(out, str, kPathEmpty, S, A);
  if (bad) return write_status(out, str, kPathInternal, S, A);
  if (len && o + len > out.arc_cap) return write_status(out, str, kPathOutputFull, S, A);
  uint32_t ct = end_t, cr = end_r;
  for (uint32_t k = len; k > 0; --k) {
    const unsigned long long ar = nb_ld<kLds>(&T.ear[(size_t)ct * n + cr]);
    const uint32_t a = (uint32_t)(ar >> 32);
    out.out_il[o + k - 1] = it.ail[a];
    out.out_ol[o + k - 1] = it.aol[a];
    out.out_w[o + k - 1] = it.aw[a];
    cr = (uint32_t)ar;
    ct = nb_ld<kLds>(&T.asrc[a]);
  }
  out.status[str] = kPathOk;
  out.path_len[str] = len;
  out.path_off[str] = len ? o : 0;
  out.final_w[str] = it.fin[end_t];
  if (out.work) {
    out.work[2 * str] = S;
    out.work[2 * str + 1] = A;
  }
}

// The LDS an item's tables take: 16 B per list entry (24 B with the text hashes of kUnique),
// five words per state, two per arc.
__host__ __device__ __forceinline__ unsigned long long nb_lds_need(uint32_t S, uint32_t A,
                                                                   uint32_t n) {
  return 16ull * n * S + 4ull * (5ull * S + 2ull * A);
}
__host__ __device__ __forceinline__ unsigned long long nb_lds_need_unique(uint32_t S, uint32_t A,
                                                                          uint32_t n) {
  return 24ull * n * S + 4ull * (5ull * S + 2ull * A);
}

// ---- LDS tier: one wave per item, the tables in dynamic LDS of p.lds_budget bytes -----------
// An item whose tables do not fit is handed to the HBM tier through p.list.
template <bool kUnique, class Shared>
__device__ __forceinline__ void nb_lds_tier(const LatNbestDev& p, uint32_t count,
                                            const BatchOutDev& out, unsigned char* nb_lds,
                                            Shared& SH) {
  const uint32_t n = p.n_best;
  uint32_t done = 0;  // (one atomic per wave, not per item)
  for (uint32_t si = blockIdx.x; si < count; si += gridDim.x) {
    const NbItem it = nb_item(p, si);
    if (nb_precheck<64>(it, n, out, si)) {
      ++done;
      continue;
    }
    const unsigned long long need =
        kUnique ? nb_lds_need_unique(it.S, it.A, n) : nb_lds_need(it.S, it.A, n);
    if (need > p.lds_budget) {  // (uniform)
      if (threadIdx.x == 0) p.list[atomicAdd(&p.ctr[kNbCtrList], 1u)] = si;
      continue;
    }
    NbTables T;
    T.eg = reinterpret_cast<unsigned long long*>(nb_lds);
    T.ear = T.eg + (size_t)it.S * n;
    T.eh = kUnique ? T.ear + (size_t)it.S * n : nullptr;
    T.depth = reinterpret_cast<uint32_t*>(T.ear + (size_t)it.S * n * (kUnique ? 2 : 1));
    T.roff = T.depth + it.S;
    T.cnt = T.roff + it.S;
    T.lvl = T.cnt + it.S;
    T.order = T.lvl + it.S;
    T.rarc = T.order + it.S;
    T.asrc = T.rarc + it.A;
    ++done;
    nbest_item<64, true, kUnique>(it, T, n, out, si, SH,
                                  __builtin_amdgcn_s_memrealtime() + p.wd_ticks, p.hash_mask);
    __syncthreads();  // (SH and the tables are the next item's)
  }
  if (threadIdx.x == 0 && done) atomicAdd(&p.ctr[kNbCtrLds], done);
}

// (FSTAMD_NBEST_NO_KERNELS: a unit that includes this header for its helpers alone, as
// lattice_posterior.hpp does, defines it so that the kernels stay lattice_nbest.hip's)
#ifndef FSTAMD_NBEST_NO_KERNELS
__global__ void __launch_bounds__(64)
lattice_nbest_lds_kernel(LatNbestDev p, uint32_t count, BatchOutDev out) {
  extern __shared__ __align__(16) unsigned char nb_lds[];
  __shared__ NbShared SH;
  nb_lds_tier<false>(p, count, out, nb_lds, SH);
}

__global__ void __launch_bounds__(64)
lattice_nbest_unique_lds_kernel(LatNbestDev p, uint32_t count, BatchOutDev out) {
  extern __shared__ __align__(16) unsigned char nb_lds[];
  __shared__ NbSharedUnique SH;
  nb_lds_tier<true>(p, count, out, nb_lds, SH);
}
#endif

// ---- HBM tier: one workgroup per listed item, the tables in the workspace -----------------
// The item's slices: list entries at state_base * n, state words at state_base, arc words at
// arc_base.
template <bool kUnique, class Shared>
__device__ __forceinline__ void nb_hbm_tier(const LatNbestDev& p, const BatchOutDev& out,
                                            Shared& SH) {
  const uint32_t n = p.n_best;
  const uint32_t count = p.ctr[kNbCtrList];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t si = p.list[li];
    const NbItem it = nb_item(p, si);
    if (it.start >= it.S) continue;  // (the LDS tier lists no such item)
    NbTables T;
    T.eg = p.eg + it.sb * n;
    T.ear = p.ear + it.sb * n;
    T.eh = kUnique ? p.eh + it.sb * n : nullptr;
    T.depth = p.depth + it.sb;
    T.roff = p.roff + it.sb;
    T.cnt = p.cnt + it.sb;
    T.lvl = p.lvl + it.sb;
    T.order = p.order + it.sb;
    T.rarc = p.rarc + it.ab;
    T.asrc = p.asrc + it.ab;
    nbest_item<kNbWG, false, kUnique>(it, T, n, out, si, SH,
                                      __builtin_amdgcn_s_memrealtime() + p.wd_ticks,
                                      p.hash_mask);
    if (threadIdx.x == 0) atomicAdd(&p.ctr[kNbCtrHbm], 1u);
    __syncthreads();  // (SH is the next item's)
  }
}

#ifndef FSTAMD_NBEST_NO_KERNELS
__global__ void __launch_bounds__(kNbWG)
lattice_nbest_hbm_kernel(LatNbestDev p, BatchOutDev out) {
  __shared__ NbShared SH;
  nb_hbm_tier<false>(p, out, SH);
}

__global__ void __launch_bounds__(kNbWG)
lattice_nbest_unique_hbm_kernel(LatNbestDev p, BatchOutDev out) {
  __shared__ NbSharedUnique SH;
  nb_hbm_tier<true>(p, out, SH);
}
#endif

}  // namespace fstamd

// lhs_prepare.hpp -- on-device preparation of a device-resident batch of general lhs
// (fst_device_compose_shortest_path_lhs): what run_lhs_shard (batch_lhs.cpp) computes on
// the host while it stages a batch, computed where the batch already is.
//
// lhs_prepare_kernel: one wavefront per item, grid-stride over the items.  Per item it
//   - validates the item as the host validator does (lhs_batch_valid, batch_entries.cpp): the
//     host cannot read these arrays.  Every index is checked against the two extents the host
//     read (LhsPrepIn::total_states / total_arcs) before it is used, so nothing outside
//     state_offsets[0 .. num], start[0 .. num), the per-state arrays [0 .. total_states (+ 1))
//     and the arc arrays [0 .. total_arcs) is read, whatever the offsets hold;
//   - writes the item's u32 arc offsets local to the item (num_states + 1 words at
//     state_off[state_base + i], the layout lhs_item reads);
//   - derives the item's flags, bit for bit run_lhs_shard's rules;
//   - writes the 32-B LhsDesc, its bases the caller's global offsets: finals and arcs are
//     used in place.
// An item that fails a check is never traversed further: its descriptor is empty with a
// harmless start and kLhsNaN | kLhsInvalid, so the general kernels report UNSUPPORTED after
// their EMPTY / ERROR_N tests (the single call's status order) without touching it.
// Batch-wide it reduces the largest out-degree (it sizes the lazy per-pop table, so it is
// exact: a wave max, then one atomic max per wave), counts the invalid items, and counts the
// pairs state_offsets[i] > state_offsets[i + 1].  Item i's words of state_off start at
// state_base + i, so they are the item's own only while the state ranges are disjoint, that
// is while state_offsets is non-decreasing over the whole batch.  When the count is not zero
// DeviceEngine::prepare_lhs runs the kernel again with kLhsInvalid in base_flags: every item
// is then invalid, and the general kernels never read a word two items could have written.
//
// lhs_lists_kernel: the two eager item lists (LhsDesc::flags & kLhsReplay or not) in
// ascending item order, as the host's loop builds them, so that route logs and tier
// hand-overs equal the host entry's.  One workgroup walks the items in chunks of its size
// with a ballot / popcount scan; the running base makes the order exact.
#pragma once

#include "device_common.hpp"

namespace fstamd {

constexpr int kLhsListsWG = 1024;

namespace lhs_prep {

__device__ __forceinline__ uint32_t sgpr(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}
__device__ __forceinline__ uint64_t sgpr64(uint64_t x) {
  return ((uint64_t)sgpr((uint32_t)(x >> 32)) << 32) | sgpr((uint32_t)x);
}
// OR / max over the wave's 64 lanes (xor butterfly), the result in an SGPR: the wave
// branches on it
__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
  for (int o = 32; o > 0; o >>= 1) x |= (uint32_t)__shfl_xor((int)x, o, 64);
  return sgpr(x);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
  for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o, 64));
  return sgpr(x);
}
// run_lhs_shard's weight rules on the bit pattern: NaN -> kLhsNaN; negative or -0.0 (the sign
// bit of a non-NaN) -> kLhsReplay; `arc`: +-inf too
__device__ __forceinline__ uint32_t weight_flags(double w, bool arc) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(w);
  const unsigned long long mag = b & 0x7FFFFFFFFFFFFFFFull;
  constexpr unsigned long long kInf = 0x7FF0000000000000ull;
  if (mag > kInf) return kLhsNaN;
  return ((b >> 63) || (arc && mag == kInf)) ? kLhsReplay : 0u;
}

}  // namespace lhs_prep

__global__ __launch_bounds__(64) void lhs_prepare_kernel(LhsPrepIn in, LhsPrepOut out) {
  using namespace lhs_prep;
  const uint32_t lane = threadIdx.x;
  uint32_t batch_deg = 0, batch_invalid = 0, batch_disorder = 0;  // (uniform)
  // kLhsInvalid in base_flags: the second pass over a batch whose state offsets decrease
  // somewhere (below); every item is invalid and nothing of it is read
  const bool none_valid = (in.base_flags & kLhsInvalid) != 0;
  for (uint32_t i = blockIdx.x; i < in.num; i += gridDim.x) {
    // the item's extents, checked before anything is read through them
    const uint64_t s0 = sgpr64(in.state_offsets[i]), s1 = sgpr64(in.state_offsets[i + 1]);
    // state_offsets must be non-decreasing over the whole batch: only then are the items'
    // state ranges disjoint, and with them their words of state_off (item i's start at
    // s0 + i).  Were two valid items to overlap there, each would overwrite offsets the
    // general kernels later read for the other.  So one decreasing pair invalidates the batch.
    if (s0 > s1) batch_disorder += 1;
    bool ok = !none_valid && s0 <= s1 && s1 <= in.total_states && s1 - s0 < (1ull << 30);
    uint64_t a0 = 0, a1 = 0;
    if (ok) {
      a0 = sgpr64(in.arc_offsets[s0]);
      a1 = sgpr64(in.arc_offsets[s1]);
      ok = a0 <= a1 && a1 <= in.total_arcs && a1 - a0 < (1ull << 32);
    }
    const uint32_t ns = ok ? (uint32_t)(s1 - s0) : 0u;
    const uint32_t start = sgpr(in.start[i]);
    if (start != kNoState && start >= ns) ok = false;
    uint32_t fl = 0, deg = 0;  // (per lane)
    if (ok) {
      // states: the local offsets, the out-degrees, the finals.  The offsets are
      // non-decreasing over [s0, s1] iff every pair below is; then each lies in [a0, a1]
      // and its distance from a0 fits 32 bits.
      uint32_t* so = out.state_off + (s0 + i);
      bool bad = false;
      for (uint64_t s = s0 + lane; s < s1; s += 64) {
        const uint64_t lo = in.arc_offsets[s], hi = in.arc_offsets[s + 1];
        const bool dec = lo > hi;
        bad |= dec;
        deg = max(deg, dec ? 0u : (uint32_t)min(hi - lo, (uint64_t)0xFFFFFFFFull));
        so[s - s0] = (uint32_t)(lo - a0);
        fl |= weight_flags(in.final_w[s], false);
      }
      if (lane == 0) so[ns] = (uint32_t)(a1 - a0);
      // validity is reduced with a ballot: a lane mask in SGPRs, uniform by construction
      ok = __ballot(bad) == 0;
    }
    if (ok) {  // arcs (never those of an item whose offsets failed)
      bool bad = false;
      for (uint64_t a = a0 + lane; a < a1; a += 64) {
        fl |= weight_flags(in.arc_w[a], true);
        if (in.arc_ol[a] == kEpsilon) fl |= kLhsEpsOut;
        bad |= in.arc_next[a] >= ns;
      }
      ok = __ballot(bad) == 0;
    }
    uint32_t flags = in.base_flags;
    if (ok) {
      flags |= wave_or(fl);
      batch_deg = max(batch_deg, wave_max(deg));
    } else {
      flags |= kLhsNaN | kLhsInvalid;
      batch_invalid += 1;
    }
    if (lane == 0) {
      uint4* d = reinterpret_cast<uint4*>(out.desc + i);
      if (ok) {
        d[0] = make_uint4((uint32_t)s0, (uint32_t)(s0 >> 32), (uint32_t)a0, (uint32_t)(a0 >> 32));
        d[1] = make_uint4(ns, ns ? start : kNoState, (uint32_t)(a1 - a0), flags);
      } else {  // empty, with a start: it reaches the kernels' flag test, after EMPTY / ERROR_N
        d[0] = make_uint4(0, 0, 0, 0);
        d[1] = make_uint4(0, 0, 0, flags);
      }
    }
  }
  if (lane == 0) {
    if (batch_deg) atomicMax(out.totals + 2, batch_deg);
    if (batch_invalid) atomicAdd(out.totals + 3, batch_invalid);
    if (batch_disorder) atomicAdd(out.totals + 4, batch_disorder);
  }
}

__global__ __launch_bounds__(kLhsListsWG) void lhs_lists_kernel(const LhsDesc* desc, uint32_t num,
                                                                uint32_t* list_nonneg,
                                                                uint32_t* list_replay,
                                                                uint32_t* totals) {
  constexpr uint32_t kWaves = kLhsListsWG / 64;
  __shared__ uint32_t wave_cnt[kWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t base = 0;  // replay items before this chunk (the same in every thread)
  for (uint64_t c = 0; c < num; c += kLhsListsWG) {
    const uint64_t i = c + tid;
    const bool in = i < num;
    const bool rep = in && (desc[i].flags & kLhsReplay);
    const unsigned long long m = __ballot(rep);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = base, total = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint32_t v = wave_cnt[w];
      if (w < wave) before += v;
      total += v;
    }
    before += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));  // replay items below i
    if (in) {
      if (rep) list_replay[before] = (uint32_t)i;
      else list_nonneg[(uint32_t)i - before] = (uint32_t)i;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    totals[0] = num - base;
    totals[1] = base;
  }
}

}  // namespace fstamd

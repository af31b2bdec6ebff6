// posterior_gather.hpp -- where a shard of fst_posterior_lhs_batch lands in the result: the
// result is in the caller's own layout (alpha, beta like final_weights, arc costs like weights),
// so a shard of items [s0, s1) owns the state range and the arc range of those items and its
// three value arrays go there as they are.  Host code with no device call of its own: `copy` is
// d2h on a stream in the entry (batch_entries.cpp) and memcpy in tools/posterior_gather_check.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace fstamd::host {

struct PosteriorRanges {
  uint64_t sb, ns;  // first state of the shard in the caller's arrays, its states
  uint64_t ab, na;  // first arc, its arcs
};

inline PosteriorRanges posterior_shard_ranges(const uint64_t* state_offsets,
                                              const uint64_t* arc_offsets, uint32_t s0,
                                              uint32_t s1) {
  PosteriorRanges r;
  r.sb = state_offsets[s0];
  r.ns = state_offsets[s1] - r.sb;
  r.ab = arc_offsets[r.sb];
  r.na = arc_offsets[state_offsets[s1]] - r.ab;
  return r;
}

// The entries in front of the first item belong to no item: +inf, like a non-OK item's.
inline void posterior_fill_front(const uint64_t* state_offsets, const uint64_t* arc_offsets,
                                 uint32_t num, double* alpha, double* beta, double* arc_cost) {
  const uint64_t s0 = num ? state_offsets[0] : 0, a0 = num ? arc_offsets[s0] : 0;
  std::fill(alpha, alpha + s0, HUGE_VAL);
  std::fill(beta, beta + s0, HUGE_VAL);
  std::fill(arc_cost, arc_cost + a0, HUGE_VAL);
}

// One shard into the result.  `vals`: the shard's alpha [ns], beta [ns], arc costs [na], one
// after the other (run_posterior_shard's block).  copy(dst, src, bytes) -> bool.
template <class Copy>
bool posterior_gather_shard(const PosteriorRanges& r, uint32_t s0, uint32_t s1,
                            const int32_t* status, const double* total, const double* vals,
                            int32_t* out_status, double* out_total, double* out_alpha,
                            double* out_beta, double* out_cost, const Copy& copy) {
  const uint64_t n = s1 - s0;
  return copy(out_status + s0, status, n * 4) && copy(out_total + s0, total, n * 8) &&
         copy(out_alpha + r.sb, vals, r.ns * 8) && copy(out_beta + r.sb, vals + r.ns, r.ns * 8) &&
         copy(out_cost + r.ab, vals + 2 * r.ns, r.na * 8);
}

}  // namespace fstamd::host

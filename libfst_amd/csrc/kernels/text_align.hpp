// text_align.hpp -- input spans per output symbol of the 1-best paths (the aligned text entry
// of fst_batch.h: which input bytes became which output bytes).
//
// One stage.  Along a path's arcs a_0 .. a_{L-1}, with nz(x) = (x != epsilon), the arc a_k that
// emits the q-th non-epsilon olabel gives
//     b[q] = sum_{t<k} nz(il_t),   e[q] = b[q] + nz(il_k),
// a half-open interval of the symbols the path consumed: one symbol for an x:y arc, empty (at
// the boundary where it was taken) for an eps:y arc; a deleted input (x:eps) belongs to no
// output.  N = sum_t nz(il_t) is what the path consumed.
//
// Several stages.  Stage s consumes stage s-1's projected output (project_output): with
// (B, E) the running map of stage s-1's M output symbols into the original input and N1 what
// stage 1 consumed,
//     B'[q] = b < M ? B[b] : N1,     E'[q] = e > b ? E[b] : B'[q].
//
// Both kernels: one wavefront per string, grid-stride, no LDS.
#pragma once

#include "device_common.hpp"

namespace fstamd {

// (b, e) of every path at offsets[i] + rank, and consumed[i] = N.  `offsets` [num + 1] are
// those of text_count or project_output for the same stage: string i owns the entries
// [offsets[i], offsets[i + 1]).  A string whose path is their source (status OK, the path
// inside the arena, no olabel above 256, as many non-epsilon olabels as entries) gets its map;
// every other string (no bytes in a text, the one dead label in a projection) gets [0, 0) on
// each of its entries and N = 0.  The status read is the stage's own, not a merged one
// (text_count's `fail`): a string that failed an earlier stage shows here through its entry
// count (none in a text, the one dead label in a projection).  So the offsets must be the ones
// written for this very stage: a string whose entry count is not its path's symbol count is
// taken for a failed one and its map is zeroed, without an error.  The first loop decides which it is from the olabels alone (a second read
// of the olabels, so that no lane stores before the wave knows the entries are the path's),
// the second writes: per 64-arc pass coalesced loads of both tapes, the ballots of the
// non-epsilon outputs and inputs, a lane's rank from the output mask, its b from the input
// mask below it plus a running input base, both bases carried across the passes.  No entry at
// or past `cap` is stored.
__global__ void __launch_bounds__(64) align_write_kernel(BatchOutDev s, uint32_t num,
                                                         const uint64_t* offsets,
                                                         uint32_t* begin, uint32_t* end,
                                                         uint64_t cap, uint32_t* consumed) {
  const uint32_t lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    const uint64_t dst0 = offsets[i];
    const uint64_t width = offsets[i + 1] - dst0;
    const uint64_t src = s.path_off[i];
    const uint32_t L = s.path_len[i];
    bool own = s.status[i] == kPathOk && src + L <= s.arc_cap;
    if (own) {
      uint64_t cnt = 0;
      bool bad = false;
      for (uint32_t k0 = 0; k0 < L; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint32_t ol = k < L ? s.out_ol[src + k] : kEpsilon;
        bad |= __ballot(ol > 256u) != 0;
        cnt += (uint32_t)__popcll(__ballot(ol != kEpsilon));
      }
      own = !bad && cnt == width;
    }
    if (!own) {
      for (uint64_t q = lane; q < width; q += 64)
        if (dst0 + q < cap) {
          begin[dst0 + q] = 0;
          end[dst0 + q] = 0;
        }
      if (lane == 0) consumed[i] = 0;
      continue;
    }
    uint64_t dst = dst0;
    uint32_t in_base = 0;
    for (uint32_t k0 = 0; k0 < L; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool in = k < L;
      const uint32_t ol = in ? s.out_ol[src + k] : kEpsilon;
      const uint32_t il = in ? s.out_il[src + k] : kEpsilon;
      const bool oz = ol != kEpsilon;
      const bool iz = il != kEpsilon;
      const unsigned long long omask = __ballot(oz);
      const unsigned long long imask = __ballot(iz);
      const uint32_t rank = (uint32_t)__popcll(omask & below);
      const uint32_t b = in_base + (uint32_t)__popcll(imask & below);
      if (oz && dst + rank < cap) {
        begin[dst + rank] = b;
        end[dst + rank] = b + (iz ? 1u : 0u);
      }
      dst += (uint32_t)__popcll(omask);
      in_base += (uint32_t)__popcll(imask);
    }
    if (lane == 0) consumed[i] = in_base;
  }
}

// The gather above: string i's outer entries [outer_off[i], outer_off[i + 1]) hold (b, e)
// into its M = inner_off[i + 1] - inner_off[i] inner symbols, whose running map (in_begin,
// in_end) sits at inner_off[i]; n1[i] = what stage 1 consumed.  out_* may be the outer arrays
// themselves (an entry is read, then written, by the one lane that owns it).  The edge cases:
// b == M (an eps:y arc after the stage's input was exhausted: the empty interval at N1) and
// M == 0 (every entry is such an arc).  No entry at or past `cap` is read or stored.
__global__ void __launch_bounds__(64) align_compose_kernel(
    uint32_t num, const uint64_t* outer_off, const uint32_t* b_in, const uint32_t* e_in,
    const uint64_t* inner_off, const uint32_t* in_begin, const uint32_t* in_end,
    const uint32_t* n1, uint32_t* out_begin, uint32_t* out_end, uint64_t cap) {
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    const uint64_t q0 = outer_off[i], q1 = min(outer_off[i + 1], cap);
    const uint64_t base = inner_off[i];
    const uint64_t M = inner_off[i + 1] - base;
    const uint32_t N1 = n1[i];
    for (uint64_t q = q0 + threadIdx.x; q < q1; q += 64) {
      const uint32_t b = b_in[q], e = e_in[q];
      const bool has = b < M;
      const uint32_t B = has ? in_begin[base + b] : N1;
      const uint32_t E = (has && e > b) ? in_end[base + b] : B;
      out_begin[q] = B;
      out_end[q] = E;
    }
  }
}

}  // namespace fstamd

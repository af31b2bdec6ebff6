// text_io.hpp -- byte strings in, byte strings out (the text entries of fst_batch.h).
//
//   widen : compileString for a whole batch (src/string.zig:24-50): label = byte + 1, flat
//           over the batch's bytes, string boundaries play no part.
//   emit  : printOutputString of every 1-best path (src/string.zig:60-97): the path's
//           non-epsilon olabels minus 1, in path order, as count -> scan -> write.  A label
//           above 256 is not a byte (the reference's @intCast would trap): the string reports
//           UNSUPPORTED with no bytes, as project_count_kernel does between stages.
//
// total_weight is the reference search's own total: dist is built arc by arc along the path
// (shortest-path.zig:72, the relax of compose-shortest-path.zig) and then times(dist, final),
// a left fold in f64.  A tree reduction over the lanes rounds differently for weights that are
// no dyadic rationals, so the fold stays serial: the lanes load 64 weights at once and every
// lane adds them in path order (L adds per string).
#pragma once

#include "device_common.hpp"

namespace fstamd {

// labels[k] = text[k] + 1 for k in [offsets[0], offsets[num]).  The dwords of `text` that lie
// whole inside that range are read as dwords (4 labels per lane, one 16-B store when the
// labels are aligned for it); the up to 3 bytes before the first and after the last such
// dword go one by one.  Nothing outside the range is read or written.
__global__ void __launch_bounds__(256) text_widen_kernel(const uint8_t* text,
                                                         const uint64_t* offsets, uint32_t num,
                                                         uint32_t* labels) {
  const uint64_t lo = offsets[0], hi = offsets[num];
  if (hi <= lo) return;
  const uint64_t head = min((uint64_t)((4u - ((uintptr_t)(text + lo) & 3u)) & 3u), hi - lo);
  const uint64_t b0 = lo + head;
  const uint64_t body = (hi - b0) >> 2;  // whole dwords
  const uint64_t t0 = b0 + 4 * body;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(text + b0);
  const bool wide = ((uintptr_t)(labels + b0) & 15u) == 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; g < body; g += stride) {
    const uint32_t v = src[g];
    const uint4 l = make_uint4((v & 0xFFu) + 1u, ((v >> 8) & 0xFFu) + 1u,
                               ((v >> 16) & 0xFFu) + 1u, (v >> 24) + 1u);
    uint32_t* d = labels + b0 + 4 * g;
    if (wide) {
      *reinterpret_cast<uint4*>(d) = l;
    } else {
      d[0] = l.x;
      d[1] = l.y;
      d[2] = l.z;
      d[3] = l.w;
    }
  }
  if (blockIdx.x == 0) {
    const uint32_t t = threadIdx.x;
    if (t < head) labels[lo + t] = (uint32_t)text[lo + t] + 1u;
    if (t < hi - t0) labels[t0 + t] = (uint32_t)text[t0 + t] + 1u;
  }
}

// lane j's f64 for every lane (j wave-uniform)
__device__ __forceinline__ double wave_read_f64(double v, uint32_t j) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)b, j);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(b >> 32), j);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// One wavefront per string (grid-stride).  status[i]: the stage's status, `fail` (when given:
// a pipeline's first failing stage) taking precedence, UNSUPPORTED for a non-byte olabel;
// counts[i]: the string's bytes (0 unless OK), counts[num] = 0 for the scan's total;
// total_w[i]: the fold above (+inf unless OK).
__global__ void __launch_bounds__(64) text_count_kernel(BatchOutDev s, uint32_t num,
                                                        const int32_t* fail, int32_t* status,
                                                        uint64_t* counts, double* total_w) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) counts[num] = 0;
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    int32_t st = s.status[i];
    if (fail && fail[i] != kPathOk) st = fail[i];
    uint32_t cnt = 0;
    double tw = w_zero();
    if (st == kPathOk) {
      const uint64_t src = s.path_off[i];
      const uint32_t L = s.path_len[i];
      if (src + L > s.arc_cap) {
        st = kPathInternal;  // a path outside the arena: an engine bug, never read
      } else {
        bool bad = false;
        double d = w_one();
        for (uint32_t k0 = 0; k0 < L; k0 += 64) {
          const uint32_t k = k0 + lane;
          const bool in = k < L;
          const uint32_t ol = in ? s.out_ol[src + k] : kEpsilon;
          const double w = in ? s.out_w[src + k] : 0.0;
          bad |= __ballot(ol > 256u) != 0;
          cnt += (uint32_t)__popcll(__ballot(ol != kEpsilon));
          const uint32_t m = min(64u, L - k0);
          for (uint32_t j = 0; j < m; ++j) d = w_times(d, wave_read_f64(w, j));
        }
        if (bad) {
          st = kPathUnsupported;
          cnt = 0;
        } else {
          tw = w_times(d, s.final_w[i]);
        }
      }
    }
    if (lane == 0) {
      status[i] = st;
      counts[i] = cnt;
      total_w[i] = tw;
    }
  }
}

// One wavefront per string (grid-stride): per 64-arc pass a coalesced olabel load, the
// ballot of the non-epsilon lanes, each such lane's rank among them, and a running base
// carried across the passes.  Every byte is stored on its own, so a string's neighbours
// (they share dwords with it) are never touched; a byte at or past `cap` is not stored.
__global__ void __launch_bounds__(64) text_write_kernel(BatchOutDev s, uint32_t num,
                                                        const int32_t* status,
                                                        const uint64_t* offsets, uint8_t* text,
                                                        uint64_t cap) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    if (status[i] != kPathOk) continue;
    const uint64_t src = s.path_off[i];
    const uint32_t L = s.path_len[i];
    if (src + L > s.arc_cap) continue;  // (text_count_kernel reported it)
    uint64_t dst = offsets[i];
    for (uint32_t k0 = 0; k0 < L; k0 += 64) {
      const uint32_t k = k0 + lane;
      const uint32_t ol = k < L ? s.out_ol[src + k] : kEpsilon;
      const bool nz = ol != kEpsilon;
      const unsigned long long mask = __ballot(nz);
      const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (nz && dst + rank < cap) text[dst + rank] = (uint8_t)(ol - 1u);
      dst += (uint32_t)__popcll(mask);
    }
  }
}

// The streamed text batch (c_api.cpp), strings the pull tier handed on: once the later tiers
// have written their paths to the arena's fixed slots, one wavefront per string (grid-stride)
// emits them as the pull tiers' chase epilogue does (emit_text_paths with one job, held by
// lane 0).  Strings whose `first` status is OK (emitted already) or EMPTY (final) are
// skipped, and so is every string the later tiers left without a path.
__global__ void __launch_bounds__(64) text_fixup_kernel(BatchOutDev s, TextOutDev tx,
                                                        const int32_t* first, uint32_t num) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = blockIdx.x; i < num; i += gridDim.x) {
    const int32_t f = first[i];
    if (f == kPathOk || f == kPathEmpty || s.status[i] != kPathOk) continue;
    const uint64_t o = s.path_off[i];
    const uint32_t L = s.path_len[i];
    // (the later tiers reserve the string's fixed slot, reserve_path; anything else would be
    // an engine bug and is never read or written through)
    if (o != s.slots[i] || L != (uint32_t)(s.slots[i + 1] - o) || o + L > s.arc_cap) {
      if (lane == 0) s.status[i] = kPathInternal;
      continue;
    }
    emit_text_paths(s, tx, 1u, i, o, L, s.final_w[i], lane, num);
  }
}

}  // namespace fstamd

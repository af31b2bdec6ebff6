// weight_codes.hpp -- the host half of the streamed batch's weight codes: one byte per arc
// becomes the arc's f64 weight through a 256-entry table (DeviceEngine's pull_codes_table).
// Plain C++ with no device or runtime dependency, so the expander also builds into a
// stand-alone checker (tools/expand_codes_check.cpp) and behind fst_debug_expand_weight_codes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#pragma GCC visibility push(hidden)  // internal: not one of the library's exports
namespace fstamd::host {

// dst[i] = table[codes[i]] for i < n.  The destination is written once and not read again
// by this thread (the result arrays of a batch: hundreds of MB), so whole 64-B lines of it go
// out with non-temporal stores: up to 7 head elements bring dst to a line boundary, then 8
// elements per line, then the tail.  dst must be 8-B aligned (it is an array of doubles);
// codes and dst must not overlap.  Reads codes[0 .. n) and table[0 .. 256), writes
// dst[0 .. n), nothing else.
inline void expand_weight_codes(const uint8_t* codes, size_t n, const double* table,
                                double* dst) {
  size_t i = 0;
#if defined(__SSE2__)
  const size_t head = (size_t)((64u - ((uintptr_t)dst & 63u)) & 63u) / 8u;
  for (; i < n && i < head; ++i) dst[i] = table[codes[i]];
  for (; i + 8 <= n; i += 8) {
    uint64_t c8;
    std::memcpy(&c8, codes + i, 8);
    for (int u = 0; u < 8; u += 2) {
      const __m128d v = _mm_set_pd(table[(c8 >> (8 * u + 8)) & 0xFFu], table[(c8 >> (8 * u)) & 0xFFu]);
      _mm_stream_pd(dst + i + u, v);
    }
  }
  _mm_sfence();
#endif
  for (; i < n; ++i) dst[i] = table[codes[i]];
}

}  // namespace fstamd::host
#pragma GCC visibility pop

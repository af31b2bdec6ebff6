// expand_codes_check.cpp -- stand-alone check of the streamed batch's host expander
// (csrc/weight_codes.hpp), for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o expand_codes_check tools/expand_codes_check.cpp && ./expand_codes_check
// Every length 0..200 at every destination offset 0..7 elements from a 64-B boundary and
// every source offset 0..7 bytes, with the codes and the destination in heap blocks of
// exactly the size read and written (so one byte too many trips the sanitizer), against a
// plain loop, bit for bit; the words around the destination keep their guard pattern.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/weight_codes.hpp"

int main() {
  double table[256];
  for (int c = 0; c < 256; ++c) table[c] = c % 3 == 0 ? c / 256.0 : c % 3 == 1 ? 0.1 * c : std::log(3.0) * c;
  table[0] = 0.0;
  table[255] = 1.0 / 3.0;
  uint32_t seed = 12345;
  auto next = [&] { return seed = seed * 1664525u + 1013904223u; };
  size_t checked = 0;
  for (size_t n = 0; n <= 200; ++n)
    for (size_t doff = 0; doff < 8; ++doff)
      for (size_t soff = 0; soff < 8; soff += (n % 5 == 0 ? 1 : 7)) {
        // destination: a 64-B aligned block of exactly doff + n doubles
        void* raw = nullptr;
        const size_t dbytes = (doff + n) * sizeof(double);
        if (posix_memalign(&raw, 64, dbytes ? dbytes : 64) != 0) return 2;
        double* const block = (double*)raw;
        for (size_t i = 0; i < doff; ++i) block[i] = -7.0;
        // codes: exactly soff + n bytes
        uint8_t* const cblock = (uint8_t*)std::malloc(soff + n ? soff + n : 1);
        for (size_t i = 0; i < soff + n; ++i) cblock[i] = (uint8_t)(next() >> 24);
        if (n) cblock[soff + n - 1] = 255, cblock[soff] = 0;
        fstamd::host::expand_weight_codes(cblock + soff, n, table, block + doff);
        for (size_t i = 0; i < doff; ++i)
          if (block[i] != -7.0) return std::printf("guard n=%zu doff=%zu\n", n, doff), 1;
        for (size_t i = 0; i < n; ++i)
          if (std::memcmp(&block[doff + i], &table[cblock[soff + i]], 8) != 0)
            return std::printf("mismatch n=%zu doff=%zu soff=%zu i=%zu\n", n, doff, soff, i), 1;
        std::free(cblock);
        std::free(raw);
        ++checked;
      }
  std::printf("expand_codes_check: ok (%zu cases)\n", checked);
  return 0;
}

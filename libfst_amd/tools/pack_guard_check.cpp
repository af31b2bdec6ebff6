// pack_guard_check.cpp -- the guard bands of tier P's packed cells, swept on the CPU: a
// stand-alone program over kernels/pull_window.hpp, the header the kernel computes its
// windows and cell offsets with and the host gate decides with.  No GPU, no library.
//
// For every jump pair with jump_back + jump_fwd <= kPackSpanMax, every current layer [cmin,
// cmax] inside a window of wk <= W cells at tmin (with tmin near state 0, where tn is
// clipped, and num_states near the window, where hi is clipped), it takes the next window
// from the header's rule and checks, for every lane of every window row and every delta a
// record can hold, that the byte offset the kernel forms
//   - is a multiple of 4 inside the padded cell array, and never negative in 32 bits,
//   - names the source's own window cell when the source lies in the window, and a guard
//     cell otherwise,
// and that every read of a label-miss row stays in the low guard.  The lane-by-delta sweep
// runs once per distinct row origin of a jump pair (the offsets depend on nothing else);
// the bounds the header states are checked to be attained nowhere beyond.
//
// Build: hipcc -O2 -std=c++17 -x c++ pack_guard_check.cpp -o pack_guard_check   (or g++),
// optionally with -fsanitize=address,undefined.  Prints "pack_guard_check: ok", exit code 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../csrc/kernels/pull_window.hpp"

using namespace fstamd;

namespace {

constexpr uint32_t W = 320;  // 64 * kPullRows (device_engine.hpp)
constexpr int64_t kCells = pack_cells(W);
long long failures = 0;
unsigned long long windows = 0, rows = 0, reads = 0;
int64_t seen_min = 1 << 30, seen_max = -1;

void fail(const char* what, uint32_t jb, uint32_t jf, int64_t a, int64_t b) {
  if (failures++ < 20)
    std::fprintf(stderr, "FAILED: %s (jump_back %u, jump_fwd %u: %lld, %lld)\n", what, jb, jf,
                 (long long)a, (long long)b);
}

// one row of 64 lanes whose lane 0 owns the target tmin + ro: every lane, every delta
void check_row(uint32_t jb, uint32_t jf, uint32_t tmin, int64_t ro) {
  ++rows;
  const uint32_t span = jb + jf;
  for (uint32_t i = 0; i < 64; ++i) {
    const uint32_t t = (uint32_t)((int64_t)tmin + ro + i);
    const uint32_t base4 = pack_hit_base4(t, tmin, 4u * jb);
    for (uint32_t dl = 0; dl <= span; ++dl) {  // delta4 = 4 * (target - source + jump_back)
      const uint32_t off = pack_src_off4(base4, 4u * dl);
      ++reads;
      if ((int32_t)off < 0 || off % 4 != 0 || (int64_t)off >= 4 * kCells) {
        fail("offset outside the padded array", jb, jf, ro + i, dl);
        continue;
      }
      const int64_t cell = off / 4;
      const int64_t src_slot = ro + i + (int64_t)jb - (int64_t)dl;  // source - tmin
      if (cell != (int64_t)kPackGuardLo + src_slot) fail("not the source's cell", jb, jf, cell, src_slot);
      const bool window = src_slot >= 0 && src_slot < (int64_t)W;
      const bool guard = cell < (int64_t)kPackGuardLo || cell >= (int64_t)kPackGuardLo + W;
      if (window == guard) fail("neither window cell nor guard cell", jb, jf, cell, src_slot);
      if (cell < seen_min) seen_min = cell;
      if (cell > seen_max) seen_max = cell;
    }
  }
}

void check_jumps(uint32_t jb, uint32_t jf) {
  const uint32_t span = jb + jf;
  if (!pack_guards_fit(jb, jf, W)) fail("the gate refuses a span <= kPackSpanMax", jb, jf, 0, 0);
  // a label-miss row: the constant base, every delta (a block without records: delta 0)
  for (uint32_t dl = 0; dl <= span; ++dl) {
    const uint32_t off = pack_src_off4(kPackMissBase4, 4u * dl);
    if ((int32_t)off < 0 || off % 4 != 0 || off / 4 >= kPackGuardLo)
      fail("a miss row's read leaves the low guard", jb, jf, off, dl);
    if ((int64_t)off / 4 < pack_miss_cell_min(jb, jf)) fail("miss bound", jb, jf, off, dl);
  }
  // row origins (target of lane 0, relative to tmin) that some window reaches, per tmin class
  const int64_t kOrgLo = -(int64_t)kPackSpanMax, kOrgN = kPackSpanMax + 2 * W;
  // tmin: at state 0 and just below jump_back (tn clipped at 0), at it, and far from it
  const uint32_t tmins[] = {0u, jb ? jb - 1 : 0u, jb, 100000u};
  // per origin the smallest tmin that reached it (the offsets are formed mod 2^32 from t and
  // tmin, but depend on their difference alone: one sweep per origin)
  std::vector<uint32_t> seen((size_t)kOrgN, 0xFFFFFFFFu);
  for (uint32_t tmin : tmins) {
    // num_states: hi clipped right at cmax, inside the jump, and not at all
    for (uint32_t ns_kind = 0; ns_kind < 3; ++ns_kind) {
      for (uint32_t wk = 1; wk <= W; ++wk) {
        // (cmin, cmax) inside [tmin, tmin + wk): the window rule sees cmin and cmax only, so
        // all pairs with cmax = tmin + wk - 1, and all with a smaller cmax under a larger wk
        const uint32_t cmax = tmin + wk - 1;
        const uint32_t ns = ns_kind == 0 ? cmax + 1 : ns_kind == 1 ? cmax + 1 + jf / 2 : 0x7FFFFFFu;
        for (uint32_t cmin = tmin; cmin <= cmax; ++cmin) {
          ++windows;
          const uint32_t tn = pull_win_tn(cmin, jb), hi = pull_win_hi(cmax, jf, ns);
          if (tn > cmin || cmin - tn > jb || (tn != 0 && cmin - tn != jb))
            fail("tn", jb, jf, tn, cmin);
          if (hi < cmax || hi > cmax + jf || hi > ns - 1 || (hi != ns - 1 && hi != cmax + jf))
            fail("hi", jb, jf, hi, cmax);
          if (pull_win_overflow(tn, hi, W)) {
            if (hi - tn + 1 <= W) fail("overflow of a window that fits", jb, jf, tn, hi);
            continue;
          }
          const uint32_t wn = pull_win_wn(tn, hi), rows_n = pull_win_rows(wn);
          if (wn > W || wn == 0 || rows_n * 64 < wn || rows_n * 64 >= wn + 64)
            fail("wn / rows_n", jb, jf, wn, rows_n);
          for (uint32_t e = 0; e < rows_n; ++e) {
            const int64_t ro = (int64_t)tn + 64 * e - (int64_t)tmin;
            if (ro < kOrgLo || ro - kOrgLo >= kOrgN) {
              fail("row origin", jb, jf, ro, e);
              continue;
            }
            uint32_t& sm = seen[(size_t)(ro - kOrgLo)];
            if (tmin < sm) sm = tmin;
          }
        }
      }
    }
  }
  for (int64_t o = 0; o < kOrgN; ++o)
    if (seen[(size_t)o] != 0xFFFFFFFFu) check_row(jb, jf, seen[(size_t)o], o + kOrgLo);
}

}  // namespace

int main() {
  static_assert(pack_guards_fit(kPackSpanMax, 0, W) && pack_guards_fit(0, kPackSpanMax, W) &&
                    pack_guards_fit(20, 43, W),
                "the guards hold the widest span");
  static_assert(!pack_guards_fit(kPackSpanMax + 1, 0, W) && !pack_guards_fit(0, kPackSpanMax + 1, W) &&
                    !pack_guards_fit(32, 32, W),
                "a wider span is refused");
  for (uint32_t jb = 0; jb <= kPackSpanMax; ++jb)
    for (uint32_t jf = 0; jb + jf <= kPackSpanMax; ++jf) {
      const int64_t lo0 = seen_min, hi0 = seen_max;
      seen_min = 1 << 30;
      seen_max = -1;
      check_jumps(jb, jf);
      // the header's bounds hold, and are the ones the gate tests
      if (seen_min < pack_src_cell_min(jb, jf) || seen_max > pack_src_cell_max(jb, jf, W))
        fail("a read beyond the header's bound", jb, jf, seen_min, seen_max);
      if (lo0 < seen_min) seen_min = lo0;
      if (hi0 > seen_max) seen_max = hi0;
    }
  std::printf("pack_guard_check: %llu windows, %llu rows, %llu reads, cells [%lld, %lld] of %lld\n",
              windows, rows, reads, (long long)seen_min, (long long)seen_max, (long long)kCells);
  if (failures) {
    std::fprintf(stderr, "pack_guard_check: %lld check(s) failed\n", failures);
    return 1;
  }
  std::puts("pack_guard_check: ok");
  return 0;
}

// pull_window.hpp -- tier P's window rule and the guard bands of its packed cells, as
// constexpr functions that host and device code share: the kernel (kernels/eager_pull.hpp)
// computes its windows and cell offsets with them, the host gate (eager_pull.hip) decides
// with them whether an rhs may take the packed cells, and tools/pack_guard_check.cpp sweeps
// them on the CPU.
//
// The window rule.  The current layer's tuples sit at states [cmin, cmax], inside a window
// of wk cells whose slot 0 is state tmin (tmin <= cmin <= cmax < tmin + wk, wk <= W).  Every
// arc s -> t of the rhs has t - s in [-jump_back, jump_fwd], so the next layer's states lie
// in [tn, hi]; that becomes the next window (wn cells, rows_n rows of 64 lanes) unless it is
// wider than W cells: OVERFLOW, the string goes to the push tiers.
//
// The guard bands (packed cells, RK 6).  The cell array is kPackGuardLo cells that never
// hold a tuple, the W window cells, then kPackGuardHi more that never hold one; window slot
// i is cell kPackGuardLo + i.  A lane of a window row owns target t = tn + i, i < 64 *
// rows_n, and reads the cell of every in-arc's source s = t - dl, dl in [-jump_back,
// jump_fwd]:
//   t - tmin >= tn - tmin >= -jump_back        (tn = cmin - jump_back >= tmin - jump_back, or
//                                               tn = 0 > tmin - jump_back when clipped)
//   t - tmin <= hi + 63 - tmin                 (64 * rows_n <= wn + 63: the last row runs up
//             <= (wk - 1) + jump_fwd + 63       to 63 lanes past the window; hi <= cmax +
//                                               jump_fwd, cmax <= tmin + wk - 1)
// so with span = jump_back + jump_fwd the source's slot s - tmin lies in
//   [-span, (W - 1) + 63 + span],
// and it is a guard cell whenever it is no window cell.  The lane's base carries the low
// guard, base4 = 4 * (t - tmin + jump_back + kPackGuardLo), and the record holds delta4 = 4 *
// (dl + jump_back) in [0, 4 * span], so base4 - delta4 = 4 * (kPackGuardLo + s - tmin) is
// never negative and needs no clamp.  A block without records holds delta4 = 0 and reads the
// lane's own base, inside the same range.  A row whose label misses takes the constant base
// 4 * (kPackGuardLo - 1): its reads land on cells [kPackGuardLo - 1 - span, kPackGuardLo - 1],
// all in the low guard.  Both need span <= kPackGuardLo - 1 and 63 + span <= kPackGuardHi;
// the one-byte delta4 needs span <= 63 as well.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define FSTAMD_HD __host__ __device__
#else
#define FSTAMD_HD
#endif

namespace fstamd {

// ---- the window rule ----
FSTAMD_HD constexpr uint32_t pull_win_tn(uint32_t cmin, uint32_t jump_back) {
  return cmin >= jump_back ? cmin - jump_back : 0u;
}
// (32-bit: the pull tiers take rhs of fewer than 2^27 states, so cmax + jump_fwd cannot wrap)
FSTAMD_HD constexpr uint32_t pull_win_hi(uint32_t cmax, uint32_t jump_fwd, uint32_t num_states) {
  return cmax + jump_fwd < num_states - 1 ? cmax + jump_fwd : num_states - 1;
}
FSTAMD_HD constexpr bool pull_win_overflow(uint32_t tn, uint32_t hi, uint32_t w) {
  return hi - tn >= w;
}
FSTAMD_HD constexpr uint32_t pull_win_wn(uint32_t tn, uint32_t hi) { return hi - tn + 1; }
FSTAMD_HD constexpr uint32_t pull_win_rows(uint32_t wn) { return (wn + 63) / 64; }

// ---- the packed cells' guard bands ----
constexpr uint32_t kPackGuardLo = 64;   // absent cells below window slot 0
constexpr uint32_t kPackGuardHi = 128;  // absent cells from window slot W on
constexpr uint32_t kPackSpanMax = 63;   // jump_back + jump_fwd: delta4 = 4 * span fits a byte
FSTAMD_HD constexpr uint32_t pack_cells(uint32_t w) { return kPackGuardLo + w + kPackGuardHi; }
// the bounds derived above, as cell indices (slot + kPackGuardLo), for a window of w cells
FSTAMD_HD constexpr int64_t pack_src_cell_min(uint32_t jump_back, uint32_t jump_fwd) {
  return (int64_t)kPackGuardLo - (int64_t)(jump_back + jump_fwd);
}
FSTAMD_HD constexpr int64_t pack_src_cell_max(uint32_t jump_back, uint32_t jump_fwd, uint32_t w) {
  return (int64_t)kPackGuardLo + (int64_t)(w - 1) + 63 + (int64_t)(jump_back + jump_fwd);
}
FSTAMD_HD constexpr int64_t pack_miss_cell_min(uint32_t jump_back, uint32_t jump_fwd) {
  return (int64_t)kPackGuardLo - 1 - (int64_t)(jump_back + jump_fwd);
}
// may an rhs with these jumps take the packed cells in windows of w cells?
FSTAMD_HD constexpr bool pack_guards_fit(uint32_t jump_back, uint32_t jump_fwd, uint32_t w) {
  return (uint64_t)jump_back + jump_fwd <= kPackSpanMax &&
         pack_src_cell_min(jump_back, jump_fwd) >= 0 &&
         pack_miss_cell_min(jump_back, jump_fwd) >= 0 &&
         pack_src_cell_max(jump_back, jump_fwd, w) < (int64_t)pack_cells(w);
}
// byte offset of the lane's own cell plus the record bias: the base of a row lane whose
// label hits (rbias4 = 4 * jump_back, RevView::rbias8 / 2).  Mod 2^32; the true value is
// never negative (t - tmin >= -jump_back)
FSTAMD_HD constexpr uint32_t pack_hit_base4(uint32_t t, uint32_t tmin, uint32_t rbias4) {
  return (t << 2) - (tmin << 2) + rbias4 + 4u * kPackGuardLo;
}
// ... and of a row lane whose label misses: every read lands in the low guard
constexpr uint32_t kPackMissBase4 = 4u * (kPackGuardLo - 1);
// byte offset of the source's cell for a record's delta4 (its top byte)
FSTAMD_HD constexpr uint32_t pack_src_off4(uint32_t base4, uint32_t delta4) { return base4 - delta4; }

}  // namespace fstamd

// pull_kernel_dispatch.hpp -- which instance of the two pull kernels a launch takes (records,
// block size, layout, waves per SIMD), shared by the two translation units that hold the
// instances: eager_pull.hip (TEXT = false: label inputs, every caller but one) and
// text_pull.hip (TEXT = true: the streamed text batch's byte inputs and text emission).  The
// text instances are a compile-time axis in a file of their own, so the label instances'
// code -- and eager_pull.hip's compile time -- stay what they were without them.  So are the
// weight-code instances of tier P (CODES = true, code_pull.hip).
#pragma once

#include <cstdio>
#include <cstdlib>

#include "device_engine.hpp"
#include "kernels/eager_pull.hpp"
#include "kernels/lazy_pull.hpp"

namespace fstamd {

namespace {
// Waves per SIMD the compiler targets: 5 fit spill-free with blocks of <= 5 records (the
// metric: 5 waves 20.3 M strings/s, 4 waves 18.5 M, 6 waves 19.8 M with spills);
// 8-record blocks need 4.

// RK: the records the kernel reads -- 0 RevRec (f64 cells), 1 rrec32, 2 rrec8 (f32 cells)
template <int KP, int WV, int RK, bool TEXT, bool CODES = false>
const void* pull_kernel_ptr(bool direct) {
  return direct ? (const void*)eager_pull_kernel<kPullRows, KP, true, WV, RK, TEXT, CODES>
                : (const void*)eager_pull_kernel<kPullRows, KP, false, WV, RK, TEXT, CODES>;
}
#ifndef FSTAMD_PULL_WAVES_SMALL  // A/B builds: waves per SIMD for blocks of <= 5 records
#define FSTAMD_PULL_WAVES_SMALL 5
#endif
#ifndef FSTAMD_PULL_WAVES_F32  // A/B builds: the same with f32 cells (8-B cells, f32 merge)
#define FSTAMD_PULL_WAVES_F32 6
#endif
// (RK 6, the packed cells: 7 waves as RK 3 -- see DESIGN.md §3.1 for the 7-against-8 A/B)
// ... and with the 8-B records: 7 waves (3 VGPRs spilled outside the layer loop) measured
// 37.1 ms per 1M metric strings, 6 waves 37.7 ms, 8 waves (10 spilled) 38.9 ms
#ifndef FSTAMD_PULL_WAVES_R8
#define FSTAMD_PULL_WAVES_R8 7
#endif
#ifndef FSTAMD_PULL_WAVES_PACK  // A/B builds: the same with packed cells (RK 6)
#define FSTAMD_PULL_WAVES_PACK FSTAMD_PULL_WAVES_R8
#endif
template <int RK, bool TEXT, bool CODES = false>
const void* pull_kernel_for(const RevView& rv) {
  const bool dir = rv.direct != 0;
  if constexpr (RK == 6) {  // (the direct layout only: DeviceFst::pack)
    switch (rv.kp) {
      case 4: return (const void*)eager_pull_kernel<kPullRows, 4, true, FSTAMD_PULL_WAVES_PACK, 6, TEXT, CODES>;
      case 5: return (const void*)eager_pull_kernel<kPullRows, 5, true, FSTAMD_PULL_WAVES_PACK, 6, TEXT, CODES>;
      default: return (const void*)eager_pull_kernel<kPullRows, 8, true, 4, 6, TEXT, CODES>;
    }
  } else {
    constexpr int wv = RK == 5 ? 4  // (f64 cells and a 2 KB weight table: 8.9 KB of LDS)
                     : RK == 4 ? FSTAMD_PULL_WAVES_SMALL  // (f64 cells)
                     : RK >= 2 ? FSTAMD_PULL_WAVES_R8 : RK ? FSTAMD_PULL_WAVES_F32 : FSTAMD_PULL_WAVES_SMALL;
    switch (rv.kp) {
      case 4: return pull_kernel_ptr<4, wv, RK, TEXT, CODES>(dir);
      case 5: return pull_kernel_ptr<5, wv, RK, TEXT, CODES>(dir);
      default: return pull_kernel_ptr<8, 4, RK, TEXT, CODES>(dir);
    }
  }
}
// the 8-B records when the rhs has them (every weight an integer <= kRec8WMax)
bool use_rec8(const RevView& rv) { return rv.rrec8 && !std::getenv("FSTAMD_NO_REC8"); }
// FSTAMD_ROUTE_LOG: which records the pull kernel reads (0 RevRec / f64 cells, 1 rrec32,
// 2 rrec8, 3 rrec4, 4 rrec4 with weight indices and f64 cells, 5 the same with a 256-entry
// table) and the weight scale 2^k of
// the integer records (tests)
int route_rk(const char* sem, int rk, const RevView& rv, bool log) {
  if (log && std::getenv("FSTAMD_ROUTE_LOG"))
    std::fprintf(stderr, "[libfst_amd route] %s pull: records %d, weight scale %g\n", sem, rk,
                 rk && rk < 4 ? 1.0 / rv.winv : 1.0);
  return rk;
}
int pull_rk(const DeviceFst& rhs, uint32_t max_len) {
  if (!pull_f32(rhs, max_len) || std::getenv("FSTAMD_P_F64"))  // f64 cells
    return rhs.rev.rrec4 && rhs.widx && !std::getenv("FSTAMD_NO_REC4")
               ? (rhs.wt_n <= kPullWt ? 4 : 5)
               : 0;
  if (rhs.rev.rrec4 && use_rec8(rhs.rev) && !std::getenv("FSTAMD_NO_REC4")) return 3;
  return use_rec8(rhs.rev) ? 2 : 1;
}
// RK 3 with packed (distance, key) cells (RK 6 of the kernel; the log still says records 3):
// the rhs has the packed records, and no distance field of the launch can wrap -- real
// distances stay below 0x7F00, and an absent slot's, which starts there and may grow by a
// weight per layer, below 2^16.  Strings longer than max_len are handed on by the kernel.
// FSTAMD_NO_PACK=1: the unpacked RK 3 path (read per call)
bool pull_pack(const DeviceFst& rhs, uint32_t max_len) {
  return rhs.pack && pull_rk(rhs, max_len) == 3 &&
         ((double)max_len + 1.0) * rhs.int_wmax < (double)0x7F00 && !std::getenv("FSTAMD_NO_PACK");
}
template <bool TEXT>
const void* pull_kernel_for(const DeviceFst& rhs, uint32_t max_len, bool log = false) {
  const int rk = route_rk("eager", pull_rk(rhs, max_len), rhs.rev, log);
  if (rk == 3) {
    const bool pack = pull_pack(rhs, max_len);
    if (log && std::getenv("FSTAMD_ROUTE_LOG"))
      std::fprintf(stderr, "[libfst_amd route] eager pull: packed cells %s\n", pack ? "on" : "off");
    if (pack) return pull_kernel_for<6, TEXT>(rhs.rev);
  }
  switch (rk) {
    case 0: return pull_kernel_for<0, TEXT>(rhs.rev);
    case 5: return pull_kernel_for<5, TEXT>(rhs.rev);
    case 4: return pull_kernel_for<4, TEXT>(rhs.rev);
    case 3: return pull_kernel_for<3, TEXT>(rhs.rev);
    case 2: return pull_kernel_for<2, TEXT>(rhs.rev);
    default: return pull_kernel_for<1, TEXT>(rhs.rev);
  }
}
// Lazy pull: 4 waves per SIMD with f64 cells (10.0 KB of LDS; round 5: 3 at 12.8 KB), 5
// with f32 cells (7.4 KB; round 3: 4 at 10.2 KB) when every distance is an integer below
// 2^24.
#ifndef FSTAMD_LP_WAVES_F32  // A/B builds
#define FSTAMD_LP_WAVES_F32 5
#endif
#ifndef FSTAMD_LP_WAVES_F64
#define FSTAMD_LP_WAVES_F64 4
#endif
constexpr int kLazyPullWaves = 3;
// B1: 1-B back records (DeviceFst::byte_back; the direct layout only)
template <int KP, int RK, bool TEXT>
const void* lazy_pull_ptr(bool direct, bool b1) {
  constexpr int wv = KP > 5 ? kLazyPullWaves  // (8-record blocks spill at 4)
                   : RK ? FSTAMD_LP_WAVES_F32 : FSTAMD_LP_WAVES_F64;
  if (!direct) return (const void*)lazy_pull_kernel<kPullRows, KP, false, wv, RK, false, TEXT>;
  return b1 ? (const void*)lazy_pull_kernel<kPullRows, KP, true, wv, RK, true, TEXT>
            : (const void*)lazy_pull_kernel<kPullRows, KP, true, wv, RK, false, TEXT>;
}
template <int RK, bool TEXT>
const void* lazy_pull_kernel_for(const DeviceFst& rhs) {
  const bool dir = rhs.rev.direct != 0, b1 = dir && rhs.byte_back;
  switch (rhs.rev.kp) {
    case 4: return lazy_pull_ptr<4, RK, TEXT>(dir, b1);
    case 5: return lazy_pull_ptr<5, RK, TEXT>(dir, b1);
    default: return lazy_pull_ptr<8, RK, TEXT>(dir, b1);
  }
}
template <bool TEXT>
const void* lazy_pull_kernel_for(const DeviceFst& rhs, uint32_t max_len, bool log = false) {
  const int rk = !lazy_pull_f32(rhs, max_len) ? 0 : use_rec8(rhs.rev) ? 2 : 1;
  if (log && std::getenv("FSTAMD_ROUTE_LOG"))
    std::fprintf(stderr, "[libfst_amd route] lazy pull: back records %d B\n",
                 rhs.rev.direct && rhs.byte_back ? 1 : 4);
  switch (route_rk("lazy", rk, rhs.rev, log)) {
    case 0: return lazy_pull_kernel_for<0, TEXT>(rhs);
    case 2: return lazy_pull_kernel_for<2, TEXT>(rhs);
    default: return lazy_pull_kernel_for<1, TEXT>(rhs);
  }
}
}  // namespace

}  // namespace fstamd

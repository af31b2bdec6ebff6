// sp_validator_check.cpp -- the argument checks of the lhs batch entries on edge inputs, as a
// stand-alone program for a sanitizer build of the host sources (no GPU needed: every call here
// ends at the validator, at the empty result, or at the GPU check that follows them).  The same
// inputs go through every host entry that takes an FstLhsBatch -- the lhs batch, the two lhs
// pipelines, the lattice lhs batch, connect, shortest path -- and the three device entries get
// their null-pointer and unknown-flag checks.
//
// Build (from libfst_amd/csrc, after `make`): compile the host units with
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off
//         -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c <unit>.cpp
// for host_fst, c_api, host_rt, batch_sharded, batch_lhs, batch_streamed and batch_entries, and
// link them with this file (same flags) and the release build/*.hip.o objects:
//   hipcc -fsanitize=address,undefined --offload-arch=gfx950 -o sp_validator_check ...
// Exit code 0 and no sanitizer report: every check below held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/fst_batch.h"

namespace {

int failures = 0;
std::string entry_name;  // the entry under test, for the messages

void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s: %s\n", entry_name.c_str(), what);
    ++failures;
  }
}

template <class R>
bool zeroed(const R& r) {
  const R z{};
  return std::memcmp(&r, &z, sizeof(r)) == 0;
}

template <class R>
R poisoned() {
  R r;
  std::memset(&r, 0x5A, sizeof(r));
  return r;
}

// An entry on an lhs batch: its call (n where it takes one), its result's release, the item
// count of a result and whether a result is the empty one with its closing offsets.
template <class R>
struct Entry {
  const char* name;
  std::function<FstError(const FstLhsBatch*, uint32_t, const FstBatchOptions*, R*)> call;
  void (*release)(R*);
};
uint32_t items(const FstBatchResult& r) { return r.num_strings; }
uint32_t items(const FstTextResult& r) { return r.num_strings; }
uint32_t items(const FstLatticeBatch& r) { return r.fsts.num_fsts; }
bool empty_ok(const FstBatchResult& r) {
  return r.num_strings == 0 && r.total_arcs == 0 && r.path_offsets && r.path_offsets[0] == 0;
}
bool empty_ok(const FstTextResult& r) {
  return r.num_strings == 0 && r.total_bytes == 0 && r.text_offsets && r.text_offsets[0] == 0;
}
bool empty_ok(const FstLatticeBatch& r) {
  return r.fsts.num_fsts == 0 && r.total_states == 0 && r.total_arcs == 0 &&
         r.fsts.state_offsets && r.fsts.state_offsets[0] == 0 && r.fsts.arc_offsets &&
         r.fsts.arc_offsets[0] == 0;
}

struct Batch {
  std::vector<uint64_t> so, ao;
  std::vector<uint32_t> start, il, ol, nx;
  std::vector<double> fin, w;
  FstLhsBatch view() const {
    FstLhsBatch L{};
    L.num_fsts = (uint32_t)start.size();
    L.state_offsets = so.data();
    L.start = start.data();
    L.final_weights = fin.data();
    L.arc_offsets = ao.data();
    L.ilabels = il.data();
    L.olabels = ol.data();
    L.weights = w.data();
    L.nextstates = nx.data();
    return L;
  }
};

// `items` items of `states` states each, state s with one arc to state (s + 1) % states.
Batch ring_batch(uint32_t items, uint32_t states) {
  Batch b;
  b.so.push_back(0);
  b.ao.push_back(0);
  for (uint32_t i = 0; i < items; ++i) {
    b.start.push_back(states ? 0u : FST_NO_STATE);
    for (uint32_t s = 0; s < states; ++s) {
      b.fin.push_back(s + 1 == states ? 0.0 : __builtin_huge_val());
      b.il.push_back(1);
      b.ol.push_back(2);
      b.w.push_back(0.5);
      b.nx.push_back((s + 1) % states);
      b.ao.push_back(b.il.size());
    }
    b.so.push_back(b.fin.size());
  }
  return b;
}

// A valid batch passes the validator; what follows needs a GPU.  Without one the entry returns
// FST_INVALID_ARG with *out zeroed, with one FST_OK and a result of the right size.
template <class R>
void expect_valid(const Entry<R>& E, const FstLhsBatch& L, uint32_t n, const char* what) {
  R r = poisoned<R>();
  const FstError e = E.call(&L, n, nullptr, &r);
  if (e == FST_OK) {
    expect(items(r) == L.num_fsts, what);
    E.release(&r);
  } else {
    expect(e == FST_INVALID_ARG && zeroed(r), what);
  }
}

template <class R>
void expect_invalid(const Entry<R>& E, const FstLhsBatch* L, const FstBatchOptions* o,
                    const char* what) {
  R r = poisoned<R>();
  expect(E.call(L, 1, o, &r) == FST_INVALID_ARG && zeroed(r), what);
}

template <class R>
void expect_invalid_batch(const Entry<R>& E, const Batch& b, const char* what) {
  const FstLhsBatch L = b.view();
  expect_invalid(E, &L, nullptr, what);
}

template <class R>
void check_entry(const Entry<R>& E) {
  entry_name = E.name;
  // null pointers
  {
    const Batch b = ring_batch(2, 3);
    const FstLhsBatch L = b.view();
    expect(E.call(&L, 1, nullptr, nullptr) == FST_INVALID_ARG, "null out");
    expect_invalid(E, nullptr, nullptr, "null lhs");
  }
  // zero items: the empty OK result, whatever n is and with no array at all
  for (uint32_t n : {0u, 1u, 2u}) {
    FstLhsBatch L{};
    R r = poisoned<R>();
    expect(E.call(&L, n, nullptr, &r) == FST_OK, "zero items");
    expect(empty_ok(r), "zero items: the closing offsets");
    E.release(&r);
    expect(zeroed(r), "zero items: freed");
  }
  // zero-state items: no final weights, no arcs, arc_offsets = {0}
  {
    Batch b = ring_batch(5, 0);
    FstLhsBatch L = b.view();
    expect_valid(E, L, 1, "zero-state items");
    L.final_weights = nullptr;
    L.ilabels = L.olabels = L.nextstates = nullptr;
    L.weights = nullptr;
    expect_valid(E, L, 1, "zero-state items without the arrays they do not need");
    b.start[2] = 0;  // a start in an item without states
    expect_invalid(E, &L, nullptr, "a start beyond an empty item");
  }
  // zero-state items between others, one-state items, self loops
  {
    Batch b = ring_batch(3, 1);
    b.so.insert(b.so.begin() + 2, b.so[1]);  // an empty item after the first
    b.start.insert(b.start.begin() + 1, FST_NO_STATE);
    expect_valid(E, b.view(), 1, "an empty item between one-state items");
    expect_valid(E, b.view(), 0, "n = 0");
    expect_valid(E, b.view(), 7, "n = 7");
  }
  // every malformed offset, start and nextstate
  {
    const Batch good = ring_batch(3, 4);
    expect_valid(E, good.view(), 1, "rings");
    Batch b = good;
    b.so[1] = b.so[2] + 1;
    expect_invalid_batch(E, b, "decreasing state offsets");
    b = good;
    b.ao[0] = 1;
    expect_invalid_batch(E, b, "arc_offsets[0] != 0");
    b = good;
    b.ao[5] = b.ao[4] - 1;
    expect_invalid_batch(E, b, "decreasing arc offsets");
    b = good;
    b.start[1] = 4;
    expect_invalid_batch(E, b, "start == the item's state count");
    b = good;
    b.nx.back() = 4;
    expect_invalid_batch(E, b, "the last nextstate one too large");
    b = good;
    b.nx.front() = 0xFFFFFFFFu;
    expect_invalid_batch(E, b, "nextstate = FST_NO_STATE");
    FstBatchOptions o{};
    o.device = -1;
    o.flags = 2;
    const FstLhsBatch L = good.view();
    expect_invalid(E, &L, &o, "an unknown option flag");
  }
  // the size limits, which the validator decides before it reads what it could not hold: 2^30
  // states in one item (from the state offsets alone), 2^32 arcs on one state
  {
    const uint64_t so[2] = {0, 1ull << 30};
    const uint32_t start[1] = {0};
    const double fin[1] = {0.0};
    const uint64_t ao[2] = {0, 0};
    FstLhsBatch L{};
    L.num_fsts = 1;
    L.state_offsets = so;
    L.start = start;
    L.final_weights = fin;
    L.arc_offsets = ao;
    expect_invalid(E, &L, nullptr, "2^30 states in one item");
    const uint64_t so1[2] = {0, 1};
    const uint64_t ao1[2] = {0, 1ull << 32};
    const uint32_t one[1] = {0};
    const double w[1] = {0.0};
    L.state_offsets = so1;
    L.arc_offsets = ao1;
    L.ilabels = L.olabels = L.nextstates = one;
    L.weights = w;
    expect_invalid(E, &L, nullptr, "2^32 arcs on one state");
  }
  // the largest offsets that are accepted and still fit in memory here: one item of 2^20 states
  // in a ring, and 2^16 items of one state
  expect_valid(E, ring_batch(1, 1u << 20).view(), 1, "one item of 2^20 states");
  expect_valid(E, ring_batch(1u << 16, 1).view(), 1, "2^16 one-state items");
}

// The three device entries: every null pointer and unknown flag is refused before anything is
// read or run (the pointers here are host memory, so nothing may be dereferenced).
void check_device_entries(FstHandle rhs) {
  const Batch b = ring_batch(2, 3);
  const FstLhsBatch L = b.view();
  int32_t st[2];
  uint32_t len[2], start[2], arcs32[8];
  uint64_t off[3], cursor[1], needed[2];
  double fin[8], w[8];
  const FstDeviceBatch good{st, len, off, fin, arcs32, arcs32, w, 8, cursor, nullptr};
  FstBatchOptions bad_flags{};
  bad_flags.device = -1;
  bad_flags.flags = 2;
  FstBatchOptions bad_sem{};
  bad_sem.device = -1;
  bad_sem.semantics = 7;
  struct Case {
    const char* what;
    const FstLhsBatch* lhs;
    FstDeviceBatch out;
    bool null_out;
    const FstBatchOptions* opts;
  };
  std::vector<Case> cases = {{"null out", &L, good, true, nullptr},
                             {"null lhs", nullptr, good, false, nullptr},
                             {"an unknown option flag", &L, good, false, &bad_flags}};
  FstLhsBatch Lx = L;
  Lx.state_offsets = nullptr;
  cases.push_back({"null state offsets", &Lx, good, false, nullptr});
  FstLhsBatch Ly = L;
  Ly.start = nullptr;
  cases.push_back({"null starts", &Ly, good, false, nullptr});
  FstLhsBatch Lz = L;
  Lz.arc_offsets = nullptr;
  cases.push_back({"null arc offsets", &Lz, good, false, nullptr});
  FstDeviceBatch o = good;
  o.arc_cursor = nullptr;
  cases.push_back({"null arc cursor", &L, o, false, nullptr});
  o = good;
  o.status = nullptr;
  cases.push_back({"null statuses", &L, o, false, nullptr});
  o = good;
  o.path_len = nullptr;
  cases.push_back({"null path lengths", &L, o, false, nullptr});
  o = good;
  o.path_offset = nullptr;
  cases.push_back({"null path offsets", &L, o, false, nullptr});
  o = good;
  o.final_weight = nullptr;
  cases.push_back({"null final weights", &L, o, false, nullptr});
  for (const Case& c : cases) {
    const FstDeviceBatch* out = c.null_out ? nullptr : &c.out;
    entry_name = "fst_device_compose_shortest_path_lhs";
    expect(fst_device_compose_shortest_path_lhs(rhs, c.lhs, 1, c.opts, out, nullptr) ==
               FST_INVALID_ARG,
           c.what);
    entry_name = "fst_device_shortest_path_lhs";
    expect(fst_device_shortest_path_lhs(c.lhs, 1, c.opts, out, nullptr) == FST_INVALID_ARG, c.what);
  }
  entry_name = "fst_device_compose_shortest_path_lhs";
  expect(fst_device_compose_shortest_path_lhs(rhs, &L, 1, &bad_sem, &good, nullptr) ==
             FST_INVALID_ARG,
         "unknown semantics");
  expect(fst_device_compose_shortest_path_lhs(rhs + 12345, &L, 1, nullptr, &good, nullptr) ==
             FST_INVALID_ARG,
         "a stale rhs handle");

  entry_name = "fst_device_compose_frozen";
  const uint64_t d_off[3] = {0, 1, 2};
  const uint32_t d_lab[2] = {1, 1};
  const FstDeviceLattices lat{st, off, start, fin, off, arcs32, arcs32, w, arcs32, 8, 8};
  auto frozen = [&](FstHandle h, const uint64_t* offsets, uint32_t lattice_flags,
                    const FstBatchOptions* opts, const FstDeviceLattices* out, uint64_t* need) {
    return fst_device_compose_frozen(h, d_lab, offsets, 2, 1, lattice_flags, opts, out, need,
                                     nullptr);
  };
  expect(frozen(rhs, d_off, 0, nullptr, nullptr, needed) == FST_INVALID_ARG, "null out");
  expect(frozen(rhs, d_off, 0, nullptr, &lat, nullptr) == FST_INVALID_ARG, "null needed");
  expect(frozen(rhs, nullptr, 0, nullptr, &lat, needed) == FST_INVALID_ARG, "null offsets");
  expect(frozen(rhs, d_off, 0, &bad_flags, &lat, needed) == FST_INVALID_ARG,
         "an unknown option flag");
  expect(frozen(rhs, d_off, 2, nullptr, &lat, needed) == FST_INVALID_ARG,
         "an unknown lattice flag");
  expect(frozen(rhs + 12345, d_off, 0, nullptr, &lat, needed) == FST_INVALID_ARG,
         "a stale rhs handle");
  FstDeviceLattices l2 = lat;
  l2.state_offsets = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG, "null state offsets");
  l2 = lat;
  l2.arc_offsets = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG, "null arc offsets");
  l2 = lat;
  l2.status = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG, "null statuses");
  l2 = lat;
  l2.start = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG, "null starts");
  l2 = lat;
  l2.final_weights = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG,
         "a state capacity without final weights");
  l2 = lat;
  l2.nextstates = nullptr;
  expect(frozen(rhs, d_off, 0, nullptr, &l2, needed) == FST_INVALID_ARG,
         "an arc capacity without nextstates");
}

}  // namespace

int main() {
  const FstHandle rhs = fst_bench_transducer(0, 4, 2);
  entry_name = "setup";
  expect(rhs != UINT64_MAX, "the rhs");
  const FstHandle two[2] = {rhs, rhs};
  check_entry(Entry<FstBatchResult>{
      "fst_shortest_path_lhs_batch",
      [](const FstLhsBatch* L, uint32_t n, const FstBatchOptions* o, FstBatchResult* r) {
        return fst_shortest_path_lhs_batch(L, n, o, r);
      },
      fst_batch_result_free});
  check_entry(Entry<FstBatchResult>{
      "fst_compose_frozen_shortest_path_lhs_batch",
      [=](const FstLhsBatch* L, uint32_t n, const FstBatchOptions* o, FstBatchResult* r) {
        return fst_compose_frozen_shortest_path_lhs_batch(rhs, L, n, o, r);
      },
      fst_batch_result_free});
  check_entry(Entry<FstBatchResult>{
      "fst_pipeline_lhs_batch",
      [&](const FstLhsBatch* L, uint32_t n, const FstBatchOptions* o, FstBatchResult* r) {
        return fst_pipeline_lhs_batch(two, 2, L, n, o, r);
      },
      fst_batch_result_free});
  check_entry(Entry<FstTextResult>{
      "fst_normalize_lhs_batch",
      [&](const FstLhsBatch* L, uint32_t, const FstBatchOptions* o, FstTextResult* r) {
        return fst_normalize_lhs_batch(two, 2, L, o, r);
      },
      fst_text_result_free});
  check_entry(Entry<FstLatticeBatch>{
      "fst_compose_frozen_lhs_batch",
      [=](const FstLhsBatch* L, uint32_t, const FstBatchOptions* o, FstLatticeBatch* r) {
        return fst_compose_frozen_lhs_batch(rhs, L, FST_LATTICE_CONNECT, o, r);
      },
      fst_lattice_batch_free});
  check_entry(Entry<FstLatticeBatch>{
      "fst_connect_lhs_batch",
      [](const FstLhsBatch* L, uint32_t, const FstBatchOptions* o, FstLatticeBatch* r) {
        return fst_connect_lhs_batch(L, o, r);
      },
      fst_lattice_batch_free});
  // the pipeline entries' own checks: no stages, a stale stage handle
  {
    entry_name = "fst_pipeline_lhs_batch";
    const Batch b = ring_batch(2, 3);
    const FstLhsBatch L = b.view();
    const FstHandle stale[2] = {rhs, rhs + 12345};
    FstBatchResult r = poisoned<FstBatchResult>();
    expect(fst_pipeline_lhs_batch(nullptr, 2, &L, 1, nullptr, &r) == FST_INVALID_ARG && zeroed(r),
           "null stages");
    r = poisoned<FstBatchResult>();
    expect(fst_pipeline_lhs_batch(two, 0, &L, 1, nullptr, &r) == FST_INVALID_ARG && zeroed(r),
           "no stages");
    r = poisoned<FstBatchResult>();
    expect(fst_pipeline_lhs_batch(stale, 2, &L, 1, nullptr, &r) == FST_INVALID_ARG && zeroed(r),
           "a stale stage handle");
    entry_name = "fst_normalize_lhs_batch";
    FstTextResult t = poisoned<FstTextResult>();
    expect(fst_normalize_lhs_batch(stale, 2, &L, nullptr, &t) == FST_INVALID_ARG && zeroed(t),
           "a stale stage handle");
  }
  check_device_entries(rhs);
  if (failures) return 1;
  std::puts("sp_validator_check: ok");
  return 0;
}

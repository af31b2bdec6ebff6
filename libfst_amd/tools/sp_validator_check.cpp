// sp_validator_check.cpp -- the argument checks of fst_shortest_path_lhs_batch on edge inputs,
// as a stand-alone program for a sanitizer build of the host sources (no GPU needed: every call
// here ends at the validator, at the empty result, or at the GPU check that follows them).
//
// Build (from libfst_amd/csrc, after `make`): compile the host units with
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off
//         -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c <unit>.cpp
// for host_fst, c_api, host_rt, batch_sharded, batch_streamed and batch_entries, and link them
// with this file (same flags) and the release build/*.hip.o objects:
//   hipcc -fsanitize=address,undefined --offload-arch=gfx950 -o sp_validator_check ...
// Exit code 0 and no sanitizer report: every check below held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fst_batch.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

bool zeroed(const FstBatchResult& r) {
  const FstBatchResult z{};
  return std::memcmp(&r, &z, sizeof(r)) == 0;
}

FstBatchResult poisoned() {
  FstBatchResult r;
  std::memset(&r, 0x5A, sizeof(r));
  return r;
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
void expect_valid(const FstLhsBatch& L, uint32_t n, const char* what) {
  FstBatchResult r = poisoned();
  const FstError e = fst_shortest_path_lhs_batch(&L, n, nullptr, &r);
  if (e == FST_OK) {
    expect(r.num_strings == L.num_fsts, what);
    fst_batch_result_free(&r);
  } else {
    expect(e == FST_INVALID_ARG && zeroed(r), what);
  }
}

void expect_invalid(const FstLhsBatch* L, const FstBatchOptions* o, const char* what) {
  FstBatchResult r = poisoned();
  expect(fst_shortest_path_lhs_batch(L, 1, o, &r) == FST_INVALID_ARG && zeroed(r), what);
}

void expect_invalid_batch(const Batch& b, const char* what) {
  const FstLhsBatch L = b.view();
  expect_invalid(&L, nullptr, what);
}

}  // namespace

int main() {
  // null pointers
  {
    const Batch b = ring_batch(2, 3);
    const FstLhsBatch L = b.view();
    expect(fst_shortest_path_lhs_batch(&L, 1, nullptr, nullptr) == FST_INVALID_ARG, "null out");
    expect_invalid(nullptr, nullptr, "null lhs");
  }
  // zero items: the empty OK result, whatever n is and with no array at all
  for (uint32_t n : {0u, 1u, 2u}) {
    FstLhsBatch L{};
    FstBatchResult r = poisoned();
    expect(fst_shortest_path_lhs_batch(&L, n, nullptr, &r) == FST_OK, "zero items");
    expect(r.num_strings == 0 && r.total_arcs == 0 && r.path_offsets && r.path_offsets[0] == 0,
           "zero items: the closing offset");
    fst_batch_result_free(&r);
    expect(zeroed(r), "zero items: freed");
  }
  // zero-state items: no final weights, no arcs, arc_offsets = {0}
  {
    Batch b = ring_batch(5, 0);
    FstLhsBatch L = b.view();
    expect_valid(L, 1, "zero-state items");
    L.final_weights = nullptr;
    L.ilabels = L.olabels = L.nextstates = nullptr;
    L.weights = nullptr;
    expect_valid(L, 1, "zero-state items without the arrays they do not need");
    b.start[2] = 0;  // a start in an item without states
    expect_invalid(&L, nullptr, "a start beyond an empty item");
  }
  // zero-state items between others, one-state items, self loops
  {
    Batch b = ring_batch(3, 1);
    b.so.insert(b.so.begin() + 2, b.so[1]);  // an empty item after the first
    b.start.insert(b.start.begin() + 1, FST_NO_STATE);
    expect_valid(b.view(), 1, "an empty item between one-state items");
    expect_valid(b.view(), 0, "n = 0");
    expect_valid(b.view(), 7, "n = 7");
  }
  // every malformed offset, start and nextstate
  {
    const Batch good = ring_batch(3, 4);
    expect_valid(good.view(), 1, "rings");
    Batch b = good;
    b.so[1] = b.so[2] + 1;
    expect_invalid_batch(b, "decreasing state offsets");
    b = good;
    b.ao[0] = 1;
    expect_invalid_batch(b, "arc_offsets[0] != 0");
    b = good;
    b.ao[5] = b.ao[4] - 1;
    expect_invalid_batch(b, "decreasing arc offsets");
    b = good;
    b.start[1] = 4;
    expect_invalid_batch(b, "start == the item's state count");
    b = good;
    b.nx.back() = 4;
    expect_invalid_batch(b, "the last nextstate one too large");
    b = good;
    b.nx.front() = 0xFFFFFFFFu;
    expect_invalid_batch(b, "nextstate = FST_NO_STATE");
    FstBatchOptions o{};
    o.device = -1;
    o.flags = 2;
    const FstLhsBatch L = good.view();
    expect_invalid(&L, &o, "an unknown option flag");
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
    expect_invalid(&L, nullptr, "2^30 states in one item");
    const uint64_t so1[2] = {0, 1};
    const uint64_t ao1[2] = {0, 1ull << 32};
    const uint32_t one[1] = {0};
    const double w[1] = {0.0};
    L.state_offsets = so1;
    L.arc_offsets = ao1;
    L.ilabels = L.olabels = L.nextstates = one;
    L.weights = w;
    expect_invalid(&L, nullptr, "2^32 arcs on one state");
  }
  // the largest offsets that are accepted and still fit in memory here: one item of 2^20 states
  // in a ring, and 2^16 items of one state
  expect_valid(ring_batch(1, 1u << 20).view(), 1, "one item of 2^20 states");
  expect_valid(ring_batch(1u << 16, 1).view(), 1, "2^16 one-state items");
  if (failures) return 1;
  std::puts("sp_validator_check: ok");
  return 0;
}

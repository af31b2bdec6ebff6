// align_host_check.cpp -- the host side of the aligned text entries on edge inputs, as a
// stand-alone program for a sanitizer build of the host sources (no GPU needed: every call here
// is the host conversion, or ends at an argument check or at the empty result).
//   - fst_batch_result_to_aligned_text against the definition of fst_batch.h, restated below,
//     on hand-built results: zero arcs, all-epsilon outputs, eps:y arcs before, between and
//     after consuming arcs, non-OK strings between OK ones, olabels above 256, and paths whose
//     lengths straddle 64;
//   - fst_normalize_text_aligned_batch's argument checks, with *out zeroed where
//     fst_normalize_text_batch zeroes its own, and the empty result.
//
// Build (from libfst_amd/csrc, after `make`): compile the host units with
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off
//         -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -c <unit>.cpp
// for host_fst, c_api, host_rt, batch_sharded, batch_lhs, batch_streamed and batch_entries, and
// link them with this file (same flags) and the release build/*.hip.o objects:
//   hipcc -fsanitize=address,undefined --offload-arch=gfx950 -o align_host_check ...
// Exit code 0 and no sanitizer report: every check below held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/fst_batch.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int id = -1) {
  if (!ok) {
    std::fprintf(stderr, "FAILED: %s (%d)\n", what, id);
    ++failures;
  }
}

struct Path {
  int32_t status;
  std::vector<uint32_t> il, ol;
};

struct Built {
  std::vector<int32_t> status;
  std::vector<uint64_t> off;
  std::vector<uint32_t> il, ol;
  std::vector<double> w, fin;
  FstBatchResult view() {
    FstBatchResult r{};
    r.num_strings = (uint32_t)status.size();
    r.status = status.data();
    r.path_offsets = off.data();
    r.ilabels = il.data();
    r.olabels = ol.data();
    r.weights = w.data();
    r.final_weights = fin.data();
    r.total_arcs = off.back();
    return r;
  }
};

Built build(const std::vector<Path>& paths) {
  Built b;
  b.off.push_back(0);
  for (const Path& p : paths) {
    b.status.push_back(p.status);
    b.il.insert(b.il.end(), p.il.begin(), p.il.end());
    b.ol.insert(b.ol.end(), p.ol.begin(), p.ol.end());
    b.w.insert(b.w.end(), p.il.size(), 0.5);
    b.fin.push_back(0.25);
    b.off.push_back(b.il.size());
  }
  return b;
}

// The definition: per non-epsilon olabel the interval of the inputs its arc consumed.
void model(const Path& p, std::vector<uint32_t>* b, std::vector<uint32_t>* e) {
  uint32_t n = 0;
  for (size_t k = 0; k < p.il.size(); ++k) {
    const uint32_t step = p.il[k] != 0;
    if (p.ol[k] != 0) {
      b->push_back(n);
      e->push_back(n + step);
    }
    n += step;
  }
}

void check_conversion(const std::vector<Path>& paths, int id) {
  Built in = build(paths);
  const FstBatchResult r = in.view();
  FstAlignedTextResult a;
  FstTextResult t;
  std::memset(&a, 0x5A, sizeof(a));
  std::memset(&t, 0x5A, sizeof(t));
  expect(fst_batch_result_to_aligned_text(&r, &a) == FST_OK, "conversion", id);
  expect(fst_batch_result_to_text(&r, &t) == FST_OK, "text conversion", id);
  const uint32_t num = r.num_strings;
  expect(a.num_strings == num && t.num_strings == num && a.total_bytes == t.total_bytes,
         "sizes", id);
  expect(std::memcmp(a.status, t.status, num * 4ull) == 0, "status", id);
  expect(std::memcmp(a.text_offsets, t.text_offsets, (num + 1ull) * 8) == 0, "offsets", id);
  expect(std::memcmp(a.total_weight, t.total_weight, num * 8ull) == 0, "weights", id);
  expect(std::memcmp(a.text, t.text, t.total_bytes) == 0, "text", id);
  for (uint32_t i = 0; i < num; ++i) {
    std::vector<uint32_t> b, e;
    bool bytes = paths[i].status == FST_PATH_OK;
    for (uint32_t x : paths[i].ol) bytes = bytes && x <= 256u;
    if (bytes) model(paths[i], &b, &e);
    const uint64_t lo = a.text_offsets[i], hi = a.text_offsets[i + 1];
    expect(hi - lo == b.size(), "entries per string", id);
    if (hi - lo != b.size()) continue;
    for (uint64_t j = lo; j < hi; ++j)
      expect(a.in_begin[j] == b[j - lo] && a.in_end[j] == e[j - lo], "interval", id);
  }
  fst_aligned_text_result_free(&a);
  fst_text_result_free(&t);
  const FstAlignedTextResult z{};
  expect(std::memcmp(&a, &z, sizeof(a)) == 0, "freed result is zeroed", id);
  fst_aligned_text_result_free(&a);  // a second free is a no-op
}

void conversions() {
  const int32_t OK = FST_PATH_OK, EMPTY = FST_PATH_EMPTY, CYCLE = FST_PATH_CYCLE;
  check_conversion({}, 0);
  check_conversion({{OK, {}, {}}}, 1);                               // zero arcs
  check_conversion({{OK, {5, 6, 7}, {0, 0, 0}}, {OK, {}, {}}}, 2);   // all-epsilon outputs
  // eps:y before, between and after the consuming arcs
  check_conversion({{OK, {0, 0, 5, 0, 6, 7, 0, 0}, {40, 41, 5, 42, 0, 7, 43, 44}}}, 3);
  // non-OK strings between OK ones (a failed string's arcs are ignored)
  check_conversion({{OK, {5, 6}, {5, 6}}, {EMPTY, {}, {}}, {CYCLE, {9, 9}, {9, 9}},
                    {OK, {0, 7}, {8, 7}}}, 4);
  // an olabel above 256: UNSUPPORTED, no entries; its neighbours keep theirs
  check_conversion({{OK, {5}, {5}}, {OK, {5, 6, 7}, {5, 257, 7}}, {OK, {5}, {0xFFFFFFFFu}},
                    {OK, {0, 6}, {6, 256}}}, 5);
  // lengths around 64, labels from a fixed generator
  uint32_t x = 12345;
  auto next = [&x] { return x = x * 1664525u + 1013904223u; };
  std::vector<Path> many;
  for (uint32_t L : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 200u}) {
    Path p{OK, {}, {}};
    for (uint32_t k = 0; k < L; ++k) {
      p.il.push_back((next() >> 8) % 3 ? (next() >> 8) % 256 + 1 : 0);
      p.ol.push_back((next() >> 8) % 3 ? (next() >> 8) % 256 + 1 : 0);
    }
    many.push_back(p);
  }
  check_conversion(many, 6);
}

template <class R>
bool zeroed(const R& r) {
  const R z{};
  return std::memcmp(&r, &z, sizeof(r)) == 0;
}

void bad_conversion_arguments() {
  FstAlignedTextResult a;
  std::memset(&a, 0x5A, sizeof(a));
  FstBatchResult r{};
  expect(fst_batch_result_to_aligned_text(nullptr, &a) == FST_INVALID_ARG, "null in");
  expect(fst_batch_result_to_aligned_text(&r, nullptr) == FST_INVALID_ARG, "null out");
  int32_t st = 0;
  double fin = 0.0, w = 1.0;
  uint64_t down[2] = {4, 2}, up[2] = {0, 1};
  uint32_t ol = 1;
  r.num_strings = 1;
  r.status = &st;
  r.final_weights = &fin;
  r.path_offsets = down;
  expect(fst_batch_result_to_aligned_text(&r, &a) == FST_INVALID_ARG && zeroed(a),
         "decreasing offsets");
  std::memset(&a, 0x5A, sizeof(a));
  r.path_offsets = up;
  r.olabels = &ol;
  r.weights = &w;  // arcs, but no ilabels
  expect(fst_batch_result_to_aligned_text(&r, &a) == FST_INVALID_ARG && zeroed(a),
         "arcs without ilabels");
  r.path_offsets = nullptr;
  std::memset(&a, 0x5A, sizeof(a));
  expect(fst_batch_result_to_aligned_text(&r, &a) == FST_INVALID_ARG, "no offsets");
}

// A one-state rhs that copies label 98, through the C API of fst.h.
FstHandle copy_rhs() {
  const FstMutableHandle m = fst_mutable_new();
  const uint32_t s = fst_mutable_add_state(m);
  fst_mutable_set_start(m, s);
  fst_mutable_set_final(m, s, 0.0);
  fst_mutable_add_arc(m, s, 98, 98, 0.0, s);
  const FstHandle h = fst_freeze(m);
  fst_mutable_free(m);
  return h;
}

void entry_arguments() {
  const FstHandle good = copy_rhs();
  expect(good != FST_INVALID_HANDLE, "rhs");
  const FstHandle hs[2] = {good, good};
  const FstHandle stale[2] = {good, FST_INVALID_HANDLE};
  const uint8_t text[4] = {97, 97, 97, 97};
  const uint64_t off[3] = {0, 2, 4}, down[3] = {0, 3, 2}, zero[1] = {0};
  FstBatchOptions flags{};
  flags.device = -1;
  flags.flags = 2;  // an unknown flag
  struct Case {
    const char* what;
    const FstHandle* stages;
    uint32_t num_stages;
    const uint8_t* text;
    const uint64_t* offsets;
    uint32_t num;
    const FstBatchOptions* opts;
  };
  const Case cases[] = {
      {"no stages", nullptr, 1, text, off, 2, nullptr},
      {"zero stages", hs, 0, text, off, 2, nullptr},
      {"no offsets", hs, 1, text, nullptr, 2, nullptr},
      {"no text for bytes", hs, 1, nullptr, off, 2, nullptr},
      {"decreasing offsets", hs, 1, text, down, 2, nullptr},
      {"unknown flags", hs, 1, text, off, 2, &flags},
      {"stale handle", stale, 2, text, off, 2, nullptr},
      {"stale handle, no strings", stale, 2, text, off, 0, nullptr},
  };
  expect(fst_normalize_text_aligned_batch(hs, 1, text, off, 2, nullptr, nullptr) ==
             FST_INVALID_ARG, "null out");
  for (const Case& c : cases) {
    FstAlignedTextResult a;
    FstTextResult t;
    std::memset(&a, 0x5A, sizeof(a));
    std::memset(&t, 0x5A, sizeof(t));
    expect(fst_normalize_text_aligned_batch(c.stages, c.num_stages, c.text, c.offsets, c.num,
                                            c.opts, &a) == FST_INVALID_ARG, c.what);
    expect(fst_normalize_text_batch(c.stages, c.num_stages, c.text, c.offsets, c.num, c.opts,
                                    &t) == FST_INVALID_ARG, c.what);
    // zeroed exactly where the text entry zeroes its own
    FstAlignedTextResult p;
    std::memset(&p, 0x5A, sizeof(p));
    expect(zeroed(t) ? zeroed(a) : std::memcmp(&a, &p, sizeof(a)) == 0, c.what);
  }
  // no strings: the empty OK result, before any GPU check
  FstAlignedTextResult a;
  std::memset(&a, 0x5A, sizeof(a));
  expect(fst_normalize_text_aligned_batch(hs, 2, nullptr, zero, 0, nullptr, &a) == FST_OK,
         "empty batch");
  expect(a.num_strings == 0 && a.total_bytes == 0 && a.text_offsets && a.text_offsets[0] == 0 &&
             a.in_begin && a.in_end, "empty result");
  fst_aligned_text_result_free(&a);
  expect(zeroed(a), "empty result freed");
  // a batch that would run: without a GPU the entry says so with *out zeroed
  std::memset(&a, 0x5A, sizeof(a));
  const FstError e = fst_normalize_text_aligned_batch(hs, 1, text, off, 2, nullptr, &a);
  if (e == FST_OK) {
    expect(a.num_strings == 2, "a run");
    fst_aligned_text_result_free(&a);
  } else {
    expect(e == FST_INVALID_ARG && zeroed(a), "no GPU");
  }
  // the device pieces check their pointers before they look for a device
  expect(fst_device_path_alignment(nullptr, 1, off, nullptr, nullptr, 0, nullptr, nullptr) ==
             FST_INVALID_ARG, "path alignment: no stage");
  expect(fst_device_compose_alignment(1, nullptr, nullptr, nullptr, off, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, 0, nullptr) == FST_INVALID_ARG,
         "compose alignment: no offsets");
  fst_free(good);
}

}  // namespace

int main() {
  conversions();
  bad_conversion_arguments();
  entry_arguments();
  fst_teardown();
  if (failures) {
    std::fprintf(stderr, "align_host_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::puts("align_host_check: ok");
  return 0;
}

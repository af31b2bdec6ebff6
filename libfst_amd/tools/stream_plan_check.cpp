// stream_plan_check.cpp -- stand-alone check of the streamed batch's host planning and
// hand-over (csrc/stream_plan.hpp), for sanitizer builds on the CPU, from libfst_amd/:
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o stream_plan_check tools/stream_plan_check.cpp && ./stream_plan_check
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=thread \
//       -o stream_plan_check_tsan tools/stream_plan_check.cpp && ./stream_plan_check_tsan
// * expander_slice tiles [a, z) exactly, interior boundaries at multiples of 8 from a, for
//   every width 0..300 and every T in 1..16;
// * stream_shard_cuts against a linear-scan restatement: no shard empty, cuts rising, the
//   last one num, for every nsh up to num;
// * paths_compact against a plain restatement, the arrays in heap blocks with guard words;
// * PartGate, RecordedGate and ThreadGroup with one publisher and several waiters, a failure
//   or an abort injected at every position: every thread ends, a part published or recorded
//   before it is still delivered, and a ThreadGroup on a gate nobody marks still joins.
#include <cstdio>

#include "../csrc/stream_plan.hpp"

using namespace fstamd::host;

#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      std::printf("stream_plan_check: " __VA_ARGS__);  \
      std::printf(" (%s)\n", #c);                      \
      return 1;                                        \
    }                                                  \
  } while (0)

static uint32_t seed = 2463534242u;
static uint32_t rnd() { return seed = seed * 1664525u + 1013904223u; }

static int check_slices() {
  for (uint64_t a : {0ull, 5ull, 1000003ull})
    for (uint64_t w = 0; w <= 300; ++w)
      for (uint32_t T = 1; T <= 16; ++T) {
        uint64_t at = a;
        for (uint32_t t = 0; t < T; ++t) {
          const auto [lo, hi] = expander_slice(a, a + w, t, T);
          CHECK(lo == at && hi >= lo, "slice w=%llu T=%u t=%u", (unsigned long long)w, T, t);
          CHECK(t == 0 || (lo - a) % 8 == 0, "boundary w=%llu T=%u t=%u", (unsigned long long)w, T, t);
          at = hi;
        }
        CHECK(at == a + w, "end w=%llu T=%u", (unsigned long long)w, T);
      }
  return 0;
}

static int check_shard_cuts() {
  for (uint32_t round = 0; round < 300; ++round) {
    const uint32_t num = 1 + rnd() % 40;
    std::vector<double> pre(num + 1, 0.0);
    for (uint32_t i = 0; i < num; ++i)  // (a third of the strings cost nothing: flat runs)
      pre[i + 1] = pre[i] + (rnd() % 3 == 0 ? 0.0 : 0.25 * (1 + rnd() % 64));
    for (uint32_t nsh = 1; nsh <= num; ++nsh) {
      const std::vector<uint32_t> got = stream_shard_cuts(pre, num, nsh);
      std::vector<uint32_t> want{0};
      for (uint32_t j = 1; j < nsh; ++j) {
        const double goal = pre[num] * j / nsh;
        uint32_t i = 0;
        while (i <= num && pre[i] < goal) ++i;  // the first prefix at or past the goal
        if (i < want.back() + 1) i = want.back() + 1;
        if (i > num - (nsh - j)) i = num - (nsh - j);
        want.push_back(i);
      }
      want.push_back(num);
      CHECK(got == want, "shard cuts num=%u nsh=%u", num, nsh);
      CHECK(got.size() == nsh + 1 && got.front() == 0 && got.back() == num, "ends num=%u nsh=%u", num, nsh);
      for (uint32_t j = 0; j < nsh; ++j) CHECK(got[j] < got[j + 1], "empty shard num=%u nsh=%u", num, nsh);
    }
  }
  return 0;
}

static int check_compact() {
  constexpr uint32_t kGuard = 0xA5A5A5A5u;
  for (uint32_t round = 0; round < 400; ++round) {
    const uint32_t num = rnd() % 24;
    std::vector<uint64_t> off(num + 1, 0);
    std::vector<int32_t> status(num);
    for (uint32_t i = 0; i < num; ++i) {
      off[i + 1] = off[i] + rnd() % 7;
      status[i] = round % 5 == 0 ? 0 : (int32_t)(rnd() % 4 == 0 ? 1 + rnd() % 3 : 0);
    }
    const uint64_t tot = off[num];
    std::vector<uint32_t> il(tot + 1, kGuard), ol(tot + 1, kGuard);
    std::vector<double> w(tot + 1, -7.0);
    for (uint64_t k = 0; k < tot; ++k) il[k] = rnd(), ol[k] = rnd(), w[k] = (double)(rnd() % 1000) / 8;
    // the restatement: the OK strings' arcs appended in order
    std::vector<uint64_t> woff;
    std::vector<uint32_t> wil, wol;
    std::vector<double> ww;
    for (uint32_t i = 0; i < num; ++i) {
      woff.push_back(wil.size());
      if (status[i] != 0) continue;
      for (uint64_t k = off[i]; k < off[i + 1]; ++k) wil.push_back(il[k]), wol.push_back(ol[k]), ww.push_back(w[k]);
    }
    woff.push_back(wil.size());
    uint64_t* const poff = (uint64_t*)std::malloc((num + 1) * 8);  // exactly num + 1 offsets
    std::memcpy(poff, off.data(), (num + 1) * 8);
    const uint64_t got = paths_compact(num, poff, status.data(), il.data(), ol.data(), w.data());
    CHECK(got == wil.size(), "compact total round %u", round);
    CHECK(std::memcmp(poff, woff.data(), (num + 1) * 8) == 0, "compact offsets round %u", round);
    std::free(poff);
    CHECK(got == 0 || (std::memcmp(il.data(), wil.data(), got * 4) == 0 &&
                       std::memcmp(ol.data(), wol.data(), got * 4) == 0 &&
                       std::memcmp(w.data(), ww.data(), got * 8) == 0),
          "compact arcs round %u", round);
    CHECK(il[tot] == kGuard && ol[tot] == kGuard && w[tot] == -7.0, "compact guard round %u", round);
  }
  return 0;
}

// One publisher, `kWaiters` consumers that take the parts in order and one that waits for all
// of them; the publisher fails before part f (f == parts: it does not).
static int check_part_gate() {
  constexpr size_t kWaiters = 4;
  for (size_t parts = 0; parts <= 6; ++parts)
    for (size_t f = 0; f <= parts; ++f) {
      PartGate gate;
      std::vector<size_t> taken(kWaiters, 0);
      bool all_returned = false;
      {
        ThreadGroup th;
        for (size_t k = 0; k < kWaiters; ++k)
          th.add([&, k] {
            for (size_t p = 0; p < parts && gate.wait_for(p); ++p) taken[k] = p + 1;
          });
        th.add([&] {
          gate.wait_all(parts);
          all_returned = true;
        });
        th.add([&] {
          for (size_t p = 0; p < f; ++p) gate.publish(p + 1);
          if (f < parts) gate.fail();
        });
      }
      for (size_t k = 0; k < kWaiters; ++k) CHECK(taken[k] == f, "part gate parts=%zu f=%zu", parts, f);
      CHECK(all_returned, "wait_all parts=%zu f=%zu", parts, f);
      for (size_t p = 0; p < f; ++p) CHECK(gate.wait_for(p), "published part lost after fail()");
      CHECK(f == parts || !gate.wait_for(f), "unpublished part delivered");
    }
  return 0;
}

// One thread marks parts [0, k) and then aborts; the waiters take the parts in order.
static int check_recorded_gate() {
  constexpr size_t kWaiters = 4;
  for (size_t parts = 1; parts <= 6; ++parts)
    for (size_t k = 0; k <= parts; ++k) {
      RecordedGate gate;
      gate.reset(parts);
      std::vector<size_t> taken(kWaiters, 0);
      {
        ThreadGroup th;
        for (size_t i = 0; i < kWaiters; ++i)
          th.add([&, i] {
            for (size_t p = 0; p < parts && gate.wait(p); ++p) taken[i] = p + 1;
          });
        th.add([&] {
          for (size_t p = 0; p < k; ++p) gate.mark(p);
          gate.abort();
        });
      }
      for (size_t i = 0; i < kWaiters; ++i) CHECK(taken[i] == k, "recorded gate parts=%zu k=%zu", parts, k);
      for (size_t p = 0; p < parts; ++p) CHECK(gate.wait(p) == (p < k), "after abort parts=%zu k=%zu", parts, k);
    }
  // a group on a gate: leaving the scope aborts first, so waiters nobody will mark for end
  for (size_t marked = 0; marked <= 3; ++marked) {
    RecordedGate gate;
    gate.reset(3);
    std::vector<size_t> taken(kWaiters, 0);
    {
      ThreadGroup th(&gate);
      for (size_t i = 0; i < kWaiters; ++i)
        th.add([&, i] {
          for (size_t p = 0; p < 3 && gate.wait(p); ++p) taken[i] = p + 1;
        });
      for (size_t p = 0; p < marked; ++p) gate.mark(p);
    }
    for (size_t i = 0; i < kWaiters; ++i) CHECK(taken[i] == marked, "group abort marked=%zu", marked);
  }
  return 0;
}

int main() {
  if (check_slices() || check_shard_cuts() || check_compact() || check_part_gate() ||
      check_recorded_gate())
    return 1;
  std::printf("stream_plan_check: ok\n");
  return 0;
}

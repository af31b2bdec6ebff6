// stream_plan.hpp -- what the streamed and pipelined host batches decide and hand over on the
// host alone: the environment knobs, the part and shard cuts, the label route's compaction,
// and the gates and thread groups the routes' host threads meet at.  Plain C++ with no device
// or runtime dependency (as weight_codes.hpp), so it also builds into a stand-alone checker
// for sanitizer builds (tools/stream_plan_check.cpp); the part planner is reachable through
// fst_debug_stream_part_cuts.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)  // internal: not one of the library's exports
namespace fstamd::host {

// The streamed batch's environment knobs, read once per call (tests change them between
// calls in one process) and passed down to the shards.
struct StreamKnobs {
  // FSTAMD_STREAM_CODES: 0 = the f64 copy-out for every part, 1 = every part's weights leave
  // as 1-B codes (default), 2 = every part but the last
  int codes_mode = 1;
  // FSTAMD_STREAM_CUTS: the parts' cuts, per mille of a shard's labels (values in 1..999;
  // set but empty: one part)
  bool cuts_set = false;
  std::vector<uint64_t> cuts_env;
  int stage = 0;              // FSTAMD_STREAM_STAGE: how the labels move (ShardRun::start_uploads)
  uint32_t expanders = 4;     // FSTAMD_STREAM_EXPANDERS: expander threads, 1..16
  bool ab_nocopy = false;     // FSTAMD_STREAM_AB=1 (A/B timing only): drops the copy-out
  uint64_t fix_few = 4096;    // FSTAMD_STREAM_FIX_FEW: fix-ups downloaded one by one up to this
  bool route_log = false;     // FSTAMD_ROUTE_LOG
  bool host_prof = false;     // FSTAMD_HOST_PROF
  bool shard_log = false;     // FSTAMD_SHARD_LOG

  static StreamKnobs from_env() {
    StreamKnobs k;
    if (const char* e = std::getenv("FSTAMD_STREAM_CODES")) {
      const int m = std::atoi(e);
      k.codes_mode = m < 0 || m > 2 ? 1 : m;
    }
    if (const char* ce = std::getenv("FSTAMD_STREAM_CUTS")) {
      k.cuts_set = true;
      for (const char* q = ce; *q;) {
        char* e = nullptr;
        const unsigned long v = std::strtoul(q, &e, 10);
        if (e == q) break;
        if (v > 0 && v < 1000) k.cuts_env.push_back(v);
        q = *e ? e + 1 : e;
      }
    }
    if (const char* e = std::getenv("FSTAMD_STREAM_STAGE")) k.stage = std::atoi(e);
    if (const char* e = std::getenv("FSTAMD_STREAM_EXPANDERS"))
      k.expanders = (uint32_t)std::min(16, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("FSTAMD_STREAM_AB")) k.ab_nocopy = std::atoi(e) == 1;
    if (const char* e = std::getenv("FSTAMD_STREAM_FIX_FEW")) k.fix_few = std::strtoull(e, nullptr, 10);
    k.route_log = std::getenv("FSTAMD_ROUTE_LOG") != nullptr;
    k.host_prof = std::getenv("FSTAMD_HOST_PROF") != nullptr;
    k.shard_log = std::getenv("FSTAMD_SHARD_LOG") != nullptr;
    return k;
  }
  // The cuts in force: FSTAMD_STREAM_CUTS, or 1/43 and 7/43 (each part's upload fits in the
  // previous part's compute), and, when every part leaves codes, shrinking parts after the big
  // one, so that little expansion is left after the last kernel.
  std::vector<uint64_t> cuts(bool all_coded) const {
    if (cuts_set) return cuts_env;
    if (all_coded) return {23, 163, 700, 900, 970};
    return {23, 163};
  }
};

// The parts of a shard of `num` strings with offsets loff[0 .. num]: {0, .., num}, cut where
// the labels pass each per-mille fraction of the shard's total (small shards: one part).  A
// cut is kept only past the previous one and before `num`.
inline std::vector<uint32_t> stream_part_cuts(const uint64_t* loff, uint32_t num,
                                              const std::vector<uint64_t>& per_mille) {
  std::vector<uint32_t> cut{0};
  const uint64_t base = loff[0], total = loff[num] - base;
  if (total >= (1u << 22) && num >= (1u << 15)) {
    for (uint64_t f : per_mille) {
      const uint64_t want = base + total * f / 1000;
      const uint32_t i = (uint32_t)(std::upper_bound(loff, loff + num, want) - loff);
      if (i > cut.back() && i < num) cut.push_back(i);
    }
  }
  cut.push_back(num);
  return cut;
}

// The shards of a streamed batch: `nsh` (1..num) contiguous string ranges {0, .., num} of
// equal estimated cost, pre[i] = the cost of strings [0, i) (read only when nsh > 1).
inline std::vector<uint32_t> stream_shard_cuts(const std::vector<double>& pre, uint32_t num,
                                               uint32_t nsh) {
  std::vector<uint32_t> cuts{0};
  for (uint32_t j = 1; j < nsh; ++j) {
    const double goal = pre[num] * j / nsh;
    uint32_t i = (uint32_t)(std::lower_bound(pre.begin(), pre.end(), goal) - pre.begin());
    i = std::max(i, cuts.back() + 1);  // never empty
    i = std::min(i, num - (nsh - j));  // at least one string for each later one
    cuts.push_back(i);
  }
  cuts.push_back(num);
  return cuts;
}

// Expander thread t of T's slice [lo, hi) of a part's elements [a, z): cut at 8 elements from
// `a` (whole lines of the weights for all but the ends), the last thread to the end.
inline std::pair<uint64_t, uint64_t> expander_slice(uint64_t a, uint64_t z, uint32_t t,
                                                    uint32_t T) {
  const uint64_t w = z - a;
  return {a + ((w * t / T) & ~7ull), t + 1 == T ? z : a + ((w * (t + 1) / T) & ~7ull)};
}

// The streamed label batch's last step, on the host: the slots of strings without a path
// dropped, moving left in input order (text_compact's twin).  In: poff[0 .. num] = the slots.
// Out: poff = the CSR offsets of the OK strings' paths, the three arc arrays compacted in
// place.  Returns the total arcs.
inline uint64_t paths_compact(uint32_t num, uint64_t* poff, const int32_t* status, uint32_t* il,
                              uint32_t* ol, double* w) {
  constexpr int32_t ok = 0;  // FST_PATH_OK (fst_batch.h), kPathOk (fst_core.hpp)
  uint64_t nbad = 0;
  for (uint32_t i = 0; i < num; ++i) nbad += status[i] != ok;
  if (!nbad) return poff[num];
  uint64_t dst = 0;
  for (uint32_t i = 0; i < num; ++i) {
    const uint64_t a = poff[i], L = poff[i + 1] - a;
    poff[i] = dst;
    if (status[i] != ok) continue;
    if (dst != a) {
      std::memmove(il + dst, il + a, L * 4);
      std::memmove(ol + dst, ol + a, L * 4);
      std::memmove(w + dst, w + a, L * 8);
    }
    dst += L;
  }
  poff[num] = dst;
  return dst;
}

// An upload thread publishes "parts [0, n) are in their stream" or that it failed; the
// threads that launch or copy wait for their part, or for all of them.
class PartGate {
 public:
  void publish(size_t n) {
    std::lock_guard<std::mutex> g(mu_);
    n_ = n;
    cv_.notify_all();
  }
  void fail() {
    std::lock_guard<std::mutex> g(mu_);
    failed_ = true;
    cv_.notify_all();
  }
  // true once part p is published; false when the publisher failed before it
  bool wait_for(size_t p) {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return failed_ || n_ > p; });
    return n_ > p;
  }
  // returns once all `parts` are published or the publisher failed
  void wait_all(size_t parts) {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return failed_ || n_ == parts; });
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  size_t n_ = 0;
  bool failed_ = false;
};

// "Part p's completion event is in its stream": marked by the thread that recorded it,
// waited for by the expanders before they synchronise the event (synchronising an event
// nobody recorded yet, or one a previous call left complete, would return at once).
// abort() releases every waiter; a part marked before it is still delivered.
class RecordedGate {
 public:
  void reset(size_t parts) { rec_.assign(parts, 0); }
  void mark(size_t p) {
    std::lock_guard<std::mutex> g(mu_);
    rec_[p] = 1;
    cv_.notify_all();
  }
  void abort() {
    std::lock_guard<std::mutex> g(mu_);
    abort_ = true;
    cv_.notify_all();
  }
  bool wait(size_t p) {  // true: marked; false: aborted before it was
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return abort_ || rec_[p]; });
    return rec_[p] != 0;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<char> rec_;
  bool abort_ = false;
};

// Threads joined when the group goes out of scope (declare it after what they use).  A group
// whose threads wait at a RecordedGate aborts the gate first, so that no return can leave it
// waiting for threads that wait for a mark that will not come.
class ThreadGroup {
 public:
  explicit ThreadGroup(RecordedGate* abort_first = nullptr) : gate_(abort_first) {}
  ~ThreadGroup() {
    if (gate_) gate_->abort();
    join();
  }
  template <class F>
  void add(F&& f) {
    th_.emplace_back(std::forward<F>(f));
  }
  void join() {
    for (auto& t : th_) t.join();
    th_.clear();
  }
  ThreadGroup(const ThreadGroup&) = delete;
  ThreadGroup& operator=(const ThreadGroup&) = delete;

 private:
  RecordedGate* gate_;
  std::vector<std::thread> th_;
};

}  // namespace fstamd::host
#pragma GCC visibility pop

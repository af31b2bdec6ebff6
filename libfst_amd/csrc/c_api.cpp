// c_api.cpp -- the fst.h C ABI of libfst_amd (fst_batch.h: batch_entries.cpp).
//
// Handle tables, snapshots and pinning follow src/c-api.zig:105-271: u64 handles
// (generation << 32 | slot), one global mutex for table bookkeeping only, compute
// outside the lock on a cloned lhs, the frozen rhs pinned (a shared_ptr copy here)
// so that fst_free() during a call defers destruction.
//
// Every compose / shortest-path entry computes on the GPU; there is no CPU
// fallback.  If no HIP device is usable the entry fails (FST_INVALID_HANDLE /
// FST_INVALID_ARG) and, once per process, says why on stderr.
#include <cmath>
#include <deque>
#include <new>

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "host_rt.hpp"

using namespace fstamd;
using namespace fstamd::host;

namespace {

// Handle tables (src/c-api.zig:132-271), sharded: a handle's low bits name one of kShards
// shards, each with its own reader-writer lock over its slots AND the contents of the
// objects they hold.  Queries take their shard shared, edits exclusive; threads working on
// their own handles (concurrent compose calls reading their results arc by arc) do not meet
// on one lock -- one table-wide lock cost a third of the calls/s at 256 threads.
template <class T>
class HandleTable {
 public:
  static constexpr uint32_t kShards = 64;
  using SharedLock = std::shared_lock<std::shared_mutex>;
  using ExclusiveLock = std::unique_lock<std::shared_mutex>;

  uint64_t insert(std::shared_ptr<T> p) {
    // a thread fills one shard (its own, by arrival order): inserts from many threads spread
    static std::atomic<uint32_t> next{0};
    thread_local uint32_t mine = next.fetch_add(1, std::memory_order_relaxed) % kShards;
    Shard& sh = shards_[mine];
    ExclusiveLock g(sh.mu);
    uint32_t local;
    if (!sh.free.empty()) {
      local = sh.free.back();
      sh.free.pop_back();
      if (++sh.gen[local] == 0) sh.gen[local] = 1;
      sh.slots[local] = std::move(p);
    } else {
      local = (uint32_t)sh.slots.size();
      if ((uint64_t)local * kShards + mine >= 0xFFFFFFFFull) return kInvalid;
      sh.slots.push_back(std::move(p));
      sh.gen.push_back(1);
    }
    return ((uint64_t)sh.gen[local] << 32) | (local * kShards + mine);
  }
  // the lock a query (shared) or an edit (exclusive) of handle h holds around get_locked
  SharedLock lock_shared(uint64_t h) const { return SharedLock(shard(h).mu); }
  ExclusiveLock lock(uint64_t h) const { return ExclusiveLock(shard(h).mu); }
  // the object of h, or null; the caller holds lock_shared(h) or lock(h)
  T* get_locked(uint64_t h) const {
    if (h == kInvalid) return nullptr;
    const uint32_t g = (uint32_t)(h >> 32), idx = (uint32_t)h;
    if (g == 0 || idx == 0xFFFFFFFFu) return nullptr;
    const Shard& sh = shard(h);
    const uint32_t local = idx / kShards;
    if (local >= sh.slots.size() || sh.gen[local] != g) return nullptr;
    return sh.slots[local].get();
  }
  // get/pin: a shared_ptr copy keeps the object alive outside the lock
  std::shared_ptr<T> get(uint64_t h) const {
    SharedLock g = lock_shared(h);
    if (!get_locked(h)) return nullptr;
    return shard(h).slots[(uint32_t)h / kShards];
  }
  bool remove(uint64_t h) {
    ExclusiveLock g = lock(h);
    if (!get_locked(h)) return false;
    Shard& sh = shard(h);
    const uint32_t local = (uint32_t)h / kShards;
    sh.slots[local].reset();
    if (++sh.gen[local] == 0) sh.gen[local] = 1;  // invalidateSlot
    sh.free.push_back(local);
    return true;
  }
  void clear() {
    for (Shard& sh : shards_) {
      ExclusiveLock g(sh.mu);
      sh.slots.clear();
      sh.gen.clear();
      sh.free.clear();
    }
  }

 private:
  struct alignas(64) Shard {
    mutable std::shared_mutex mu;
    std::vector<std::shared_ptr<T>> slots;
    std::vector<uint32_t> gen;
    std::vector<uint32_t> free;
  };
  Shard& shard(uint64_t h) { return shards_[(uint32_t)h % kShards]; }
  const Shard& shard(uint64_t h) const { return shards_[(uint32_t)h % kShards]; }
  Shard shards_[kShards];
};

HandleTable<MutableFst> g_mut;
HandleTable<FrozenFst> g_fst;

bool trace_enabled() {  // LIBFST_TRACE_COMPOSE, src/c-api.zig:55-64
  static const bool on = std::getenv("LIBFST_TRACE_COMPOSE") != nullptr;
  return on;
}

void trace(const char* tag, uint64_t a, uint64_t b, size_t in_s, size_t in_a, size_t out_s,
           size_t out_a, double us, double kernel_ms) {
  if (!trace_enabled()) return;
  std::fprintf(stderr,
               "[libfst] %s op=fst_compose_frozen a=%llu b=%llu in_states=%zu in_arcs=%zu "
               "out_states=%zu out_arcs=%zu elapsed_us=%lld kernel_us=%lld\n",
               tag, (unsigned long long)a, (unsigned long long)b, in_s, in_a, out_s, out_a,
               (long long)us, (long long)(kernel_ms * 1000.0));
}

// Result FST of one string: linear chain, or the empty FST (src/ops/*:382-400).
MutableFst chain_result(const HostPaths& h, uint32_t i) {
  MutableFst r;
  if (h.status[i] != kPathOk) return r;
  const uint32_t P = h.len[i];
  r.add_states(P + 1);
  r.set_start(0);
  r.set_final(P, h.fin[i]);
  for (uint32_t k = 0; k < P; ++k) {
    const uint64_t o = h.off[i] + k;
    r.add_arc(k, Arc{h.il[o], h.ol[o], h.w[o], k + 1});
  }
  return r;
}

// A MutableFst flattened to CSR on the host (arcs in insertion order), the device upload's
// source.  Large FSTs are flattened on host threads by state ranges (fst_shortest_path on a
// 10 M-arc lattice: a deep copy plus a push_back pass took ~150 ms).
// Host array without value-initialisation (the flatten writes every element, on the
// threads that first touch its pages).
// The arrays live in the pinned host pool (pin_alloc), so their upload is one DMA per
// array without the runtime's staging copies (config 1's lattice, 10 M arcs: ~200 MB).
template <class T>
struct RawVec {
  T* p = nullptr;
  size_t n = 0;
  RawVec() = default;
  RawVec(const RawVec&) = delete;
  RawVec& operator=(const RawVec&) = delete;
  ~RawVec() { pin_release(p); }
  void resize(size_t k) {
    pin_release(p);
    p = k ? (T*)pin_alloc(k * sizeof(T)) : nullptr;
    if (k && !p) throw std::bad_alloc();  // as new T[k] did
    n = k;
  }
  size_t size() const { return n; }
  T* data() { return p; }
  const T* data() const { return p; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

struct HostGraph {
  std::vector<uint32_t> soff;
  RawVec<uint32_t> il, ol, nx;
  RawVec<double> w, fin;
  uint32_t start = kNoState, maxdeg = 0;
  bool nonneg = true;  // every arc and final weight >= +0.0 (no -0.0, no NaN)
  bool nan = false;    // some arc or final weight is NaN
  bool eps_out = false;

  explicit HostGraph(const MutableFst& a) {
    const uint32_t ns = (uint32_t)a.num_states();
    start = a.start();
    soff.assign(ns + 1, 0);
    fin.resize(ns);
    for (uint32_t s = 0; s < ns; ++s) {
      const uint32_t d = (uint32_t)a.num_arcs(s);
      soff[s + 1] = soff[s] + d;
      maxdeg = std::max(maxdeg, d);
    }
    const size_t na = soff[ns];
    il.resize(na);
    ol.resize(na);
    nx.resize(na);
    w.resize(na);
    auto neg = [](double x) { return x < 0.0 || std::isnan(x) || (x == 0.0 && std::signbit(x)); };
    const uint32_t nt = na < (1u << 18) ? 1u
                        : std::min<uint32_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<uint8_t> flags(nt, 0);  // per thread: 1 negative, 2 NaN, 4 output epsilon
    auto fill = [&](uint32_t t) {
      const uint32_t lo = (uint32_t)((uint64_t)ns * t / nt), hi = (uint32_t)((uint64_t)ns * (t + 1) / nt);
      uint8_t fl = 0;
      for (uint32_t s = lo; s < hi; ++s) {
        fin[s] = a.final_weight(s);
        if (neg(fin[s])) fl |= 1;
        if (std::isnan(fin[s])) fl |= 2;
        uint32_t k = soff[s];
        for (const Arc& x : a.arcs(s)) {
          il[k] = x.ilabel;
          ol[k] = x.olabel;
          w[k] = x.weight;
          nx[k] = x.nextstate;
          if (x.olabel == kEpsilon) fl |= 4;
          if (neg(x.weight)) fl |= 1;
          if (std::isnan(x.weight)) fl |= 2;
          ++k;
        }
      }
      flags[t] = fl;
    };
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < nt; ++t) th.emplace_back(fill, t);
    fill(0);
    for (auto& x : th) x.join();
    for (uint8_t fl : flags) {
      if (fl & 1) nonneg = false;
      if (fl & 2) nan = true;
      if (fl & 4) eps_out = true;
    }
  }
};

// A HostGraph on the device: the lhs of the single-call compose entries, or the FST itself
// for fst_shortest_path.
struct GraphUpload {
  DevBuf off, il, ol, w, nx, fin;
  GraphInput g{};
  bool ok = false;
  bool nonneg = true;
  bool nan = false;
  // Uploads on `stream` (the call's engine stream) and waits for them: the host arrays may
  // be a temporary.
  GraphUpload(const MutableFst& a, hipStream_t stream) : GraphUpload(HostGraph(a), stream) {}
  GraphUpload(const HostGraph& h, hipStream_t stream)
      : off(h.soff.size() * 4ull), il(h.il.size() * 4), ol(h.ol.size() * 4), w(h.w.size() * 8),
        nx(h.nx.size() * 4), fin(h.fin.size() * 8ull) {
    nonneg = h.nonneg;
    nan = h.nan;
    const uint32_t ns = (uint32_t)h.fin.size();
    const size_t na = h.il.size();
    if (!off.p || !il.p || !ol.p || !w.p || !nx.p || !fin.p) return;
    const auto h2d = [stream](void* d, const void* src, size_t b) {
      return b == 0 || hipMemcpyAsync(d, src, b, hipMemcpyHostToDevice, stream) == hipSuccess;
    };
    bool good = h2d(off.p, h.soff.data(), (ns + 1) * 4ull) && h2d(il.p, h.il.data(), na * 4) &&
                h2d(ol.p, h.ol.data(), na * 4) && h2d(w.p, h.w.data(), na * 8) &&
                h2d(nx.p, h.nx.data(), na * 4) && h2d(fin.p, h.fin.data(), ns * 8ull);
    good = hipStreamSynchronize(stream) == hipSuccess && good;
    g.state_off = (const uint32_t*)off.p;
    g.arc_il = (const uint32_t*)il.p;
    g.arc_ol = (const uint32_t*)ol.p;
    g.arc_w = (const double*)w.p;
    g.arc_next = (const uint32_t*)nx.p;
    g.final_w = (const double*)fin.p;
    g.num_states = ns;
    g.start = h.start;
    g.max_outdeg = h.maxdeg;
    g.eps_out = h.eps_out ? 1u : 0u;
    ok = good;
  }
};

// A single-call lhs that is exactly a compileString acceptor (src/string.zig:24-50: states
// 0..L, arc k = (c, c, One, k + 1), final(L) = One, no other final) is the batch API's chain
// input: its labels.  Such a call runs the batch engines on one string (the layered pull
// tiers, the dense replay), not the general-lhs hashed replay: 1^64 on the metric rhs took
// 93 ms there (one wave popping 8,385 tuples through HBM tables).
bool as_chain(const MutableFst& a, std::vector<uint32_t>* labels) {
  const size_t ns = a.num_states();
  if (ns == 0 || a.start() != 0 || ns > (1u << 30)) return false;
  auto bits = [](double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
  };
  const uint32_t L = (uint32_t)(ns - 1);
  labels->resize(L);
  for (uint32_t k = 0; k <= L; ++k) {
    const auto& arcs = a.arcs(k);
    if (k == L) {
      if (!arcs.empty() || bits(a.final_weight(k)) != bits(w_one())) return false;
      break;
    }
    if (arcs.size() != 1 || !std::isinf(a.final_weight(k)) || a.final_weight(k) < 0) return false;
    const Arc& x = arcs[0];
    if (x.nextstate != k + 1 || x.ilabel != x.olabel || bits(x.weight) != bits(w_one()))
      return false;
    (*labels)[k] = x.ilabel;
  }
  return true;
}

// Lazy 1-best of one general lhs on the GPU (single-call C ABI path).
int run_lazy_single(const MutableFst& a, FrozenFst& b, uint32_t n, MutableFst* result,
                    double* kernel_ms) {
  const int dev = current_device();
  if (dev < 0) return -1;
  DeviceFst* D = b.device(dev);
  if (!D) return -1;
  DeviceEngine::Lease E = DeviceEngine::acquire(dev);
  if (!E) return -1;
  const hipStream_t stream = E.stream();
  GraphUpload up(a, stream);
  if (!up.ok) return -1;
  GraphInput g = up.g;
  // Grow the tuple capacity on overflow (the reference has no limit but memory).
  for (uint32_t ncap = 1u << 14; ncap <= (1u << 26); ncap <<= 2) {
    g.ncap = ncap;
    const uint64_t arc_cap = std::max<uint64_t>(ncap, 1024);
    DevOut out(1, arc_cap);
    if (!out.ok()) return -1;
    LaunchStats st;
    if (E->run_graph(*D, g, n, 0, out.v, stream, &st) != hipSuccess) return -1;
    if (hipStreamSynchronize(stream) != hipSuccess) return -1;
    HostPaths h;
    if (!out.download(1, &h, stream)) return -1;
    t_last_stats = st;
    if (kernel_ms) *kernel_ms = st.kernel_ms;
    const int32_t s = h.status[0];
    if (s == kPathOverflow || s == kPathOutputFull) continue;
    if (s == kPathErrorN) return 2;
    if (s == kPathCycle) return 3;
    *result = chain_result(h, 0);  // OK or EMPTY
    return 0;
  }
  return -1;
}

// ---- Small batches: the coalesced single calls (one utterance each) and small host
// batches.  Per call the regular path costs ~10 uploads / downloads / synchronisations of
// ~10-25 us each beside a ~160 us kernel (WeText-scale tagger, profiles/r05/s2): here the
// inputs go up in one copy from one pinned block, the outputs live in one device block
// that comes down in one copy (the whole arena: it is small), and the only host waits are
// the engines' own routing reads and that final download.  A result the arena could not
// hold (OUTPUT_FULL) reruns on the regular path.
constexpr uint64_t kSmallLabels = 1u << 16;
constexpr uint32_t kSmallStrings = 1u << 12;
constexpr int kSmallRetry = -2;

int run_small_batch(DeviceEngine::Lease& E, DeviceFst& D, const uint32_t* labels,
                    const uint64_t* offsets, uint32_t num, uint64_t total, uint32_t max_len,
                    uint32_t n, int semantics, HostPaths* h) {
  const hipStream_t stream = E.stream();
  const uint64_t cap = std::max<uint64_t>((D.has_eps ? 4 : 1) * total + 16, 1024);
  auto al = [](uint64_t b) { return (b + 255) & ~255ull; };
  // device block: inputs [offsets | labels], then outputs [status | len | off | fin |
  // cursor | il | ol | w], each region 256-B aligned
  const uint64_t o_off = 0, o_lab = al((num + 1) * 8ull), in_bytes = o_lab + total * 4;
  const uint64_t o_st = al(in_bytes), o_len = o_st + al(num * 4ull), o_po = o_len + al(num * 4ull),
                 o_fin = o_po + al(num * 8ull), o_cur = o_fin + al(num * 8ull),
                 o_il = o_cur + 256, o_ol = o_il + al(cap * 4), o_w = o_ol + al(cap * 4),
                 end = o_w + cap * 8;
  DevBuf blk(end);
  PinnedVec<uint8_t> hin(in_bytes), hout(end - o_st);
  if (!blk.p) return FST_OOM;
  // every return before the final synchronisation drains the stream first: `blk`, `hin`
  // and `hout` go back to their pools on return, and an upload, a kernel (run_chain can
  // fail after launching some) or the download may still be using them
  StreamDrain drain{{stream}};
  uint64_t* ho = (uint64_t*)(hin.data() + o_off);
  for (uint32_t i = 0; i <= num; ++i) ho[i] = offsets[i] - offsets[0];
  if (total) std::memcpy(hin.data() + o_lab, labels + offsets[0], total * 4);
  uint8_t* p = (uint8_t*)blk.p;
  if (hipMemcpyAsync(p, hin.data(), in_bytes, hipMemcpyHostToDevice, stream) != hipSuccess)
    return FST_OOM;
  ChainInput in{(const uint32_t*)(p + o_lab), (const uint64_t*)(p + o_off), num, max_len};
  BatchOutDev v{(int32_t*)(p + o_st), (uint32_t*)(p + o_len), (uint64_t*)(p + o_po),
                (double*)(p + o_fin), (uint32_t*)(p + o_il), (uint32_t*)(p + o_ol),
                (double*)(p + o_w), cap, (unsigned long long*)(p + o_cur), nullptr};
  if (t_prof) t_prof->lap(0);
  LaunchStats st;
  st.defer = true;  // (kernel time read after the download's synchronisation)
  const bool launched = E->run_chain(D, in, n, semantics, v, stream, &st) == hipSuccess &&
                        !fault_inject("small_after_launch");
  if (!launched ||
      hipMemcpyAsync(hout.data(), p + o_st, end - o_st, hipMemcpyDeviceToHost, stream) !=
          hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  drain.done = true;
  (void)E->finish_deferred(&st);
  t_last_stats = st;
  if (t_prof) {
    t_prof->lap(2);
    ++t_prof->runs;
  }
  const uint8_t* q = hout.data() - o_st;  // (offsets below are block offsets)
  const int32_t* status = (const int32_t*)(q + o_st);
  for (uint32_t i = 0; i < num; ++i)
    if (status[i] == kPathOutputFull) return kSmallRetry;
  const uint64_t used = std::min<uint64_t>(*(const uint64_t*)(q + o_cur), cap);
  h->status.resize(num);
  h->len.resize(num);
  h->off.resize(num);
  h->fin.resize(num);
  h->il.resize(used);
  h->ol.resize(used);
  h->w.resize(used);
  std::memcpy(h->status.data(), status, num * 4ull);
  std::memcpy(h->len.data(), q + o_len, num * 4ull);
  std::memcpy(h->off.data(), q + o_po, num * 8ull);
  std::memcpy(h->fin.data(), q + o_fin, num * 8ull);
  if (used) {
    std::memcpy(h->il.data(), q + o_il, used * 4);
    std::memcpy(h->ol.data(), q + o_ol, used * 4);
    std::memcpy(h->w.data(), q + o_w, used * 8);
  }
  if (t_prof) t_prof->lap(3);
  return FST_OK;
}

}  // namespace

// The call runs on the engine `E` leases (its stream; E->dev() is the device).
FstError host::run_chain_batch_host(DeviceEngine::Lease& E, FrozenFst& b, const uint32_t* labels,
                                    const uint64_t* offsets, uint32_t num, uint32_t n,
                                    int semantics, HostPaths* h, std::unique_ptr<DevOut>* keep) {
  const int dev = E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b.device(dev);
  if (!D) return FST_OOM;
  const hipStream_t stream = E.stream();
  const uint64_t total = num ? offsets[num] - offsets[0] : 0;
  uint32_t max_len = 0;
  for (uint32_t i = 0; i < num; ++i)
    max_len = std::max<uint32_t>(max_len, (uint32_t)(offsets[i + 1] - offsets[i]));
  if (!keep && num && total <= kSmallLabels && num <= kSmallStrings) {
    const int r = run_small_batch(E, *D, labels, offsets, num, total, max_len, n, semantics, h);
    if (r != kSmallRetry) return (FstError)r;
  }
  std::vector<uint64_t> rebased(num + 1);
  for (uint32_t i = 0; i <= num; ++i) rebased[i] = offsets[i] - offsets[0];
  DevBuf d_lab(total * 4), d_off((num + 1) * 8ull);
  if (!d_lab.p || !d_off.p) return FST_OOM;
  // (pageable sources: hipMemcpyAsync stages them before it returns)
  if (total && hipMemcpyAsync(d_lab.p, labels + offsets[0], total * 4, hipMemcpyHostToDevice,
                              stream) != hipSuccess)
    return FST_OOM;
  if (hipMemcpyAsync(d_off.p, rebased.data(), (num + 1) * 8ull, hipMemcpyHostToDevice, stream) !=
      hipSuccess)
    return FST_OOM;
  ChainInput in{(const uint32_t*)d_lab.p, (const uint64_t*)d_off.p, num, max_len};
  if (t_prof) t_prof->lap(0);
  return run_chain_batch_dev(E, *D, in, total, n, semantics, h, keep);
}

namespace {

// ---- Coalesced single calls ----------------------------------------------------------
// fst_compose_frozen_shortest_path on a compileString lhs is one chain string.  Calls that
// arrive while a batch is in flight are combined (flat combining): the first caller of an
// idle device becomes a leader, takes every queued call (grouped by rhs and n), runs them
// as one batch on an engine lease and hands each caller its path; up to chain_leaders()
// batches run at once (separate engines and streams).  A lone caller runs its own string
// with no added latency; N concurrent callers share launches and host <-> device trips, so
// calls/s grows with N (the reference scales calls over threads, README.md:68-82).
// FSTAMD_COALESCE=0 runs every call on its own.
struct ChainCall {
  std::shared_ptr<FrozenFst> rhs;
  uint32_t n = 1;
  const std::vector<uint32_t>* labels = nullptr;
  // result
  FstError err = FST_OOM;
  int32_t status = kPathInternal;
  // the batch's host result, shared by its callers: each copies its own path out (the
  // leader allocating and the callers freeing one arc vector per call had the callers
  // queue on the leader's malloc arena)
  std::shared_ptr<const HostPaths> paths;
  uint32_t index = 0;
  double fin = 0;
  LaunchStats stats;
  // combiner hand-off: each caller sleeps on its own word (a futex), so a finished batch
  // wakes exactly its callers, which return without touching the combiner's lock, and one
  // queued caller to lead next.  The queue and the leader count stay under
  // ChainCombiner::mu; the lock-free word took the wake-ups of 256 waiting threads off it
  // (each had re-taken the lock on waking: half the process's CPU time at 256 threads).
  std::atomic<uint32_t> word{0};  // kCallWaiting / kCallLead / kCallDone
  bool taken = false;             // in a leader's batch (under ChainCombiner::mu)
};
constexpr uint32_t kCallWaiting = 0, kCallLead = 1, kCallDone = 2;

void call_wake(std::atomic<uint32_t>& w) {
  // after a post the caller may already have returned and its frame be reused: a wake on
  // that address is at most a spurious one, and every waiter re-checks its word
  syscall(SYS_futex, reinterpret_cast<uint32_t*>(&w), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
}
void call_wait(std::atomic<uint32_t>& w) {  // until the word leaves kCallWaiting
  while (w.load(std::memory_order_acquire) == kCallWaiting)
    syscall(SYS_futex, reinterpret_cast<uint32_t*>(&w), FUTEX_WAIT_PRIVATE, kCallWaiting, nullptr,
            nullptr, 0);
}
// a queued caller (under ChainCombiner::mu): a leader slot is free
void call_hint_lead(ChainCall* c) {
  uint32_t z = kCallWaiting;
  if (c->word.compare_exchange_strong(z, kCallLead, std::memory_order_acq_rel)) call_wake(c->word);
}

struct ChainCombiner {
  std::mutex mu;
  std::deque<ChainCall*> q;
  int leaders = 0;
};
// leaders at once (each on its own engine lease); FSTAMD_CHAIN_LEADERS overrides (A/B)
int chain_leaders() {
  static const int n = [] {
    const char* e = std::getenv("FSTAMD_CHAIN_LEADERS");
    return e && std::atoi(e) > 0 ? std::atoi(e) : 2;
  }();
  return n;
}
constexpr size_t kChainMaxBatch = 1u << 16;

ChainCombiner& chain_combiner(int dev) {
  static std::mutex mu;
  static auto* cs = new std::vector<std::unique_ptr<ChainCombiner>>();  // never destroyed
  std::lock_guard<std::mutex> g(mu);
  if ((int)cs->size() <= dev) cs->resize(dev + 1);
  if (!(*cs)[dev]) (*cs)[dev].reset(new ChainCombiner());
  return *(*cs)[dev];
}

void run_chain_calls(int dev, std::vector<ChainCall*>& calls) {
  // group by (rhs, n): one batch per group, strings in arrival order
  std::stable_sort(calls.begin(), calls.end(), [](const ChainCall* x, const ChainCall* y) {
    return std::make_pair(x->rhs.get(), x->n) < std::make_pair(y->rhs.get(), y->n);
  });
  for (size_t g0 = 0; g0 < calls.size();) {
    size_t g1 = g0 + 1;
    while (g1 < calls.size() && calls[g1]->rhs == calls[g0]->rhs && calls[g1]->n == calls[g0]->n)
      ++g1;
    const uint32_t num = (uint32_t)(g1 - g0);
    std::vector<uint64_t> offs(num + 1, 0);
    for (uint32_t i = 0; i < num; ++i) offs[i + 1] = offs[i] + calls[g0 + i]->labels->size();
    std::vector<uint32_t> labels(offs[num]);
    for (uint32_t i = 0; i < num; ++i)
      std::copy(calls[g0 + i]->labels->begin(), calls[g0 + i]->labels->end(),
                labels.begin() + offs[i]);
    auto hp = std::make_shared<HostPaths>();
    HostPaths& h = *hp;
    FstError e = FST_INVALID_ARG;
    HostProf prof;  // FSTAMD_HOST_PROF=1: the phases of this coalesced batch
    t_prof = prof.on ? &prof : nullptr;
    {
      DeviceEngine::Lease E = DeviceEngine::acquire(dev);
      if (E)
        e = run_chain_batch_host(E, *calls[g0]->rhs, labels.data(), offs.data(), num,
                                 calls[g0]->n, FST_SEM_LAZY, &h);
    }
    if (t_prof) {
      prof.lap(5);
      char what[96];
      std::snprintf(what, sizeof(what), "chain call batch (%u string(s))", num);
      prof.print(what);
      t_prof = nullptr;
    }
    for (uint32_t i = 0; i < num; ++i) {
      ChainCall* c = calls[g0 + i];
      c->err = e;
      c->stats = t_last_stats;
      if (e != FST_OK) continue;
      c->status = h.status[i];
      if (c->status != kPathOk) continue;
      c->fin = h.fin[i];
      c->paths = hp;
      c->index = i;
    }
    g0 = g1;
  }
}

FstError coalesced_chain_call(int dev, ChainCall* c) {
  if (dev < 0) return FST_INVALID_ARG;
  static const bool on = [] {
    const char* e = std::getenv("FSTAMD_COALESCE");
    return !(e && std::atoi(e) == 0);
  }();
  if (!on) {
    std::vector<ChainCall*> one{c};
    run_chain_calls(dev, one);
    return c->err;
  }
  ChainCombiner& C = chain_combiner(dev);
  std::unique_lock<std::mutex> lk(C.mu);
  C.q.push_back(c);
  // a call leads when a leader slot is free and no leader has taken it yet; a slot is only
  // ever taken here, by the thread itself under the lock, and given back by the same thread
  // after its batch, so slots can be neither lost nor duplicated (round-3 ADVICE)
  while (c->taken || C.leaders >= chain_leaders()) {
    lk.unlock();
    call_wait(c->word);
    lk.lock();
    if (c->word.load(std::memory_order_acquire) == kCallDone) return c->err;
    uint32_t h = kCallLead;  // hinted: look again (a done word is never rewritten)
    c->word.compare_exchange_strong(h, kCallWaiting, std::memory_order_acq_rel);
  }
  ++C.leaders;
  // this call first, then the oldest queued ones
  auto it = std::find(C.q.begin(), C.q.end(), c);
  C.q.erase(it);
  C.q.push_front(c);
  const size_t take = std::min(C.q.size(), kChainMaxBatch);
  std::vector<ChainCall*> batch(C.q.begin(), C.q.begin() + take);
  C.q.erase(C.q.begin(), C.q.begin() + take);
  for (ChainCall* x : batch) x->taken = true;
  // a second free slot: let the oldest remaining caller lead a batch beside this one
  if (!C.q.empty() && C.leaders < chain_leaders()) call_hint_lead(C.q.front());
  lk.unlock();
  run_chain_calls(dev, batch);
  for (ChainCall* x : batch) {
    if (x == c) continue;
    x->word.store(kCallDone, std::memory_order_release);
    call_wake(x->word);
  }
  lk.lock();
  --C.leaders;
  if (!C.q.empty()) call_hint_lead(C.q.front());
  return c->err;
}

}  // namespace

std::shared_ptr<FrozenFst> host::frozen_get(uint64_t h) { return g_fst.get(h); }
uint64_t host::frozen_insert(std::shared_ptr<FrozenFst> f) { return g_fst.insert(std::move(f)); }
MutableRead host::mutable_read(uint64_t h) {
  auto g = g_mut.lock_shared(h);
  return MutableRead{std::move(g), g_mut.get_locked(h)};
}

bool host::gpu_available() {
  static int ok = -1;
  static std::mutex mu;
  std::lock_guard<std::mutex> g(mu);
  if (ok < 0) {
    int n = 0;
    ok = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    if (!ok)
      std::fprintf(stderr,
                   "[libfst_amd] no usable HIP device: compose/shortest-path entries fail "
                   "(there is no CPU fallback)\n");
  }
  return ok == 1;
}

extern "C" {

// ---- MutableFst lifecycle -----------------------------------------------------------

FstMutableHandle fst_mutable_new(void) {
  return g_mut.insert(std::make_shared<MutableFst>());
}

FstMutableHandle fst_mutable_clone(FstMutableHandle handle) {
  std::shared_ptr<MutableFst> copy;
  {
    auto g = g_mut.lock_shared(handle);
    const MutableFst* m = g_mut.get_locked(handle);
    if (!m) return kInvalid;
    copy = std::make_shared<MutableFst>(*m);
  }
  return g_mut.insert(std::move(copy));
}

void fst_mutable_free(FstMutableHandle handle) { g_mut.remove(handle); }

uint32_t fst_mutable_add_state(FstMutableHandle handle) {
  auto g = g_mut.lock(handle);
  MutableFst* m = g_mut.get_locked(handle);
  if (!m) return FST_NO_STATE;
  return m->add_state();
}

FstError fst_mutable_set_start(FstMutableHandle handle, uint32_t state) {
  auto g = g_mut.lock(handle);
  MutableFst* m = g_mut.get_locked(handle);
  if (!m) return FST_INVALID_ARG;
  if (state >= m->num_states()) return FST_INVALID_STATE;
  m->set_start(state);
  return FST_OK;
}

FstError fst_mutable_set_final(FstMutableHandle handle, uint32_t state, double weight) {
  auto g = g_mut.lock(handle);
  MutableFst* m = g_mut.get_locked(handle);
  if (!m) return FST_INVALID_ARG;
  if (state >= m->num_states()) return FST_INVALID_STATE;
  m->set_final(state, weight);
  return FST_OK;
}

FstError fst_mutable_add_arc(FstMutableHandle handle, uint32_t src, uint32_t ilabel,
                             uint32_t olabel, double weight, uint32_t nextstate) {
  auto g = g_mut.lock(handle);
  MutableFst* m = g_mut.get_locked(handle);
  if (!m) return FST_INVALID_ARG;
  if (src >= m->num_states()) return FST_INVALID_STATE;
  if (nextstate >= m->num_states()) return FST_INVALID_STATE;
  m->add_arc(src, Arc{ilabel, olabel, weight, nextstate});
  return FST_OK;
}

uint32_t fst_mutable_start(FstMutableHandle handle) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  return m ? m->start() : FST_NO_STATE;
}

uint32_t fst_mutable_num_states(FstMutableHandle handle) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  return m ? (uint32_t)m->num_states() : 0;
}

uint32_t fst_mutable_num_arcs(FstMutableHandle handle, uint32_t state) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  if (!m || state >= m->num_states()) return 0;
  return (uint32_t)m->num_arcs(state);
}

double fst_mutable_final_weight(FstMutableHandle handle, uint32_t state) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  if (!m || state >= m->num_states()) return w_zero();
  return m->final_weight(state);
}

uint32_t fst_mutable_get_arcs(FstMutableHandle handle, uint32_t state, FstArc* buf,
                              uint32_t buf_len) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  if (!m || state >= m->num_states()) return 0;
  const auto& arcs = m->arcs(state);
  const uint32_t count = std::min<uint32_t>((uint32_t)arcs.size(), buf_len);
  if (buf)
    for (uint32_t i = 0; i < count; ++i)
      buf[i] = FstArc{arcs[i].ilabel, arcs[i].olabel, arcs[i].weight, arcs[i].nextstate};
  return count;
}

// ---- Freeze / frozen ----------------------------------------------------------------

FstHandle fst_freeze(FstMutableHandle mutable_handle) {
  std::shared_ptr<MutableFst> snap;
  {
    auto g = g_mut.lock_shared(mutable_handle);
    const MutableFst* m = g_mut.get_locked(mutable_handle);
    if (!m) return kInvalid;
    snap = std::make_shared<MutableFst>(*m);  // clone under the lock (c-api.zig:507-517)
  }
  auto f = FrozenFst::from_mutable(*snap, kWeightTropical);
  return g_fst.insert(std::move(f));
}

void fst_free(FstHandle handle) { g_fst.remove(handle); }

uint32_t fst_start(FstHandle handle) {
  auto f = g_fst.get(handle);
  return f ? f->start() : FST_NO_STATE;
}

uint32_t fst_num_states(FstHandle handle) {
  auto f = g_fst.get(handle);
  return f ? f->num_states() : 0;
}

uint32_t fst_num_arcs(FstHandle handle, uint32_t state) {
  auto f = g_fst.get(handle);
  if (!f || state >= f->num_states()) return 0;
  return f->num_arcs(state);
}

double fst_final_weight(FstHandle handle, uint32_t state) {
  auto f = g_fst.get(handle);
  if (!f || state >= f->num_states()) return w_zero();
  return f->final_weight(state);
}

uint32_t fst_get_arcs(FstHandle handle, uint32_t state, FstArc* buf, uint32_t buf_len) {
  auto f = g_fst.get(handle);
  if (!f || state >= f->num_states()) return 0;
  const StateEntry& e = f->states()[state];
  const uint32_t count = std::min(e.num_arcs, buf_len);
  if (buf)
    for (uint32_t i = 0; i < count; ++i) {
      const PackedArc& a = f->arcs()[e.arc_offset + i];
      buf[i] = FstArc{a.ilabel, a.olabel, a.weight, a.nextstate};
    }
  return count;
}

// ---- Binary I/O (src/io/binary.zig:9-36) ----------------------------------------------

FstHandle fst_load(const char* path) {
  if (!path) return kInvalid;
  auto f = FrozenFst::load_file(path, kWeightTropical, nullptr);  // binary.zig:16-36
  if (!f) return kInvalid;
  return g_fst.insert(std::move(f));
}

// src/c-api.zig:588-599: the whole file (at most 64 MiB, as readFileAlloc's limit there),
// parsed by readText; no label shift.
FstMutableHandle fst_read_text(const char* path) {
  if (!path) return kInvalid;
  std::vector<char> data;
  if (!read_file(path, 64l << 20, &data)) return kInvalid;
  auto m = std::make_shared<MutableFst>();
  if (!MutableFst::read_text(data.data(), data.size(), m.get())) return kInvalid;
  return g_mut.insert(std::move(m));
}

FstError fst_save(FstHandle handle, const char* path) {
  if (!path) return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> f = g_fst.get(handle);
  if (!f) return FST_INVALID_ARG;
  FILE* fp = std::fopen(path, "wb");
  if (!fp) return FST_IO_ERROR;
  const bool ok = std::fwrite(f->bytes(), 1, f->size(), fp) == f->size();
  std::fclose(fp);
  return ok ? FST_OK : FST_IO_ERROR;
}

// ---- The hot path -----------------------------------------------------------------

FstMutableHandle fst_compose_frozen_shortest_path(FstMutableHandle a_handle, FstHandle b_handle,
                                                  uint32_t n) {
  const auto t0 = std::chrono::steady_clock::now();
  auto us = [&] {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  };
  std::shared_ptr<MutableFst> a;
  std::shared_ptr<FrozenFst> b;
  // a compileString acceptor is snapshotted as its labels alone (the chain route below
  // needs nothing else); any other lhs as a deep copy
  std::vector<uint32_t> chain;
  bool is_chain = false;
  size_t a_states = 0, a_arcs = 0;
  bool a_start = false;
  {
    auto g = g_mut.lock_shared(a_handle);
    const MutableFst* ha = g_mut.get_locked(a_handle);
    if (!ha) {
      trace("sp_invalid_a", a_handle, b_handle, 0, 0, 0, 0, us(), 0);
      return kInvalid;
    }
    is_chain = as_chain(*ha, &chain);
    if (!is_chain) a = std::make_shared<MutableFst>(*ha);  // snapshot (c-api.zig:754)
    a_states = ha->num_states();
    a_arcs = is_chain ? chain.size() : ha->total_arcs();
    a_start = ha->start() != kNoState;
    b = g_fst.get(b_handle);                // pin (c-api.zig:759)
    if (!b) {
      trace("sp_invalid_b", a_handle, b_handle, a_states, a_arcs, 0, 0, us(), 0);
      return kInvalid;
    }
  }
  MutableFst result;
  // compose-shortest-path.zig:30-33: empty checks first, then n.
  if (!a_start || b->start() == kNoState || n == 0) {
    // empty result
  } else if (n != 1) {
    trace("sp_compose_error", a_handle, b_handle, a_states, a_arcs, 0, 0, us(), 0);
    return kInvalid;
  } else {
    if (!gpu_available()) return kInvalid;
    double kms = 0;
    int rc = -1;
    if (is_chain) {  // the batch engines on one string, coalesced with the chain calls of
                     // other threads (ChainCombiner)
      ChainCall c;
      c.rhs = b;
      c.n = n;
      c.labels = &chain;
      const FstError e = coalesced_chain_call(current_device(), &c);
      if (e == FST_OK) {
        if (c.status == kPathOk) {
          const HostPaths& h = *c.paths;
          const uint32_t P = h.len[c.index];
          const uint64_t o = h.off[c.index];
          result.add_states(P + 1);
          result.set_start(0);
          result.set_final(P, c.fin);
          for (uint32_t k = 0; k < P; ++k)
            result.add_arc(k, Arc{h.il[o + k], h.ol[o + k], h.w[o + k], k + 1});
          rc = 0;
        } else if (c.status == kPathEmpty) {
          rc = 0;  // the empty FST
        } else if (c.status == kPathCycle) {
          rc = 3;  // as the general path: the reference would not terminate
        }
        t_last_stats = c.stats;
        kms = c.stats.kernel_ms;
      }
    }
    // anything else (a general lhs; a string the batch engines handed back): one general lhs
    if (rc < 0) {
      if (!a) a = std::make_shared<MutableFst>(MutableFst::compile_chain(chain));
      rc = run_lazy_single(*a, *b, n, &result, &kms);
    }
    if (rc != 0) {
      trace("sp_compose_error", a_handle, b_handle, a_states, a_arcs, 0, 0, us(), kms);
      return kInvalid;
    }
  }
  trace("sp_ok", a_handle, b_handle, a_states, a_arcs, result.num_states(),
        result.total_arcs(), us(), t_last_stats.kernel_ms);
  return g_mut.insert(std::make_shared<MutableFst>(std::move(result)));
}

FstMutableHandle fst_compose_frozen(FstMutableHandle a_handle, FstHandle b_handle) {
  // src/c-api.zig:675-742 -> src/ops/compose.zig:29-198 on the GPU (kernels/eager_bfs.hpp):
  // the whole lattice, states numbered in BFS discovery order, arcs in compose order.
  const auto t0 = std::chrono::steady_clock::now();
  auto us = [&] {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  };
  std::shared_ptr<MutableFst> a;
  std::shared_ptr<FrozenFst> b;
  {
    auto g = g_mut.lock_shared(a_handle);
    const MutableFst* ha = g_mut.get_locked(a_handle);
    if (!ha) {
      trace("invalid_a", a_handle, b_handle, 0, 0, 0, 0, us(), 0);
      return kInvalid;
    }
    a = std::make_shared<MutableFst>(*ha);  // snapshot (c-api.zig:686)
    b = g_fst.get(b_handle);                // pin (c-api.zig:691)
    if (!b) {
      trace("invalid_b", a_handle, b_handle, a->num_states(), a->total_arcs(), 0, 0, us(), 0);
      return kInvalid;
    }
  }
  if (!gpu_available()) return kInvalid;
  const int dev = current_device();
  DeviceFst* D = dev >= 0 ? b->device(dev) : nullptr;
  if (!D) return kInvalid;
  const bool hprof = std::getenv("FSTAMD_HOST_PROF") != nullptr;
  HostLattice lat;
  LaunchStats st;
  double t_up0 = 0, t_up1 = 0;
  {
    DeviceEngine::Lease E = DeviceEngine::acquire(dev);
    if (!E) return kInvalid;
    const hipStream_t stream = E.stream();
    t_up0 = us();
    GraphUpload up(*a, stream);
    if (!up.ok) return kInvalid;
    t_up1 = us();
    if (E->compose_lattice(*D, up.g, &lat, &st, stream) != hipSuccess || lat.status != kPathOk) {
      trace("compose_error", a_handle, b_handle, a->num_states(), a->total_arcs(), 0, 0, us(),
            st.kernel_ms);
      return kInvalid;
    }
  }
  t_last_stats = st;
  const double t_gpu = us();
  MutableFst result;
  if (lat.n_nodes > 0) {
    result.add_states(lat.n_nodes);
    result.set_start(0);
    // states in contiguous ranges, one host thread each (a 10 M-arc lattice: ~80 ms on
    // one thread); every state's arc vector is its own allocation
    auto build = [&](uint32_t lo, uint32_t hi) {
      for (uint32_t s2 = lo; s2 < hi; ++s2) {
        if (!w_is_zero(lat.nfin[s2])) result.set_final(s2, lat.nfin[s2]);
        const uint32_t k0 = lat.aoff[s2], k1 = lat.aoff[s2 + 1];
        result.reserve_arcs(s2, k1 - k0);
        for (uint32_t k = k0; k < k1; ++k)
          result.add_arc(s2, Arc{lat.ail[k], lat.aol[k], lat.aw[k], lat.anext[k]});
      }
    };
    const uint32_t nt = lat.n_arcs < (1u << 18) ? 1u
                        : std::min<uint32_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (uint32_t t = 1; t < nt; ++t)
      th.emplace_back(build, (uint32_t)((uint64_t)lat.n_nodes * t / nt),
                      (uint32_t)((uint64_t)lat.n_nodes * (t + 1) / nt));
    build(0, (uint32_t)((uint64_t)lat.n_nodes / nt));
    for (auto& x : th) x.join();
  }
  if (hprof)
    std::fprintf(stderr,
                 "[libfst_amd host] fst_compose_frozen: upload %.2f compose+download %.2f "
                 "(kernel %.2f, %u launch(es)) result %.2f ms\n",
                 (t_up1 - t_up0) / 1e3, (t_gpu - t_up1) / 1e3, st.kernel_ms, st.launches,
                 (us() - t_gpu) / 1e3);
  trace("ok", a_handle, b_handle, a->num_states(), a->total_arcs(), result.num_states(),
        result.total_arcs(), us(), st.kernel_ms);
  return g_mut.insert(std::make_shared<MutableFst>(std::move(result)));
}

FstMutableHandle fst_shortest_path(FstMutableHandle handle, uint32_t n) {
  // src/c-api.zig:897-916 -> src/ops/shortest-path.zig:18-139 on the GPU.
  const bool hprof = std::getenv("FSTAMD_HOST_PROF") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  auto ms = [&] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  std::unique_ptr<HostGraph> m;
  {
    auto g = g_mut.lock_shared(handle);
    const MutableFst* h = g_mut.get_locked(handle);
    if (!h) return kInvalid;
    m = std::make_unique<HostGraph>(*h);  // snapshot, flattened to CSR under the lock
  }
  const double t_snap = ms();
  MutableFst result;
  const uint32_t m_states = (uint32_t)m->fin.size();
  if (m->start == kNoState || n == 0) {  // :21-23 -> empty
  } else if (n != 1) {                   // :24 UnsupportedNShortest
    return kInvalid;
  } else {
    if (!gpu_available()) return kInvalid;
    const int dev = current_device();
    if (dev < 0) return kInvalid;
    DeviceEngine::Lease E = DeviceEngine::acquire(dev);
    if (!E) return kInvalid;
    const hipStream_t stream = E.stream();
    GraphUpload up(*m, stream);
    m.reset();
    const double t_up = ms();
    // Non-negative weights: the parallel fixpoint (eager_bfs.hpp); a negative weight:
    // the exact replay of the reference's heap order (sp_replay_kernel).  NaN has no
    // order in the reference's compare (std.math.order): reported as an error.
    if (!up.ok || up.nan) return kInvalid;
    const uint64_t cap = std::max<uint64_t>(m_states + 16, 1024);
    DevOut out(1, cap);
    if (!out.ok()) return kInvalid;
    LaunchStats st;
    HostPaths hp;
    if (E->shortest_path_graph(up.g, n, out.v, &st, stream, up.nonneg) != hipSuccess)
      return kInvalid;
    if (!out.download(1, &hp, stream)) return kInvalid;
    t_last_stats = st;
    if (hp.status[0] == kPathCycle || hp.status[0] == kPathInternal ||
        hp.status[0] == kPathOutputFull)
      return kInvalid;
    result = chain_result(hp, 0);  // OK or EMPTY
    if (hprof)
      std::fprintf(stderr,
                   "[libfst_amd host] fst_shortest_path call: snapshot %.2f upload %.2f engine + "
                   "result %.2f ms\n", t_snap, t_up - t_snap, ms() - t_up);
  }
  return g_mut.insert(std::make_shared<MutableFst>(std::move(result)));
}

// ---- Strings ------------------------------------------------------------------------

FstMutableHandle fst_compile_string(const uint8_t* input, uint32_t len) {
  if (!input) return kInvalid;
  return g_mut.insert(
      std::make_shared<MutableFst>(MutableFst::compile_string(input, len, input, len)));
}

static int32_t print_impl(FstMutableHandle handle, uint8_t* buf, uint32_t buf_len, bool out_tape) {
  auto g = g_mut.lock_shared(handle);
  const MutableFst* m = g_mut.get_locked(handle);
  if (!m) return -1;
  std::vector<uint8_t> s;
  if (!m->print_string(out_tape, &s)) return -1;
  if (s.size() > buf_len) return -1;
  if (buf && !s.empty()) std::memcpy(buf, s.data(), s.size());
  return (int32_t)s.size();
}

int32_t fst_print_string(FstMutableHandle handle, uint8_t* buf, uint32_t buf_len) {
  return print_impl(handle, buf, buf_len, false);
}

int32_t fst_print_output_string(FstMutableHandle handle, uint8_t* buf, uint32_t buf_len) {
  return print_impl(handle, buf, buf_len, true);
}

void fst_teardown(void) {
  g_mut.clear();
  g_fst.clear();
  pool_release(-1);
  pin_pool_clear();
}

// (fst_batch.h: beside the coalescer whose state it reads)
int32_t fst_debug_coalescer_state(int32_t device, uint32_t* queued) {
  if (device < 0) return -1;
  ChainCombiner& C = chain_combiner(device);
  std::lock_guard<std::mutex> g(C.mu);
  if (queued) *queued = (uint32_t)C.q.size();
  return C.leaders;
}

}  // extern "C"

// batch_streamed.cpp -- the streamed host batch.
// One device, an rhs without input epsilons whose first tier is a pull tier (the metric's
// case: DeviceEngine::pull_first).  Every path then has exactly L arcs, so string i's path
// can sit at its own label offsets (BatchOutDev::slots) and the result's CSR offsets are
// the rebased input offsets.  The batch runs as a few parts of growing size (labels 1/43,
// 6/43, 36/43: each part's upload fits in the previous part's compute), alternating
// between two engines (streams), each part's launch waiting on its labels' upload event;
// the second engine's kernels fill the GPU while the first one's drain.  Meanwhile:
//  * other host threads copy the labels into result.ilabels (on an OK path il[k] = label
//    k: the result's ilabels are the input labels);
//  * the pull tier copies each finished path's olabels and weights into the (pinned,
//    device-mapped) result with whole-line stores as it goes (copy_out_paths): no D2H of
//    paths, no compaction pass on the device;
//  * statuses and final weights (12 B per string) come down per part;
//  * strings the pull tier handed on are finished by the later tiers in the device arena
//    (same slots) and downloaded after them; strings without a path are compacted out.
// No kernel ever waits on the host or another queue (only stream-ordered event waits).
// Labels read from host memory instead (zero-copy) measured 34.5 vs 30.6 ms per 1M metric
// strings: a PCIe read at every string's start.  Returns kStreamNotApplicable when the mode
// does not apply; the caller then takes the pipelined path.
#include <condition_variable>
#include <map>

#include "host_rt.hpp"
#include "weight_codes.hpp"

namespace fstamd::host {
namespace {

// FSTAMD_STREAM_CODES: 0 = the f64 copy-out for every part, 1 = every part's weights leave
// as 1-B codes (default), 2 = every part but the last
int stream_codes_mode() {
  const char* e = std::getenv("FSTAMD_STREAM_CODES");
  const int m = e ? std::atoi(e) : 1;
  return m < 0 || m > 2 ? 1 : m;
}

// The parts' cuts, per mille of a shard's labels: FSTAMD_STREAM_CUTS, or 1/43 and 7/43 (each
// part's upload fits in the previous part's compute), and, when every part leaves codes,
// shrinking parts after the big one, so that little expansion is left after the last kernel.
std::vector<uint64_t> stream_cuts(bool all_coded) {
  std::vector<uint64_t> pm{23, 163};
  if (all_coded) pm = {23, 163, 700, 900, 970};
  if (const char* ce = std::getenv("FSTAMD_STREAM_CUTS")) {
    pm.clear();
    for (const char* q = ce; *q;) {
      char* e = nullptr;
      const unsigned long v = std::strtoul(q, &e, 10);
      if (e == q) break;
      if (v > 0 && v < 1000) pm.push_back(v);
      q = *e ? e + 1 : e;
    }
  }
  return pm;
}
constexpr size_t kStreamMaxParts = 64;

// a block of the pinned host pool, given back on scope exit
struct PinBlock {
  void* p = nullptr;
  void reset(void* q) {
    if (p) pin_release(p);
    p = q;
  }
  ~PinBlock() { reset(nullptr); }
  PinBlock() = default;
  PinBlock(const PinBlock&) = delete;
  PinBlock& operator=(const PinBlock&) = delete;
};

struct StreamKit {  // per calling thread and device: the upload stream and its events
  hipStream_t up = nullptr;
  std::vector<hipEvent_t> ev;
  bool init(int dev) {
    if (!up && hipSetDevice(dev) == hipSuccess)
      (void)hipStreamCreateWithFlags(&up, hipStreamNonBlocking);
    return up != nullptr;
  }
  bool events(size_t n) {
    while (ev.size() < n) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
      ev.push_back(e);
    }
    return true;
  }
};

// StreamKits are leased per call from a process-wide pool per device (a kit per calling
// thread leaked a stream and its events for every thread that ever entered the batch
// API): the pool holds at most as many kits as calls ever ran at once on the device.
// (Never destroyed: the process may exit after the runtime's teardown.)
class KitLease {
 public:
  explicit KitLease(int dev) : dev_(dev) {
    Pool& P = pool();
    {
      std::lock_guard<std::mutex> g(P.mu);
      auto& v = P.free[dev];
      if (!v.empty()) {
        k_ = v.back();
        v.pop_back();
      }
    }
    if (!k_) k_ = new StreamKit;
    if (!k_->init(dev)) {
      give_back();
      k_ = nullptr;
    }
  }
  ~KitLease() { give_back(); }
  StreamKit* operator->() const { return k_; }
  explicit operator bool() const { return k_ != nullptr; }
  KitLease(const KitLease&) = delete;
  KitLease& operator=(const KitLease&) = delete;

 private:
  struct Pool {
    std::mutex mu;
    std::map<int, std::vector<StreamKit*>> free;
  };
  static Pool& pool() {
    static Pool* p = new Pool;
    return *p;
  }
  void give_back() {
    if (!k_) return;
    Pool& P = pool();
    std::lock_guard<std::mutex> g(P.mu);
    P.free[dev_].push_back(k_);
    k_ = nullptr;
  }
  int dev_;
  StreamKit* k_ = nullptr;
};

// One shard of a streamed batch: strings [s0, s1) on device `dev`, everything but the
// result's final CSR compaction.  The result is already allocated and its offsets `poff`
// (the batch's rebased input offsets) filled; the shard's paths sit at those offsets (its
// labels at poff[s0] and up, its device buffers indexed from there), its statuses, final
// weights and pull-tier statuses at string s0 and up.
struct StreamShard {
  int dev = 0;
  uint32_t s0 = 0, s1 = 0;
  FstError err = FST_OK;
  double wall_ms = 0;
  uint32_t launches = 0;
};

FstError stream_shard(StreamShard& S, DeviceFst& D, const StreamIo& io, const uint64_t* poff,
                      uint32_t max_len, uint32_t n, int semantics, int32_t* first_all,
                      std::mutex* later_mu) {
  const bool tm = io.text_mode();
  FstBatchResult* const out = io.out;  // (label mode)
  // the later tiers of the shards of one device run one shard at a time, each to the end of
  // its leases (declared after this lock, so released before it): the heavy replays size
  // their workspaces from the free HBM, which a concurrent shard's would have taken
  std::unique_lock<std::mutex> later_lock(*later_mu, std::defer_lock);
  const int dev = S.dev;
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const uint32_t num = S.s1 - S.s0;
  const uint64_t lbase = poff[S.s0], total = poff[S.s1] - lbase;
  if (num == 0) return FST_OK;
  KitLease K(dev);
  if (!K) return FST_OOM;
  const hipStream_t up = K->up;
  // the shard's offsets from its first label (shard 0 of the batch: poff itself)
  PinnedVec<uint64_t> loff_own(lbase ? num + 1 : 0);
  const uint64_t* loff = poff + S.s0;
  if (lbase) {
    for (uint32_t i = 0; i <= num; ++i) loff_own[i] = poff[S.s0 + i] - lbase;
    loff = loff_own.data();
  }
  const uint32_t* lsrc = io.labels ? io.labels + lbase : nullptr;
  const uint8_t* tsrc = io.text ? io.text + lbase : nullptr;
  uint32_t* const il_out = tm ? nullptr : out->ilabels + lbase;
  struct Threads {  // joined on every return (declared after what they use)
    std::vector<std::thread> th;
    void join() {
      for (auto& t : th) t.join();
      th.clear();
    }
    ~Threads() { join(); }
  };

  // ---- parts: string ranges cut at these fractions of the labels (per mille; small
  // shards: one part; stream_cuts).  FSTAMD_STREAM_CUTS overrides (A/B, one box, f64
  // copy-out: "23,163" 30.9 ms per 1M metric strings, "167" 31.2, "100,400" 31.0, "125"
  // 31.5) ----
  // Weight codes: when this rhs, these semantics and this max_len take tier
  // P's code instances (pull_codes_table: pull_rk / pull_pack decide) the coded parts' weights
  // cross the link as one byte per arc into a pinned staging block, and expander threads turn
  // each part's codes into the result's f64 weights once that part's completion event has
  // passed, while the later parts run.  The last part's expansion stands exposed after the
  // last kernel, so the coded route ends on shrinking parts.
  double code_table[256];
  int codes_mode = tm ? 0 : stream_codes_mode();
  if (codes_mode && !pull_codes_table(D, semantics, max_len, code_table)) codes_mode = 0;
  PinBlock staging;  // the shard's codes, indexed like its labels
  if (codes_mode) {
    staging.reset(pin_alloc(std::max<uint64_t>(total, 1)));  // (the copy-out stays inside each string)
    if (!staging.p || !pin_is_pinned(staging.p)) {  // (the pool gave pageable memory)
      staging.reset(nullptr);
      codes_mode = 0;
    }
  }
  std::vector<uint32_t> cut{0};
  if (total >= (1u << 22) && num >= (1u << 15)) {
    for (uint64_t f : stream_cuts(codes_mode == 1)) {
      const uint64_t want = total * f / 1000;
      const uint32_t i = (uint32_t)(std::upper_bound(loff, loff + num, want) - loff);
      if (i > cut.back() && i < num) cut.push_back(i);
    }
  }
  cut.push_back(num);
  const size_t parts = cut.size() - 1;
  // one upload event and one completion event a part (run_streamed has checked that this
  // device's kit and events exist before it allocated the result)
  if (parts > kStreamMaxParts || !K->events(2 * parts)) return FST_OOM;
  // parts [0, ncoded) leave codes; mode 2: the last part keeps the f64 copy-out
  const size_t ncoded = codes_mode == 1 ? parts : codes_mode == 2 ? parts - 1 : 0;
  if (std::getenv("FSTAMD_ROUTE_LOG"))
    std::fprintf(stderr, "[libfst_amd route] stream: weight codes %s, mode %d, parts %zu\n",
                 ncoded ? "on" : "off", ncoded ? codes_mode : 0, parts);

  // ---- engines and device buffers ----
  DeviceEngine::Lease EA = DeviceEngine::acquire(dev);
  if (!EA) return FST_INVALID_ARG;
  DeviceEngine::Lease EB;
  if (parts > 1) EB = DeviceEngine::try_acquire(dev);  // (none free: one engine in order)
  const hipStream_t sA = EA.stream(), sB = EB ? EB.stream() : nullptr;
  // (text mode: d_lab holds the bytes themselves)
  DevBuf d_lab(std::max<uint64_t>(total, 1) * (tm ? 1 : 4)), d_off((num + 1) * 8ull),
      d_first(std::max<size_t>(num, 1) * 4ull), d_ctr(64 * 4);  // item counter per part
  DevOut o(num, total + 4);
  if (!d_lab.p || !d_off.p || !d_first.p || !d_ctr.p || !o.ok()) return FST_OOM;
  // the device byte arena of the codes (indexed like the path arena)
  std::unique_ptr<DevBuf> d_codes;
  if (ncoded) {
    d_codes = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1));
    if (!d_codes->p) return FST_OOM;
  }
  // text mode: byte counts and total weights per string, and one TextOutDev per part (the
  // kernels reach it through BatchOutDev::text), uploaded with the offsets
  // (d_lab4: the widened labels of a shard that hands strings on, allocated only then)
  std::unique_ptr<DevBuf> d_nb, d_tw, d_tx, d_lab4;
  std::vector<TextOutDev> txs;  // (outlives the streams' work: declared before sync_all)
  if (tm) {
    d_nb = std::make_unique<DevBuf>(std::max<size_t>(num, 1) * 4ull);
    d_tw = std::make_unique<DevBuf>(std::max<size_t>(num, 1) * 8ull);
    d_tx = std::make_unique<DevBuf>(64 * sizeof(TextOutDev));
    if (!d_nb->p || !d_tw->p || !d_tx->p) return FST_OOM;
    for (size_t p = 0; p < parts; ++p)
      txs.push_back(TextOutDev{io.tout->text + lbase, (uint32_t*)d_nb->p + cut[p],
                               (double*)d_tw->p + cut[p]});
  }
  // the arena's path arrays shifted so that each element shares its host twin's address
  // modulo 16 (the copy-out's 16-B units, kernels/device_common.hpp copy_out_paths)
  BatchOutDev vb = o.v;
  vb.out_il += lbase & 3u;
  vb.out_ol += lbase & 3u;
  vb.out_w += lbase & 1u;
  // every return: no kernel or copy still uses the buffers or the result
  StreamDrain sync_all{{up, sA, sB}};

  // ---- uploads (offsets, then each part's labels: one event per part) ----
  // Two ways to move the labels (FSTAMD_STREAM_STAGE): 0 = the runtime stages the pageable
  // source itself while other threads copy it into the result's ilabels (the labels cross
  // host DRAM twice); 1 = threads copy each chunk into the result's (pinned) ilabels and
  // the chunk's DMA reads it from there (once).
  const char* stage_env = std::getenv("FSTAMD_STREAM_STAGE");
  const int stage_mode = stage_env ? std::atoi(stage_env) : 0;
  struct Ready {
    std::mutex mu;
    std::condition_variable cv;
    size_t n = 0;
    bool failed = false;
  } R;
  Threads Th;
  Th.th.emplace_back([&] {
    // (the fills first, on the idle GPU: every string INTERNAL until a tier finishes it,
    // the parts' item counters zero; the parts wait on events recorded after them)
    bool ok = hipSetDevice(dev) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)o.status.p, kPathInternal, num, up) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)d_first.p, kPathInternal, num, up) == hipSuccess &&
              hipMemsetAsync(d_ctr.p, 0, 64 * 4, up) == hipSuccess &&
              hipMemcpyAsync(d_off.p, loff, (num + 1) * 8ull, hipMemcpyHostToDevice, up) ==
                  hipSuccess &&
              (!tm || hipMemcpyAsync(d_tx->p, txs.data(), parts * sizeof(TextOutDev),
                                     hipMemcpyHostToDevice, up) == hipSuccess);
    constexpr uint64_t kChunk = 1ull << 21;  // labels per staged chunk (8 MB)
    for (size_t p = 0; p < parts && ok; ++p) {
      const uint64_t a = loff[cut[p]], z = loff[cut[p + 1]];
      if (tm) {  // the part's bytes, as they are
        ok = z == a || hipMemcpyAsync((uint8_t*)d_lab.p + a, tsrc + a, z - a,
                                      hipMemcpyHostToDevice, up) == hipSuccess;
      } else if (stage_mode == 1) {
        for (uint64_t c = a; c < z && ok; c += kChunk) {
          const uint64_t e = std::min(z, c + kChunk), w = e - c;
          const uint64_t T = w >= (1u << 19) ? 4 : 1;
          std::vector<std::thread> cp;
          for (uint64_t t = 1; t < T; ++t)
            cp.emplace_back([&, t, T] {
              std::memcpy(il_out + c + w * t / T, lsrc + c + w * t / T,
                          (w * (t + 1) / T - w * t / T) * 4);
            });
          std::memcpy(il_out + c, lsrc + c, (w / T) * 4);
          for (auto& x : cp) x.join();
          ok = hipMemcpyAsync((uint32_t*)d_lab.p + c, il_out + c, w * 4, hipMemcpyHostToDevice,
                              up) == hipSuccess;
        }
      } else {
        // (a pageable source is staged through pinned memory before this returns)
        ok = z == a || hipMemcpyAsync((uint32_t*)d_lab.p + a, lsrc + a, (z - a) * 4,
                                      hipMemcpyHostToDevice, up) == hipSuccess;
      }
      ok = ok && hipEventRecord(K->ev[p], up) == hipSuccess;
      std::lock_guard<std::mutex> g(R.mu);
      if (ok) R.n = p + 1;
      R.cv.notify_all();
    }
    std::lock_guard<std::mutex> g(R.mu);
    if (!ok) R.failed = true;
    R.cv.notify_all();
  });
  if (!tm && stage_mode != 1) {
    // the result's ilabels, once the uploads are staged: the runtime's staging copies of
    // a pageable source read the same pages, and the kernels wait for them, not for these
    const uint64_t T = total >= (1u << 20) ? 3 : 1;
    for (uint64_t t = 0; t < T; ++t)
      Th.th.emplace_back([&, t, T] {
        {
          std::unique_lock<std::mutex> g(R.mu);
          R.cv.wait(g, [&] { return R.failed || R.n == parts; });
        }
        const uint64_t a = total * t / T, z = total * (t + 1) / T;
        if (z > a) std::memcpy(il_out + a, lsrc + a, (z - a) * 4);
      });
  }

  // ---- the expanders: thread t of T takes the t-th slice of every coded part, in part
  // order.  It waits (host side) until the part's completion event has been recorded --
  // synchronising an event nobody recorded yet, or one a previous call left complete, would
  // return at once -- then for the event itself, and only then reads the part's codes.
  // Nothing polls memory the device writes.  Joined on every return (declared after the
  // staging block, the result and the streams' drain). ----
  struct Recorded {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> rec;
    bool abort = false;
  } X;
  X.rec.assign(parts, 0);
  auto x_abort = [&] {
    std::lock_guard<std::mutex> g(X.mu);
    X.abort = true;
    X.cv.notify_all();
  };
  std::atomic<bool> x_failed{false};
  // (FSTAMD_HOST_PROF: when each part's event passed and when its expansion ended, ms from
  // the expanders' start, per thread)
  const bool x_prof = std::getenv("FSTAMD_HOST_PROF") != nullptr;
  const auto tx0 = std::chrono::steady_clock::now();
  auto x_ms = [&] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tx0).count();
  };
  std::vector<double> x_ev, x_end;  // [thread * ncoded + part]
  Threads Ex;
  if (ncoded) {
    const char* xe = std::getenv("FSTAMD_STREAM_EXPANDERS");
    const uint32_t T = (uint32_t)std::min(16, std::max(1, xe ? std::atoi(xe) : 4));
    const uint8_t* const codes = (const uint8_t*)staging.p;
    double* const w_out = out->weights + lbase;
    x_ev.assign(T * ncoded, 0.0);
    x_end.assign(T * ncoded, 0.0);
    for (uint32_t t = 0; t < T; ++t)
      Ex.th.emplace_back([&, t, T, codes, w_out] {
        if (hipSetDevice(dev) != hipSuccess) {
          x_failed = true;
          return;
        }
        for (size_t p = 0; p < ncoded; ++p) {
          {
            std::unique_lock<std::mutex> g(X.mu);
            X.cv.wait(g, [&] { return X.abort || X.rec[p]; });
            if (!X.rec[p]) return;
          }
          if (hipEventSynchronize(K->ev[parts + p]) != hipSuccess) {
            x_failed = true;
            return;
          }
          if (x_prof) x_ev[t * ncoded + p] = x_ms();
          // (slices cut at 8 elements: whole lines of the weights for all but the ends)
          const uint64_t a = loff[cut[p]], z = loff[cut[p + 1]], w = z - a;
          const uint64_t lo = a + ((w * t / T) & ~7ull), hi = t + 1 == T ? z : a + ((w * (t + 1) / T) & ~7ull);
          if (hi > lo) expand_weight_codes(codes + lo, hi - lo, code_table, w_out + lo);
          if (x_prof) x_end[t * ncoded + p] = x_ms();
        }
      });
  }

  // ---- the parts: engine A takes parts 0, 2, .., engine B 1, 3, .. (A all without B) ----
  std::vector<FstError> perr(parts, FST_OK);
  // (A/B timing only: FSTAMD_STREAM_AB=1 drops the copy-out; the result then lacks paths)
  const char* abe = std::getenv("FSTAMD_STREAM_AB");
  const bool ab_nocopy = abe && std::atoi(abe) == 1;
  auto drive = [&](DeviceEngine::Lease& E, hipStream_t s, size_t p0, size_t step) {
    if (hipSetDevice(dev) != hipSuccess) {
      perr[p0] = FST_INVALID_ARG;
      x_abort();
      return;
    }
    for (size_t p = p0; p < parts; p += step) {
      {
        std::unique_lock<std::mutex> g(R.mu);
        R.cv.wait(g, [&] { return R.failed || R.n > p; });
        if (R.n <= p) {
          perr[p] = FST_OOM;
          x_abort();
          return;
        }
      }
      const uint32_t s0 = cut[p], np = cut[p + 1] - cut[p];
      ChainInput in{(const uint32_t*)d_lab.p, (const uint64_t*)d_off.p + s0, np, max_len};
      if (tm) in.text = (const uint8_t*)d_lab.p;  // (the bytes, in the labels' place)
      BatchOutDev v = vb;
      v.status += s0;
      v.path_len += s0;
      v.path_off += s0;
      v.final_w += s0;
      v.slots = (const uint64_t*)d_off.p + s0;
      const bool coded = p < ncoded;
      if (tm) {
        v.text = (const TextOutDev*)d_tx->p + p;
      } else if (coded) {  // the byte arenas in the weights' places (kernels/eager_pull.hpp CODES)
        v.host_ol = out->olabels + lbase;
        v.out_w = (double*)d_codes->p;
        v.host_w = (double*)staging.p;
      } else {
        v.host_ol = out->olabels + lbase;
        v.host_w = out->weights + lbase;
      }
      // (label mode only: without its emission the text route has no result at all)
      if (ab_nocopy && !tm && !coded) v.host_ol = nullptr, v.host_w = nullptr;
      v.first_status = (int32_t*)d_first.p + s0;
      // the pull tier alone: no fill, copy or host synchronisation between parts (a fill
      // or copy is a blit kernel that waits for CU slots behind the other engine's
      // persistent kernel, and had held this engine's next part back); the later tiers
      // and the downloads come after the last part
      if (hipStreamWaitEvent(s, K->ev[p], 0) != hipSuccess ||
          E->launch_pull_part(D, in, n, semantics, v, s, (unsigned int*)d_ctr.p + p, tm, coded) !=
              hipSuccess ||
          (coded && hipEventRecord(K->ev[parts + p], s) != hipSuccess)) {
        perr[p] = FST_OOM;
        x_abort();
        return;
      }
      if (coded) {  // the part's completion event is in the stream: its expanders may wait
        std::lock_guard<std::mutex> g(X.mu);
        X.rec[p] = 1;
        X.cv.notify_all();
      }
    }
  };
  const auto tk0 = std::chrono::steady_clock::now();
  {
    Threads P;
    if (EB) P.th.emplace_back([&] { drive(EB, sB, 1, 2); });
    drive(EA, sA, 0, EB ? 2 : 1);
    P.join();
  }
  for (hipStream_t x : {up, sA, sB})
    if (x && hipStreamSynchronize(x) != hipSuccess) return FST_OOM;
  for (size_t p = 0; p < parts; ++p)
    if (perr[p] != FST_OK) return perr[p];
  int32_t* const st_out = (tm ? io.tout->status : out->status) + S.s0;
  // (text mode: the total weights in the final weights' place, and the byte counts)
  double* const fin_out = (tm ? io.tout->total_weight : out->final_weights) + S.s0;
  const void* const d_fin = tm ? d_tw->p : o.fin.p;
  int32_t* const first = first_all + S.s0;
  // statuses, final weights and the pull tier's statuses in one download each
  auto download = [&](bool with_first) {
    return d2h(st_out, o.status.p, num * 4ull, sA) && d2h(fin_out, d_fin, num * 8ull, sA) &&
           (!tm || d2h(io.nbytes + S.s0, d_nb->p, num * 4ull, sA)) &&
           (!with_first || d2h(first, d_first.p, num * 4ull, sA)) &&
           hipStreamSynchronize(sA) == hipSuccess;
  };
  // (an error return here leaves expanders in flight: they are joined on the way out)
  if (!download(true) || fault_inject("stream_after_pull")) return FST_OOM;
  // the expanders, before anything else writes the result's weights: what the later tiers
  // finish is downloaded over whatever the expanders made of those strings' unwritten codes
  Ex.join();
  if (x_failed) return FST_OOM;
  if (x_prof && ncoded) {
    const size_t T = x_ev.size() / ncoded;
    for (size_t p = 0; p < ncoded; ++p) {
      double e0 = x_ev[p], e1 = 0;
      for (size_t t = 0; t < T; ++t) {
        e0 = std::min(e0, x_ev[t * ncoded + p]);
        e1 = std::max(e1, x_end[t * ncoded + p]);
      }
      std::fprintf(stderr, "[libfst_amd stream] part %zu labels %llu event +%.3f ms expanded +%.3f ms\n",
                   p, (unsigned long long)(loff[cut[p + 1]] - loff[cut[p]]), e0, e1);
    }
    std::fprintf(stderr, "[libfst_amd stream] expanders joined +%.3f ms\n", x_ms());
  }
  // the later tiers, once, over the strings the pull tier handed on (in the device arena,
  // the same slots) -- only when it handed some on (the metric: none), then the statuses
  // and final weights again
  bool handed = false;
  for (uint32_t i = 0; i < num && !handed; ++i) handed = first[i] != kPathOk && first[i] != kPathEmpty;
  uint32_t launches = (uint32_t)parts;
  if (tm && std::getenv("FSTAMD_SHARD_LOG")) {  // tests (text mode): what the pull tier handed on
    uint32_t nh = 0;
    for (uint32_t i = 0; i < num; ++i) nh += first[i] != kPathOk && first[i] != kPathEmpty;
    std::fprintf(stderr, "[libfst_amd stream] dev %d strings %u..%u parts %zu handed-on %u\n", dev,
                 S.s0, S.s1, parts, nh);
  }
  if (handed) {
    later_lock.lock();
    ChainInput in{(const uint32_t*)d_lab.p, (const uint64_t*)d_off.p, num, max_len};
    // text mode: the later tiers read 4-B labels -- the shard's bytes widened once, now
    // (only batches that hand strings on pay for the buffer and the kernel)
    if (tm) {
      d_lab4 = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1) * 4);
      if (!d_lab4->p ||
          EA->widen_text((const uint8_t*)d_lab.p, (const uint64_t*)d_off.p, num,
                         (uint32_t*)d_lab4->p, sA) != hipSuccess)
        return FST_OOM;
      in.labels = (const uint32_t*)d_lab4->p;
    }
    BatchOutDev v = vb;
    v.slots = (const uint64_t*)d_off.p;
    EA->set_after_pull(true);
    hipError_t e = EA->run_chain(D, in, n, semantics, v, sA, nullptr);
    EA->set_after_pull(false);
    // text mode: the paths the later tiers left in the arena's slots, emitted as the pull
    // tier's are (the same slots of the result)
    if (tm && e == hipSuccess)
      e = EA->text_fixup(v, TextOutDev{io.tout->text + lbase, (uint32_t*)d_nb->p,
                                       (double*)d_tw->p},
                         (const int32_t*)d_first.p, num, sA);
    if (e != hipSuccess || !download(false)) return FST_OOM;
    ++launches;
  }

  // ---- paths the later tiers wrote (device arena, same slots) ----
  uint64_t nfix = 0;
  if (!tm)
    for (uint32_t i = 0; i < num; ++i) nfix += st_out[i] == kPathOk && first[i] != kPathOk;
  if (nfix) {
    bool ok = true;
    const char* few_env = std::getenv("FSTAMD_STREAM_FIX_FEW");  // (tests: 0 = bulk copy)
    const uint64_t few = few_env ? std::strtoull(few_env, nullptr, 10) : 4096ull;
    if (nfix <= few) {
      for (uint32_t i = 0; i < num && ok; ++i)
        if (st_out[i] == kPathOk && first[i] != kPathOk) {
          const uint64_t a = loff[i], L = loff[i + 1] - a;
          ok = d2h(out->olabels + lbase + a, vb.out_ol + a, L * 4, sA) &&
               d2h(out->weights + lbase + a, vb.out_w + a, L * 8, sA);
        }
    } else {  // many: the whole arena (every pull-tier chase writes its path there too)
      ok = d2h(out->olabels + lbase, vb.out_ol, total * 4, sA) &&
           d2h(out->weights + lbase, vb.out_w, total * 8, sA);
    }
    if (!ok || hipStreamSynchronize(sA) != hipSuccess) return FST_OOM;
    // ... but not the weights of the coded parts' pull-tier paths: those exist as codes
    // alone, and are expanded again over what the bulk download put in their slots
    if (nfix > few && ncoded)
      for (uint32_t i = 0; i < cut[ncoded]; ++i)
        if (first[i] == kPathOk) {
          const uint64_t a = loff[i], L = loff[i + 1] - a;
          expand_weight_codes((const uint8_t*)staging.p + a, L, code_table,
                              out->weights + lbase + a);
        }
  }
  Th.join();
  S.launches = launches;
  S.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0)
                  .count();
  return FST_OK;
}

}  // namespace

// The streamed text batch's last step, on the host: the fixed text slots closed up into the
// CSR result, moving left in input order (as the label route drops the slots of strings
// without a path).  In: offsets = the slots, nbytes[i] = what the device wrote into slot i
// (kTextNotBytes: a path with an olabel > 256), status.  Out: offsets = the prefix sum of the
// OK strings' byte counts, the text compacted in place; UNSUPPORTED for the kTextNotBytes
// strings, +inf total weight and no bytes for every non-OK string.  A count beyond its slot
// (an engine bug) reads INTERNAL and moves nothing.  Returns the total.
uint64_t text_compact(uint32_t num, uint64_t* offsets, const uint32_t* nbytes, int32_t* status,
                      double* total_weight, uint8_t* text) {
  uint64_t dst = 0;
  for (uint32_t i = 0; i < num; ++i) {
    const uint64_t a = offsets[i], cap = offsets[i + 1] - a;
    offsets[i] = dst;
    if (status[i] == kPathOk && nbytes[i] == kTextNotBytes) status[i] = kPathUnsupported;
    if (status[i] == kPathOk && nbytes[i] > cap) status[i] = kPathInternal;
    if (status[i] != kPathOk) {
      total_weight[i] = w_zero();
      continue;
    }
    const uint64_t nb = nbytes[i];
    if (dst != a && nb) std::memmove(text + dst, text + a, nb);
    dst += nb;
  }
  offsets[num] = dst;
  return dst;
}

// The streamed host batch over `devices` (one shard per device, or `nsh` shards round
// robin: FST_BATCH_DEVICES): the result is allocated once, every shard streams into its own
// slice of it (fixed slots: no compaction between shards, no gather), then strings without
// a path are compacted out on the host.  Shards are contiguous string ranges of equal
// estimated cost (FrozenFst::chain_cost), as in run_sharded.
// `io`: the mode (StreamIo) with the caller's labels or bytes (indexed by `offsets`) and its
// result.  Text mode: the text result is allocated with one byte per input byte (the slots),
// the shards emit into it, and text_compact closes the short slots up.
int run_streamed(const std::vector<int>& devices, uint32_t nsh, FrozenFst& b, StreamIo io,
                 const uint64_t* offsets, uint32_t num, uint32_t n, int semantics) {
  const bool tm = io.text_mode();
  FstBatchResult* const out = io.out;  // (label mode)
  DeviceRestore_ restore;
  std::vector<DeviceFst*> Ds(devices.size(), nullptr);
  for (size_t d = 0; d < devices.size(); ++d) {  // (the rhs goes to every device first)
    if (hipSetDevice(devices[d]) != hipSuccess) return FST_INVALID_ARG;
    Ds[d] = b.device(devices[d]);
    if (!Ds[d]) return FST_OOM;
    if (Ds[d]->has_eps || !DeviceEngine::pull_first(*Ds[d], semantics))
      return kStreamNotApplicable;
  }
  // before the result exists: a call with more parts than the route takes, or whose stream
  // kit or events cannot be created, goes the pipelined way instead of failing
  {
    const size_t max_parts = std::max(stream_cuts(false).size(), stream_cuts(true).size()) + 1;
    if (max_parts > kStreamMaxParts) return kStreamNotApplicable;
    for (int dev : devices) {
      KitLease K(dev);
      if (!K || !K->events(2 * max_parts)) return kStreamNotApplicable;
    }
  }
  const uint64_t base0 = offsets[0], total = offsets[num] - base0;
  if (tm) {
    FstTextResult* const t = io.tout;
    if (!alloc_text_result(t, num, total)) return FST_OOM;
    if (!pin_is_pinned(t->status) || !pin_is_pinned(t->text_offsets) ||
        !pin_is_pinned(t->total_weight) || !pin_is_pinned(t->text)) {
      fst_text_result_free(t);
      return kStreamNotApplicable;
    }
  } else {
    if (!alloc_result(out, num, total)) return FST_OOM;
    if (!pin_is_pinned(out->ilabels) || !pin_is_pinned(out->olabels) ||
        !pin_is_pinned(out->weights) || !pin_is_pinned(out->path_offsets) ||
        !pin_is_pinned(out->status) || !pin_is_pinned(out->final_weights)) {
      fst_batch_result_free(out);
      return kStreamNotApplicable;
    }
  }
  if (io.labels) io.labels += base0;
  if (io.text) io.text += base0;
  PinnedVec<uint32_t> nbytes(tm ? std::max<uint32_t>(num, 1) : 0);
  io.nbytes = tm ? nbytes.data() : nullptr;

  // ---- the result's CSR offsets (= the rebased input offsets) and max_len; text mode: the
  // text slots, which text_compact turns into the CSR offsets in the end ----
  uint64_t* const poff = tm ? io.tout->text_offsets : out->path_offsets;
  uint32_t max_len = 0;
  {
    const uint32_t nt = num >= (1u << 18) ? 4 : 1;
    std::vector<uint32_t> mx(nt, 0);
    auto rebase = [&](uint32_t t) {
      uint32_t m = 0;
      for (uint64_t i = (uint64_t)num * t / nt, e = (uint64_t)num * (t + 1) / nt; i < e; ++i) {
        poff[i] = offsets[i] - base0;
        m = std::max<uint32_t>(m, (uint32_t)(offsets[i + 1] - offsets[i]));
      }
      mx[t] = m;
    };
    std::vector<std::thread> R;
    for (uint32_t t = 1; t < nt; ++t) R.emplace_back(rebase, t);
    rebase(0);
    for (auto& t : R) t.join();
    for (uint32_t m : mx) max_len = std::max(max_len, m);
    poff[num] = total;
  }

  // ---- shards: contiguous string ranges of equal estimated cost ----
  nsh = std::max<uint32_t>(1, std::min<uint32_t>(nsh, num));
  std::vector<StreamShard> sh(nsh);
  const bool shard_log = std::getenv("FSTAMD_SHARD_LOG") != nullptr;
  std::vector<double> pre;  // cost of strings [0, i) (chain_cost per distinct length)
  if (nsh > 1 || shard_log) {
    std::vector<double> cl(max_len + 1, -1.0);
    pre.assign(num + 1, 0.0);
    for (uint32_t i = 0; i < num; ++i) {
      const uint32_t L = (uint32_t)(poff[i + 1] - poff[i]);
      if (cl[L] < 0) cl[L] = b.chain_cost(L);
      pre[i + 1] = pre[i] + cl[L];
    }
  }
  {
    std::vector<uint32_t> cuts{0};
    if (nsh > 1) {
      for (uint32_t j = 1; j < nsh; ++j) {
        const double goal = pre[num] * j / nsh;
        uint32_t i = (uint32_t)(std::lower_bound(pre.begin(), pre.end(), goal) - pre.begin());
        i = std::max(i, cuts.back() + 1);          // never empty
        i = std::min(i, num - (nsh - j));           // at least one string for each later one
        cuts.push_back(i);
      }
    }
    cuts.push_back(num);
    for (uint32_t j = 0; j < nsh; ++j) {
      sh[j].dev = devices[j % devices.size()];
      sh[j].s0 = cuts[j];
      sh[j].s1 = cuts[j + 1];
    }
  }
  if (shard_log)  // tests: the shard plan and the route
    for (uint32_t j = 0; j < nsh; ++j)
      std::fprintf(stderr, "[libfst_amd shard] %u dev %d strings %u..%u cost %.6g route %s\n", j,
                   sh[j].dev, sh[j].s0, sh[j].s1, pre[sh[j].s1] - pre[sh[j].s0],
                   tm ? "streamed-text" : "streamed");

  PinnedVec<int32_t> first(std::max<uint32_t>(num, 1));
  std::vector<std::mutex> later_mu(devices.size());  // (stream_shard: per device)
  if (t_prof) t_prof->lap(0);
  const auto tk0 = std::chrono::steady_clock::now();
  {
    auto run = [&](uint32_t j) {
      StreamShard& S = sh[j];
      const size_t d = (size_t)(j % devices.size());
      S.err = stream_shard(S, *Ds[d], io, poff, max_len, n, semantics, first.data(),
                           &later_mu[d]);
    };
    std::vector<std::thread> th;
    for (uint32_t j = 1; j < nsh; ++j) th.emplace_back(run, j);
    run(0);
    for (auto& t : th) t.join();
  }
  LaunchStats agg{};  // (the parts overlap on two streams: their wall time, not a sum)
  agg.engine = semantics == 1 ? 0 : 7;
  for (const StreamShard& S : sh) {
    if (S.err != FST_OK) return S.err;
    agg.launches += S.launches;
  }
  agg.kernel_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0).count();
  t_last_stats = agg;
  if (t_prof) t_prof->lap(2);

  if (tm) {  // ---- short text slots closed up (in order, moving left) ----
    FstTextResult* const t = io.tout;
    t->total_bytes = text_compact(num, poff, io.nbytes, t->status, t->total_weight, t->text);
  } else {  // ---- strings without a path: their slots dropped (in order, moving left) ----
    uint64_t nbad = 0;
    for (uint32_t i = 0; i < num; ++i) nbad += out->status[i] != kPathOk;
    if (nbad) {
      uint64_t dst = 0;
      for (uint32_t i = 0; i < num; ++i) {
        const uint64_t a = poff[i], L = poff[i + 1] - a;
        poff[i] = dst;
        if (out->status[i] != kPathOk) continue;
        if (dst != a) {
          std::memmove(out->ilabels + dst, out->ilabels + a, L * 4);
          std::memmove(out->olabels + dst, out->olabels + a, L * 4);
          std::memmove(out->weights + dst, out->weights + a, L * 8);
        }
        dst += L;
      }
      poff[num] = dst;
    }
    out->total_arcs = poff[num];
  }
  if (t_prof) {
    t_prof->runs = (int)agg.launches;
    t_prof->lap(3);
  }
  return FST_OK;
}

}  // namespace fstamd::host

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
#include <atomic>
#include <map>

#include "host_rt.hpp"
#include "weight_codes.hpp"

namespace fstamd::host {
namespace {

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

// One run of stream_shard: what the shard owns, and the phases stream_shard calls in order.
//
// The order of the owning members below is the lifetime contract.  Members go in reverse, so
// every return of every phase
//   1. aborts the expanders' gate and joins them (a recorded part is still expanded),
//   2. joins the uploader and the ilabel copiers (the second engine's driver never outlives
//      drive_parts),
//   3. drains `up`, `sA` and `sB`: no kernel or copy still uses the buffers or the result,
//   4. releases txs, the text-mode buffers, the code arena and the device buffers,
//   5. the engine leases,
//   6. the part cuts, the pinned staging block and the shard's own offsets,
//   7. the stream kit,
//   8. and last the per-device later_mu lock: the later tiers of the shards of one device run
//      one shard at a time, each to the end of its leases (the heavy replays size their
//      workspaces from the free HBM, which a concurrent shard's would have taken).
// A new owner goes where its users come after it and what it uses comes before it.
struct ShardRun {
  // ---- the call ----
  StreamShard& S;
  DeviceFst& D;
  const StreamIo& io;
  const StreamKnobs& knobs;
  const uint64_t* const poff;
  const uint32_t max_len, n;
  const int semantics;
  const bool tm = io.text_mode();
  FstBatchResult* const out = io.out;  // (label mode)
  const int dev = S.dev;
  const uint32_t num = S.s1 - S.s0;
  const uint64_t lbase = poff[S.s0], total = poff[S.s1] - lbase;
  const uint32_t* const lsrc = io.labels ? io.labels + lbase : nullptr;
  const uint8_t* const tsrc = io.text ? io.text + lbase : nullptr;
  uint32_t* const il_out = tm ? nullptr : out->ilabels + lbase;
  int32_t* const st_out = (tm ? io.tout->status : out->status) + S.s0;
  // (text mode: the total weights in the final weights' place)
  double* const fin_out = (tm ? io.tout->total_weight : out->final_weights) + S.s0;
  int32_t* const first;  // the pull tier's statuses
  // ---- the plan ----
  const uint64_t* loff = poff + S.s0;  // the shard's offsets from its first label
  double code_table[256];
  int codes_mode = 0;
  size_t parts = 0, ncoded = 0;  // parts [0, ncoded) leave codes
  hipStream_t up = nullptr, sA = nullptr, sB = nullptr;
  BatchOutDev vb{};
  uint32_t launches = 0;
  std::chrono::steady_clock::time_point tk0, tx0;  // the parts' and the expanders' start
  // ---- the owners, in the order of the contract ----
  std::unique_lock<std::mutex> later_lock;
  KitLease K;
  PinnedVec<uint64_t> loff_own;  // (shard 0 of the batch reads poff itself)
  PinBlock staging;              // the shard's codes, indexed like its labels
  std::vector<uint32_t> cut;
  DeviceEngine::Lease EA, EB;
  // (text mode: d_lab holds the bytes themselves; d_ctr: an item counter per part)
  std::unique_ptr<DevBuf> d_lab, d_off, d_first, d_ctr;
  std::unique_ptr<DevOut> o;
  std::unique_ptr<DevBuf> d_codes;  // the device byte arena of the codes (indexed like the path arena)
  // text mode: byte counts and total weights per string, and one TextOutDev per part (the
  // kernels reach it through BatchOutDev::text), uploaded with the offsets
  // (d_lab4: the widened labels of a shard that hands strings on, allocated only then)
  std::unique_ptr<DevBuf> d_nb, d_tw, d_tx, d_lab4;
  std::vector<TextOutDev> txs;
  StreamDrain drain{{nullptr, nullptr, nullptr}};
  PartGate uploaded;
  ThreadGroup uploads;
  RecordedGate recorded;
  std::atomic<bool> x_failed{false};
  std::vector<double> x_ev, x_end;  // [thread * ncoded + part] (FSTAMD_HOST_PROF)
  std::vector<FstError> perr;
  ThreadGroup expanders{&recorded};

  ShardRun(StreamShard& S_, DeviceFst& D_, const StreamIo& io_, const StreamKnobs& knobs_,
           const uint64_t* poff_, uint32_t max_len_, uint32_t n_, int semantics_,
           int32_t* first_all, std::mutex* later_mu)
      : S(S_), D(D_), io(io_), knobs(knobs_), poff(poff_), max_len(max_len_), n(n_),
        semantics(semantics_), first(first_all + S_.s0), later_lock(*later_mu, std::defer_lock),
        K(S_.dev) {}

  double x_ms() const {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tx0).count();
  }

  // Phase 1.  Decides the weight-code mode and the parts; owns the staging block afterwards.
  //
  // Parts: string ranges cut at fractions of the labels (stream_part_cuts, StreamKnobs::cuts).
  // FSTAMD_STREAM_CUTS overrides (A/B, one box, f64 copy-out: "23,163" 30.9 ms per 1M metric
  // strings, "167" 31.2, "100,400" 31.0, "125" 31.5).
  // Weight codes: when this rhs, these semantics and this max_len take tier
  // P's code instances (pull_codes_table: pull_rk / pull_pack decide) the coded parts' weights
  // cross the link as one byte per arc into a pinned staging block, and expander threads turn
  // each part's codes into the result's f64 weights once that part's completion event has
  // passed, while the later parts run.  The last part's expansion stands exposed after the
  // last kernel, so the coded route ends on shrinking parts.
  FstError plan() {
    if (!K) return FST_OOM;
    up = K->up;
    if (lbase) {
      loff_own.resize(num + 1);
      for (uint32_t i = 0; i <= num; ++i) loff_own[i] = poff[S.s0 + i] - lbase;
      loff = loff_own.data();
    }
    codes_mode = tm ? 0 : knobs.codes_mode;
    if (codes_mode && !pull_codes_table(D, semantics, max_len, code_table)) codes_mode = 0;
    if (codes_mode) {
      staging.reset(pin_alloc(std::max<uint64_t>(total, 1)));  // (the copy-out stays inside each string)
      if (!staging.p || !pin_is_pinned(staging.p)) {  // (the pool gave pageable memory)
        staging.reset(nullptr);
        codes_mode = 0;
      }
    }
    cut = stream_part_cuts(loff, num, knobs.cuts(codes_mode == 1));
    parts = cut.size() - 1;
    // one upload event and one completion event a part (run_streamed has checked that this
    // device's kit and events exist before it allocated the result)
    if (parts > kStreamMaxParts || !K->events(2 * parts)) return FST_OOM;
    // mode 2: the last part keeps the f64 copy-out
    ncoded = codes_mode == 1 ? parts : codes_mode == 2 ? parts - 1 : 0;
    if (knobs.route_log)
      std::fprintf(stderr, "[libfst_amd route] stream: weight codes %s, mode %d, parts %zu\n",
                   ncoded ? "on" : "off", ncoded ? codes_mode : 0, parts);
    return FST_OK;
  }

  // Phase 2.  Leases the engines and allocates the device buffers; from here every return
  // drains the three streams.
  FstError acquire() {
    EA = DeviceEngine::acquire(dev);
    if (!EA) return FST_INVALID_ARG;
    if (parts > 1) EB = DeviceEngine::try_acquire(dev);  // (none free: one engine in order)
    sA = EA.stream();
    sB = EB ? EB.stream() : nullptr;
    d_lab = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1) * (tm ? 1 : 4));
    d_off = std::make_unique<DevBuf>((num + 1) * 8ull);
    d_first = std::make_unique<DevBuf>(std::max<size_t>(num, 1) * 4ull);
    d_ctr = std::make_unique<DevBuf>(64 * 4);
    o = std::make_unique<DevOut>(num, total + 4);
    if (!d_lab->p || !d_off->p || !d_first->p || !d_ctr->p || !o->ok()) return FST_OOM;
    if (ncoded) {
      d_codes = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1));
      if (!d_codes->p) return FST_OOM;
    }
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
    vb = o->v;
    vb.out_il += lbase & 3u;
    vb.out_ol += lbase & 3u;
    vb.out_w += lbase & 1u;
    drain.s[0] = up, drain.s[1] = sA, drain.s[2] = sB;
    return FST_OK;
  }

  // Phase 3.  Starts the uploader (offsets, then each part's labels: one event per part) and
  // the threads that copy the labels into the result's ilabels.
  // Two ways to move the labels (FSTAMD_STREAM_STAGE): 0 = the runtime stages the pageable
  // source itself while other threads copy it into the result's ilabels (the labels cross
  // host DRAM twice); 1 = threads copy each chunk into the result's (pinned) ilabels and
  // the chunk's DMA reads it from there (once).
  void start_uploads() {
    uploads.add([this] { upload(); });
    if (!tm && knobs.stage != 1) {
      // the result's ilabels, once the uploads are staged: the runtime's staging copies of
      // a pageable source read the same pages, and the kernels wait for them, not for these
      const uint64_t T = total >= (1u << 20) ? 3 : 1;
      for (uint64_t t = 0; t < T; ++t)
        uploads.add([this, t, T] {
          uploaded.wait_all(parts);
          const uint64_t a = total * t / T, z = total * (t + 1) / T;
          if (z > a) std::memcpy(il_out + a, lsrc + a, (z - a) * 4);
        });
    }
  }
  void upload() {
    // (the fills first, on the idle GPU: every string INTERNAL until a tier finishes it,
    // the parts' item counters zero; the parts wait on events recorded after them)
    bool ok = hipSetDevice(dev) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)o->status.p, kPathInternal, num, up) == hipSuccess &&
              hipMemsetD32Async((hipDeviceptr_t)d_first->p, kPathInternal, num, up) == hipSuccess &&
              hipMemsetAsync(d_ctr->p, 0, 64 * 4, up) == hipSuccess &&
              hipMemcpyAsync(d_off->p, loff, (num + 1) * 8ull, hipMemcpyHostToDevice, up) ==
                  hipSuccess &&
              (!tm || hipMemcpyAsync(d_tx->p, txs.data(), parts * sizeof(TextOutDev),
                                     hipMemcpyHostToDevice, up) == hipSuccess);
    constexpr uint64_t kChunk = 1ull << 21;  // labels per staged chunk (8 MB)
    for (size_t p = 0; p < parts && ok; ++p) {
      const uint64_t a = loff[cut[p]], z = loff[cut[p + 1]];
      if (tm) {  // the part's bytes, as they are
        ok = z == a || hipMemcpyAsync((uint8_t*)d_lab->p + a, tsrc + a, z - a,
                                      hipMemcpyHostToDevice, up) == hipSuccess;
      } else if (knobs.stage == 1) {
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
          ok = hipMemcpyAsync((uint32_t*)d_lab->p + c, il_out + c, w * 4, hipMemcpyHostToDevice,
                              up) == hipSuccess;
        }
      } else {
        // (a pageable source is staged through pinned memory before this returns)
        ok = z == a || hipMemcpyAsync((uint32_t*)d_lab->p + a, lsrc + a, (z - a) * 4,
                                      hipMemcpyHostToDevice, up) == hipSuccess;
      }
      ok = ok && hipEventRecord(K->ev[p], up) == hipSuccess;
      if (ok) uploaded.publish(p + 1);
    }
    if (!ok) uploaded.fail();
  }

  // Phase 4.  Starts the expanders: thread t of T takes the t-th slice of every coded part,
  // in part order.  It waits (host side) until the part's completion event has been recorded,
  // then for the event itself, and only then reads the part's codes.  Nothing polls memory
  // the device writes.
  void start_expanders() {
    recorded.reset(parts);
    tx0 = std::chrono::steady_clock::now();
    if (!ncoded) return;
    const uint32_t T = knobs.expanders;
    x_ev.assign(T * ncoded, 0.0);
    x_end.assign(T * ncoded, 0.0);
    for (uint32_t t = 0; t < T; ++t) expanders.add([this, t, T] { expand(t, T); });
  }
  void expand(uint32_t t, uint32_t T) {
    const uint8_t* const codes = (const uint8_t*)staging.p;
    double* const w_out = out->weights + lbase;
    if (hipSetDevice(dev) != hipSuccess) {
      x_failed = true;
      return;
    }
    for (size_t p = 0; p < ncoded; ++p) {
      if (!recorded.wait(p)) return;
      if (hipEventSynchronize(K->ev[parts + p]) != hipSuccess) {
        x_failed = true;
        return;
      }
      // (FSTAMD_HOST_PROF: when each part's event passed and when its expansion ended, ms
      // from the expanders' start, per thread)
      if (knobs.host_prof) x_ev[t * ncoded + p] = x_ms();
      const auto [lo, hi] = expander_slice(loff[cut[p]], loff[cut[p + 1]], t, T);
      if (hi > lo) expand_weight_codes(codes + lo, hi - lo, code_table, w_out + lo);
      if (knobs.host_prof) x_end[t * ncoded + p] = x_ms();
    }
  }

  // Phase 5.  Launches the parts: engine A takes parts 0, 2, .., engine B 1, 3, .. on a
  // thread of its own (A all without B).  Errors land in perr.
  void drive_parts() {
    perr.assign(parts, FST_OK);
    tk0 = std::chrono::steady_clock::now();
    ThreadGroup second;
    if (EB) second.add([this] { drive(EB, sB, 1, 2); });
    drive(EA, sA, 0, EB ? 2 : 1);
  }
  void drive(DeviceEngine::Lease& E, hipStream_t s, size_t p0, size_t step) {
    auto fail = [&](size_t p, FstError e) {
      perr[p] = e;
      recorded.abort();
    };
    if (hipSetDevice(dev) != hipSuccess) return fail(p0, FST_INVALID_ARG);
    for (size_t p = p0; p < parts; p += step) {
      if (!uploaded.wait_for(p)) return fail(p, FST_OOM);
      const uint32_t s0 = cut[p], np = cut[p + 1] - cut[p];
      ChainInput in{(const uint32_t*)d_lab->p, (const uint64_t*)d_off->p + s0, np, max_len};
      if (tm) in.text = (const uint8_t*)d_lab->p;  // (the bytes, in the labels' place)
      BatchOutDev v = vb;
      v.status += s0;
      v.path_len += s0;
      v.path_off += s0;
      v.final_w += s0;
      v.slots = (const uint64_t*)d_off->p + s0;
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
      if (knobs.ab_nocopy && !tm && !coded) v.host_ol = nullptr, v.host_w = nullptr;
      v.first_status = (int32_t*)d_first->p + s0;
      // the pull tier alone: no fill, copy or host synchronisation between parts (a fill
      // or copy is a blit kernel that waits for CU slots behind the other engine's
      // persistent kernel, and had held this engine's next part back); the later tiers
      // and the downloads come after the last part
      if (hipStreamWaitEvent(s, K->ev[p], 0) != hipSuccess ||
          E->launch_pull_part(D, in, n, semantics, v, s, (unsigned int*)d_ctr->p + p, tm, coded) !=
              hipSuccess ||
          (coded && hipEventRecord(K->ev[parts + p], s) != hipSuccess))
        return fail(p, FST_OOM);
      // the part's completion event is in the stream: its expanders may wait
      if (coded) recorded.mark(p);
    }
  }

  // Statuses, final weights (text mode: total weights and byte counts) and, with_first, the
  // pull tier's statuses, in one download each on sA, waited for.
  bool download(bool with_first) {
    return d2h(st_out, o->status.p, num * 4ull, sA) &&
           d2h(fin_out, tm ? d_tw->p : o->fin.p, num * 8ull, sA) &&
           (!tm || d2h(io.nbytes + S.s0, d_nb->p, num * 4ull, sA)) &&
           (!with_first || d2h(first, d_first->p, num * 4ull, sA)) &&
           hipStreamSynchronize(sA) == hipSuccess;
  }

  // Phase 6.  Waits for the uploads and the parts, reports a part's error, brings the
  // statuses down.  (An error return here may leave expanders in flight.)
  FstError sync_and_download() {
    for (hipStream_t x : {up, sA, sB})
      if (x && hipStreamSynchronize(x) != hipSuccess) return FST_OOM;
    for (size_t p = 0; p < parts; ++p)
      if (perr[p] != FST_OK) return perr[p];
    if (!download(true) || fault_inject("stream_after_pull")) return FST_OOM;
    return FST_OK;
  }

  // Phase 7.  Joins the expanders, before anything else writes the result's weights: what the
  // later tiers finish is downloaded over whatever the expanders made of those strings'
  // unwritten codes.
  FstError join_expanders() {
    expanders.join();
    if (x_failed) return FST_OOM;
    if (knobs.host_prof && ncoded) {
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
    return FST_OK;
  }

  // Phase 8.  The later tiers, once, over the strings the pull tier handed on (in the device
  // arena, the same slots) -- only when it handed some on (the metric: none), then the
  // statuses and final weights again.  Takes later_mu and keeps it to the end of the run.
  FstError later_tiers() {
    auto handed_on = [&](uint32_t i) { return first[i] != kPathOk && first[i] != kPathEmpty; };
    bool handed = false;
    for (uint32_t i = 0; i < num && !handed; ++i) handed = handed_on(i);
    launches = (uint32_t)parts;
    if (tm && knobs.shard_log) {  // tests (text mode): what the pull tier handed on
      uint32_t nh = 0;
      for (uint32_t i = 0; i < num; ++i) nh += handed_on(i);
      std::fprintf(stderr, "[libfst_amd stream] dev %d strings %u..%u parts %zu handed-on %u\n", dev,
                   S.s0, S.s1, parts, nh);
    }
    if (!handed) return FST_OK;
    later_lock.lock();
    ChainInput in{(const uint32_t*)d_lab->p, (const uint64_t*)d_off->p, num, max_len};
    // text mode: the later tiers read 4-B labels -- the shard's bytes widened once, now
    // (only batches that hand strings on pay for the buffer and the kernel)
    if (tm) {
      d_lab4 = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1) * 4);
      if (!d_lab4->p ||
          EA->widen_text((const uint8_t*)d_lab->p, (const uint64_t*)d_off->p, num,
                         (uint32_t*)d_lab4->p, sA) != hipSuccess)
        return FST_OOM;
      in.labels = (const uint32_t*)d_lab4->p;
    }
    BatchOutDev v = vb;
    v.slots = (const uint64_t*)d_off->p;
    EA->set_after_pull(true);
    hipError_t e = EA->run_chain(D, in, n, semantics, v, sA, nullptr);
    EA->set_after_pull(false);
    // text mode: the paths the later tiers left in the arena's slots, emitted as the pull
    // tier's are (the same slots of the result)
    if (tm && e == hipSuccess)
      e = EA->text_fixup(v, TextOutDev{io.tout->text + lbase, (uint32_t*)d_nb->p,
                                       (double*)d_tw->p},
                         (const int32_t*)d_first->p, num, sA);
    if (e != hipSuccess || !download(false)) return FST_OOM;
    ++launches;
    return FST_OK;
  }

  // Phase 9.  Brings down the paths the later tiers wrote (device arena, same slots): one by
  // one when few, else the whole arena.
  FstError download_fixups() {
    auto fixed = [&](uint32_t i) { return st_out[i] == kPathOk && first[i] != kPathOk; };
    uint64_t nfix = 0;
    if (!tm)
      for (uint32_t i = 0; i < num; ++i) nfix += fixed(i);
    if (!nfix) return FST_OK;
    bool ok = true;
    const uint64_t few = knobs.fix_few;  // (tests: 0 = bulk copy)
    if (nfix <= few) {
      for (uint32_t i = 0; i < num && ok; ++i)
        if (fixed(i)) {
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
    return FST_OK;
  }

  // Phase 10.  Joins the uploader and the copiers: the result's ilabels are complete.
  void finish() {
    uploads.join();
    S.launches = launches;
    S.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk0)
                    .count();
  }
};

FstError stream_shard(StreamShard& S, DeviceFst& D, const StreamIo& io, const StreamKnobs& knobs,
                      const uint64_t* poff, uint32_t max_len, uint32_t n, int semantics,
                      int32_t* first_all, std::mutex* later_mu) {
  if (hipSetDevice(S.dev) != hipSuccess) return FST_INVALID_ARG;
  if (S.s1 == S.s0) return FST_OK;
  ShardRun R(S, D, io, knobs, poff, max_len, n, semantics, first_all, later_mu);
  FstError e = R.plan();
  if (e == FST_OK) e = R.acquire();
  if (e != FST_OK) return e;
  R.start_uploads();
  R.start_expanders();
  R.drive_parts();
  e = R.sync_and_download();
  if (e == FST_OK) e = R.join_expanders();
  if (e == FST_OK) e = R.later_tiers();
  if (e == FST_OK) e = R.download_fixups();
  if (e == FST_OK) R.finish();
  return e;
}

// every array of a result came pinned from the pool (or the caller takes another route)
template <class... P>
bool all_pinned(const P*... p) {
  return (pin_is_pinned(p) && ...);
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
  const StreamKnobs knobs = StreamKnobs::from_env();
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
    const size_t max_parts = std::max(knobs.cuts(false).size(), knobs.cuts(true).size()) + 1;
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
    if (!all_pinned(t->status, t->text_offsets, t->total_weight, t->text)) {
      fst_text_result_free(t);
      return kStreamNotApplicable;
    }
  } else {
    if (!alloc_result(out, num, total)) return FST_OOM;
    if (!all_pinned(out->ilabels, out->olabels, out->weights, out->path_offsets, out->status,
                    out->final_weights)) {
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
  const bool shard_log = knobs.shard_log;
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
    const std::vector<uint32_t> cuts = stream_shard_cuts(pre, num, nsh);
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
  std::vector<std::mutex> later_mu(devices.size());  // (ShardRun::later_tiers: per device)
  if (t_prof) t_prof->lap(0);
  const auto tk0 = std::chrono::steady_clock::now();
  {
    auto run = [&](uint32_t j) {
      StreamShard& S = sh[j];
      const size_t d = (size_t)(j % devices.size());
      S.err = stream_shard(S, *Ds[d], io, knobs, poff, max_len, n, semantics, first.data(),
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
    out->total_arcs =
        paths_compact(num, poff, out->status, out->ilabels, out->olabels, out->weights);
  }
  if (t_prof) {
    t_prof->runs = (int)agg.launches;
    t_prof->lap(3);
  }
  return FST_OK;
}

}  // namespace fstamd::host

// host_rt.hpp -- what the host units of the C ABI share (internal, not installed): the
// pooled buffers, the per-call profile, the shard types and the batch routes' signatures.
// c_api.cpp holds the handle tables and the single calls, host_rt.cpp the pools and small
// helpers, batch_sharded.cpp (chains through the path arena), batch_lhs.cpp (general lhs and the
// lattice batch) and batch_streamed.cpp the routes, batch_entries.cpp fst_batch.h.
// stream_plan.hpp (included here, no HIP in it) holds what those routes decide and hand over on
// the host alone: the streamed batch's knobs (StreamKnobs), its part and shard cuts, the label
// route's compaction, and the gates and thread groups (PartGate, RecordedGate, ThreadGroup)
// of run_pipelined's uploader and of batch_streamed.cpp's ShardRun.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <vector>

#include "../../include/fst_batch.h"
#include "device_engine.hpp"
#include "host_fst.hpp"
#include "stream_plan.hpp"

#pragma GCC visibility push(hidden)  // internal: nothing here joins the library's exports
namespace fstamd::host {

constexpr uint64_t kInvalid = UINT64_MAX;

// ---- c_api.cpp: the handle tables, as the batch entries use them ----
std::shared_ptr<FrozenFst> frozen_get(uint64_t h);     // pinned (a shared_ptr copy), or null
uint64_t frozen_insert(std::shared_ptr<FrozenFst> f);  // the new handle, or kInvalid
struct MutableRead {  // a mutable FST (null: a stale handle) and the shared lock it is read under
  std::shared_lock<std::shared_mutex> lock;
  const MutableFst* fst;
};
MutableRead mutable_read(uint64_t h);
bool gpu_available();

// ---- host_rt.cpp ----
int current_device();  // -1 without one
// Tests only: FSTAMD_FAULT_INJECT=<site> makes the named error branch fire after its work
// is in flight on the GPU (tests/test_gpu_error_paths.py: the buffers a failing call hands
// back to the pools must not still be in use by its copies or kernels).
bool fault_inject(const char* site);
// The whole file at `path` if it has at most max_bytes (the text loaders' limits).
bool read_file(const char* path, long max_bytes, std::vector<char>* data);

// Frees the cached device blocks of `dev` (every device when dev < 0); the calling thread's
// current device is restored.
void pool_release(int dev);
void* pin_alloc(size_t n);  // the pinned host pool (result arrays, staging blocks)
void pin_release(void* p);
bool pin_is_pinned(const void* p);  // a pooled block from hipHostMalloc (device-mapped)
void pin_pool_clear();

// RAII device buffer (pooled)
struct DevBuf {
  void* p = nullptr;
  size_t cls = 0;
  int dev = 0;
  explicit DevBuf(size_t n);
  ~DevBuf();
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

struct HostPaths {  // pinned: each array is one DMA (single calls download all of them)
  PinnedVec<int32_t> status;
  PinnedVec<uint32_t> len;
  PinnedVec<uint64_t> off;
  PinnedVec<double> fin;
  PinnedVec<uint32_t> il, ol;
  PinnedVec<double> w;
};

// Device outputs for `num` strings with `arc_cap` arena slots.
struct DevOut {
  DevBuf status, len, off, fin, il, ol, w, cursor;
  BatchOutDev v{};
  DevOut(uint32_t num, uint64_t arc_cap);
  bool ok() const {
    return status.p && len.p && off.p && fin.p && il.p && ol.p && w.p && cursor.p;
  }
  bool download(uint32_t num, HostPaths* h, hipStream_t stream) const;
};

// An asynchronous device-to-host copy on `stream` (nothing to do for 0 bytes); true = queued.
bool d2h(void* dst, const void* src, size_t bytes, hipStream_t stream);
// Eight bytes of device memory (an arena cursor, a last offset), read and waited for.
bool read_u64(void* dst, const void* dev_src, hipStream_t stream);

// Waits for up to three streams when it goes out of scope, unless `done` was set: what is
// declared before it (pooled buffers, pinned staging, a result the caller frees on error)
// outlives the copies and kernels queued on them.
struct StreamDrain {
  hipStream_t s[3];
  bool done = false;
  ~StreamDrain() {
    if (!done)
      for (hipStream_t x : s)
        if (x) (void)hipStreamSynchronize(x);
  }
};

// Gives the calling thread its current HIP device back when it goes out of scope.
struct DeviceRestore_ {
  int dev = -1;
  DeviceRestore_() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceRestore_() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};

// FSTAMD_HOST_PROF=1: wall time per host phase of the batch calls, printed to stderr at
// the end of each call (where a host API call spends its time beside the kernels).
struct HostProf {
  bool on = std::getenv("FSTAMD_HOST_PROF") != nullptr;
  double ms[8] = {};  // inputs H2D, output alloc, engine + sync, download, project, result
  int runs = 0;       // engine runs (a full arena reruns the batch with 4x the arcs)
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(int i) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    ms[i] += std::chrono::duration<double, std::milli>(n - t).count();
    t = n;
  }
  void print(const char* what) const {
    if (!on) return;
    std::fprintf(stderr,
                 "[libfst_amd host] %s: inputs %.2f alloc %.2f engine %.2f download %.2f "
                 "project %.2f result %.2f ms (engine: %d launch(es))\n",
                 what, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], runs);
  }
};
// (declared constant-initialised: the units read them directly, with no call to a TLS
// initialisation wrapper, which a hidden symbol in a shared library could not resolve)
[[clang::require_constant_initialization]] extern thread_local HostProf* t_prof;  // or null
[[clang::require_constant_initialization]] extern thread_local LaunchStats t_last_stats;

// ---- Host batches in shards (one device, or several: FST_BATCH_DEVICES) ---------------
// A shard is strings [s0, s1) of the caller's arrays on one device: computed on an engine
// lease (its device outputs kept), compacted to CSR on the device (count, scan, gather:
// DeviceEngine::compact_paths), then downloaded straight into the caller's result at the
// shard's string and arc offsets.
// A lattice shard (fst_compose_frozen_batch, fst_connect_lhs_batch; batch_lhs.cpp): the arena
// the emitting kernels filled, the trim's workspace, and -- after the sink's compaction -- the
// shard in FstLhsBatch's layout on the device.
// Release order: shard_lattice_compact releases `trim` and `arena` once its gather has been
// waited for; `csr` lives until the shard's download has.  Each `v` is the kernels' view of the
// buffers beside it.  Whoever queues work on them declares its StreamDrain after the LatShard.
struct LatShard {
  struct Arena {
    std::unique_ptr<DevBuf> item, fin, aoff, il, ol, w, next, cursor;
    // fst_connect_lhs_batch: `v` points into the staged items (run_connect_shard), kept here
    std::shared_ptr<void> input;
    LatticeOutDev v{};
    // `num` items, the capacities multiples of 4; false: out of memory
    bool alloc(uint32_t num, uint64_t state_cap, uint64_t arc_cap);
    void release() { *this = Arena(); }
  } arena;
  // FST_LATTICE_CONNECT / fst_connect_lhs_batch: the trim's workspace (trim_lattices), alive
  // until the filtering gather has run
  struct Trim {
    std::unique_ptr<DevBuf> mark, queue, roff, rcur, rsrc, list, ctr, start;
    LatTrimDev v{};
    void release() { *this = Trim(); }
  } trim;
  bool connect = false;
  struct Csr {  // the compacted shard
    std::unique_ptr<DevBuf> status, soff, start, fin, aoffs, il, ol, w, next;
    // the arrays there are so far (the counting step has the per-item ones alone)
    LatticeCsrDev view(uint64_t state_cap, uint64_t arc_cap) const;
  } csr;
};

// The aligned text entry's carrier through the stages of a shard (null for every other entry):
// the running map of the last projected stage's output symbols into the string's own input --
// 8 B per symbol, (b, e) at `off` [num + 1], a copy of that projection's offsets -- and n1, what
// stage 1 consumed per string.  Empty (no `b`) until the first projection.
struct AlignMap {
  std::unique_ptr<DevBuf> off, b, e, n1;
};

struct Shard {
  int dev = 0;
  uint32_t s0 = 0, s1 = 0;
  // result strings per item: 1, or fst_nbest_lhs_batch's n (run_sharded's `per`); the label
  // gather then moves strings [s0 * per, s1 * per)
  uint32_t per = 1;
  DeviceEngine::Lease E;
  std::unique_ptr<DevOut> keep;
  std::unique_ptr<LatShard> lat;  // lattice entries (keep: the statuses)
  uint64_t tot2 = 0;              // lattice entries: tot = states, tot2 = arcs
  std::unique_ptr<DevBuf> fail;  // pipelines: the first failing stage per string
  std::unique_ptr<DevBuf> st, off, fin, il, ol, w;
  std::unique_ptr<DevBuf> text;  // text entries: the emitted bytes (fin: the total weights)
  uint64_t tot = 0;              // arcs of the compacted shard (text entries: bytes)
  // the aligned text entry: the carrier run_stages_after feeds, and the result's two maps
  // ([tot] each, per string) beside `text`
  std::unique_ptr<AlignMap> align;
  std::unique_ptr<DevBuf> in_begin, in_end;
  FstError err = FST_OK;
  LaunchStats stats;
};

// What becomes of a computed shard: `compact` (on the shard's lease, after the engines) brings
// its result into CSR order on the device and sets S.tot; `alloc` makes the host result once
// every shard's total is known; `download` copies a shard in at its string range and at the
// sum of the earlier shards' totals; `finish` closes the offsets.  Two totals each (S.tot,
// S.tot2): the lattice sink's states and arcs; the label and text sinks use the first alone.
struct ShardSink {
  std::function<FstError(Shard&)> compact;
  std::function<bool(uint64_t, uint64_t)> alloc;
  std::function<FstError(Shard&, uint64_t, uint64_t)> download;
  std::function<void(uint64_t, uint64_t)> finish;
};
using ShardCompute = std::function<FstError(Shard&)>;

// ---- batch_sharded.cpp: chains through the path arena ----
// One engine run into a path arena of `arc_cap` slots, rerun with a larger arena while a
// string is OUTPUT_FULL.  `launch` queues the engine on `stream`; `failed` names it in the
// error message.  With `keep` the device outputs stay alive and `h` receives only the
// statuses; without it `h` receives everything.  `fine_laps`: the chain route's profile
// also times the arena allocation and the download on their own.
using ArenaLaunch = std::function<hipError_t(const BatchOutDev&, LaunchStats*)>;
FstError run_arena(hipStream_t stream, uint32_t num, uint64_t arc_cap, const char* failed,
                   bool fine_laps, const ArenaLaunch& launch, HostPaths* h,
                   std::unique_ptr<DevOut>* keep);
// One batch on device inputs; the path arena grows on OUTPUT_FULL.  With `keep` the
// device outputs stay alive (pipelines) and `h` receives only the statuses.
FstError run_chain_batch_dev(DeviceEngine::Lease& E, DeviceFst& D, const ChainInput& in,
                             uint64_t total_labels, uint32_t n, int semantics, HostPaths* h,
                             std::unique_ptr<DevOut>* keep);
// A chain batch's strings on the device: the offsets rebased to the batch's first element, and
// its `elem`-byte elements (4: labels, 1: the text entry's bytes).  upload_chain queues the two
// copies on `stream`; the caller keeps *u until the stream has been waited for.
struct ChainUpload {
  std::vector<uint64_t> rebased;
  std::unique_ptr<DevBuf> data, off;
  uint64_t total = 0;
  uint32_t max_len = 0;
};
FstError upload_chain(const void* data, size_t elem, const uint64_t* offsets, uint32_t num,
                      hipStream_t stream, ChainUpload* u);
bool alloc_result(FstBatchResult* out, uint32_t num, uint64_t tot);
bool alloc_text_result(FstTextResult* out, uint32_t num, uint64_t tot);
bool alloc_aligned_text_result(FstAlignedTextResult* out, uint32_t num, uint64_t tot);
// Runs `compute` (the engines: it fills S.keep and, for pipelines, S.fail) over the shards
// of a batch and gathers their results through `sink`.  Shards are contiguous string ranges of
// equal estimated cost (cost[i]: the work estimate of string i); shard j runs on
// devices[j % devices.size()] on a host thread of its own (inline for one shard).
FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     const ShardSink& sink);
// ... into a label result: compact_paths on the device, then the arc arrays by DMA.  `per`:
// result strings per item (the result has num * per, Shard::per is set before `compute` runs).
FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstBatchResult* out, uint32_t per = 1);
// ... into a text result (fst_normalize_text_batch): text_count / text_write on the device.
FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstTextResult* out);
// ... into an aligned text result (fst_normalize_text_aligned_batch): the same, then the input
// span of every output byte (align_write / align_compose).  `compute` sets S.align.
FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstAlignedTextResult* out);
FstError run_pipelined(int dev, FrozenFst& b, const uint32_t* labels, const uint64_t* offsets,
                       uint32_t num, uint32_t n, int semantics, uint32_t parts,
                       FstBatchResult* out);
// The compute steps of a chain shard: a pipeline's stages from labels or from bytes.  `offsets`
// are the caller's, indexed from the shard's first string.
using Stages = std::vector<std::shared_ptr<FrozenFst>>;
FstError run_pipeline_shard(Shard& S, const Stages& fs, const uint32_t* labels,
                            const uint64_t* offsets, uint32_t n, int semantics);
FstError run_text_shard(Shard& S, const Stages& fs, const uint8_t* text, const uint64_t* offsets,
                        int semantics);
// S.fail of a shard whose first stage is about to run or has just finished: no failure yet.
FstError clear_stage_failures(Shard& S);
// The stages [first, fs.size()) of one shard, from a finished stage: S.keep holds stage
// first - 1's outputs (whatever entry produced them: a chain stage, a general-lhs batch) and
// S.fail the failures so far.  Each stage's 1-best output tape is projected into the next
// stage's chain inputs on the device.  With S.align (the aligned text entry) each finished
// stage's input spans are composed into the running map right after its projection.
FstError run_stages_after(Shard& S, const Stages& fs, size_t first, uint32_t n, int semantics,
                          HostPaths* h);

// ---- batch_lhs.cpp: general lhs, and the lattice batch with its own arena ----
// The compute steps of a shard of general lhs; `L` is the caller's batch, the shard its items
// [S.s0, S.s1), staged into one block and uploaded with one DMA (stage_lhs_items).
FstError run_lhs_shard(Shard& S, FrozenFst& b, const FstLhsBatch& L, uint32_t n, int semantics);
// ... and a pipeline on a general first stage: run_lhs_shard on fs[0], then the chain stages
// fs[1 ..] on its 1-best output tapes (S.fail: the first failing stage, when there are several).
FstError run_lhs_pipeline_shard(Shard& S, const Stages& fs, const FstLhsBatch& L, uint32_t n,
                                int semantics);
// fst_shortest_path_lhs_batch's shard: the items staged the same way, then fst_shortest_path of
// each (DeviceEngine::run_sp_batch) into a path arena of the shard's states; S.keep = the paths.
FstError run_sp_shard(Shard& S, const FstLhsBatch& L, uint32_t n);
// fst_nbest_lhs_batch's shard: the same staging, then DeviceEngine::run_nbest_batch into n
// strings per item and a path arena of n times the shard's states; S.keep = the paths.
// unique: fst_nbest_unique_lhs_batch's (one path per output text).
FstError run_nbest_shard(Shard& S, const FstLhsBatch& L, uint32_t n, bool unique);
// fst_posterior_lhs_batch's shard: the same staging, then DeviceEngine::run_posterior_batch;
// S.keep = the statuses and totals, S.w = alpha, beta and the arc costs, S.tot / S.tot2 = the
// shard's states / arcs.
FstError run_posterior_shard(Shard& S, const FstLhsBatch& L);
// fst_connect_lhs_batch's shard: the items staged the same way, then trimmed.
FstError run_connect_shard(Shard& S, const FstLhsBatch& L);
// fst_prune_lhs_batch's shard: the items staged the same way, then prune_lattices.
FstError run_prune_shard(Shard& S, const FstLhsBatch& L, double beam);
// The compute steps of a lattice shard: chains from the caller's labels, or general lhs staged
// as run_lhs_shard stages them; S.lat = the filled arena, S.keep = the statuses.
FstError run_lattice_chain_shard(Shard& S, FrozenFst& b, const uint32_t* labels,
                                 const uint64_t* offsets, uint32_t lattice_flags);
FstError run_lattice_lhs_shard(Shard& S, FrozenFst& b, const FstLhsBatch& L,
                               uint32_t lattice_flags);
// One engine run into a lattice arena (first size: the estimates, or FSTAMD_LATTICE_ARENA=
// states,arcs), rerun once the cursors say what the batch needs while an item is OUTPUT_FULL.
FstError run_lattice_arena(DeviceEngine::Lease& E, DeviceFst& D, const ChainInput& in,
                           const GraphInput* lhs, uint32_t lattice_flags, uint64_t est_states,
                           uint64_t est_arcs, std::unique_ptr<LatShard>* lat,
                           std::unique_ptr<DevOut>* keep);
// Connect of every OK item of L's arena (kernels/lattice_trim.hpp): the sweep tier, the linear
// tier for what it handed on, then the map and the trimmed counts in LatItem.  With
// L.trim.start (the stand-alone entry) the accessibility pass runs first.  Adds its launches
// and kernel time to t_last_stats; synchronises `stream`.
// totals (optional): states before / after, arcs before / after.
FstError trim_lattices(DeviceEngine::Lease& E, const int32_t* status, LatShard& L, uint32_t num,
                       hipStream_t stream, unsigned long long* totals = nullptr);
// The beam cut and connect of every item of `b` (a batch in device memory: staged, or prepared
// in place): DeviceEngine::run_prune_batch into a shadow arena (the batch's own arrays with the
// cut's finals and targets), then trim_lattices on it.  *lat = that arena, ready for
// compact_lattices with its trim; *keep = the statuses.  Sets t_last_stats (engine 15;
// prep_launches: the caller's preparation kernels); synchronises `stream`.
FstError prune_lattices(DeviceEngine::Lease& E, const LhsBatchDev& b, double beam,
                        uint32_t prep_launches, hipStream_t stream,
                        std::unique_ptr<LatShard>* lat, std::unique_ptr<DevOut>* keep);
// run_sharded into a lattice result (fst_compose_frozen_batch): compact_lattices on the device,
// both offset arrays rebased per shard.
FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstLatticeBatch* out);
bool alloc_lattice_result(FstLatticeBatch* out, uint32_t num, uint64_t states, uint64_t arcs);

// ---- c_api.cpp: a chain batch from host arrays on the engine `E` leases; fills `h` in input
// order (small batches in one block, see run_small_batch), or keeps the device outputs ----
FstError run_chain_batch_host(DeviceEngine::Lease& E, FrozenFst& b, const uint32_t* labels,
                              const uint64_t* offsets, uint32_t num, uint32_t n, int semantics,
                              HostPaths* h, std::unique_ptr<DevOut>* keep = nullptr);

// ---- batch_streamed.cpp ----
// What a streamed batch reads and writes.
//   label mode (fst_compose_frozen_shortest_path_batch): 4-B labels up; each finished path's
//     olabels and weights written into the result by the pull tier (copy_out_paths), the
//     ilabels staged by host threads.
//   text mode (fst_normalize_text_batch): the bytes up as they are -- the pull tiers read
//     them (ChainInput::text; no widen kernel and no 4-B label buffer on the way: a widen per
//     part would queue for CU slots behind the other engine's persistent kernel, as fills
//     and blits did) -- and each finished path's text written into its fixed text slot
//     [poff[i], poff[i + 1]) of the result by the chase epilogue (emit_text_paths): with no
//     input epsilon in the rhs a path has as many arcs as its string has bytes and every arc
//     emits at most one.  Per string 20 B come down (status, byte count, total weight, the
//     pull tier's status); no ilabel staging.  The slots are global byte offsets, so the
//     shards of a call write one result and a single host compaction (text_compact) follows.
struct StreamIo {
  const uint32_t* labels = nullptr;  // label mode: the batch's labels from its first one
  FstBatchResult* out = nullptr;
  const uint8_t* text = nullptr;     // text mode: the batch's bytes from its first one
  FstTextResult* tout = nullptr;
  uint32_t* nbytes = nullptr;        // text mode: [num] (pinned) bytes the device wrote
  bool text_mode() const { return tout != nullptr; }
};
// run_streamed's answer when the mode does not apply (the caller takes another route)
constexpr int kStreamNotApplicable = -1;
int run_streamed(const std::vector<int>& devices, uint32_t nsh, FrozenFst& b, StreamIo io,
                 const uint64_t* offsets, uint32_t num, uint32_t n, int semantics);
uint64_t text_compact(uint32_t num, uint64_t* offsets, const uint32_t* nbytes, int32_t* status,
                      double* total_weight, uint8_t* text);

}  // namespace fstamd::host
#pragma GCC visibility pop

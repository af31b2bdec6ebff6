// batch_sharded.cpp -- host batches through the path arena: one engine run with arena
// growth, the shards of a call and their result sinks (labels, text, lattices), the pipelined
// one-device batch, and the per-shard compute steps (pipeline stages, text, general lhs,
// pipelines on a general first stage, and the lattice batch with its own arena).
#include <cmath>

#include "host_rt.hpp"

namespace fstamd::host {
namespace {

// One engine run into a path arena of `arc_cap` slots, rerun with a larger arena while a
// string is OUTPUT_FULL.  `launch` queues the engine on `stream`; `failed` names it in the
// error message.  With `keep` the device outputs stay alive and `h` receives only the
// statuses; without it `h` receives everything.  `fine_laps`: the chain route's profile
// also times the arena allocation and the download on their own.
using ArenaLaunch = std::function<hipError_t(const BatchOutDev&, LaunchStats*)>;
FstError run_arena(hipStream_t stream, uint32_t num, uint64_t arc_cap, const char* failed,
                   bool fine_laps, const ArenaLaunch& launch, HostPaths* h,
                   std::unique_ptr<DevOut>* keep) {
  // test override: the first arena size, grown x4 per attempt (so that 6 attempts can run
  // out, tests/test_gpu_watchdog.py) instead of sized from the demand
  bool fixed_growth = false;
  if (const char* e = std::getenv("FSTAMD_ARENA_ARCS"))
    if (*e) {
      arc_cap = std::max<uint64_t>(std::strtoull(e, nullptr, 10), 1);
      fixed_growth = true;
    }
  constexpr int kAttempts = 6;
  for (int attempt = 0; attempt < kAttempts; ++attempt) {
    if (t_prof && fine_laps) t_prof->lap(7);
    auto out = std::make_unique<DevOut>(num, arc_cap);
    if (!out->ok()) return FST_OOM;
    if (t_prof && fine_laps) t_prof->lap(1);
    LaunchStats st;
    hipError_t err = launch(out->v, &st);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    if (t_prof) {
      t_prof->lap(2);
      ++t_prof->runs;
    }
    if (err != hipSuccess) {
      std::fprintf(stderr, "[libfst_amd] %s: %s\n", failed, hipGetErrorString(err));
      return FST_OOM;
    }
    t_last_stats = st;
    if (keep) {
      h->status.resize(num);
      if (!d2h(h->status.data(), out->v.status, num * 4ull, stream) ||
          hipStreamSynchronize(stream) != hipSuccess)
        return FST_OOM;
    } else if (!out->download(num, h, stream)) {
      return FST_OOM;
    }
    if (t_prof && fine_laps) t_prof->lap(3);
    bool full = false;
    for (uint32_t i = 0; i < num; ++i) full |= h->status[i] == kPathOutputFull;
    // The last attempt's result stands: strings still OUTPUT_FULL keep that status (the
    // caller sees FST_PATH_OUTPUT_FULL per string), and `keep` is always set on FST_OK.
    if (!full || attempt + 1 == kAttempts) {
      if (keep) *keep = std::move(out);
      return FST_OK;
    }
    // every engine reserves a path with atomicAdd on the cursor before it checks the
    // capacity, so the cursor ends at the arcs the whole batch needs: one rerun suffices
    unsigned long long need = 0;
    if (!read_u64(&need, out->v.cursor, stream)) return FST_OOM;
    arc_cap = fixed_growth ? arc_cap * 4 : std::max<uint64_t>(arc_cap * 2, need + 1024);
  }
  return FST_OOM;  // unreachable: the last attempt returns above
}

// The offsets of a batch from its first label, and its longest string.
uint32_t rebase_offsets(const uint64_t* offsets, uint32_t num, std::vector<uint64_t>* rebased) {
  uint32_t max_len = 0;
  rebased->resize(num + 1);
  for (uint32_t i = 0; i < num; ++i) {
    (*rebased)[i] = offsets[i] - offsets[0];
    max_len = std::max<uint32_t>(max_len, (uint32_t)(offsets[i + 1] - offsets[i]));
  }
  (*rebased)[num] = offsets[num] - offsets[0];
  return max_len;
}

FstError shard_compact(Shard& S) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  const DevOut& o = *S.keep;
  unsigned long long used = 0;
  if (!read_u64(&used, o.cursor.p, stream)) return FST_OOM;
  used = std::min<unsigned long long>(used, o.v.arc_cap);
  S.st = std::make_unique<DevBuf>(num * 4ull);
  S.off = std::make_unique<DevBuf>((num + 1ull) * 8);
  S.fin = std::make_unique<DevBuf>(num * 8ull);
  S.il = std::make_unique<DevBuf>(used * 4);
  S.ol = std::make_unique<DevBuf>(used * 4);
  S.w = std::make_unique<DevBuf>(used * 8);
  if (!S.st->p || !S.off->p || !S.fin->p || !S.il->p || !S.ol->p || !S.w->p) return FST_OOM;
  if (S.E->compact_paths(o.v, num, S.fail ? (const int32_t*)S.fail->p : nullptr,
                         (int32_t*)S.st->p, (uint64_t*)S.off->p, (uint32_t*)S.il->p,
                         (uint32_t*)S.ol->p, (double*)S.w->p, (double*)S.fin->p, used, &S.tot,
                         stream) != hipSuccess)
    return FST_OOM;
  if (S.tot > used) return FST_OOM;  // an engine bug (the gather wrote nothing past `used`)
  return FST_OK;
}

// D2H of a compacted shard into the (pinned) result, asynchronously on `stream`: no
// synchronisation and no offset fix-up (the pipelined host batch does both once at the end).
bool shard_download_async(Shard& S, FstBatchResult* out, uint64_t arc_base, hipStream_t stream) {
  const uint32_t num = S.s1 - S.s0;
  return d2h(out->status + S.s0, S.st->p, num * 4ull, stream) &&
         d2h(out->final_weights + S.s0, S.fin->p, num * 8ull, stream) &&
         d2h(out->path_offsets + S.s0, S.off->p, num * 8ull, stream) &&
         d2h(out->ilabels + arc_base, S.il->p, S.tot * 4, stream) &&
         d2h(out->olabels + arc_base, S.ol->p, S.tot * 4, stream) &&
         d2h(out->weights + arc_base, S.w->p, S.tot * 8, stream);
}

// The same on the shard's stream, one synchronisation, then its path offsets moved by the
// shard's first arc.
FstError shard_download(Shard& S, FstBatchResult* out, uint64_t arc_base) {
  const hipStream_t stream = S.E.stream();
  if (!shard_download_async(S, out, arc_base, stream) || hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  if (arc_base)
    for (uint32_t i = S.s0; i < S.s1; ++i) out->path_offsets[i] += arc_base;
  return FST_OK;
}

// ---- Text results (fst_normalize_text_batch) -------------------------------------------
// The text phase of a shard, in compact_paths' place: count and scan the output bytes of the
// last stage's paths, then write them (DeviceEngine::text_count / text_write).
FstError shard_text(Shard& S) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  const DevOut& o = *S.keep;
  S.st = std::make_unique<DevBuf>(num * 4ull);
  S.off = std::make_unique<DevBuf>((num + 1ull) * 8);
  S.fin = std::make_unique<DevBuf>(num * 8ull);
  if (!S.st->p || !S.off->p || !S.fin->p) return FST_OOM;
  if (S.E->text_count(o.v, num, S.fail ? (const int32_t*)S.fail->p : nullptr, (int32_t*)S.st->p,
                      (uint64_t*)S.off->p, (double*)S.fin->p, &S.tot, stream) != hipSuccess)
    return FST_OOM;
  S.text = std::make_unique<DevBuf>(S.tot);
  if (!S.text->p) return FST_OOM;
  // (synchronised: the download may run on another engine's stream)
  if (S.E->text_write(o.v, num, (const int32_t*)S.st->p, (const uint64_t*)S.off->p,
                      (uint8_t*)S.text->p, S.tot, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  S.keep.reset();  // the path arena is not downloaded
  return FST_OK;
}

FstError shard_text_download(Shard& S, FstTextResult* out, uint64_t byte_base) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  if (!(d2h(out->status + S.s0, S.st->p, num * 4ull, stream) &&
        d2h(out->total_weight + S.s0, S.fin->p, num * 8ull, stream) &&
        d2h(out->text_offsets + S.s0, S.off->p, num * 8ull, stream) &&
        d2h(out->text + byte_base, S.text->p, S.tot, stream)) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  if (byte_base)
    for (uint32_t i = S.s0; i < S.s1; ++i) out->text_offsets[i] += byte_base;
  return FST_OK;
}

// ---- Lattice results (fst_compose_frozen_batch) ----------------------------------------
// The lattice sink's compaction: count and scan (the totals come back), the shard's arrays in
// FstLhsBatch's layout sized from them, then the gather; the arena goes back to the pool.
FstError shard_lattice_compact(Shard& S) {
  if (!S.lat) return FST_OOM;
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  LatShard& Ls = *S.lat;
  // a failure drains the stream before the shard's buffers go back to the pool
  StreamDrain drain{{stream}};
  Ls.status = std::make_unique<DevBuf>(num * 4ull);
  Ls.soff = std::make_unique<DevBuf>((num + 1ull) * 8);
  Ls.start = std::make_unique<DevBuf>(num * 4ull);
  if (!Ls.status->p || !Ls.soff->p || !Ls.start->p) return FST_OOM;
  LatticeCsrDev csr{};
  csr.status = (int32_t*)Ls.status->p;
  csr.state_offsets = (uint64_t*)Ls.soff->p;
  csr.start = (uint32_t*)Ls.start->p;
  uint64_t needed[2] = {0, 0};
  if (S.E->compact_lattices_count(S.keep->v.status, Ls.arena, num, csr, needed, stream) !=
      hipSuccess)
    return FST_OOM;
  // an engine bug: OK items own more than the arena holds
  if (needed[0] > Ls.arena.state_cap || needed[1] > Ls.arena.arc_cap) return FST_OOM;
  Ls.fin = std::make_unique<DevBuf>(needed[0] * 8);
  Ls.aoffs = std::make_unique<DevBuf>((needed[0] + 1) * 8);
  Ls.il = std::make_unique<DevBuf>(needed[1] * 4);
  Ls.ol = std::make_unique<DevBuf>(needed[1] * 4);
  Ls.next = std::make_unique<DevBuf>(needed[1] * 4);
  Ls.w = std::make_unique<DevBuf>(needed[1] * 8);
  if (!Ls.fin->p || !Ls.aoffs->p || !Ls.il->p || !Ls.ol->p || !Ls.next->p || !Ls.w->p)
    return FST_OOM;
  csr.final_w = (double*)Ls.fin->p;
  csr.arc_offsets = (uint64_t*)Ls.aoffs->p;
  csr.il = (uint32_t*)Ls.il->p;
  csr.ol = (uint32_t*)Ls.ol->p;
  csr.w = (double*)Ls.w->p;
  csr.next = (uint32_t*)Ls.next->p;
  csr.state_cap = needed[0];
  csr.arc_cap = needed[1];
  // (synchronised: the download may run on another engine's stream)
  if (S.E->compact_lattices(Ls.arena, num, csr, stream, Ls.connect ? &Ls.trim : nullptr) !=
          hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  drain.done = true;
  for (auto* b : {&Ls.tmark, &Ls.tqueue, &Ls.troff, &Ls.trcur, &Ls.trsrc, &Ls.tlist, &Ls.tctr,
                  &Ls.tstart})
    b->reset();
  Ls.input.reset();
  Ls.item.reset();
  Ls.afin.reset();
  Ls.aaoff.reset();
  Ls.ail.reset();
  Ls.aol.reset();
  Ls.aw.reset();
  Ls.anext.reset();
  S.tot = needed[0];
  S.tot2 = needed[1];
  return FST_OK;
}

// D2H of a compacted lattice shard at its item range, its first state and its first arc; the
// two offset arrays are then moved by those bases (the closing entries: the sink's finish).
FstError shard_lattice_download(Shard& S, FstLatticeBatch* out, uint64_t sbase, uint64_t abase) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  const LatShard& Ls = *S.lat;
  const FstLhsBatch& F = out->fsts;
  uint64_t* soff = const_cast<uint64_t*>(F.state_offsets);
  uint64_t* aoff = const_cast<uint64_t*>(F.arc_offsets);
  if (!(d2h(out->status + S.s0, Ls.status->p, num * 4ull, stream) &&
        d2h(const_cast<uint32_t*>(F.start) + S.s0, Ls.start->p, num * 4ull, stream) &&
        d2h(soff + S.s0, Ls.soff->p, num * 8ull, stream) &&
        d2h(const_cast<double*>(F.final_weights) + sbase, Ls.fin->p, S.tot * 8, stream) &&
        d2h(aoff + sbase, Ls.aoffs->p, S.tot * 8, stream) &&
        d2h(const_cast<uint32_t*>(F.ilabels) + abase, Ls.il->p, S.tot2 * 4, stream) &&
        d2h(const_cast<uint32_t*>(F.olabels) + abase, Ls.ol->p, S.tot2 * 4, stream) &&
        d2h(const_cast<uint32_t*>(F.nextstates) + abase, Ls.next->p, S.tot2 * 4, stream) &&
        d2h(const_cast<double*>(F.weights) + abase, Ls.w->p, S.tot2 * 8, stream)) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  if (sbase)
    for (uint32_t i = S.s0; i < S.s1; ++i) soff[i] += sbase;
  if (abase)
    for (uint64_t s = sbase; s < sbase + S.tot; ++s) aoff[s] += abase;
  return FST_OK;
}

// One chain stage of a shard on device inputs: S.keep = its outputs (`h`: the statuses, one
// pinned block for all the stages of a shard).
FstError run_chain_stage(Shard& S, FrozenFst& f, const DevBuf& lab, const DevBuf& off,
                         uint64_t in_total, uint32_t max_len, uint32_t n, int semantics,
                         HostPaths* h) {
  const uint32_t num_strings = S.s1 - S.s0;
  DeviceFst* D = f.device(S.dev);
  if (!D) return FST_OOM;
  ChainInput in{{(const uint32_t*)lab.p}, (const uint64_t*)off.p, num_strings, max_len};
  S.keep.reset();
  FstError e = run_chain_batch_dev(S.E, *D, in, in_total, n, semantics, h, &S.keep);
  if (e != FST_OK) return e;
  return S.keep ? FST_OK : FST_OOM;  // run_chain_batch_dev sets it on FST_OK
}

// S.fail of a shard whose first stage is about to run or has just finished: no failure yet.
FstError clear_stage_failures(Shard& S) {
  const uint32_t num_strings = S.s1 - S.s0;
  S.fail = std::make_unique<DevBuf>(num_strings * 4ull);  // first failing stage per string
  if (!S.fail->p ||
      hipMemsetAsync(S.fail->p, 0, num_strings * 4ull, S.E.stream()) != hipSuccess)
    return FST_OOM;
  return FST_OK;
}

// The stages [first, fs.size()) of one shard, from a finished stage: S.keep holds stage
// first - 1's outputs (whatever entry produced them: a chain stage, a general-lhs batch) and
// S.fail the failures so far.  Each stage's 1-best output tape is projected into the next
// stage's chain inputs on the device.
FstError run_stages_after(Shard& S, const Stages& fs, size_t first, uint32_t n, int semantics,
                          HostPaths* h) {
  DeviceEngine::Lease& E = S.E;
  const uint32_t num_strings = S.s1 - S.s0;
  const hipStream_t stream = E.stream();
  for (size_t k = first; k < fs.size(); ++k) {
    // project the finished stage's outputs into this stage's inputs, on the device
    unsigned long long used = 0;
    if (!read_u64(&used, S.keep->v.cursor, stream)) return FST_OOM;
    DevBuf lab((used + num_strings) * 4), off((num_strings + 1ull) * 8);
    DevBuf pst(num_strings * 4ull);
    if (!lab.p || !off.p || !pst.p) return FST_OOM;
    // a failure below drains the stream before the three go back to the pool
    StreamDrain drain{{stream}};
    uint32_t max_len = 0;
    if (E->project_output(S.keep->v, num_strings, (uint32_t*)lab.p, (uint64_t*)off.p,
                          (int32_t*)pst.p, &max_len, stream) != hipSuccess ||
        E->merge_status((int32_t*)S.fail->p, (const int32_t*)pst.p, num_strings, stream) !=
            hipSuccess)
      return FST_OOM;
    // (synchronises: pst may go back to the pool)
    uint64_t in_total = 0;
    if (!read_u64(&in_total, (uint64_t*)off.p + num_strings, stream)) return FST_OOM;
    if (t_prof) t_prof->lap(4);
    // (the stage synchronises the stream before lab and off go back to the pool)
    if (FstError e = run_chain_stage(S, *fs[k], lab, off, in_total, max_len, n, semantics, h);
        e != FST_OK)
      return e;
    drain.done = true;
  }
  return FST_OK;
}

// The stages of one shard on device inputs (labels `lab`, offsets `off`, in_total labels).
FstError run_pipeline_stages(Shard& S, const Stages& fs, std::unique_ptr<DevBuf> lab,
                             std::unique_ptr<DevBuf> off, uint64_t in_total, uint32_t max_len,
                             uint32_t n, int semantics) {
  if (FstError e = clear_stage_failures(S); e != FST_OK) return e;
  HostPaths h;
  if (FstError e = run_chain_stage(S, *fs[0], *lab, *off, in_total, max_len, n, semantics, &h);
      e != FST_OK)
    return e;
  // (the stage synchronised the stream: its inputs go back to the pool before the next
  // stage's are allocated)
  lab.reset();
  off.reset();
  return run_stages_after(S, fs, 1, n, semantics, &h);
}

}  // namespace

FstError run_chain_batch_dev(DeviceEngine::Lease& E, DeviceFst& D, const ChainInput& in,
                             uint64_t total_labels, uint32_t n, int semantics, HostPaths* h,
                             std::unique_ptr<DevOut>* keep) {
  const hipStream_t stream = E.stream();
  // Arena: chains without rhs epsilons produce exactly L arcs per path; with them a path
  // also carries the rhs epsilon arcs (a tagger's or verbalizer's multi-symbol outputs),
  // so start at 4 arcs per label rather than run the whole batch twice on OUTPUT_FULL.
  const uint64_t arc_cap = std::max<uint64_t>((D.has_eps ? 4 : 1) * total_labels + 16, 1024);
  return run_arena(
      stream, in.num_strings, arc_cap, "batch engine failed", true,
      [&](const BatchOutDev& v, LaunchStats* st) {
        return E->run_chain(D, in, n, semantics, v, stream, st);
      },
      h, keep);
}

bool alloc_result(FstBatchResult* out, uint32_t num, uint64_t tot) {
  out->num_strings = num;
  out->total_arcs = tot;
  out->status = (int32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
  out->path_offsets = (uint64_t*)pin_alloc((num + 1ull) * 8);
  out->final_weights = (double*)pin_alloc(std::max<size_t>(num, 1) * 8);
  out->ilabels = (uint32_t*)pin_alloc(std::max<uint64_t>(tot, 1) * 4);
  out->olabels = (uint32_t*)pin_alloc(std::max<uint64_t>(tot, 1) * 4);
  out->weights = (double*)pin_alloc(std::max<uint64_t>(tot, 1) * 8);
  return out->status && out->path_offsets && out->final_weights && out->ilabels &&
         out->olabels && out->weights;
}

bool alloc_text_result(FstTextResult* out, uint32_t num, uint64_t tot) {
  out->num_strings = num;
  out->total_bytes = tot;
  out->status = (int32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
  out->text_offsets = (uint64_t*)pin_alloc((num + 1ull) * 8);
  out->total_weight = (double*)pin_alloc(std::max<size_t>(num, 1) * 8);
  out->text = (uint8_t*)pin_alloc(std::max<uint64_t>(tot, 1));
  return out->status && out->text_offsets && out->total_weight && out->text;
}

FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     const ShardSink& sink) {
  // shard 0 runs on the calling thread and switches its current device: give the caller
  // its device back on every return (later calls that use current_device() rely on it)
  DeviceRestore_ restore;
  nsh = std::max<uint32_t>(1, std::min<uint32_t>(nsh, std::max<uint32_t>(num, 1)));
  std::vector<Shard> sh(nsh);
  if (nsh == 1) {
    sh[0].dev = devices[0];
    sh[0].s0 = 0;
    sh[0].s1 = num;
  } else {
    double total = 0;
    for (double c : cost) total += c;
    uint32_t i = 0;
    double acc = 0;
    for (uint32_t j = 0; j < nsh; ++j) {
      sh[j].dev = devices[j % devices.size()];
      sh[j].s0 = i;
      const double goal = total * (j + 1) / nsh;
      // leave at least one string for each later shard
      while (i < num && (j + 1 == nsh || (acc + cost[i] <= goal && num - i > nsh - 1 - j))) {
        acc += cost[i];
        ++i;
      }
      if (j + 1 < nsh && i == sh[j].s0 && i < num) acc += cost[i++];  // never empty
      sh[j].s1 = (j + 1 == nsh) ? num : i;
    }
  }
  if (std::getenv("FSTAMD_SHARD_LOG"))  // tests: the shard plan
    for (uint32_t j = 0; j < nsh; ++j) {
      double c = 0;
      for (uint32_t i = sh[j].s0; i < sh[j].s1 && i < cost.size(); ++i) c += cost[i];
      std::fprintf(stderr, "[libfst_amd shard] %u dev %d strings %u..%u cost %.6g route sharded\n", j,
                   sh[j].dev, sh[j].s0, sh[j].s1, c);
    }
  auto phase1 = [&](Shard& S) {
    if (hipSetDevice(S.dev) != hipSuccess) {
      S.err = FST_INVALID_ARG;
      return;
    }
    S.E = DeviceEngine::acquire(S.dev);
    if (!S.E) {
      S.err = FST_INVALID_ARG;
      return;
    }
    S.err = compute(S);
    S.stats = t_last_stats;
    if (S.err == FST_OK && !S.keep) S.err = FST_OOM;
    if (S.err == FST_OK) S.err = sink.compact(S);
    // no lease is held between the phases: a shard waiting for an engine never holds one
    // (two sharded calls on one device cannot deadlock)
    S.E = DeviceEngine::Lease();
  };
  auto phase2 = [&](Shard& S, uint64_t base, uint64_t base2) {
    if (hipSetDevice(S.dev) != hipSuccess) {
      S.err = FST_OOM;
      return;
    }
    S.E = DeviceEngine::acquire(S.dev);
    S.err = S.E ? sink.download(S, base, base2) : FST_OOM;
    S.E = DeviceEngine::Lease();
  };
  auto each = [&](const std::function<void(uint32_t)>& f) {
    if (nsh == 1) return f(0);
    std::vector<std::thread> th;
    for (uint32_t j = 1; j < nsh; ++j) th.emplace_back(f, j);
    f(0);
    for (auto& x : th) x.join();
  };
  each([&](uint32_t j) { phase1(sh[j]); });
  uint64_t tot = 0, tot2 = 0;
  for (Shard& S : sh) {
    if (S.err != FST_OK) return S.err;
    tot += S.tot;
    tot2 += S.tot2;
  }
  if (t_prof) t_prof->lap(4);
  if (!sink.alloc(tot, tot2)) return FST_OOM;
  std::vector<uint64_t> base(nsh, 0), base2(nsh, 0);
  for (uint32_t j = 1; j < nsh; ++j) {
    base[j] = base[j - 1] + sh[j - 1].tot;
    base2[j] = base2[j - 1] + sh[j - 1].tot2;
  }
  each([&](uint32_t j) { phase2(sh[j], base[j], base2[j]); });
  sink.finish(tot, tot2);
  LaunchStats agg = sh[0].stats;  // the slowest shard's kernel time, launches summed
  for (uint32_t j = 1; j < nsh; ++j) {
    agg.kernel_ms = std::max(agg.kernel_ms, sh[j].stats.kernel_ms);
    agg.launches += sh[j].stats.launches;
  }
  t_last_stats = agg;
  for (Shard& S : sh)
    if (S.err != FST_OK) return S.err;
  if (t_prof) t_prof->lap(3);
  return FST_OK;
}

FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstBatchResult* out) {
  const ShardSink sink{shard_compact,
                       [=](uint64_t tot, uint64_t) { return alloc_result(out, num, tot); },
                       [=](Shard& S, uint64_t base, uint64_t) {
                         return shard_download(S, out, base);
                       },
                       [=](uint64_t tot, uint64_t) { out->path_offsets[num] = tot; }};
  return run_sharded(devices, nsh, num, cost, compute, sink);
}

FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstLatticeBatch* out) {
  const ShardSink sink{shard_lattice_compact,
                       [=](uint64_t states, uint64_t arcs) {
                         return alloc_lattice_result(out, num, states, arcs);
                       },
                       [=](Shard& S, uint64_t sbase, uint64_t abase) {
                         return shard_lattice_download(S, out, sbase, abase);
                       },
                       [=](uint64_t states, uint64_t arcs) {
                         const_cast<uint64_t*>(out->fsts.state_offsets)[num] = states;
                         const_cast<uint64_t*>(out->fsts.arc_offsets)[states] = arcs;
                       }};
  return run_sharded(devices, nsh, num, cost, compute, sink);
}

FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstTextResult* out) {
  const ShardSink sink{shard_text,
                       [=](uint64_t tot, uint64_t) { return alloc_text_result(out, num, tot); },
                       [=](Shard& S, uint64_t base, uint64_t) {
                         return shard_text_download(S, out, base);
                       },
                       [=](uint64_t tot, uint64_t) { out->text_offsets[num] = tot; }};
  return run_sharded(devices, nsh, num, cost, compute, sink);
}

// One device, one large batch on an rhs without input epsilons (a path has exactly L arcs,
// so the result is allocated before any shard finishes): the strings run as consecutive
// sub-shards on one engine, and the download of sub-shard j (a second stream, waiting for
// j's compaction only) runs while sub-shard j + 1 computes -- round 3's host batch ran its
// ~1 GB D2H after all the kernels.  Results are identical to the one-shard path.
FstError run_pipelined(int dev, FrozenFst& b, const uint32_t* labels, const uint64_t* offsets,
                       uint32_t num, uint32_t n, int semantics, uint32_t parts,
                       FstBatchResult* out) {
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b.device(dev);
  if (!D) return FST_OOM;
  DeviceEngine::Lease E = DeviceEngine::acquire(dev);
  if (!E) return FST_INVALID_ARG;
  const hipStream_t stream = E.stream();
  struct OwnStream {  // a stream of the call's own and its events: drained, then destroyed
    hipStream_t s = nullptr;
    std::vector<hipEvent_t> ev;
    ~OwnStream() {
      if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
      }
      for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
  } C;  // the downloads' stream and the compaction events it waits for
  if (hipStreamCreateWithFlags(&C.s, hipStreamNonBlocking) != hipSuccess) return FST_OOM;
  std::vector<uint64_t> rebased;
  rebase_offsets(offsets, num, &rebased);
  const uint64_t total = rebased[num];
  DevBuf d_lab(total * 4), d_off((num + 1) * 8ull);
  if (!d_lab.p || !d_off.p) return FST_OOM;
  if (hipMemcpyAsync(d_off.p, rebased.data(), (num + 1) * 8ull, hipMemcpyHostToDevice, stream) !=
      hipSuccess)
    return FST_OOM;
  std::vector<Shard> sh(parts);
  // every return drains the engine stream before the buffers its kernels use (d_lab, d_off,
  // the sub-shards' outputs: declared above, destroyed after this) go back to the pool
  StreamDrain sync_engine{{stream}};
  for (uint32_t j = 0; j < parts; ++j) {
    sh[j].dev = dev;
    sh[j].s0 = (uint32_t)((uint64_t)num * j / parts);
    sh[j].s1 = (uint32_t)((uint64_t)num * (j + 1) / parts);
  }
  // The labels go up per sub-shard on a thread and stream of their own (a pageable source
  // is staged through pinned memory on the copying thread), so sub-shard j + 1's upload
  // runs while sub-shard j computes; the engine's stream waits on each upload's event.
  struct Uploader : OwnStream {  // (the thread joined before the stream goes)
    PartGate gate;
    ThreadGroup th;
  } U;
  if (hipStreamCreateWithFlags(&U.s, hipStreamNonBlocking) != hipSuccess) return FST_OOM;
  U.ev.assign(parts, nullptr);
  for (uint32_t j = 0; j < parts; ++j)
    if (hipEventCreateWithFlags(&U.ev[j], hipEventDisableTiming) != hipSuccess) return FST_OOM;
  U.th.add([&, dev] {
    bool ok = hipSetDevice(dev) == hipSuccess;
    for (uint32_t j = 0; j < parts && ok; ++j) {
      const uint64_t a = rebased[sh[j].s0], z = rebased[sh[j].s1];
      ok = ok && (z == a || hipMemcpyAsync((uint32_t*)d_lab.p + a, labels + offsets[0] + a,
                                           (z - a) * 4, hipMemcpyHostToDevice, U.s) == hipSuccess);
      ok = ok && hipEventRecord(U.ev[j], U.s) == hipSuccess;
      if (ok) U.gate.publish(j + 1);
    }
    if (!ok) U.gate.fail();
  });
  if (t_prof) t_prof->lap(0);
  if (!alloc_result(out, num, total)) return FST_OOM;  // paths of L arcs: <= total arcs
  // every return below first waits for the downloads in flight: on an error the caller
  // frees the result, whose pinned pages must not be written after that
  StreamDrain sync_copies{{C.s}};
  uint64_t base = 0;
  for (uint32_t j = 0; j < parts; ++j) {
    Shard& S = sh[j];
    if (!U.gate.wait_for(j)) return FST_OOM;
    if (hipStreamWaitEvent(stream, U.ev[j], 0) != hipSuccess) return FST_OOM;
    uint32_t ml = 0;
    for (uint32_t i = S.s0; i < S.s1; ++i) ml = std::max<uint32_t>(ml, (uint32_t)(rebased[i + 1] - rebased[i]));
    // the sub-shard reads the whole upload: its offsets index the one label array
    ChainInput in{(const uint32_t*)d_lab.p, (const uint64_t*)d_off.p + S.s0, S.s1 - S.s0, ml};
    HostPaths h;
    if (FstError e = run_chain_batch_dev(E, *D, in, rebased[S.s1] - rebased[S.s0], n, semantics,
                                         &h, &S.keep);
        e != FST_OK)
      return e;
    S.stats = t_last_stats;
    S.E = std::move(E);  // shard_compact runs on the lease's stream
    const FstError ce = shard_compact(S);
    E = std::move(S.E);
    if (ce != FST_OK) return ce;
    if (base + S.tot > total) return FST_OOM;  // (a path longer than its string: impossible)
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return FST_OOM;
    C.ev.push_back(ev);
    if (hipEventRecord(ev, stream) != hipSuccess || hipStreamWaitEvent(C.s, ev, 0) != hipSuccess ||
        !shard_download_async(S, out, base, C.s))
      return FST_OOM;
    S.keep.reset();  // (the path arena: compaction copied what the download needs)
    base += S.tot;
  }
  if (hipStreamSynchronize(C.s) != hipSuccess) return FST_OOM;
  if (t_prof) t_prof->lap(3);
  uint64_t acc = 0;
  for (uint32_t j = 0; j < parts; ++j) {
    if (acc)
      for (uint32_t i = sh[j].s0; i < sh[j].s1; ++i) out->path_offsets[i] += acc;
    acc += sh[j].tot;
  }
  out->path_offsets[num] = base;
  out->total_arcs = base;
  LaunchStats agg = sh[0].stats;
  agg.kernel_ms = 0;
  agg.launches = 0;
  for (const Shard& S : sh) {
    agg.kernel_ms += S.stats.kernel_ms;
    agg.launches += S.stats.launches;
  }
  t_last_stats = agg;
  return FST_OK;
}

// One shard of a pipeline: every stage on the shard's device, each stage's 1-best output tape
// projected into the next stage's inputs on the device; S.keep = the last stage's outputs,
// S.fail = the first failing stage per string.
FstError run_pipeline_shard(Shard& S, const Stages& fs, const uint32_t* labels,
                            const uint64_t* offsets, uint32_t n, int semantics) {
  const uint32_t num_strings = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  // stage-1 inputs
  std::vector<uint64_t> rebased;
  const uint32_t max_len = rebase_offsets(offsets, num_strings, &rebased);
  const uint64_t total = rebased[num_strings];
  auto lab = std::make_unique<DevBuf>(total * 4), off = std::make_unique<DevBuf>((num_strings + 1ull) * 8);
  if (!lab->p || !off->p) return FST_OOM;
  if (total && hipMemcpyAsync(lab->p, labels + offsets[0], total * 4, hipMemcpyHostToDevice,
                              stream) != hipSuccess)
    return FST_OOM;
  if (hipMemcpyAsync(off->p, rebased.data(), (num_strings + 1ull) * 8, hipMemcpyHostToDevice,
                     stream) != hipSuccess)
    return FST_OOM;
  if (t_prof) t_prof->lap(0);
  return run_pipeline_stages(S, fs, std::move(lab), std::move(off), total, max_len, n, semantics);
}

// The text entry's shard: the bytes and their offsets go up as they are, the device widens
// them to stage-1 labels (DeviceEngine::widen_text), then the same stages.
FstError run_text_shard(Shard& S, const Stages& fs, const uint8_t* text, const uint64_t* offsets,
                        int semantics) {
  const uint32_t num_strings = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  std::vector<uint64_t> rebased;
  const uint32_t max_len = rebase_offsets(offsets, num_strings, &rebased);
  const uint64_t total = rebased[num_strings];
  // `bytes` is read by the widen kernel only; it and `rebased` live until the first stage
  // has synchronised the stream, and every failure drains the stream before they go
  StreamDrain drain{{stream}};
  DevBuf bytes(total);
  auto lab = std::make_unique<DevBuf>(total * 4), off = std::make_unique<DevBuf>((num_strings + 1ull) * 8);
  if (!bytes.p || !lab->p || !off->p) return FST_OOM;
  if (total && hipMemcpyAsync(bytes.p, text + offsets[0], total, hipMemcpyHostToDevice, stream) !=
                   hipSuccess)
    return FST_OOM;
  if (hipMemcpyAsync(off->p, rebased.data(), (num_strings + 1ull) * 8, hipMemcpyHostToDevice,
                     stream) != hipSuccess)
    return FST_OOM;
  if (S.E->widen_text((const uint8_t*)bytes.p, (const uint64_t*)off->p, num_strings,
                      (uint32_t*)lab->p, stream) != hipSuccess)
    return FST_OOM;
  if (t_prof) t_prof->lap(0);
  const FstError e =
      run_pipeline_stages(S, fs, std::move(lab), std::move(off), total, max_len, 1, semantics);
  drain.done = e == FST_OK;  // (run_chain_batch_dev synchronised it)
  return e;
}

// The items of one shard (items [i0, i1) of the caller's batch) staged into one pinned block --
// descriptors, per-state arc offsets local to the item, finals, the four arc arrays, the two
// eager item lists -- and uploaded with one DMA.  The 1-best shard (run_lhs_shard) and the
// lattice shard (run_lattice_lhs_shard) share it.
namespace {
struct LhsStaged {
  std::unique_ptr<DevBuf> blk;
  PinnedVec<uint8_t> hin;
  ChainInput in{};
  GraphInput g{};
  const uint32_t* items_nonneg = nullptr;
  const uint32_t* items_replay = nullptr;
  uint32_t num_nonneg = 0, num_replay = 0;
  uint64_t num_states = 0, num_arcs = 0;
};

// Queues the upload on `stream`; the caller drains the stream before *st goes (the upload or
// a kernel may still be using its two blocks).
FstError stage_lhs_items(Shard& S, DeviceFst* D, const FstLhsBatch& L, hipStream_t stream,
                         LhsStaged* st) {
  const uint32_t i0 = S.s0, num = S.s1 - S.s0;
  const uint64_t sb = L.state_offsets[i0], ns = L.state_offsets[S.s1] - sb;
  const uint64_t ab = L.arc_offsets[sb], na = L.arc_offsets[L.state_offsets[S.s1]] - ab;
  auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
  const uint64_t o_desc = 0, o_soff = al(num * 32ull), o_fin = o_soff + al((ns + num) * 4),
                 o_w = o_fin + al(ns * 8), o_il = o_w + al(na * 8), o_ol = o_il + al(na * 4),
                 o_nx = o_ol + al(na * 4), o_la = o_nx + al(na * 4), o_lb = o_la + al(num * 4ull),
                 end = o_lb + al(num * 4ull);
  st->blk = std::make_unique<DevBuf>(end);
  st->hin.resize(end);
  DevBuf& blk = *st->blk;
  PinnedVec<uint8_t>& hin = st->hin;
  if (!blk.p) return FST_OOM;
  LhsDesc* desc = (LhsDesc*)(hin.data() + o_desc);
  uint32_t* soff = (uint32_t*)(hin.data() + o_soff);
  uint32_t* la = (uint32_t*)(hin.data() + o_la);
  uint32_t* lb = (uint32_t*)(hin.data() + o_lb);
  if (ns) std::memcpy(hin.data() + o_fin, L.final_weights + sb, ns * 8);
  if (na) {
    std::memcpy(hin.data() + o_w, L.weights + ab, na * 8);
    std::memcpy(hin.data() + o_il, L.ilabels + ab, na * 4);
    std::memcpy(hin.data() + o_ol, L.olabels + ab, na * 4);
    std::memcpy(hin.data() + o_nx, L.nextstates + ab, na * 4);
  }
  uint32_t n_a = 0, n_b = 0, max_outdeg = 0;
  const auto neg = [](double x) { return x < 0.0 || (x == 0.0 && std::signbit(x)); };
  for (uint32_t i = 0; i < num; ++i) {
    const uint64_t s0 = L.state_offsets[i0 + i], s1 = L.state_offsets[i0 + i + 1];
    const uint64_t a0 = L.arc_offsets[s0], a1 = L.arc_offsets[s1];
    LhsDesc& d = desc[i];
    d.state_base = s0 - sb;
    d.arc_base = a0 - ab;
    d.num_states = (uint32_t)(s1 - s0);
    d.start = d.num_states ? L.start[i0 + i] : kNoState;
    d.num_arcs = (uint32_t)(a1 - a0);
    uint32_t fl = 0;
    if (D && D->nan) fl |= kLhsNaN;  // (no rhs: fst_connect_lhs_batch, which reads no flag)
    if (D && !D->nonneg) fl |= kLhsReplay;
    uint32_t* so = soff + (s0 - sb) + i;
    for (uint64_t s = s0; s <= s1; ++s) so[s - s0] = (uint32_t)(L.arc_offsets[s] - a0);
    for (uint64_t s = s0; s < s1; ++s) {
      max_outdeg = std::max(max_outdeg, so[s - s0 + 1] - so[s - s0]);
      const double f = L.final_weights[s];
      if (std::isnan(f)) fl |= kLhsNaN;
      if (neg(f)) fl |= kLhsReplay;
    }
    for (uint64_t a = a0; a < a1; ++a) {
      const double w = L.weights[a];
      if (std::isnan(w)) fl |= kLhsNaN;
      if (neg(w) || std::isinf(w)) fl |= kLhsReplay;
      if (L.olabels[a] == kEpsilon) fl |= kLhsEpsOut;
    }
    d.flags = fl;
    if (fl & kLhsReplay) lb[n_b++] = i;
    else la[n_a++] = i;
  }
  if (max_outdeg >= (1u << 30)) return FST_OOM;  // the lazy per-pop table is 2 * deg + 2 entries
  if (hipMemcpyAsync(blk.p, hin.data(), end, hipMemcpyHostToDevice, stream) != hipSuccess)
    return FST_OOM;
  uint8_t* p = (uint8_t*)blk.p;
  ChainInput& in = st->in;
  in.lhs_desc = (const LhsDesc*)(p + o_desc);
  in.num_strings = num;
  GraphInput& g = st->g;
  g.state_off = (const uint32_t*)(p + o_soff);
  g.final_w = (const double*)(p + o_fin);
  g.arc_w = (const double*)(p + o_w);
  g.arc_il = (const uint32_t*)(p + o_il);
  g.arc_ol = (const uint32_t*)(p + o_ol);
  g.arc_next = (const uint32_t*)(p + o_nx);
  g.start = kNoState;
  g.max_outdeg = max_outdeg;
  st->items_nonneg = (const uint32_t*)(p + o_la);
  st->items_replay = (const uint32_t*)(p + o_lb);
  st->num_nonneg = n_a;
  st->num_replay = n_b;
  st->num_states = ns;
  st->num_arcs = na;
  if (t_prof) t_prof->lap(0);
  return FST_OK;
}
}  // namespace

// One shard of general lhs on the shard's engine: the staged items through
// DeviceEngine::run_lhs_batch, its arena grown on OUTPUT_FULL as run_chain_batch_dev's is.
FstError run_lhs_shard(Shard& S, FrozenFst& b, const FstLhsBatch& L, uint32_t n, int semantics) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b.device(dev);
  if (!D) return FST_OOM;
  const hipStream_t stream = S.E.stream();
  LhsStaged st;
  // every return drains the stream before the staged blocks go back to their pools: the
  // upload or a kernel (the engine can fail after launching some) may still be using them
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, D, L, stream, &st); e != FST_OK) return e;
  HostPaths h;  // (the statuses)
  return run_arena(
      stream, S.s1 - S.s0, std::max<uint64_t>(4 * st.num_arcs + 16, 1024),
      "lhs batch engine failed", false,
      [&](const BatchOutDev& v, LaunchStats* ls) {
        LhsRoute route;
        return S.E->run_lhs_batch(*D, st.in, st.g, n, semantics, st.items_nonneg, st.num_nonneg,
                                  st.items_replay, st.num_replay, v, stream, ls, &route);
      },
      &h, &S.keep);
}

// One shard of fst_shortest_path_lhs_batch: the staged items through DeviceEngine::run_sp_batch,
// which reads the staged block in place.  An OK path has at most num_states - 1 arcs (a longer
// back-pointer walk is a cycle), so an arena of the shard's states is never too small: no
// OUTPUT_FULL, no rerun.
FstError run_sp_shard(Shard& S, const FstLhsBatch& L, uint32_t n) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const hipStream_t stream = S.E.stream();
  const uint32_t num = S.s1 - S.s0;
  LhsStaged st;
  // every return drains the stream before the staged blocks and the arena go back to their pools
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, nullptr, L, stream, &st); e != FST_OK) return e;
  auto out = std::make_unique<DevOut>(num, std::max<uint64_t>(st.num_states, 1));
  if (!out->ok()) return FST_OOM;
  if (t_prof) t_prof->lap(1);
  LaunchStats ls;
  LhsRoute route;
  const hipError_t err =
      S.E->run_sp_batch(st.in, st.g, st.num_states, st.num_arcs, n, st.items_nonneg,
                        st.num_nonneg, st.items_replay, st.num_replay, out->v, stream, &ls, &route);
  if (t_prof) {
    t_prof->lap(2);
    ++t_prof->runs;
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "[libfst_amd] lattice shortest path failed: %s\n", hipGetErrorString(err));
    return FST_OOM;
  }
  t_last_stats = ls;
  S.keep = std::move(out);
  return FST_OK;  // (the drain: run_sp_batch synchronised, nothing is left to wait for)
}

// ---- Lattice shards ---------------------------------------------------------------------

bool alloc_lattice_result(FstLatticeBatch* out, uint32_t num, uint64_t states, uint64_t arcs) {
  FstLhsBatch& F = out->fsts;
  F.num_fsts = num;
  out->total_states = states;
  out->total_arcs = arcs;
  out->status = (int32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
  F.state_offsets = (uint64_t*)pin_alloc((num + 1ull) * 8);
  F.start = (uint32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
  F.final_weights = (double*)pin_alloc(std::max<uint64_t>(states, 1) * 8);
  F.arc_offsets = (uint64_t*)pin_alloc((states + 1) * 8);
  F.ilabels = (uint32_t*)pin_alloc(std::max<uint64_t>(arcs, 1) * 4);
  F.olabels = (uint32_t*)pin_alloc(std::max<uint64_t>(arcs, 1) * 4);
  F.nextstates = (uint32_t*)pin_alloc(std::max<uint64_t>(arcs, 1) * 4);
  F.weights = (double*)pin_alloc(std::max<uint64_t>(arcs, 1) * 8);
  return out->status && F.state_offsets && F.start && F.final_weights && F.arc_offsets &&
         F.ilabels && F.olabels && F.nextstates && F.weights;
}

// ---- Lattice trim (connect) ---------------------------------------------------------------

FstError trim_lattices(DeviceEngine::Lease& E, const int32_t* status, LatShard& L, uint32_t num,
                       hipStream_t stream) {
  if (num == 0) return FST_OK;
  const LatticeOutDev& a = L.arena;
  const bool access = L.tstart != nullptr;
  uint32_t sweeps = 4;  // a compose lattice settles in one or two; tests: FSTAMD_TRIM_SWEEPS
  if (const char* e = std::getenv("FSTAMD_TRIM_SWEEPS"))
    if (*e) sweeps = (uint32_t)std::min<unsigned long long>(std::strtoull(e, nullptr, 10), 1u << 20);
  uint32_t cap = 0xFFFFFFFFu;
  if (const char* g = std::getenv("FSTAMD_GRAPH_GRID"))
    if (std::atoi(g) > 0) cap = (uint32_t)std::atoi(g);
  const uint32_t cus = (uint32_t)std::max(E->num_cus(), 1);
  const uint32_t grid_wave = std::max<uint32_t>(1, std::min({num, cus * 32, cap}));
  const uint32_t grid_wg = std::max<uint32_t>(1, std::min({num, cus * 8, cap}));
  const uint64_t sb = (a.state_cap + 4) * 4, ab = (a.arc_cap + 4) * 4;
  L.tmark = std::make_unique<DevBuf>(sb);
  L.tlist = std::make_unique<DevBuf>(num * 4ull);
  L.tctr = std::make_unique<DevBuf>(64);
  if (access) L.tqueue = std::make_unique<DevBuf>(sb);
  if (!L.tmark->p || !L.tlist->p || !L.tctr->p || (access && !L.tqueue->p)) return FST_OOM;
  // every return drains the stream before the workspace (and the caller's arena) can go
  StreamDrain drain{{stream}};
  LatTrimDev& t = L.trim;
  t.mark = (uint32_t*)L.tmark->p;
  t.queue = access ? (uint32_t*)L.tqueue->p : nullptr;
  t.roff = t.rcur = t.rsrc = nullptr;
  t.list = (uint32_t*)L.tlist->p;
  t.tot = (unsigned long long*)L.tctr->p;
  t.ctr = (uint32_t*)((uint8_t*)L.tctr->p + 32);
  t.start = access ? (const uint32_t*)L.tstart->p : nullptr;
  t.sweeps = sweeps;
  t.access = access ? 1u : 0u;
  struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } ev;
  if (hipEventCreate(&ev.e[0]) != hipSuccess || hipEventCreate(&ev.e[1]) != hipSuccess)
    return FST_OOM;
  uint32_t launches = 0;
  if (hipMemsetAsync(L.tctr->p, 0, 64, stream) != hipSuccess ||
      hipEventRecord(ev.e[0], stream) != hipSuccess)
    return FST_OOM;
  if (access) {
    if (launch_trim_access(a, t, status, num, grid_wg, stream) != hipSuccess) return FST_OOM;
    ++launches;
  }
  if (launch_trim_sweep(a, t, status, num, grid_wave, stream) != hipSuccess) return FST_OOM;
  ++launches;
  PinnedVec<uint32_t> back(16);  // tot[4] as 8 words, then ctr
  if (!d2h(back.data(), L.tctr->p, 64, stream) || hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  const uint32_t handed = back[8 + kTrimCtrList];
  if (handed > num) return FST_OOM;  // (a bug: the list holds an item at most once)
  if (handed) {
    L.troff = std::make_unique<DevBuf>(sb);
    L.trcur = std::make_unique<DevBuf>(sb);
    L.trsrc = std::make_unique<DevBuf>(ab);
    if (!L.tqueue) L.tqueue = std::make_unique<DevBuf>(sb);
    if (!L.troff->p || !L.trcur->p || !L.trsrc->p || !L.tqueue->p) return FST_OOM;
    t.roff = (uint32_t*)L.troff->p;
    t.rcur = (uint32_t*)L.trcur->p;
    t.rsrc = (uint32_t*)L.trsrc->p;
    t.queue = (uint32_t*)L.tqueue->p;
    if (launch_trim_linear(a, t, status, std::max<uint32_t>(1, std::min({handed, cus * 8, cap})),
                           stream) != hipSuccess)
      return FST_OOM;
    ++launches;
  }
  if (launch_trim_finalize(a, t, status, num, grid_wave, stream) != hipSuccess) return FST_OOM;
  ++launches;
  if (hipEventRecord(ev.e[1], stream) != hipSuccess ||
      !d2h(back.data(), L.tctr->p, 64, stream) || hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  drain.done = true;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) != hipSuccess) ms = 0.f;
  t_last_stats.kernel_ms += ms;
  t_last_stats.launches += launches;
  if (std::getenv("FSTAMD_ROUTE_LOG")) {
    unsigned long long tot[4];
    std::memcpy(tot, back.data(), sizeof(tot));
    std::fprintf(stderr,
                 "[libfst_amd route] lattice trim: items %u | sweep %u linear %u | states %llu -> "
                 "%llu arcs %llu -> %llu | %.3f ms\n",
                 back[8 + kTrimCtrSweep] + back[8 + kTrimCtrLinear], back[8 + kTrimCtrSweep],
                 back[8 + kTrimCtrLinear], tot[0], tot[1], tot[2], tot[3], ms);
  }
  return FST_OK;
}

FstError run_connect_shard(Shard& S, const FstLhsBatch& L) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const hipStream_t stream = S.E.stream();
  const uint32_t num = S.s1 - S.s0;
  auto st = std::make_shared<LhsStaged>();
  auto Lt = std::make_unique<LatShard>();
  auto out = std::make_unique<DevOut>(num, 1);  // the statuses: every item is OK
  // every return drains the stream before the staged blocks and the arena's buffers go
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, nullptr, L, stream, st.get()); e != FST_OK) return e;
  Lt->item = std::make_unique<DevBuf>(num * sizeof(LatItem));
  Lt->tstart = std::make_unique<DevBuf>(num * 4ull);
  if (!out->ok() || !Lt->item->p || !Lt->tstart->p) return FST_OOM;
  // the arena is the staged batch itself, read in place (item i's arc offsets sit i words on)
  LatticeOutDev& a = Lt->arena;
  a.item = (LatItem*)Lt->item->p;
  a.fin = const_cast<double*>(st->g.final_w);
  a.aoff = const_cast<uint32_t*>(st->g.state_off);
  a.il = const_cast<uint32_t*>(st->g.arc_il);
  a.ol = const_cast<uint32_t*>(st->g.arc_ol);
  a.w = const_cast<double*>(st->g.arc_w);
  a.next = const_cast<uint32_t*>(st->g.arc_next);
  a.state_cap = st->num_states;
  a.arc_cap = st->num_arcs;
  Lt->connect = true;
  Lt->trim.aoff_skew = 1;
  if (launch_trim_stage(st->in.lhs_desc, num, a.item, out->v.status, (uint32_t*)Lt->tstart->p,
                        stream) != hipSuccess)
    return FST_OOM;
  LaunchStats ls;
  ls.engine = 11;
  ls.launches = 1;
  ls.grid = std::max<uint32_t>(1, std::min<uint32_t>(num, (uint32_t)S.E->num_cus() * 32));
  t_last_stats = ls;
  if (FstError e = trim_lattices(S.E, out->v.status, *Lt, num, stream); e != FST_OK) return e;
  drain.done = true;  // (trim_lattices synchronised it)
  Lt->input = std::move(st);
  S.lat = std::move(Lt);
  S.keep = std::move(out);
  return FST_OK;
}

FstError run_lattice_arena(DeviceEngine::Lease& E, DeviceFst& D, const ChainInput& in,
                           const GraphInput* lhs, uint32_t lattice_flags, uint64_t est_states,
                           uint64_t est_arcs, std::unique_ptr<LatShard>* lat,
                           std::unique_ptr<DevOut>* keep) {
  const hipStream_t stream = E.stream();
  const uint32_t num = in.num_strings;
  uint64_t cap[2] = {est_states, est_arcs};
  if (const char* e = std::getenv("FSTAMD_LATTICE_ARENA"))  // tests: the arena's first size
    if (*e) {
      char* end = nullptr;
      cap[0] = std::strtoull(e, &end, 10);
      cap[1] = end && *end == ',' ? std::strtoull(end + 1, nullptr, 10) : cap[0];
    }
  constexpr int kAttempts = 4;
  for (int attempt = 0; attempt < kAttempts; ++attempt) {
    for (uint64_t& c : cap) c = (std::max<uint64_t>(c, 4) + 3) & ~3ull;
    auto L = std::make_unique<LatShard>();
    auto out = std::make_unique<DevOut>(num, 1);  // statuses; no path is written
    L->item = std::make_unique<DevBuf>(num * sizeof(LatItem));
    L->afin = std::make_unique<DevBuf>(cap[0] * 8);
    L->aaoff = std::make_unique<DevBuf>(cap[0] * 4);
    L->ail = std::make_unique<DevBuf>(cap[1] * 4);
    L->aol = std::make_unique<DevBuf>(cap[1] * 4);
    L->anext = std::make_unique<DevBuf>(cap[1] * 4);
    L->aw = std::make_unique<DevBuf>(cap[1] * 8);
    L->cursor = std::make_unique<DevBuf>(16);
    if (!out->ok() || !L->item->p || !L->afin->p || !L->aaoff->p || !L->ail->p || !L->aol->p ||
        !L->anext->p || !L->aw->p || !L->cursor->p)
      return FST_OOM;
    LatticeOutDev& a = L->arena;
    a.item = (LatItem*)L->item->p;
    a.fin = (double*)L->afin->p;
    a.aoff = (uint32_t*)L->aaoff->p;
    a.il = (uint32_t*)L->ail->p;
    a.ol = (uint32_t*)L->aol->p;
    a.next = (uint32_t*)L->anext->p;
    a.w = (double*)L->aw->p;
    a.state_cap = cap[0];
    a.arc_cap = cap[1];
    a.cursor = (unsigned long long*)L->cursor->p;
    a.project = (lattice_flags & FST_LATTICE_PROJECT_OUTPUT) ? 1u : 0u;
    PinnedVec<int32_t> status(num);
    unsigned long long need[2] = {0, 0};
    // a failure drains the stream before the arena and the read-back targets above go
    StreamDrain drain{{stream}};
    LaunchStats st;
    LhsRoute route;
    hipError_t err = E->run_lattice_batch(D, in, lhs, a, out->v, stream, &st, &route);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    if (t_prof) {
      t_prof->lap(2);
      ++t_prof->runs;
    }
    if (err != hipSuccess) {
      std::fprintf(stderr, "[libfst_amd] lattice batch engine failed: %s\n",
                   hipGetErrorString(err));
      return FST_OOM;
    }
    t_last_stats = st;
    if (!d2h(status.data(), out->v.status, num * 4ull, stream) ||
        !d2h(need, a.cursor, sizeof(need), stream) || hipStreamSynchronize(stream) != hipSuccess)
      return FST_OOM;
    drain.done = true;
    bool full = false;
    for (uint32_t i = 0; i < num; ++i) full |= status[i] == kPathOutputFull;
    // the last attempt's result stands: items still OUTPUT_FULL keep that status
    if (!full || attempt + 1 == kAttempts) {
      if (lattice_flags & FST_LATTICE_CONNECT) {
        L->connect = true;
        if (FstError e = trim_lattices(E, out->v.status, *L, num, stream); e != FST_OK) return e;
      }
      *lat = std::move(L);
      *keep = std::move(out);
      return FST_OK;
    }
    // every item reserves with atomicAdd before it checks the capacities, so the cursors end
    // at what the items that reached the emission need: one rerun suffices
    cap[0] = std::max<uint64_t>(cap[0], need[0]);
    cap[1] = std::max<uint64_t>(cap[1], need[1]);
  }
  return FST_OOM;  // unreachable: the last attempt returns above
}

FstError run_lattice_chain_shard(Shard& S, FrozenFst& b, const uint32_t* labels,
                                 const uint64_t* offsets, uint32_t lattice_flags) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b.device(dev);
  if (!D) return FST_OOM;
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  std::vector<uint64_t> rebased;
  const uint32_t max_len = rebase_offsets(offsets, num, &rebased);
  const uint64_t total = rebased[num];
  DevBuf lab(total * 4), off((num + 1ull) * 8);
  if (!lab.p || !off.p) return FST_OOM;
  // every return drains the stream before the inputs go back to the pool
  StreamDrain drain{{stream}};
  if (total && hipMemcpyAsync(lab.p, labels + offsets[0], total * 4, hipMemcpyHostToDevice,
                              stream) != hipSuccess)
    return FST_OOM;
  if (hipMemcpyAsync(off.p, rebased.data(), (num + 1ull) * 8, hipMemcpyHostToDevice, stream) !=
      hipSuccess)
    return FST_OOM;
  if (t_prof) t_prof->lap(0);
  ChainInput in{{(const uint32_t*)lab.p}, (const uint64_t*)off.p, num, max_len};
  // a guess (8 tuples per label, 2 arcs per tuple); the cursors correct it in one rerun
  const uint64_t est = 8 * (total + num) + 4ull * num + 1024;
  return run_lattice_arena(S.E, *D, in, nullptr, lattice_flags, est, 2 * est, &S.lat, &S.keep);
}

FstError run_lattice_lhs_shard(Shard& S, FrozenFst& b, const FstLhsBatch& L,
                               uint32_t lattice_flags) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b.device(dev);
  if (!D) return FST_OOM;
  const hipStream_t stream = S.E.stream();
  LhsStaged st;
  StreamDrain drain{{stream}};  // (as run_lhs_shard)
  if (FstError e = stage_lhs_items(S, D, L, stream, &st); e != FST_OK) return e;
  const uint64_t est = 8 * (st.num_states + st.num_arcs + (S.s1 - S.s0)) + 1024;
  return run_lattice_arena(S.E, *D, st.in, &st.g, lattice_flags, est, 2 * est, &S.lat, &S.keep);
}

// One shard of a pipeline on a general first stage: stage 1 is run_lhs_shard as it stands,
// then the chain stages from its finished outputs (the projection step of
// run_pipeline_stages); S.keep = the last stage's outputs, S.fail = the first failing stage.
FstError run_lhs_pipeline_shard(Shard& S, const Stages& fs, const FstLhsBatch& L, uint32_t n,
                                int semantics) {
  if (FstError e = run_lhs_shard(S, *fs[0], L, n, semantics); e != FST_OK) return e;
  if (fs.size() == 1) return FST_OK;
  if (!S.keep) return FST_OOM;  // run_arena sets it on FST_OK
  HostPaths h;  // (the statuses of each stage)
  // every failure return drains the stream before h, S.fail and the stages' buffers go
  StreamDrain drain{{S.E.stream()}};
  FstError e = clear_stage_failures(S);
  if (e == FST_OK) e = run_stages_after(S, fs, 1, n, semantics, &h);
  drain.done = e == FST_OK;  // (the last stage synchronised it)
  return e;
}

}  // namespace fstamd::host

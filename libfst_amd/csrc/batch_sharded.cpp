// batch_sharded.cpp -- host batches of chains through the path arena: one engine run with arena
// growth (run_arena, which batch_lhs.cpp uses too), the shards of a call (run_sharded) with the
// label and text sinks, the pipelined one-device batch, and the chain shards' compute steps
// (pipeline stages, text).  General lhs, the lattice batch and its sink: batch_lhs.cpp.
#include "host_rt.hpp"

namespace fstamd::host {

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

namespace {

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
  const uint32_t num = (S.s1 - S.s0) * S.per;
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
  const uint32_t first = S.s0 * S.per, num = (S.s1 - S.s0) * S.per;
  return d2h(out->status + first, S.st->p, num * 4ull, stream) &&
         d2h(out->final_weights + first, S.fin->p, num * 8ull, stream) &&
         d2h(out->path_offsets + first, S.off->p, num * 8ull, stream) &&
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
    for (uint32_t i = S.s0 * S.per; i < S.s1 * S.per; ++i) out->path_offsets[i] += arc_base;
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

// ---- Aligned text results (fst_normalize_text_aligned_batch) ---------------------------
// shard_text, then the last stage's (b, e) at the text offsets (the text's bytes and the
// projected symbols are one sequence) composed through the running map of the stages before
// it (S.align: empty for one stage, whose own map is the result).
FstError shard_text_aligned(Shard& S) {
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
  S.in_begin = std::make_unique<DevBuf>(std::max<uint64_t>(S.tot, 1) * 4);
  S.in_end = std::make_unique<DevBuf>(std::max<uint64_t>(S.tot, 1) * 4);
  DevBuf consumed(num * 4ull);
  if (!S.text->p || !S.in_begin->p || !S.in_end->p || !consumed.p) return FST_OOM;
  // every return below waits for the stream before `consumed`, the arena and the running map
  // go back to the pool
  StreamDrain drain{{stream}};
  uint32_t* b = (uint32_t*)S.in_begin->p;
  uint32_t* e = (uint32_t*)S.in_end->p;
  if (S.E->text_write(o.v, num, (const int32_t*)S.st->p, (const uint64_t*)S.off->p,
                      (uint8_t*)S.text->p, S.tot, stream) != hipSuccess ||
      S.E->align_write(o.v, num, (const uint64_t*)S.off->p, b, e, S.tot, (uint32_t*)consumed.p,
                       stream) != hipSuccess)
    return FST_OOM;
  const AlignMap& run = *S.align;
  if (run.b && S.E->align_compose(num, (const uint64_t*)S.off->p, b, e,
                                  (const uint64_t*)run.off->p, (const uint32_t*)run.b->p,
                                  (const uint32_t*)run.e->p, (const uint32_t*)run.n1->p, b, e,
                                  S.tot, stream) != hipSuccess)
    return FST_OOM;
  // (synchronised: the download may run on another engine's stream)
  if (hipStreamSynchronize(stream) != hipSuccess) return FST_OOM;
  drain.done = true;
  S.align.reset();
  S.keep.reset();  // the path arena is not downloaded
  return FST_OK;
}

// The text's four arrays, and the two maps at the shard's first byte: their indices are per
// string, so nothing is rebased.
FstError shard_text_aligned_download(Shard& S, FstAlignedTextResult* out, uint64_t byte_base) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  if (!(d2h(out->status + S.s0, S.st->p, num * 4ull, stream) &&
        d2h(out->total_weight + S.s0, S.fin->p, num * 8ull, stream) &&
        d2h(out->text_offsets + S.s0, S.off->p, num * 8ull, stream) &&
        d2h(out->text + byte_base, S.text->p, S.tot, stream) &&
        d2h(out->in_begin + byte_base, S.in_begin->p, S.tot * 4, stream) &&
        d2h(out->in_end + byte_base, S.in_end->p, S.tot * 4, stream)) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  if (byte_base)
    for (uint32_t i = S.s0; i < S.s1; ++i) out->text_offsets[i] += byte_base;
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

}  // namespace

FstError clear_stage_failures(Shard& S) {
  const uint32_t num_strings = S.s1 - S.s0;
  S.fail = std::make_unique<DevBuf>(num_strings * 4ull);  // first failing stage per string
  if (!S.fail->p ||
      hipMemsetAsync(S.fail->p, 0, num_strings * 4ull, S.E.stream()) != hipSuccess)
    return FST_OOM;
  return FST_OK;
}

namespace {

// The aligned text entry between two stages: the finished stage's (b, e, N) at its projection
// offsets `off` (`total` symbols), composed into the running map S.align, which it replaces.
// Synchronises the shard's stream on every return past the allocations: the stage that follows
// hands the arena these kernels read back to the pool, and so does this with the map it replaces.
FstError align_projected(Shard& S, const DevBuf& off, uint64_t total) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  AlignMap& run = *S.align;
  AlignMap next;
  next.off = std::make_unique<DevBuf>((num + 1ull) * 8);
  next.b = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1) * 4);
  next.e = std::make_unique<DevBuf>(std::max<uint64_t>(total, 1) * 4);
  next.n1 = std::make_unique<DevBuf>(num * 4ull);
  if (!next.off->p || !next.b->p || !next.e->p || !next.n1->p) return FST_OOM;
  StreamDrain drain{{stream}};  // (declared after `next`: its blocks outlive the kernels)
  uint32_t* nb = (uint32_t*)next.b->p;
  uint32_t* ne = (uint32_t*)next.e->p;
  if (hipMemcpyAsync(next.off->p, off.p, (num + 1ull) * 8, hipMemcpyDeviceToDevice, stream) !=
          hipSuccess ||
      S.E->align_write(S.keep->v, num, (const uint64_t*)off.p, nb, ne, total,
                       (uint32_t*)next.n1->p, stream) != hipSuccess)
    return FST_OOM;
  if (run.b) {
    if (S.E->align_compose(num, (const uint64_t*)off.p, nb, ne, (const uint64_t*)run.off->p,
                           (const uint32_t*)run.b->p, (const uint32_t*)run.e->p,
                           (const uint32_t*)run.n1->p, nb, ne, total, stream) != hipSuccess)
      return FST_OOM;
    next.n1.swap(run.n1);  // n1 stays stage 1's
  }
  if (hipStreamSynchronize(stream) != hipSuccess) return FST_OOM;
  drain.done = true;
  run = std::move(next);  // (the map it replaces goes back to the pool: nothing reads it now)
  return FST_OK;
}

}  // namespace

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
    // (before the stage resets S.keep: the map reads the finished stage's arena)
    if (S.align)
      if (FstError e = align_projected(S, off, in_total); e != FST_OK) return e;
    if (t_prof) t_prof->lap(4);
    // (the stage synchronises the stream before lab and off go back to the pool)
    if (FstError e = run_chain_stage(S, *fs[k], lab, off, in_total, max_len, n, semantics, h);
        e != FST_OK)
      return e;
    drain.done = true;
  }
  return FST_OK;
}

namespace {

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

bool alloc_aligned_text_result(FstAlignedTextResult* out, uint32_t num, uint64_t tot) {
  out->num_strings = num;
  out->total_bytes = tot;
  out->status = (int32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
  out->text_offsets = (uint64_t*)pin_alloc((num + 1ull) * 8);
  out->total_weight = (double*)pin_alloc(std::max<size_t>(num, 1) * 8);
  out->text = (uint8_t*)pin_alloc(std::max<uint64_t>(tot, 1));
  out->in_begin = (uint32_t*)pin_alloc(std::max<uint64_t>(tot, 1) * 4);
  out->in_end = (uint32_t*)pin_alloc(std::max<uint64_t>(tot, 1) * 4);
  return out->status && out->text_offsets && out->total_weight && out->text && out->in_begin &&
         out->in_end;
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
                     FstBatchResult* out, uint32_t per) {
  const uint32_t strings = num * per;
  const ShardSink sink{shard_compact,
                       [=](uint64_t tot, uint64_t) { return alloc_result(out, strings, tot); },
                       [=](Shard& S, uint64_t base, uint64_t) {
                         return shard_download(S, out, base);
                       },
                       [=](uint64_t tot, uint64_t) { out->path_offsets[strings] = tot; }};
  if (per == 1) return run_sharded(devices, nsh, num, cost, compute, sink);
  return run_sharded(
      devices, nsh, num, cost,
      [&](Shard& S) {
        S.per = per;
        return compute(S);
      },
      sink);
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

FstError run_sharded(const std::vector<int>& devices, uint32_t nsh, uint32_t num,
                     const std::vector<double>& cost, const ShardCompute& compute,
                     FstAlignedTextResult* out) {
  const ShardSink sink{shard_text_aligned,
                       [=](uint64_t tot, uint64_t) {
                         return alloc_aligned_text_result(out, num, tot);
                       },
                       [=](Shard& S, uint64_t base, uint64_t) {
                         return shard_text_aligned_download(S, out, base);
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
    ChainInput in{{(const uint32_t*)d_lab.p}, (const uint64_t*)d_off.p + S.s0, S.s1 - S.s0, ml};
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

FstError upload_chain(const void* data, size_t elem, const uint64_t* offsets, uint32_t num,
                      hipStream_t stream, ChainUpload* u) {
  u->max_len = rebase_offsets(offsets, num, &u->rebased);
  u->total = u->rebased[num];
  u->data = std::make_unique<DevBuf>(u->total * elem);
  u->off = std::make_unique<DevBuf>((num + 1ull) * 8);
  if (!u->data->p || !u->off->p) return FST_OOM;
  if (u->total && hipMemcpyAsync(u->data->p, (const uint8_t*)data + offsets[0] * elem,
                                 u->total * elem, hipMemcpyHostToDevice, stream) != hipSuccess)
    return FST_OOM;
  if (hipMemcpyAsync(u->off->p, u->rebased.data(), (num + 1ull) * 8, hipMemcpyHostToDevice,
                     stream) != hipSuccess)
    return FST_OOM;
  return FST_OK;
}

// One shard of a pipeline: every stage on the shard's device, each stage's 1-best output tape
// projected into the next stage's inputs on the device; S.keep = the last stage's outputs,
// S.fail = the first failing stage per string.
FstError run_pipeline_shard(Shard& S, const Stages& fs, const uint32_t* labels,
                            const uint64_t* offsets, uint32_t n, int semantics) {
  ChainUpload u;  // stage-1 inputs
  if (FstError e = upload_chain(labels, 4, offsets, S.s1 - S.s0, S.E.stream(), &u); e != FST_OK)
    return e;
  if (t_prof) t_prof->lap(0);
  return run_pipeline_stages(S, fs, std::move(u.data), std::move(u.off), u.total, u.max_len, n,
                             semantics);
}

// The text entry's shard: the bytes and their offsets go up as they are, the device widens
// them to stage-1 labels (DeviceEngine::widen_text), then the same stages.
FstError run_text_shard(Shard& S, const Stages& fs, const uint8_t* text, const uint64_t* offsets,
                        int semantics) {
  const uint32_t num_strings = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  // u.data (the bytes) is read by the widen kernel only; it and u.rebased live until the first
  // stage has synchronised the stream, and every failure drains the stream before they go
  ChainUpload u;
  std::unique_ptr<DevBuf> lab;
  StreamDrain drain{{stream}};
  if (FstError e = upload_chain(text, 1, offsets, num_strings, stream, &u); e != FST_OK) return e;
  lab = std::make_unique<DevBuf>(u.total * 4);
  if (!lab->p) return FST_OOM;
  if (S.E->widen_text((const uint8_t*)u.data->p, (const uint64_t*)u.off->p, num_strings,
                      (uint32_t*)lab->p, stream) != hipSuccess)
    return FST_OOM;
  if (t_prof) t_prof->lap(0);
  const FstError e = run_pipeline_stages(S, fs, std::move(lab), std::move(u.off), u.total,
                                         u.max_len, 1, semantics);
  drain.done = e == FST_OK;  // (run_chain_batch_dev synchronised it)
  return e;
}

}  // namespace fstamd::host

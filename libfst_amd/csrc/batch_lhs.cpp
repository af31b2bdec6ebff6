// batch_lhs.cpp -- host batches of general lhs (lattices, confusion networks) and the lattice
// batch: the staging of a shard's items into one block (stage_lhs_items), the shard steps on it
// (1-best, pipelines on a general first stage, shortest path, n-best, posteriors, connect, prune),
// the lattice
// arena with its reruns, the trim and prune drivers, the two lattice shard steps, and the lattice
// sink of run_sharded.
// run_arena, run_sharded itself and the chain stages: batch_sharded.cpp.
#include <cmath>

#include "host_rt.hpp"

namespace fstamd::host {

// The items of one shard (items [i0, i1) of the caller's batch) staged into one pinned block --
// descriptors, per-state arc offsets local to the item, finals, the four arc arrays, the two
// eager item lists -- and uploaded with one DMA.  The 1-best shard (run_lhs_shard) and the
// lattice shard (run_lattice_lhs_shard) share it.
namespace {
struct LhsStaged {
  std::unique_ptr<DevBuf> blk;
  PinnedVec<uint8_t> hin;
  LhsBatchDev b;  // (pointers into blk)
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
    uint32_t fl = lhs_base_flags(D);  // (no rhs: connect, which reads no flag; shortest path)
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
  LhsBatchDev& b = st->b;
  b.in.lhs_desc = (const LhsDesc*)(p + o_desc);
  b.in.num_strings = num;
  GraphInput& g = b.lhs;
  g.state_off = (const uint32_t*)(p + o_soff);
  g.final_w = (const double*)(p + o_fin);
  g.arc_w = (const double*)(p + o_w);
  g.arc_il = (const uint32_t*)(p + o_il);
  g.arc_ol = (const uint32_t*)(p + o_ol);
  g.arc_next = (const uint32_t*)(p + o_nx);
  g.start = kNoState;
  g.max_outdeg = max_outdeg;
  b.items_nonneg = (const uint32_t*)(p + o_la);
  b.items_replay = (const uint32_t*)(p + o_lb);
  b.num_nonneg = n_a;
  b.num_replay = n_b;
  b.total_states = ns;
  b.total_arcs = na;
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
      stream, S.s1 - S.s0, std::max<uint64_t>(4 * st.b.total_arcs + 16, 1024),
      "lhs batch engine failed", false,
      [&](const BatchOutDev& v, LaunchStats* ls) {
        return S.E->run_lhs_batch(*D, st.b, n, semantics, v, stream, ls, nullptr);
      },
      &h, &S.keep);
}

namespace {
// The shard step of the two entries that reduce the staged items to paths with no compose: `run`
// is an engine call that reads the staged block in place and synchronises the stream; `per`
// strings per item.  A path of theirs has fewer arcs than its item has states (a longer
// back-pointer walk is a cycle; an n-best item is acyclic), so an arena of `per` times the
// shard's states is never too small: no OUTPUT_FULL, no rerun.
template <class Run>
FstError staged_paths_shard(Shard& S, const FstLhsBatch& L, uint32_t per, const char* failed,
                            const Run& run) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const hipStream_t stream = S.E.stream();
  const uint32_t num = S.s1 - S.s0;
  LhsStaged st;
  // every return drains the stream before the staged blocks and the arena go back to their pools
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, nullptr, L, stream, &st); e != FST_OK) return e;
  auto out = std::make_unique<DevOut>(num * per, std::max<uint64_t>(st.b.total_states * per, 1));
  if (!out->ok()) return FST_OOM;
  if (t_prof) t_prof->lap(1);
  LaunchStats ls;
  const hipError_t err = run(st.b, out->v, stream, &ls);
  if (t_prof) {
    t_prof->lap(2);
    ++t_prof->runs;
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "[libfst_amd] %s failed: %s\n", failed, hipGetErrorString(err));
    return FST_OOM;
  }
  t_last_stats = ls;
  S.keep = std::move(out);
  return FST_OK;  // (the drain: `run` synchronised, nothing is left to wait for)
}
}  // namespace

// One shard of fst_shortest_path_lhs_batch: the staged items through DeviceEngine::run_sp_batch.
FstError run_sp_shard(Shard& S, const FstLhsBatch& L, uint32_t n) {
  return staged_paths_shard(
      S, L, 1, "lattice shortest path",
      [&](const LhsBatchDev& b, const BatchOutDev& v, hipStream_t stream, LaunchStats* ls) {
        return S.E->run_sp_batch(b, n, v, stream, ls, nullptr);
      });
}

// One shard of fst_nbest_lhs_batch, with `unique` of fst_nbest_unique_lhs_batch: the same
// through DeviceEngine::run_nbest_batch, n strings per item (run_sharded's `per`).
FstError run_nbest_shard(Shard& S, const FstLhsBatch& L, uint32_t n, bool unique) {
  return staged_paths_shard(
      S, L, n, unique ? "lattice n-best (unique)" : "lattice n-best",
      [&](const LhsBatchDev& b, const BatchOutDev& v, hipStream_t stream, LaunchStats* ls) {
        return S.E->run_nbest_batch(b, n, unique, v, stream, ls, nullptr);
      });
}

// One shard of fst_posterior_lhs_batch: the staged items through
// DeviceEngine::run_posterior_batch, which reads the staged block in place and synchronises the
// stream.  S.keep holds the statuses and, as its final weights, the totals; S.w the shard's
// alpha, beta (S.tot states each) and arc costs (S.tot2 arcs), in the shard's own order.
FstError run_posterior_shard(Shard& S, const FstLhsBatch& L) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const hipStream_t stream = S.E.stream();
  const uint32_t num = S.s1 - S.s0;
  LhsStaged st;
  // every return drains the stream before the staged blocks and the outputs go back to their pools
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, nullptr, L, stream, &st); e != FST_OK) return e;
  const uint64_t ns = st.b.total_states, na = st.b.total_arcs;
  auto out = std::make_unique<DevOut>(num, 1);
  auto vals = std::make_unique<DevBuf>((2 * ns + na + 2) * 8);
  if (!out->ok() || !vals->p) return FST_OOM;
  if (t_prof) t_prof->lap(1);
  LatPostDev v{};
  v.status = out->v.status;
  v.total = out->v.final_w;
  v.alpha = (double*)vals->p;
  v.beta = v.alpha + ns;
  v.arc_cost = v.beta + ns;
  LaunchStats ls;
  const hipError_t err = S.E->run_posterior_batch(st.b, v, stream, &ls, nullptr);
  if (t_prof) {
    t_prof->lap(2);
    ++t_prof->runs;
  }
  if (err != hipSuccess) {
    std::fprintf(stderr, "[libfst_amd] lattice posterior failed: %s\n", hipGetErrorString(err));
    return FST_OOM;
  }
  t_last_stats = ls;
  S.keep = std::move(out);
  S.w = std::move(vals);
  S.tot = ns;
  S.tot2 = na;
  return FST_OK;  // (the drain: the engine synchronised, nothing is left to wait for)
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
                       hipStream_t stream, unsigned long long* totals) {
  if (totals) std::memset(totals, 0, 4 * sizeof(*totals));
  if (num == 0) return FST_OK;
  const LatticeOutDev& a = L.arena.v;
  LatShard::Trim& W = L.trim;
  const bool access = W.start != nullptr;
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
  W.mark = std::make_unique<DevBuf>(sb);
  W.list = std::make_unique<DevBuf>(num * 4ull);
  W.ctr = std::make_unique<DevBuf>(64);
  if (access) W.queue = std::make_unique<DevBuf>(sb);
  if (!W.mark->p || !W.list->p || !W.ctr->p || (access && !W.queue->p)) return FST_OOM;
  // every return drains the stream before the workspace (and the caller's arena) can go
  StreamDrain drain{{stream}};
  LatTrimDev& t = W.v;
  t.mark = (uint32_t*)W.mark->p;
  t.queue = access ? (uint32_t*)W.queue->p : nullptr;
  t.roff = t.rcur = t.rsrc = nullptr;
  t.list = (uint32_t*)W.list->p;
  t.tot = (unsigned long long*)W.ctr->p;
  t.ctr = (uint32_t*)((uint8_t*)W.ctr->p + 32);
  t.start = access ? (const uint32_t*)W.start->p : nullptr;
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
  if (hipMemsetAsync(W.ctr->p, 0, 64, stream) != hipSuccess ||
      hipEventRecord(ev.e[0], stream) != hipSuccess)
    return FST_OOM;
  if (access) {
    if (launch_trim_access(a, t, status, num, grid_wg, stream) != hipSuccess) return FST_OOM;
    ++launches;
  }
  if (launch_trim_sweep(a, t, status, num, grid_wave, stream) != hipSuccess) return FST_OOM;
  ++launches;
  PinnedVec<uint32_t> back(16);  // tot[4] as 8 words, then ctr
  if (!d2h(back.data(), W.ctr->p, 64, stream) || hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  const uint32_t handed = back[8 + kTrimCtrList];
  if (handed > num) return FST_OOM;  // (a bug: the list holds an item at most once)
  if (handed) {
    W.roff = std::make_unique<DevBuf>(sb);
    W.rcur = std::make_unique<DevBuf>(sb);
    W.rsrc = std::make_unique<DevBuf>(ab);
    if (!W.queue) W.queue = std::make_unique<DevBuf>(sb);
    if (!W.roff->p || !W.rcur->p || !W.rsrc->p || !W.queue->p) return FST_OOM;
    t.roff = (uint32_t*)W.roff->p;
    t.rcur = (uint32_t*)W.rcur->p;
    t.rsrc = (uint32_t*)W.rsrc->p;
    t.queue = (uint32_t*)W.queue->p;
    if (launch_trim_linear(a, t, status, std::max<uint32_t>(1, std::min({handed, cus * 8, cap})),
                           stream) != hipSuccess)
      return FST_OOM;
    ++launches;
  }
  if (launch_trim_finalize(a, t, status, num, grid_wave, stream) != hipSuccess) return FST_OOM;
  ++launches;
  if (hipEventRecord(ev.e[1], stream) != hipSuccess ||
      !d2h(back.data(), W.ctr->p, 64, stream) || hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  drain.done = true;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) != hipSuccess) ms = 0.f;
  t_last_stats.kernel_ms += ms;
  t_last_stats.launches += launches;
  if (totals) std::memcpy(totals, back.data(), 4 * sizeof(*totals));
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
  Lt->arena.item = std::make_unique<DevBuf>(num * sizeof(LatItem));
  Lt->trim.start = std::make_unique<DevBuf>(num * 4ull);
  if (!out->ok() || !Lt->arena.item->p || !Lt->trim.start->p) return FST_OOM;
  // the arena is the staged batch itself, read in place (item i's arc offsets sit i words on)
  const GraphInput& g = st->b.lhs;
  LatticeOutDev& a = Lt->arena.v;
  a.item = (LatItem*)Lt->arena.item->p;
  a.fin = const_cast<double*>(g.final_w);
  a.aoff = const_cast<uint32_t*>(g.state_off);
  a.il = const_cast<uint32_t*>(g.arc_il);
  a.ol = const_cast<uint32_t*>(g.arc_ol);
  a.w = const_cast<double*>(g.arc_w);
  a.next = const_cast<uint32_t*>(g.arc_next);
  a.state_cap = st->b.total_states;
  a.arc_cap = st->b.total_arcs;
  Lt->connect = true;
  Lt->trim.v.aoff_skew = 1;
  if (launch_trim_stage(st->b.in.lhs_desc, num, a.item, out->v.status,
                        (uint32_t*)Lt->trim.start->p, stream) != hipSuccess)
    return FST_OOM;
  LaunchStats ls;
  ls.engine = 11;
  ls.launches = 1;
  ls.grid = std::max<uint32_t>(1, std::min<uint32_t>(num, (uint32_t)S.E->num_cus() * 32));
  t_last_stats = ls;
  if (FstError e = trim_lattices(S.E, out->v.status, *Lt, num, stream); e != FST_OK) return e;
  drain.done = true;  // (trim_lattices synchronised it)
  Lt->arena.input = std::move(st);
  S.lat = std::move(Lt);
  S.keep = std::move(out);
  return FST_OK;
}

// ---- Lattice prune (beam) -----------------------------------------------------------------

FstError prune_lattices(DeviceEngine::Lease& E, const LhsBatchDev& b, double beam,
                        uint32_t prep_launches, hipStream_t stream,
                        std::unique_ptr<LatShard>* lat, std::unique_ptr<DevOut>* keep) {
  const uint32_t num = b.in.num_strings;
  auto Lt = std::make_unique<LatShard>();
  auto out = std::make_unique<DevOut>(num, 1);  // the statuses
  // every return drains the stream before the shadow arrays and the trim's workspace go
  StreamDrain drain{{stream}};
  Lt->arena.item = std::make_unique<DevBuf>(std::max<size_t>(num, 1) * sizeof(LatItem));
  Lt->arena.fin = std::make_unique<DevBuf>((b.total_states + 4) * 8);
  Lt->arena.next = std::make_unique<DevBuf>((b.total_arcs + 4) * 4);
  Lt->trim.start = std::make_unique<DevBuf>(std::max<size_t>(num, 1) * 4ull);
  if (!out->ok() || !Lt->arena.item->p || !Lt->arena.fin->p || !Lt->arena.next->p ||
      !Lt->trim.start->p)
    return FST_OOM;
  // the arena is the batch itself, read in place (item i's arc offsets sit i words on), with
  // the mark pass's finals and targets in place of its own
  const GraphInput& g = b.lhs;
  LatticeOutDev& a = Lt->arena.v;
  a.item = (LatItem*)Lt->arena.item->p;
  a.fin = (double*)Lt->arena.fin->p;
  a.aoff = const_cast<uint32_t*>(g.state_off);
  a.il = const_cast<uint32_t*>(g.arc_il);
  a.ol = const_cast<uint32_t*>(g.arc_ol);
  a.w = const_cast<double*>(g.arc_w);
  a.next = (uint32_t*)Lt->arena.next->p;
  a.state_cap = b.total_states;
  a.arc_cap = b.total_arcs;
  Lt->connect = true;
  Lt->trim.v.aoff_skew = 1;
  LatPruneDev v{};
  v.item = a.item;
  v.status = out->v.status;
  v.start = (uint32_t*)Lt->trim.start->p;
  v.sfin = a.fin;
  v.snext = a.next;
  LaunchStats ls;
  LhsRoute route;
  const hipError_t err = E->run_prune_batch(b, beam, v, stream, &ls, &route);
  if (err != hipSuccess) {
    std::fprintf(stderr, "[libfst_amd] lattice prune failed: %s\n", hipGetErrorString(err));
    return FST_OOM;
  }
  ls.launches += prep_launches;
  t_last_stats = ls;
  unsigned long long tot[4];
  if (FstError e = trim_lattices(E, out->v.status, *Lt, num, stream, tot); e != FST_OK) return e;
  drain.done = true;  // (trim_lattices synchronised it)
  if (std::getenv("FSTAMD_ROUTE_LOG"))
    std::fprintf(stderr,
                 "[libfst_amd route] lattice prune: items %u | wave %u frontier %u | states %llu -> "
                 "%llu arcs %llu -> %llu | %.3f ms\n",
                 num, route.t[0], route.t[1], tot[0], tot[1], tot[2], tot[3],
                 t_last_stats.kernel_ms);
  *lat = std::move(Lt);
  *keep = std::move(out);
  return FST_OK;
}

FstError run_prune_shard(Shard& S, const FstLhsBatch& L, double beam) {
  const int dev = S.E->dev();
  if (hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  const hipStream_t stream = S.E.stream();
  auto st = std::make_shared<LhsStaged>();
  // every return drains the stream before the staged blocks go
  StreamDrain drain{{stream}};
  if (FstError e = stage_lhs_items(S, nullptr, L, stream, st.get()); e != FST_OK) return e;
  if (FstError e = prune_lattices(S.E, st->b, beam, 0, stream, &S.lat, &S.keep); e != FST_OK)
    return e;
  drain.done = true;  // (prune_lattices synchronised it)
  S.lat->arena.input = std::move(st);
  return FST_OK;
}

bool LatShard::Arena::alloc(uint32_t num, uint64_t state_cap, uint64_t arc_cap) {
  item = std::make_unique<DevBuf>(num * sizeof(LatItem));
  fin = std::make_unique<DevBuf>(state_cap * 8);
  aoff = std::make_unique<DevBuf>(state_cap * 4);
  il = std::make_unique<DevBuf>(arc_cap * 4);
  ol = std::make_unique<DevBuf>(arc_cap * 4);
  next = std::make_unique<DevBuf>(arc_cap * 4);
  w = std::make_unique<DevBuf>(arc_cap * 8);
  cursor = std::make_unique<DevBuf>(16);
  v = LatticeOutDev{(LatItem*)item->p, (double*)fin->p,    (uint32_t*)aoff->p,
                    (uint32_t*)il->p,  (uint32_t*)ol->p,   (double*)w->p,
                    (uint32_t*)next->p, state_cap,         arc_cap,
                    (unsigned long long*)cursor->p, 0u};
  return v.item && v.fin && v.aoff && v.il && v.ol && v.w && v.next && v.cursor;
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
    if (!L->arena.alloc(num, cap[0], cap[1]) || !out->ok()) return FST_OOM;
    LatticeOutDev& a = L->arena.v;
    a.project = (lattice_flags & FST_LATTICE_PROJECT_OUTPUT) ? 1u : 0u;
    PinnedVec<int32_t> status(num);
    unsigned long long need[2] = {0, 0};
    // a failure drains the stream before the arena and the read-back targets above go
    StreamDrain drain{{stream}};
    LaunchStats st;
    hipError_t err = E->run_lattice_batch(D, in, lhs, a, out->v, stream, &st, nullptr);
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
  ChainUpload u;
  // every return drains the stream before the inputs go back to the pool
  StreamDrain drain{{stream}};
  if (FstError e = upload_chain(labels, 4, offsets, num, stream, &u); e != FST_OK) return e;
  if (t_prof) t_prof->lap(0);
  ChainInput in{{(const uint32_t*)u.data->p}, (const uint64_t*)u.off->p, num, u.max_len};
  // a guess (8 tuples per label, 2 arcs per tuple); the cursors correct it in one rerun
  const uint64_t est = 8 * (u.total + num) + 4ull * num + 1024;
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
  const uint64_t est = 8 * (st.b.total_states + st.b.total_arcs + (S.s1 - S.s0)) + 1024;
  return run_lattice_arena(S.E, *D, st.b.in, &st.b.lhs, lattice_flags, est, 2 * est, &S.lat, &S.keep);
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

namespace {
void* buf_ptr(const std::unique_ptr<DevBuf>& b) { return b ? b->p : nullptr; }
}  // namespace

LatticeCsrDev LatShard::Csr::view(uint64_t state_cap, uint64_t arc_cap) const {
  return LatticeCsrDev{(int32_t*)buf_ptr(status), (uint64_t*)buf_ptr(soff), (uint32_t*)buf_ptr(start),
                       (double*)buf_ptr(fin),     (uint64_t*)buf_ptr(aoffs), (uint32_t*)buf_ptr(il),
                       (uint32_t*)buf_ptr(ol),    (double*)buf_ptr(w),       (uint32_t*)buf_ptr(next),
                       state_cap,                 arc_cap};
}

namespace {

// ---- Lattice results (fst_compose_frozen_batch) ----------------------------------------
// The lattice sink's compaction: count and scan (the totals come back), the shard's arrays in
// FstLhsBatch's layout sized from them, then the gather; the arena goes back to the pool.
FstError shard_lattice_compact(Shard& S) {
  if (!S.lat) return FST_OOM;
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  LatShard& Ls = *S.lat;
  LatShard::Csr& C = Ls.csr;
  const LatticeOutDev& arena = Ls.arena.v;
  // a failure drains the stream before the shard's buffers go back to the pool
  StreamDrain drain{{stream}};
  C.status = std::make_unique<DevBuf>(num * 4ull);
  C.soff = std::make_unique<DevBuf>((num + 1ull) * 8);
  C.start = std::make_unique<DevBuf>(num * 4ull);
  if (!C.status->p || !C.soff->p || !C.start->p) return FST_OOM;
  uint64_t needed[2] = {0, 0};
  if (S.E->compact_lattices_count(S.keep->v.status, arena, num, C.view(0, 0), needed, stream) !=
      hipSuccess)
    return FST_OOM;
  // an engine bug: OK items own more than the arena holds
  if (needed[0] > arena.state_cap || needed[1] > arena.arc_cap) return FST_OOM;
  C.fin = std::make_unique<DevBuf>(needed[0] * 8);
  C.aoffs = std::make_unique<DevBuf>((needed[0] + 1) * 8);
  C.il = std::make_unique<DevBuf>(needed[1] * 4);
  C.ol = std::make_unique<DevBuf>(needed[1] * 4);
  C.next = std::make_unique<DevBuf>(needed[1] * 4);
  C.w = std::make_unique<DevBuf>(needed[1] * 8);
  if (!C.fin->p || !C.aoffs->p || !C.il->p || !C.ol->p || !C.next->p || !C.w->p) return FST_OOM;
  // (synchronised: the download may run on another engine's stream)
  if (S.E->compact_lattices(arena, num, C.view(needed[0], needed[1]), stream,
                            Ls.connect ? &Ls.trim.v : nullptr) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  drain.done = true;
  Ls.trim.release();
  Ls.arena.release();
  S.tot = needed[0];
  S.tot2 = needed[1];
  return FST_OK;
}

// D2H of a compacted lattice shard at its item range, its first state and its first arc; the
// two offset arrays are then moved by those bases (the closing entries: the sink's finish).
FstError shard_lattice_download(Shard& S, FstLatticeBatch* out, uint64_t sbase, uint64_t abase) {
  const uint32_t num = S.s1 - S.s0;
  const hipStream_t stream = S.E.stream();
  const LatShard::Csr& C = S.lat->csr;
  const FstLhsBatch& F = out->fsts;
  uint64_t* soff = const_cast<uint64_t*>(F.state_offsets);
  uint64_t* aoff = const_cast<uint64_t*>(F.arc_offsets);
  if (!(d2h(out->status + S.s0, C.status->p, num * 4ull, stream) &&
        d2h(const_cast<uint32_t*>(F.start) + S.s0, C.start->p, num * 4ull, stream) &&
        d2h(soff + S.s0, C.soff->p, num * 8ull, stream) &&
        d2h(const_cast<double*>(F.final_weights) + sbase, C.fin->p, S.tot * 8, stream) &&
        d2h(aoff + sbase, C.aoffs->p, S.tot * 8, stream) &&
        d2h(const_cast<uint32_t*>(F.ilabels) + abase, C.il->p, S.tot2 * 4, stream) &&
        d2h(const_cast<uint32_t*>(F.olabels) + abase, C.ol->p, S.tot2 * 4, stream) &&
        d2h(const_cast<uint32_t*>(F.nextstates) + abase, C.next->p, S.tot2 * 4, stream) &&
        d2h(const_cast<double*>(F.weights) + abase, C.w->p, S.tot2 * 8, stream)) ||
      hipStreamSynchronize(stream) != hipSuccess)
    return FST_OOM;
  if (sbase)
    for (uint32_t i = S.s0; i < S.s1; ++i) soff[i] += sbase;
  if (abase)
    for (uint64_t s = sbase; s < sbase + S.tot; ++s) aoff[s] += abase;
  return FST_OK;
}

}  // namespace

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

}  // namespace fstamd::host

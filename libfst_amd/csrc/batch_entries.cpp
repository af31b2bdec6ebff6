// batch_entries.cpp -- the fst_batch.h C ABI: argument checks, the choice of route (streamed,
// pipelined, sharded), the device-side entries.  (fst_debug_coalescer_state: c_api.cpp.)

#include <algorithm>
#include <cmath>

#include "host_rt.hpp"
#include "posterior_gather.hpp"
#include "weight_codes.hpp"

using namespace fstamd;
using namespace fstamd::host;

namespace {

bool flags_ok(const FstBatchOptions* opts) { return !opts || !(opts->flags & ~FST_BATCH_DEVICES); }

bool offsets_monotone(const uint64_t* offsets, uint32_t num) {
  for (uint32_t i = 0; i < num; ++i)
    if (offsets[i + 1] < offsets[i]) return false;
  return true;
}

bool stream_enabled() {  // FSTAMD_STREAM=0 turns the streamed routes off
  const char* se = std::getenv("FSTAMD_STREAM");
  return !(se && std::strcmp(se, "0") == 0);
}

// The devices and shard count of a host batch call (FstBatchOptions, fst_batch.h).
FstError batch_devices(const FstBatchOptions* opts, std::vector<int>* devices, uint32_t* nsh) {
  devices->clear();
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FST_INVALID_ARG;
  if (opts && (opts->flags & FST_BATCH_DEVICES) && opts->device_mask) {
    for (int d = 0; d < 64; ++d)
      if (opts->device_mask >> d & 1) {
        if (d >= count) return FST_INVALID_ARG;
        devices->push_back(d);
      }
  } else {
    int dev = opts ? opts->device : -1;
    if (dev < 0) dev = current_device();
    if (dev < 0 || dev >= count) return FST_INVALID_ARG;
    devices->push_back(dev);
  }
  *nsh = (uint32_t)devices->size();
  if (opts && (opts->flags & FST_BATCH_DEVICES) && opts->num_shards)
    *nsh = std::max<uint32_t>(opts->num_shards, 1);
  return FST_OK;
}

// A host batch entry after its argument checks: open() needs a GPU, reads the options and
// starts the profile (t_prof, until the entry returns); close() frees the result or prints it.
struct BatchCall {
  int semantics = FST_SEM_LAZY;
  std::vector<int> devices;
  uint32_t nsh = 1;
  HostProf prof;
  FstError open(const FstBatchOptions* opts) {
    if (!gpu_available()) return FST_INVALID_ARG;
    semantics = opts ? (int)opts->semantics : FST_SEM_LAZY;
    if (FstError e = batch_devices(opts, &devices, &nsh); e != FST_OK) return e;
    prof = HostProf();
    t_prof = &prof;
    return FST_OK;
  }
  template <class R>
  FstError close(FstError e, const char* name, R* out, void (*release)(R*)) {
    if (e != FST_OK) {
      release(out);
      return e;
    }
    prof.lap(5);
    prof.print(name);
    return FST_OK;
  }
  ~BatchCall() {
    if (t_prof == &prof) t_prof = nullptr;
  }
};

// run_sharded's costs: the first stage's work (later stages' inputs are not known yet)
std::vector<double> chain_costs(const FrozenFst& b, const uint64_t* offsets, uint32_t num,
                                uint32_t nsh) {
  std::vector<double> cost(nsh > 1 ? num : 0);
  for (size_t i = 0; i < cost.size(); ++i) cost[i] = b.chain_cost(offsets[i + 1] - offsets[i]);
  return cost;
}

// The engine of a device-side entry: leased on the current device, working on the caller's
// stream `*s`.  Empty without a GPU, a current device or an engine.
DeviceEngine::Lease current_engine(void* stream, hipStream_t* s) {
  DeviceEngine::Lease E;
  const int dev = gpu_available() ? current_device() : -1;
  if (dev >= 0) E = DeviceEngine::acquire(dev);
  if (E) *s = E.use((hipStream_t)stream);
  return E;
}

BatchOutDev dev_out(const FstDeviceBatch* o) {
  return BatchOutDev{o->status,  o->path_len, o->path_offset,  o->final_weight,
                     o->ilabels, o->olabels,  o->weights,      o->arc_capacity,
                     (unsigned long long*)o->arc_cursor, o->work};
}

// A frozen FST from its blob (len >= sizeof(Header)), in one of the two semirings of
// weight.zig (fst.zig:43-47); null otherwise.
std::shared_ptr<FrozenFst> frozen_from_bytes(const uint8_t* bytes, uint64_t len) {
  Header h;
  std::memcpy(&h, bytes, sizeof(h));
  if (h.weight_type != kWeightTropical && h.weight_type != kWeightLog) return nullptr;
  return FrozenFst::from_bytes(bytes, len, h.weight_type, nullptr);
}

// The argument checks of the lhs batch entry, on the host alone.
bool lhs_batch_valid(const FstLhsBatch* L) {
  if (!L) return false;
  const uint32_t num = L->num_fsts;
  if (num == 0) return true;
  if (!L->state_offsets || !L->start || !L->arc_offsets) return false;
  // (the sizes first, from the state offsets alone: nothing below reads 2^30 states)
  for (uint32_t i = 0; i < num; ++i) {
    if (L->state_offsets[i + 1] < L->state_offsets[i]) return false;
    if (L->state_offsets[i + 1] - L->state_offsets[i] >= (1ull << 30)) return false;
  }
  if (L->arc_offsets[0] != 0) return false;
  const uint64_t s_end = L->state_offsets[num];
  if (s_end && !L->final_weights) return false;
  for (uint64_t s = 0; s < s_end; ++s)
    if (L->arc_offsets[s + 1] < L->arc_offsets[s]) return false;
  if (L->arc_offsets[s_end] && (!L->ilabels || !L->olabels || !L->weights || !L->nextstates))
    return false;
  for (uint32_t i = 0; i < num; ++i) {
    const uint64_t s0 = L->state_offsets[i], s1 = L->state_offsets[i + 1];
    const uint64_t ns = s1 - s0, a0 = L->arc_offsets[s0], a1 = L->arc_offsets[s1];
    // bfs_key holds s1 in 30 bits; the item's arc offsets are u32 on the device
    if (ns >= (1ull << 30) || a1 - a0 >= (1ull << 32)) return false;
    if (L->start[i] != FST_NO_STATE && L->start[i] >= ns) return false;
    for (uint64_t a = a0; a < a1; ++a)
      if (L->nextstates[a] >= ns) return false;
  }
  return true;
}

// The empty OK result of a batch of no items.
FstError empty_result(FstBatchResult* out) {
  if (!alloc_result(out, 0, 0)) {
    fst_batch_result_free(out);
    return FST_OOM;
  }
  out->path_offsets[0] = 0;
  return FST_OK;
}
FstError empty_result(FstTextResult* out) {
  if (!alloc_text_result(out, 0, 0)) {
    fst_text_result_free(out);
    return FST_OOM;
  }
  out->text_offsets[0] = 0;
  return FST_OK;
}

FstError empty_result(FstAlignedTextResult* out) {
  if (!alloc_aligned_text_result(out, 0, 0)) {
    fst_aligned_text_result_free(out);
    return FST_OOM;
  }
  out->text_offsets[0] = 0;
  return FST_OK;
}

// ... of the lattice entries: no item, state_offsets = {0}, arc_offsets = {0}.
FstError empty_result(FstLatticeBatch* out) {
  if (!alloc_lattice_result(out, 0, 0, 0)) {
    fst_lattice_batch_free(out);
    return FST_OOM;
  }
  const_cast<uint64_t*>(out->fsts.state_offsets)[0] = 0;
  const_cast<uint64_t*>(out->fsts.arc_offsets)[0] = 0;
  return FST_OK;
}
// The n of the two n-best entries: 1 .. FST_NBEST_MAX, and num * n result strings index in 32 bits.
bool nbest_slots_ok(uint32_t num, uint32_t n) {
  return n >= 1 && n <= FST_NBEST_MAX && (uint64_t)num * n < (1ull << 32);
}
bool lattice_flags_ok(uint32_t f) {
  return !(f & ~(FST_LATTICE_PROJECT_OUTPUT | FST_LATTICE_CONNECT));  // (bit 1 stays unknown)
}

// run_sharded's costs of a batch of general lhs: arcs + 1 per item.
std::vector<double> lhs_costs(const FstLhsBatch& lhs, uint32_t nsh) {
  std::vector<double> cost(nsh > 1 ? lhs.num_fsts : 0);
  for (size_t i = 0; i < cost.size(); ++i)
    cost[i] = (double)(lhs.arc_offsets[lhs.state_offsets[i + 1]] -
                       lhs.arc_offsets[lhs.state_offsets[i]]) + 1.0;
  return cost;
}

// A checked batch of general lhs in shards balanced by lhs_costs: `shard` computes one (it gets
// the call for its semantics) into a label, text or lattice result.  The empty batch is its OK
// result before any GPU check.  `any_semantics`: the entry never looks at opts->semantics.
// `per`: strings per item of a label result (fst_nbest_lhs_batch's n).
template <class R, class F>
FstError lhs_sharded(const FstLhsBatch* lhs, const FstBatchOptions* opts, bool any_semantics,
                     R* out, const char* name, void (*release)(R*), const F& shard,
                     uint32_t per = 1) {
  if (lhs->num_fsts == 0) return empty_result(out);
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  if (!any_semantics && call.semantics != FST_SEM_LAZY && call.semantics != FST_SEM_EAGER)
    return FST_INVALID_ARG;
  const std::vector<double> cost = lhs_costs(*lhs, call.nsh);
  const auto compute = [&](Shard& S) { return shard(S, call); };
  FstError e;
  if constexpr (std::is_same_v<R, FstBatchResult>)
    e = run_sharded(call.devices, call.nsh, lhs->num_fsts, cost, compute, out, per);
  else
    e = run_sharded(call.devices, call.nsh, lhs->num_fsts, cost, compute, out);
  return call.close(e, name, out, release);
}

// ... through `fs` (one stage: the lhs batch entry; several: stage 1 on the lhs, then chain
// stages on the 1-best output tapes).
template <class R>
FstError lhs_stages_impl(const Stages& fs, const FstLhsBatch* lhs, uint32_t n,
                         const FstBatchOptions* opts, R* out, const char* name,
                         void (*release)(R*)) {
  return lhs_sharded(lhs, opts, false, out, name, release, [&](Shard& S, const BatchCall& call) {
    return run_lhs_pipeline_shard(S, fs, *lhs, n, call.semantics);
  });
}

FstError lhs_batch_impl(FstHandle b_handle, const FstLhsBatch* lhs, uint32_t n,
                        const FstBatchOptions* opts, FstBatchResult* out) {
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  return lhs_stages_impl(Stages{b}, lhs, n, opts, out,
                         "fst_compose_frozen_shortest_path_lhs_batch", fst_batch_result_free);
}

// The stage handles of a pipeline entry, pinned; false: none, or a stale one.
bool get_stages(const FstHandle* stages, uint32_t num_stages, Stages* fs) {
  if (!stages || num_stages == 0) return false;
  fs->resize(num_stages);
  for (uint32_t k = 0; k < num_stages; ++k)
    if (!((*fs)[k] = frozen_get(stages[k]))) return false;
  return true;
}

// The argument checks of the two lhs pipeline entries (`out` checked and zeroed before): the
// lhs batch entry's, plus the stages.
bool lhs_pipeline_args(const FstHandle* stages, uint32_t num_stages, const FstLhsBatch* lhs,
                       const FstBatchOptions* opts, Stages* fs) {
  return lhs_batch_valid(lhs) && flags_ok(opts) && get_stages(stages, num_stages, fs);
}

// The prepare kernel's inputs for a device-resident lhs batch: the caller's device pointers and
// the two extents of their arrays (the last state offset, the last arc offset), which the host
// reads and trusts (fst_batch.h); the prepare kernel checks every other offset against them.
FstError device_lhs_extents(const FstLhsBatch* d_lhs, hipStream_t s, LhsPrepIn* in) {
  const uint32_t num = d_lhs->num_fsts;
  in->num = num;
  in->state_offsets = d_lhs->state_offsets;
  in->start = d_lhs->start;
  in->final_w = d_lhs->final_weights;
  in->arc_offsets = d_lhs->arc_offsets;
  in->arc_ol = d_lhs->olabels;
  in->arc_w = d_lhs->weights;
  in->arc_next = d_lhs->nextstates;
  if (num) {
    if (!read_u64(&in->total_states, d_lhs->state_offsets + num, s)) return FST_OOM;
    if (!read_u64(&in->total_arcs, d_lhs->arc_offsets + in->total_states, s)) return FST_OOM;
  }
  if ((in->total_states && !d_lhs->final_weights) ||
      (in->total_arcs &&
       (!d_lhs->ilabels || !d_lhs->olabels || !d_lhs->weights || !d_lhs->nextstates)))
    return FST_INVALID_ARG;
  return FST_OK;
}

// The frame of a device-side entry after its argument checks: the caller's device given back
// when the entry returns, the device of `opts` (or the current one) made current, the rhs on it
// (when there is one), an engine leased onto the caller's stream, and the drain: every return
// waits for what the call queued, so the engine's workspaces are its own again.  The members
// stand in the order the entries used to declare them; what the drain must outlive it
// (fst_device_compose_frozen's arena) is declared before the frame.
struct DeviceCall {
  DeviceRestore_ restore;
  int dev = -1;
  DeviceFst* D = nullptr;
  DeviceEngine::Lease E;
  hipStream_t s = nullptr;
  StreamDrain drain{{nullptr}, true};
  FstError open(const FstBatchOptions* opts, FrozenFst* b, void* stream) {
    if (!gpu_available()) return FST_INVALID_ARG;
    dev = opts && opts->device >= 0 ? opts->device : current_device();
    if (dev < 0 || hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
    if (b && !(D = b->device(dev))) return FST_OOM;
    E = DeviceEngine::acquire(dev);
    if (!E) return FST_INVALID_ARG;
    drain.s[0] = s = E.use((hipStream_t)stream);
    drain.done = false;
    return FST_OK;
  }
};

// The argument checks the two device-resident lhs entries share.
bool device_lhs_args_ok(const FstLhsBatch* d_lhs) {
  return d_lhs &&
         (!d_lhs->num_fsts || (d_lhs->state_offsets && d_lhs->start && d_lhs->arc_offsets));
}
bool device_batch_out_ok(const FstDeviceBatch* o, uint32_t num) {
  return o && o->arc_cursor &&
         (!num || (o->status && o->path_len && o->path_offset && o->final_weight));
}

// ... and their preparation: the extents, then the prepare kernel (the rhs's flags with c.D).
FstError device_lhs_prepare(DeviceCall& c, const FstLhsBatch* d_lhs, LhsBatchDev* batch,
                            LhsPrepared* p) {
  LhsPrepIn in{};
  if (FstError e = device_lhs_extents(d_lhs, c.s, &in); e != FST_OK) return e;
  return c.E->prepare_lhs(c.D, in, d_lhs->ilabels, c.s, batch, p) == hipSuccess ? FST_OK
                                                                               : FST_OOM;
}

}  // namespace

extern "C" {

FstError fst_compose_frozen_shortest_path_batch(FstHandle b_handle, const uint32_t* labels,
                                                const uint64_t* offsets, uint32_t num_strings,
                                                uint32_t n, const FstBatchOptions* opts,
                                                FstBatchResult* out) {
  if (!out || !offsets || (!labels && num_strings && offsets[num_strings] != offsets[0]))
    return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(offsets, num_strings) || !flags_ok(opts)) return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const int semantics = call.semantics;
  // an rhs without input epsilons and a pull tier first: the streamed batch, on one device
  // or sharded over several
  if (num_strings > 0 && stream_enabled()) {
    StreamIo io;
    io.labels = labels;
    io.out = out;
    const int e =
        run_streamed(call.devices, call.nsh, *b, io, offsets, num_strings, n, semantics);
    if (e != kStreamNotApplicable)
      return call.close((FstError)e, "fst_compose_frozen_shortest_path_batch (streamed)", out,
                        fst_batch_result_free);
  }
  // one device and a large batch on an rhs without input epsilons: pipelined sub-shards
  // (FSTAMD_PIPELINE=0 keeps the one-shard path; FSTAMD_PIPELINE=k forces k sub-shards)
  const char* pe = std::getenv("FSTAMD_PIPELINE");
  const int want = pe && *pe ? std::atoi(pe) : -1;
  uint32_t parts =
      want > 0 ? (uint32_t)want : (uint32_t)std::min<uint64_t>(8, num_strings / (1u << 17));
  parts = std::min<uint32_t>(parts, std::max<uint32_t>(num_strings, 1));
  const bool single = call.devices.size() == 1 && call.nsh == 1;
  if (single && want != 0 && parts >= 2) {
    // (before hipSetDevice: every path out of this block gives the caller its device back)
    DeviceRestore_ restore;
    const int dev = call.devices[0];
    DeviceFst* D = nullptr;
    if (hipSetDevice(dev) == hipSuccess) D = b->device(dev);
    if (D && !D->has_eps)
      return call.close(
          run_pipelined(dev, *b, labels, offsets, num_strings, n, semantics, parts, out),
          "fst_compose_frozen_shortest_path_batch (pipelined)", out, fst_batch_result_free);
  }
  const FstError e = run_sharded(
      call.devices, call.nsh, num_strings, chain_costs(*b, offsets, num_strings, call.nsh),
      [&](Shard& S) {
        HostPaths h;
        return run_chain_batch_host(S.E, *b, labels, offsets + S.s0, S.s1 - S.s0, n, semantics,
                                    &h, &S.keep);
      },
      out);
  return call.close(e, "fst_compose_frozen_shortest_path_batch", out, fst_batch_result_free);
}

void fst_batch_result_free(FstBatchResult* r) {
  if (!r) return;
  pin_release(r->status);
  pin_release(r->path_offsets);
  pin_release(r->ilabels);
  pin_release(r->olabels);
  pin_release(r->weights);
  pin_release(r->final_weights);
  std::memset(r, 0, sizeof(*r));
}

// ---- Batch of general lhs (lattices, confusion networks, n-best unions) ----------------

FstError fst_compose_frozen_shortest_path_lhs_batch(FstHandle b_handle, const FstLhsBatch* lhs,
                                                    uint32_t n, const FstBatchOptions* opts,
                                                    FstBatchResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!lhs_batch_valid(lhs) || !flags_ok(opts)) return FST_INVALID_ARG;
  return lhs_batch_impl(b_handle, lhs, n, opts, out);
}

FstError fst_compose_frozen_shortest_path_handles_batch(FstHandle b_handle,
                                                        const FstMutableHandle* a, uint32_t num,
                                                        uint32_t n, const FstBatchOptions* opts,
                                                        FstBatchResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if ((num && !a) || !flags_ok(opts)) return FST_INVALID_ARG;
  // each lhs flattened to CSR under its own lock (the single call's snapshot, c-api.zig:754)
  std::vector<uint64_t> state_offsets(num + 1, 0), arc_offsets(1, 0);
  std::vector<uint32_t> start(num), il, ol, nx;
  std::vector<double> fin, w;
  for (uint32_t i = 0; i < num; ++i) {
    const MutableRead r = mutable_read(a[i]);
    const MutableFst* m = r.fst;
    if (!m) return FST_INVALID_ARG;
    const uint32_t ns = (uint32_t)m->num_states();
    start[i] = m->start();
    state_offsets[i + 1] = state_offsets[i] + ns;
    for (uint32_t s = 0; s < ns; ++s) {
      fin.push_back(m->final_weight(s));
      for (const Arc& x : m->arcs(s)) {
        il.push_back(x.ilabel);
        ol.push_back(x.olabel);
        w.push_back(x.weight);
        nx.push_back(x.nextstate);
      }
      arc_offsets.push_back(il.size());
    }
  }
  const FstLhsBatch L{num,       state_offsets.data(), start.data(), fin.data(), arc_offsets.data(),
                      il.data(), ol.data(),            w.data(),     nx.data()};
  if (!lhs_batch_valid(&L)) return FST_INVALID_ARG;
  return lhs_batch_impl(b_handle, &L, n, opts, out);
}

FstError fst_pipeline_lhs_batch(const FstHandle* stages, uint32_t num_stages,
                                const FstLhsBatch* lhs, uint32_t n, const FstBatchOptions* opts,
                                FstBatchResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  Stages fs;
  if (!lhs_pipeline_args(stages, num_stages, lhs, opts, &fs)) return FST_INVALID_ARG;
  return lhs_stages_impl(fs, lhs, n, opts, out, "fst_pipeline_lhs_batch", fst_batch_result_free);
}

FstError fst_normalize_lhs_batch(const FstHandle* stages, uint32_t num_stages,
                                 const FstLhsBatch* lhs, const FstBatchOptions* opts,
                                 FstTextResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  Stages fs;
  if (!lhs_pipeline_args(stages, num_stages, lhs, opts, &fs)) return FST_INVALID_ARG;
  return lhs_stages_impl(fs, lhs, 1, opts, out, "fst_normalize_lhs_batch", fst_text_result_free);
}

// ---- Lattices out (fst_compose_frozen for a batch) -------------------------------------

FstError fst_compose_frozen_batch(FstHandle b_handle, const uint32_t* labels,
                                  const uint64_t* offsets, uint32_t num_strings,
                                  uint32_t lattice_flags, const FstBatchOptions* opts,
                                  FstLatticeBatch* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets || (!labels && num_strings && offsets[num_strings] != offsets[0]))
    return FST_INVALID_ARG;
  if (!offsets_monotone(offsets, num_strings) || !flags_ok(opts) ||
      !lattice_flags_ok(lattice_flags))
    return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  if (num_strings == 0) return empty_result(out);
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const FstError e = run_sharded(
      call.devices, call.nsh, num_strings, chain_costs(*b, offsets, num_strings, call.nsh),
      [&](Shard& S) {
        return run_lattice_chain_shard(S, *b, labels, offsets + S.s0, lattice_flags);
      },
      out);
  return call.close(e, "fst_compose_frozen_batch", out, fst_lattice_batch_free);
}

FstError fst_compose_frozen_lhs_batch(FstHandle b_handle, const FstLhsBatch* lhs,
                                      uint32_t lattice_flags, const FstBatchOptions* opts,
                                      FstLatticeBatch* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!lhs_batch_valid(lhs) || !flags_ok(opts) || !lattice_flags_ok(lattice_flags))
    return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  return lhs_sharded(lhs, opts, true, out, "fst_compose_frozen_lhs_batch", fst_lattice_batch_free,
                     [&](Shard& S, const BatchCall&) {
                       return run_lattice_lhs_shard(S, *b, *lhs, lattice_flags);
                     });
}

// Connect of every item of an lhs batch: no rhs, no engine ladder; the items are staged as the
// lhs entries stage them and trimmed in place of a compose (run_connect_shard).
FstError fst_connect_lhs_batch(const FstLhsBatch* lhs, const FstBatchOptions* opts,
                               FstLatticeBatch* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!lhs_batch_valid(lhs) || !flags_ok(opts)) return FST_INVALID_ARG;
  return lhs_sharded(lhs, opts, true, out, "fst_connect_lhs_batch", fst_lattice_batch_free,
                     [&](Shard& S, const BatchCall&) { return run_connect_shard(S, *lhs); });
}

// Beam pruning of every item of an lhs batch: staged as connect stages them, then the cut and the
// trim on a shadow of the staged items (run_prune_shard).
FstError fst_prune_lhs_batch(const FstLhsBatch* lhs, double beam, const FstBatchOptions* opts,
                             FstLatticeBatch* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  // (the beam before the validator, which reads lhs's arrays; !(beam >= 0): NaN too)
  if (!(beam >= 0.0) || !lhs_batch_valid(lhs) || !flags_ok(opts)) return FST_INVALID_ARG;
  return lhs_sharded(lhs, opts, true, out, "fst_prune_lhs_batch", fst_lattice_batch_free,
                     [&](Shard& S, const BatchCall&) { return run_prune_shard(S, *lhs, beam); });
}

// fst_shortest_path of every item of an lhs batch: no rhs, no compose; the items are staged as
// the lhs entries stage them and reduced to their 1-best paths in place (run_sp_shard).
FstError fst_shortest_path_lhs_batch(const FstLhsBatch* lhs, uint32_t n,
                                     const FstBatchOptions* opts, FstBatchResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!lhs_batch_valid(lhs) || !flags_ok(opts)) return FST_INVALID_ARG;
  return lhs_sharded(lhs, opts, true, out, "fst_shortest_path_lhs_batch", fst_batch_result_free,
                     [&](Shard& S, const BatchCall&) { return run_sp_shard(S, *lhs, n); });
}

// The n best distinct paths of every item of an lhs batch: staged as above, n strings per item
// (run_nbest_shard; the gather moves a shard's items [s0, s1) as strings [s0 * n, s1 * n)).
// unique: the n best paths of distinct output texts, the same frame.
static FstError nbest_lhs_entry(const FstLhsBatch* lhs, uint32_t n, bool unique,
                                const FstBatchOptions* opts, FstBatchResult* out,
                                const char* name) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  // (n and the slot count before the validator: it reads num_fsts entries of the arrays)
  if (!lhs || !nbest_slots_ok(lhs->num_fsts, n) || !lhs_batch_valid(lhs) || !flags_ok(opts))
    return FST_INVALID_ARG;
  return lhs_sharded(
      lhs, opts, true, out, name, fst_batch_result_free,
      [&](Shard& S, const BatchCall&) { return run_nbest_shard(S, *lhs, n, unique); }, n);
}

FstError fst_nbest_lhs_batch(const FstLhsBatch* lhs, uint32_t n, const FstBatchOptions* opts,
                             FstBatchResult* out) {
  return nbest_lhs_entry(lhs, n, false, opts, out, "fst_nbest_lhs_batch");
}

FstError fst_nbest_unique_lhs_batch(const FstLhsBatch* lhs, uint32_t n,
                                    const FstBatchOptions* opts, FstBatchResult* out) {
  return nbest_lhs_entry(lhs, n, true, opts, out, "fst_nbest_unique_lhs_batch");
}

// Arc posteriors of every item of an lhs batch: staged as above (run_posterior_shard).  The
// result is in the caller's own layout, so nothing is compacted: a shard's totals are its items'
// states and arcs, and its download puts the three value arrays at the offsets of its first item
// (posterior_gather.hpp, checked on its own by tools/posterior_gather_check.cpp).
FstError fst_posterior_lhs_batch(const FstLhsBatch* lhs, const FstBatchOptions* opts,
                                 FstPosteriorResult* out) {
  if (!out) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!lhs_batch_valid(lhs) || !flags_ok(opts)) return FST_INVALID_ARG;
  const uint32_t num = lhs->num_fsts;
  const uint64_t states = num ? lhs->state_offsets[num] : 0;
  const uint64_t arcs = num ? lhs->arc_offsets[states] : 0;
  const auto alloc = [=](uint64_t, uint64_t) {
    out->num_fsts = num;
    out->total_states = states;
    out->total_arcs = arcs;
    out->status = (int32_t*)pin_alloc(std::max<size_t>(num, 1) * 4);
    out->total = (double*)pin_alloc(std::max<size_t>(num, 1) * 8);
    out->alpha = (double*)pin_alloc(std::max<uint64_t>(states, 1) * 8);
    out->beta = (double*)pin_alloc(std::max<uint64_t>(states, 1) * 8);
    out->arc_cost = (double*)pin_alloc(std::max<uint64_t>(arcs, 1) * 8);
    if (!out->status || !out->total || !out->alpha || !out->beta || !out->arc_cost) return false;
    posterior_fill_front(lhs->state_offsets, lhs->arc_offsets, num, out->alpha, out->beta,
                         out->arc_cost);
    return true;
  };
  if (num == 0) {
    if (alloc(0, 0)) return FST_OK;
    fst_posterior_result_free(out);
    return FST_OOM;
  }
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const ShardSink sink{
      [](Shard&) { return FST_OK; }, alloc,
      [=](Shard& S, uint64_t, uint64_t) {
        const hipStream_t stream = S.E.stream();
        const PosteriorRanges r =
            posterior_shard_ranges(lhs->state_offsets, lhs->arc_offsets, S.s0, S.s1);
        if (r.ns != S.tot || r.na != S.tot2) return FST_OOM;  // (a bug: the shard staged these)
        const auto copy = [&](void* dst, const void* src, uint64_t bytes) {
          return d2h(dst, src, bytes, stream);
        };
        return posterior_gather_shard(r, S.s0, S.s1, (const int32_t*)S.keep->status.p,
                                      (const double*)S.keep->fin.p, (const double*)S.w->p,
                                      out->status, out->total, out->alpha, out->beta,
                                      out->arc_cost, copy) &&
                       hipStreamSynchronize(stream) == hipSuccess
                   ? FST_OK
                   : FST_OOM;
      },
      [](uint64_t, uint64_t) {}};
  const FstError e = run_sharded(
      call.devices, call.nsh, num, lhs_costs(*lhs, call.nsh),
      [&](Shard& S) { return run_posterior_shard(S, *lhs); }, sink);
  return call.close(e, "fst_posterior_lhs_batch", out, fst_posterior_result_free);
}

void fst_posterior_result_free(FstPosteriorResult* r) {
  if (!r) return;
  pin_release(r->status);
  pin_release(r->total);
  pin_release(r->alpha);
  pin_release(r->beta);
  pin_release(r->arc_cost);
  std::memset(r, 0, sizeof(*r));
}

// -log confidences of the strings of an n-best result: host arithmetic alone, no GPU.
FstError fst_batch_result_path_costs(const FstBatchResult* paths, uint32_t per,
                                     const double* total, uint32_t num_fsts, double* out) {
  if (!paths || !total || !out || per == 0 || (uint64_t)num_fsts * per != paths->num_strings)
    return FST_INVALID_ARG;
  for (uint32_t i = 0; i < num_fsts; ++i)
    for (uint32_t k = 0; k < per; ++k) {
      const uint64_t s = (uint64_t)i * per + k;
      double c = HUGE_VAL;
      if (paths->status[s] == FST_PATH_OK) {
        c = 0.0;
        for (uint64_t a = paths->path_offsets[s]; a < paths->path_offsets[s + 1]; ++a)
          c = c + paths->weights[a];
        c = (c + paths->final_weights[s]) - total[i];
      }
      out[s] = c;
    }
  return FST_OK;
}

void fst_lattice_batch_free(FstLatticeBatch* r) {
  if (!r) return;
  pin_release(r->status);
  pin_release(const_cast<uint64_t*>(r->fsts.state_offsets));
  pin_release(const_cast<uint32_t*>(r->fsts.start));
  pin_release(const_cast<double*>(r->fsts.final_weights));
  pin_release(const_cast<uint64_t*>(r->fsts.arc_offsets));
  pin_release(const_cast<uint32_t*>(r->fsts.ilabels));
  pin_release(const_cast<uint32_t*>(r->fsts.olabels));
  pin_release(const_cast<double*>(r->fsts.weights));
  pin_release(const_cast<uint32_t*>(r->fsts.nextstates));
  std::memset(r, 0, sizeof(*r));
}

// Chains in, lattices out, all on the device: the chain instances into an arena of the
// library's own (grown from the cursors as the host entry's), then the compaction straight
// into the caller's arrays when they hold the batch.
FstError fst_device_compose_frozen(FstHandle b_handle, const uint32_t* d_labels,
                                   const uint64_t* d_offsets, uint32_t num_strings,
                                   uint32_t max_len, uint32_t lattice_flags,
                                   const FstBatchOptions* opts, const FstDeviceLattices* o,
                                   uint64_t needed[2], void* stream) {
  if (!o || !needed || !d_offsets || !flags_ok(opts) || !lattice_flags_ok(lattice_flags))
    return FST_INVALID_ARG;
  if (!o->state_offsets || !o->arc_offsets || (num_strings && (!o->status || !o->start)))
    return FST_INVALID_ARG;
  if ((o->state_capacity && !o->final_weights) ||
      (o->arc_capacity && (!o->ilabels || !o->olabels || !o->weights || !o->nextstates)))
    return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  // the arena and the statuses are declared before the drain (the frame's), so they are
  // destroyed after it: every return waits for what the call queued (the gather reads the
  // arena) before those blocks go back to the pool
  std::unique_ptr<LatShard> lat;
  std::unique_ptr<DevOut> keep;
  DeviceCall call;
  if (FstError e = call.open(opts, b.get(), stream); e != FST_OK) return e;
  DeviceEngine::Lease& E = call.E;
  const hipStream_t s = call.s;
  needed[0] = needed[1] = 0;
  ChainInput in{{d_labels}, d_offsets, num_strings, max_len};
  uint64_t first = 0, last = 0;
  if (num_strings && (!read_u64(&first, d_offsets, s) || !read_u64(&last, d_offsets + num_strings, s)))
    return FST_OOM;
  if (last < first) return FST_INVALID_ARG;
  const uint64_t est = 8 * ((last - first) + num_strings) + 4ull * num_strings + 1024;
  if (FstError e = run_lattice_arena(E, *call.D, in, nullptr, lattice_flags, est, 2 * est, &lat, &keep);
      e != FST_OK)
    return e;
  const LatticeCsrDev csr{o->status,      o->state_offsets, o->start,   o->final_weights,
                          o->arc_offsets, o->ilabels,       o->olabels, o->weights,
                          o->nextstates,  o->state_capacity, o->arc_capacity};
  const LatticeOutDev& arena = lat->arena.v;
  if (E->compact_lattices_count(keep->v.status, arena, num_strings, csr, needed, s) != hipSuccess)
    return FST_OOM;
  if (needed[0] > arena.state_cap || needed[1] > arena.arc_cap) return FST_OOM;
  // too small: the statuses and `needed` stand, nothing else is written
  if (needed[0] > csr.state_cap || needed[1] > csr.arc_cap) return FST_OK;
  if (E->compact_lattices(arena, num_strings, csr, s, lat->connect ? &lat->trim.v : nullptr) !=
      hipSuccess)
    return FST_OOM;
  return FST_OK;  // (the drain waits for the gather, then `keep` and `lat` go)
}

// The device-resident form: d_lhs's arrays are device memory, used in place.  The host reads
// the two extents (the last state offset, the last arc offset) and nothing else of them; the
// prepare kernel (DeviceEngine::prepare_lhs) validates the items and derives what
// run_lhs_shard derives on the host, then the same engine runs.
FstError fst_device_compose_shortest_path_lhs(FstHandle b_handle, const FstLhsBatch* d_lhs,
                                              uint32_t n, const FstBatchOptions* opts,
                                              const FstDeviceBatch* o, void* stream) {
  if (!device_lhs_args_ok(d_lhs) || !device_batch_out_ok(o, d_lhs->num_fsts) || !flags_ok(opts))
    return FST_INVALID_ARG;
  const int semantics = opts ? (int)opts->semantics : FST_SEM_LAZY;
  if (semantics != FST_SEM_LAZY && semantics != FST_SEM_EAGER) return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  DeviceCall call;
  if (FstError e = call.open(opts, b.get(), stream); e != FST_OK) return e;
  LhsBatchDev batch;
  LhsPrepared p;
  if (FstError e = device_lhs_prepare(call, d_lhs, &batch, &p); e != FST_OK) return e;
  // the lazy per-pop table is 2 * deg + 2 entries
  if (batch.lhs.max_outdeg >= (1u << 30)) return FST_OOM;
  LaunchStats st;
  if (call.E->run_lhs_batch(*call.D, batch, n, semantics, dev_out(o), call.s, &st, nullptr) !=
      hipSuccess)
    return FST_OOM;
  st.launches += p.launches;
  t_last_stats = st;
  // (run_lhs_batch waited for its last tier: with stats it ends on an event of the stream;
  // an empty batch queued one memset, which the drain still waits for)
  call.drain.done = d_lhs->num_fsts != 0;
  return FST_OK;
}

// fst_shortest_path of a device-resident lhs batch: prepared as above but with no rhs (the
// items' flags are their own), then DeviceEngine::run_sp_batch into the caller's arena.
FstError fst_device_shortest_path_lhs(const FstLhsBatch* d_lhs, uint32_t n,
                                      const FstBatchOptions* opts, const FstDeviceBatch* o,
                                      void* stream) {
  if (!device_lhs_args_ok(d_lhs) || !device_batch_out_ok(o, d_lhs->num_fsts) || !flags_ok(opts))
    return FST_INVALID_ARG;
  DeviceCall call;
  if (FstError e = call.open(opts, nullptr, stream); e != FST_OK) return e;
  LhsBatchDev batch;
  LhsPrepared p;
  if (FstError e = device_lhs_prepare(call, d_lhs, &batch, &p); e != FST_OK) return e;
  LaunchStats st;
  if (call.E->run_sp_batch(batch, n, dev_out(o), call.s, &st, nullptr) != hipSuccess)
    return FST_OOM;
  st.launches += p.launches;
  t_last_stats = st;
  call.drain.done = true;  // (run_sp_batch synchronised the stream)
  return FST_OK;
}

// Beam pruning of a device-resident lhs batch: prepared like the shortest path's, the cut and the
// trim on a shadow of the caller's arrays (prune_lattices), then fst_device_compose_frozen's
// compaction straight into the caller's result when it holds the pruned batch.
FstError fst_device_prune_lhs(const FstLhsBatch* d_lhs, double beam, const FstBatchOptions* opts,
                              const FstDeviceLattices* o, uint64_t needed[2], void* stream) {
  if (!(beam >= 0.0) || !device_lhs_args_ok(d_lhs) || !o || !needed || !flags_ok(opts))
    return FST_INVALID_ARG;
  const uint32_t num = d_lhs->num_fsts;
  if (!o->state_offsets || !o->arc_offsets || (num && (!o->status || !o->start)))
    return FST_INVALID_ARG;
  if ((o->state_capacity && !o->final_weights) ||
      (o->arc_capacity && (!o->ilabels || !o->olabels || !o->weights || !o->nextstates)))
    return FST_INVALID_ARG;
  // (declared before the frame's drain, so destroyed after it: the gather reads them)
  std::unique_ptr<LatShard> lat;
  std::unique_ptr<DevOut> keep;
  DeviceCall call;
  if (FstError e = call.open(opts, nullptr, stream); e != FST_OK) return e;
  const hipStream_t s = call.s;
  needed[0] = needed[1] = 0;
  if (num == 0) {
    LaunchStats st;
    st.engine = 15;
    t_last_stats = st;
    return hipMemsetAsync(o->state_offsets, 0, 8, s) == hipSuccess &&
                   hipMemsetAsync(o->arc_offsets, 0, 8, s) == hipSuccess
               ? FST_OK
               : FST_OOM;
  }
  LhsBatchDev batch;
  LhsPrepared p;
  if (FstError e = device_lhs_prepare(call, d_lhs, &batch, &p); e != FST_OK) return e;
  if (FstError e = prune_lattices(call.E, batch, beam, p.launches, s, &lat, &keep); e != FST_OK)
    return e;
  const LatticeCsrDev csr{o->status,      o->state_offsets, o->start,   o->final_weights,
                          o->arc_offsets, o->ilabels,       o->olabels, o->weights,
                          o->nextstates,  o->state_capacity, o->arc_capacity};
  const LatticeOutDev& arena = lat->arena.v;
  if (call.E->compact_lattices_count(keep->v.status, arena, num, csr, needed, s) != hipSuccess)
    return FST_OOM;
  if (needed[0] > arena.state_cap || needed[1] > arena.arc_cap) return FST_OOM;
  // too small: the statuses and `needed` stand, nothing else is written
  if (needed[0] > csr.state_cap || needed[1] > csr.arc_cap) return FST_OK;
  if (call.E->compact_lattices(arena, num, csr, s, &lat->trim.v) != hipSuccess) return FST_OOM;
  return FST_OK;  // (the drain waits for the gather, then `keep` and `lat` go)
}

// The n best paths of a device-resident lhs batch: prepared like the shortest path's, then
// DeviceEngine::run_nbest_batch into the caller's arena, n strings per item.  unique: the n best
// paths of distinct output texts.
static FstError device_nbest_entry(const FstLhsBatch* d_lhs, uint32_t n, bool unique,
                                   const FstBatchOptions* opts, const FstDeviceBatch* o,
                                   void* stream) {
  if (!device_lhs_args_ok(d_lhs) || !device_batch_out_ok(o, d_lhs->num_fsts) || !flags_ok(opts) ||
      !nbest_slots_ok(d_lhs->num_fsts, n))
    return FST_INVALID_ARG;
  DeviceCall call;
  if (FstError e = call.open(opts, nullptr, stream); e != FST_OK) return e;
  LhsBatchDev batch;
  LhsPrepared p;
  if (FstError e = device_lhs_prepare(call, d_lhs, &batch, &p); e != FST_OK) return e;
  LaunchStats st;
  if (call.E->run_nbest_batch(batch, n, unique, dev_out(o), call.s, &st, nullptr) != hipSuccess)
    return FST_OOM;
  st.launches += p.launches;
  t_last_stats = st;
  call.drain.done = true;  // (run_nbest_batch synchronised the stream)
  return FST_OK;
}

FstError fst_device_nbest_lhs(const FstLhsBatch* d_lhs, uint32_t n, const FstBatchOptions* opts,
                              const FstDeviceBatch* o, void* stream) {
  return device_nbest_entry(d_lhs, n, false, opts, o, stream);
}

FstError fst_device_nbest_unique_lhs(const FstLhsBatch* d_lhs, uint32_t n,
                                     const FstBatchOptions* opts, const FstDeviceBatch* o,
                                     void* stream) {
  return device_nbest_entry(d_lhs, n, true, opts, o, stream);
}

// Arc posteriors of a device-resident lhs batch: prepared like the shortest path's, then
// DeviceEngine::run_posterior_batch straight into the caller's arrays, which are indexed by the
// items' own (global) bases.
FstError fst_device_posterior_lhs(const FstLhsBatch* d_lhs, const FstBatchOptions* opts,
                                  const FstDevicePosteriors* o, void* stream) {
  if (!device_lhs_args_ok(d_lhs) || !o || !flags_ok(opts)) return FST_INVALID_ARG;
  const uint32_t num = d_lhs->num_fsts;
  if (num && (!o->status || !o->total)) return FST_INVALID_ARG;
  DeviceCall call;
  if (FstError e = call.open(opts, nullptr, stream); e != FST_OK) return e;
  LaunchStats st;
  st.engine = 16;
  if (num == 0) {
    t_last_stats = st;
    call.drain.done = true;  // (nothing was queued)
    return FST_OK;
  }
  LhsBatchDev batch;
  LhsPrepared p;
  if (FstError e = device_lhs_prepare(call, d_lhs, &batch, &p); e != FST_OK) return e;
  if (batch.total_arcs && !o->arc_cost) return FST_INVALID_ARG;
  LatPostDev v{};
  v.status = o->status;
  v.total = o->total;
  v.alpha = o->alpha;
  v.beta = o->beta;
  v.arc_cost = o->arc_cost;
  if (call.E->run_posterior_batch(batch, v, call.s, &st, nullptr) != hipSuccess) return FST_OOM;
  st.launches += p.launches;
  t_last_stats = st;
  call.drain.done = true;  // (run_posterior_batch synchronised the stream)
  return FST_OK;
}

FstError fst_device_project_output(const FstDeviceBatch* o, uint32_t num_strings,
                                   uint32_t* d_next_labels, uint64_t* d_next_offsets,
                                   int32_t* d_proj_status, uint32_t* max_len, void* stream) {
  if (!o || !d_next_offsets || !d_proj_status || (num_strings && !d_next_labels))
    return FST_INVALID_ARG;
  uint32_t ml = 0;
  hipStream_t s = nullptr;
  DeviceEngine::Lease E = current_engine(stream, &s);
  if (!E) return FST_INVALID_ARG;
  if (E->project_output(dev_out(o), num_strings, d_next_labels, d_next_offsets, d_proj_status,
                        &ml, s) != hipSuccess)
    return FST_OOM;
  if (max_len) *max_len = ml;
  return FST_OK;
}

FstError fst_pipeline_batch(const FstHandle* stages, uint32_t num_stages, const uint32_t* labels,
                            const uint64_t* offsets, uint32_t num_strings, uint32_t n,
                            const FstBatchOptions* opts, FstBatchResult* out) {
  if (!out || !stages || num_stages == 0 || !offsets ||
      (!labels && num_strings && offsets[num_strings] != offsets[0]))
    return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(offsets, num_strings) || !flags_ok(opts)) return FST_INVALID_ARG;
  Stages fs;
  if (!get_stages(stages, num_stages, &fs)) return FST_INVALID_ARG;
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const FstError e = run_sharded(
      call.devices, call.nsh, num_strings, chain_costs(*fs[0], offsets, num_strings, call.nsh),
      [&](Shard& S) {
        return run_pipeline_shard(S, fs, labels, offsets + S.s0, n, call.semantics);
      },
      out);
  return call.close(e, "fst_pipeline_batch", out, fst_batch_result_free);
}

// ---- Text entries (fst_batch.h) ---------------------------------------------------------

FstError fst_normalize_text_batch(const FstHandle* stages, uint32_t num_stages,
                                  const uint8_t* text, const uint64_t* offsets,
                                  uint32_t num_strings, const FstBatchOptions* opts,
                                  FstTextResult* out) {
  if (!out || !stages || num_stages == 0 || !offsets ||
      (!text && num_strings && offsets[num_strings] != offsets[0]))
    return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(offsets, num_strings) || !flags_ok(opts)) return FST_INVALID_ARG;
  Stages fs;
  if (!get_stages(stages, num_stages, &fs)) return FST_INVALID_ARG;
  if (num_strings == 0) return empty_result(out);  // nothing to run
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const int semantics = call.semantics;
  // one stage on an rhs without input epsilons and a pull tier first: the streamed text
  // batch, on one device or sharded over several
  if (num_stages == 1 && stream_enabled()) {
    StreamIo io;
    io.text = text;
    io.tout = out;
    const int e =
        run_streamed(call.devices, call.nsh, *fs[0], io, offsets, num_strings, 1, semantics);
    if (e != kStreamNotApplicable)
      return call.close((FstError)e, "fst_normalize_text_batch (streamed)", out,
                        fst_text_result_free);
  }
  const FstError e = run_sharded(
      call.devices, call.nsh, num_strings, chain_costs(*fs[0], offsets, num_strings, call.nsh),
      [&](Shard& S) { return run_text_shard(S, fs, text, offsets + S.s0, semantics); }, out);
  return call.close(e, "fst_normalize_text_batch", out, fst_text_result_free);
}

void fst_text_result_free(FstTextResult* r) {
  if (!r) return;
  pin_release(r->status);
  pin_release(r->text_offsets);
  pin_release(r->text);
  pin_release(r->total_weight);
  std::memset(r, 0, sizeof(*r));
}

FstError fst_device_compile_text(const uint8_t* d_text, const uint64_t* d_offsets,
                                 uint32_t num_strings, uint32_t* d_labels, void* stream) {
  if (!d_offsets) return FST_INVALID_ARG;
  hipStream_t s = nullptr;
  DeviceEngine::Lease E = current_engine(stream, &s);
  if (!E) return FST_INVALID_ARG;
  return E->widen_text(d_text, d_offsets, num_strings, d_labels, s) == hipSuccess ? FST_OK
                                                                                 : FST_OOM;
}

FstError fst_device_emit_text(const FstDeviceBatch* o, uint32_t num_strings, uint8_t* d_text,
                              uint64_t text_capacity, uint64_t* d_text_offsets,
                              int32_t* d_status, double* d_total_weight, uint64_t* total_bytes,
                              void* stream) {
  if (!o || !d_text_offsets || !d_status || !d_total_weight || (text_capacity && !d_text))
    return FST_INVALID_ARG;
  const BatchOutDev v = dev_out(o);
  hipStream_t s = nullptr;
  DeviceEngine::Lease E = current_engine(stream, &s);
  if (!E) return FST_INVALID_ARG;
  uint64_t tot = 0;
  if (E->text_count(v, num_strings, nullptr, d_status, d_text_offsets, d_total_weight, &tot, s) !=
          hipSuccess ||
      E->text_write(v, num_strings, d_status, d_text_offsets, d_text, text_capacity, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return FST_OOM;
  if (total_bytes) *total_bytes = tot;
  return FST_OK;
}

FstError fst_batch_result_to_text(const FstBatchResult* in, FstTextResult* out) {
  if (!in || !out) return FST_INVALID_ARG;
  const uint32_t num = in->num_strings;
  if (num && (!in->status || !in->path_offsets || !in->final_weights)) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(in->path_offsets, num)) return FST_INVALID_ARG;
  if (num && in->path_offsets[num] != in->path_offsets[0] && (!in->olabels || !in->weights))
    return FST_INVALID_ARG;
  // pass 1: statuses and byte counts; pass 2: the bytes and the fold
  std::vector<int32_t> st(num);
  std::vector<uint64_t> cnt(num, 0);
  uint64_t tot = 0;
  for (uint32_t i = 0; i < num; ++i) {
    st[i] = in->status[i];
    if (st[i] != kPathOk) continue;
    uint64_t c = 0;
    for (uint64_t k = in->path_offsets[i]; k < in->path_offsets[i + 1]; ++k) {
      if (in->olabels[k] > 256u) {
        st[i] = kPathUnsupported;
        break;
      }
      c += in->olabels[k] != kEpsilon;
    }
    if (st[i] == kPathOk) cnt[i] = c;
    tot += cnt[i];
  }
  if (!alloc_text_result(out, num, tot)) {
    fst_text_result_free(out);
    return FST_OOM;
  }
  uint64_t w = 0;
  for (uint32_t i = 0; i < num; ++i) {
    out->status[i] = st[i];
    out->text_offsets[i] = w;
    out->total_weight[i] = w_zero();
    if (st[i] != kPathOk) continue;
    double d = w_one();
    for (uint64_t k = in->path_offsets[i]; k < in->path_offsets[i + 1]; ++k) {
      if (in->olabels[k] != kEpsilon) out->text[w++] = (uint8_t)(in->olabels[k] - 1u);
      d = w_times(d, in->weights[k]);
    }
    out->total_weight[i] = w_times(d, in->final_weights[i]);
  }
  out->text_offsets[num] = w;
  return FST_OK;
}

// ---- Aligned text entries (fst_batch.h) -------------------------------------------------

FstError fst_normalize_text_aligned_batch(const FstHandle* stages, uint32_t num_stages,
                                          const uint8_t* text, const uint64_t* offsets,
                                          uint32_t num_strings, const FstBatchOptions* opts,
                                          FstAlignedTextResult* out) {
  if (!out || !stages || num_stages == 0 || !offsets ||
      (!text && num_strings && offsets[num_strings] != offsets[0]))
    return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(offsets, num_strings) || !flags_ok(opts)) return FST_INVALID_ARG;
  Stages fs;
  if (!get_stages(stages, num_stages, &fs)) return FST_INVALID_ARG;
  if (num_strings == 0) return empty_result(out);  // nothing to run
  BatchCall call;
  if (FstError e = call.open(opts); e != FST_OK) return e;
  const int semantics = call.semantics;
  // (the sharded route alone: the streamed route's pull kernels write no ilabels)
  const FstError e = run_sharded(
      call.devices, call.nsh, num_strings, chain_costs(*fs[0], offsets, num_strings, call.nsh),
      [&](Shard& S) {
        S.align = std::make_unique<AlignMap>();
        return run_text_shard(S, fs, text, offsets + S.s0, semantics);
      },
      out);
  return call.close(e, "fst_normalize_text_aligned_batch", out, fst_aligned_text_result_free);
}

void fst_aligned_text_result_free(FstAlignedTextResult* r) {
  if (!r) return;
  pin_release(r->status);
  pin_release(r->text_offsets);
  pin_release(r->text);
  pin_release(r->total_weight);
  pin_release(r->in_begin);
  pin_release(r->in_end);
  std::memset(r, 0, sizeof(*r));
}

FstError fst_device_path_alignment(const FstDeviceBatch* o, uint32_t num_strings,
                                   const uint64_t* d_offsets, uint32_t* d_begin,
                                   uint32_t* d_end, uint64_t capacity, uint32_t* d_consumed,
                                   void* stream) {
  if (!o || !d_offsets || (num_strings && !d_consumed) || (capacity && (!d_begin || !d_end)))
    return FST_INVALID_ARG;
  hipStream_t s = nullptr;
  DeviceEngine::Lease E = current_engine(stream, &s);
  if (!E) return FST_INVALID_ARG;
  return E->align_write(dev_out(o), num_strings, d_offsets, d_begin, d_end, capacity, d_consumed,
                        s) == hipSuccess
             ? FST_OK
             : FST_OOM;
}

FstError fst_device_compose_alignment(uint32_t num_strings, const uint64_t* d_outer_offsets,
                                      const uint32_t* d_b, const uint32_t* d_e,
                                      const uint64_t* d_inner_offsets,
                                      const uint32_t* d_inner_begin,
                                      const uint32_t* d_inner_end, const uint32_t* d_consumed,
                                      uint32_t* d_out_begin, uint32_t* d_out_end,
                                      uint64_t capacity, void* stream) {
  if (!d_outer_offsets || !d_inner_offsets || (num_strings && !d_consumed) ||
      (capacity && (!d_b || !d_e || !d_out_begin || !d_out_end)))
    return FST_INVALID_ARG;
  hipStream_t s = nullptr;
  DeviceEngine::Lease E = current_engine(stream, &s);
  if (!E) return FST_INVALID_ARG;
  return E->align_compose(num_strings, d_outer_offsets, d_b, d_e, d_inner_offsets, d_inner_begin,
                          d_inner_end, d_consumed, d_out_begin, d_out_end, capacity,
                          s) == hipSuccess
             ? FST_OK
             : FST_OOM;
}

FstError fst_batch_result_to_aligned_text(const FstBatchResult* in, FstAlignedTextResult* out) {
  if (!in || !out) return FST_INVALID_ARG;
  const uint32_t num = in->num_strings;
  if (num && (!in->status || !in->path_offsets || !in->final_weights)) return FST_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!offsets_monotone(in->path_offsets, num)) return FST_INVALID_ARG;
  if (num && in->path_offsets[num] != in->path_offsets[0] &&
      (!in->ilabels || !in->olabels || !in->weights))
    return FST_INVALID_ARG;
  // the text first (statuses, offsets, bytes, the fold), then the map of every OK string
  FstTextResult t;
  if (FstError e = fst_batch_result_to_text(in, &t); e != FST_OK) return e;
  out->num_strings = t.num_strings;
  out->status = t.status;
  out->text_offsets = t.text_offsets;
  out->text = t.text;
  out->total_weight = t.total_weight;
  out->total_bytes = t.total_bytes;
  out->in_begin = (uint32_t*)pin_alloc(std::max<uint64_t>(t.total_bytes, 1) * 4);
  out->in_end = (uint32_t*)pin_alloc(std::max<uint64_t>(t.total_bytes, 1) * 4);
  if (!out->in_begin || !out->in_end) {
    fst_aligned_text_result_free(out);
    return FST_OOM;
  }
  for (uint32_t i = 0; i < num; ++i) {
    if (out->status[i] != kPathOk) continue;
    uint64_t w = out->text_offsets[i];
    uint32_t b = 0;
    for (uint64_t k = in->path_offsets[i]; k < in->path_offsets[i + 1]; ++k) {
      const uint32_t step = in->ilabels[k] != kEpsilon;
      if (in->olabels[k] != kEpsilon) {
        out->in_begin[w] = b;
        out->in_end[w++] = b + step;
      }
      b += step;
    }
  }
  return FST_OK;
}

FstError fst_device_compose_shortest_path(FstHandle b_handle, const uint32_t* d_labels,
                                          const uint64_t* d_offsets, uint32_t num_strings,
                                          uint32_t max_len, uint32_t n,
                                          const FstBatchOptions* opts, const FstDeviceBatch* o,
                                          void* stream) {
  // (outside DeviceCall: no device restore, no flags_ok check and no drain, as it always was)
  if (!o || !d_offsets) return FST_INVALID_ARG;
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  if (!gpu_available()) return FST_INVALID_ARG;
  int dev = opts && opts->device >= 0 ? opts->device : current_device();
  if (dev < 0 || hipSetDevice(dev) != hipSuccess) return FST_INVALID_ARG;
  DeviceFst* D = b->device(dev);
  if (!D) return FST_OOM;
  ChainInput in{{d_labels}, d_offsets, num_strings, max_len};
  DeviceEngine::Lease E = DeviceEngine::acquire(dev);
  if (!E) return FST_INVALID_ARG;
  const hipStream_t s = E.use((hipStream_t)stream);
  LaunchStats st;
  const int semantics = opts ? (int)opts->semantics : FST_SEM_LAZY;
  if (E->run_chain(*D, in, n, semantics, dev_out(o), s, &st) != hipSuccess) return FST_OOM;
  t_last_stats = st;
  return FST_OK;
}

FstError fst_device_prepare(FstHandle b_handle, int32_t device) {
  std::shared_ptr<FrozenFst> b = frozen_get(b_handle);
  if (!b) return FST_INVALID_ARG;
  if (!gpu_available()) return FST_INVALID_ARG;
  const int dev = device >= 0 ? device : current_device();
  return b->device(dev) ? FST_OK : FST_OOM;
}

FstHandle fst_device_adopt_blob(const void* d_blob, uint64_t len, int32_t device,
                                const void* host_copy) {
  if (!d_blob || len < sizeof(Header)) return kInvalid;
  if (!gpu_available()) return kInvalid;
  const int dev = device >= 0 ? device : current_device();
  if (hipSetDevice(dev) != hipSuccess) return kInvalid;
  std::vector<uint8_t> bytes(len);
  if (host_copy) std::memcpy(bytes.data(), host_copy, len);
  else if (hipMemcpy(bytes.data(), d_blob, len, hipMemcpyDeviceToHost) != hipSuccess)
    return kInvalid;
  auto f = frozen_from_bytes(bytes.data(), len);
  if (!f) return kInvalid;
  DeviceFst* D = DeviceFst::adopt(d_blob, *f, dev);
  if (!D) return kInvalid;
  f->adopt_device(dev, D);
  return frozen_insert(std::move(f));
}

FstError fst_last_launch_stats(FstLaunchStats* out) {
  if (!out) return FST_INVALID_ARG;
  out->kernel_ms = t_last_stats.kernel_ms;
  out->launches = t_last_stats.launches;
  out->engine = t_last_stats.engine;
  out->grid = t_last_stats.grid;
  return FST_OK;
}

FstHandle fst_batch_load_bytes(const void* bytes, uint64_t len) {
  if (!bytes || len < sizeof(Header)) return kInvalid;
  auto f = frozen_from_bytes((const uint8_t*)bytes, len);
  return f ? frozen_insert(std::move(f)) : kInvalid;
}

FstHandle fst_batch_load(const char* path) {
  if (!path) return kInvalid;
  auto f = FrozenFst::load_file(path, FrozenFst::kAnyWeightType, nullptr);
  if (!f) return kInvalid;
  return frozen_insert(std::move(f));
}

FstHandle fst_load_att(const char* path, uint32_t flags) {
  if (!path || (flags & ~FST_ATT_SHIFT_BYTE_LABELS)) return kInvalid;
  std::vector<char> data;  // att2lfst.zig:40-45 (.limited(256 MiB))
  if (!read_file(path, 256l << 20, &data)) return kInvalid;
  MutableFst m;
  if (!MutableFst::read_text(data.data(), data.size(), &m)) return kInvalid;
  if (flags & FST_ATT_SHIFT_BYTE_LABELS) m.shift_labels();
  return frozen_insert(FrozenFst::from_mutable(m, kWeightTropical));
}

double fst_chain_cost(FstHandle b, uint64_t len) {
  auto f = frozen_get(b);
  return f ? f->chain_cost(len) : -1.0;
}

uint64_t fst_debug_text_compact(uint32_t num_strings, uint64_t* offsets, const uint32_t* nbytes,
                                int32_t* status, double* total_weight, uint8_t* text) {
  if (!offsets || (num_strings && (!nbytes || !status || !total_weight))) return 0;
  return text_compact(num_strings, offsets, nbytes, status, total_weight, text);
}

void fst_debug_expand_weight_codes(const uint8_t* codes, uint64_t n, const double* table,
                                   double* dst) {
  if (!n || !codes || !table || !dst) return;
  expand_weight_codes(codes, (size_t)n, table, dst);
}

uint32_t fst_debug_stream_part_cuts(const uint64_t* offsets, uint32_t num_strings,
                                    const uint64_t* per_mille, uint32_t num_per_mille,
                                    uint32_t* cuts) {
  if (!offsets || !cuts || (num_per_mille && !per_mille)) return 0;
  const std::vector<uint32_t> c = stream_part_cuts(
      offsets, num_strings, std::vector<uint64_t>(per_mille, per_mille + num_per_mille));
  std::copy(c.begin(), c.end(), cuts);
  return (uint32_t)c.size();
}

int32_t fst_weight_type(FstHandle b) {
  auto f = frozen_get(b);
  return f ? (int32_t)f->weight_type() : -1;
}

// Reference bench rhs generators (bench/optimize-bench.zig:219-306).
FstHandle fst_bench_transducer(uint32_t kind, uint32_t T, uint32_t B) {
  return fst_bench_transducer_wt(kind, T, B, kWeightTropical);
}

FstHandle fst_bench_transducer_wt(uint32_t kind, uint32_t T, uint32_t B, uint32_t weight_type) {
  if (weight_type != kWeightTropical && weight_type != kWeightLog) return kInvalid;
  MutableFst m;
  if (kind == 0) {  // buildAmbiguousChainTransducer, :250-277
    m.add_states(T + 1);
    m.set_start(0);
    for (uint32_t i = 0; i <= T; ++i) m.set_final(i, w_one());
    const uint32_t fan = std::max<uint32_t>(1, std::min<uint32_t>(B, 4));
    for (uint32_t i = 0; i <= T; ++i) {
      m.add_arc(i, Arc{1, 1, w_one(), i});
      for (uint32_t b = 0; b < fan; ++b)
        m.add_arc(i, Arc{1, ((i + b) % 255) + 1, (double)b, std::min(i + b + 1, T)});
    }
  } else if (kind == 1) {  // buildEpsilonDenseTransducer, :219-248
    m.add_states(T + 1);
    m.set_start(0);
    for (uint32_t i = 0; i <= T; ++i) m.set_final(i, w_one());
    for (uint32_t i = 0; i < T; ++i) {
      m.add_arc(i, Arc{0, 0, w_one(), i + 1});
      for (uint32_t b = 0; b < B; ++b)
        m.add_arc(i, Arc{1, ((i + b) % 255) + 1, (double)b, std::min(i + (b % 4) + 1, T)});
    }
  } else if (kind == 2) {  // transducer_for_freeze, :290-306
    if (T == 0) return kInvalid;
    m.add_states(T);
    m.set_start(0);
    for (uint32_t i = 0; i < T; ++i) {
      m.set_final(i, w_one());
      for (uint32_t b = 0; b < B; ++b)
        m.add_arc(i, Arc{(b % 255) + 1, ((i + b) % 255) + 1, (double)b,
                         (uint32_t)(((uint64_t)i + b + 1) % T)});
    }
  } else {
    return kInvalid;
  }
  return frozen_insert(FrozenFst::from_mutable(m, (uint8_t)weight_type));
}

}  // extern "C"

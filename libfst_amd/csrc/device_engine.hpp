// device_engine.hpp -- device-resident frozen FSTs and the batch engines.
//
// Engines:
//   eager-layered : FST_SEM_EAGER on lattices that are layered by input position
//                   (rhs without epsilon input arcs, inputs without label 0).
//                   One workgroup per string, per-layer LDS hash tables; ids,
//                   distances and back-pointers reproduce compose.zig's BFS ids and
//                   shortest-path.zig's tie rules.
//   lazy-wave     : FST_SEM_LAZY, exact replay of composeShortestPath's Dijkstra
//                   (one wavefront per string, workspace in HBM).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <new>
#include <vector>

#include "fst_core.hpp"

namespace fstamd {

class FrozenFst;

// RhsView::sspan[s].z when the state's arcs carry more than one ilabel / no arcs.
constexpr uint32_t kSpanMixed = 0xFFFFFFFEu;
constexpr uint32_t kSpanNone = 0xFFFFFFFFu;
// The device arc mirror (RhsView::rec) has kRecPad zeroed records past num_arcs, so a
// kernel may read rec[lo + j] for any lo <= num_arcs and j < kRecPad unconditionally.
constexpr uint32_t kRecPad = 16;
// Input label no rhs arc carries: a pipeline string that failed an earlier stage.
constexpr uint32_t kDeadLabel = 0xFFFFFFFFu;

// Read-only view of a device-resident rhs (the kernels' only rhs interface).
struct RhsView {
  const uint2* span;        // [num_states] (arc_offset, num_arcs)
  const double* final_w;    // [num_states]
  const uint32_t* il;       // [num_arcs] sorted ilabels per state span
  const ArcRec* rec;        // [num_arcs] {nextstate, olabel, weight}
  const uint4* sspan;       // [num_states] {arc_offset, num_arcs, ilabel shared by all
                            //  arcs of the state | kSpanMixed | kSpanNone, leading epsilon
                            //  arcs of a kSpanMixed state (ilabel 0 sorts first) else 0}
  uint32_t num_states;
  uint32_t num_arcs;
  uint32_t start;
  uint32_t max_span;        // largest per-state arc count
  uint32_t jump_back;       // max (s - t) over arcs s -> t (0 if none goes backwards)
  uint32_t jump_fwd;        // max (t - s) over arcs s -> t: a layer's targets lie within
                            // [min state - jump_back, max state + jump_fwd]
  // [num_states] for states with several ilabels: {first ilabel a, last ilabel z, arcs
  // carrying a, 1 when every other arc carries z}: a two-label state (an epsilon run then
  // one label, the epsilon-dense rhs) answers arcsByIlabel without a search
  const uint4* sspan2;
};

// Reverse arc mirror for the pull tier (kernels/eager_pull.hpp): the in-arcs of every rhs
// state t, grouped by ilabel, each group in padded blocks of `kp` records.  Record m of a
// block: 8 * the source state (its LDS cell offset before the window shift), y = (j << 17)
// | (m << 13) with j = the arc's position in its source's run of equal ilabels (the
// candidate order of compose.zig:93-121) | kRevPos when the weight is > 0, and the weight.
// Padding records have src = 0xFFFFFFF8.  Block 0 is all padding (the null block).
// y's flag of a positive-weight arc: bit 12, below m; the pull keys OR y with the cell's
// byte offset (< 4096), so the flag never decides a key comparison (keys of two in-arcs
// always differ in rank, j or m) and is masked off with the offset (& 0xFFF)
constexpr uint32_t kRevPos = 0x1000u;
struct RevRec {
  uint32_t src;
  uint32_t y;
  double weight;
};
static_assert(sizeof(RevRec) == 16, "RevRec is one 16-byte load");
struct RevView {
  const uint4* rspan;     // [num_states + kPullW] one group: {first record, nblocks, ilabel,
                          // 0}; several: {first gtab entry, groups, kSpanMixed, 0}; none (and
                          // the padding past the last state): {0, 0, kSpanNone, 0}
  const uint4* gtab;      // groups of multi-label states {ilabel, first record, nblocks, 0}
  const RevRec* rrec;     // [nblocks * kp]
  const uint32_t* rolab;  // [nblocks * kp] olabel of each record (backtrace only)
  uint32_t kp;            // records per block
  uint32_t gsearch;       // binary-search steps over the longest gtab run (0: no gtab)
  uint32_t direct;        // 1: block 0 of state t at record t * kp (every state has at most
                          // one in-label group); rspan.x = the record of its block 1
  // [nblocks * kp] the same records with an f32 weight and the olabel: {src, y, f32 bits of
  // the weight, olabel}; only when every arc weight is an integer in [0, 2^24) (exact in
  // f32; DeviceFst::int_wmax), else null
  const uint4* rrec32;
  // [nblocks * kp] the records in 8 B: {src, y | weight}, only when every arc weight is an
  // integer in [0, kRec8WMax] (it sits in y's low 3 bits, below the byte offset the keys OR
  // in), else null
  const uint2* rrec8;
  // direct layout: rspan split for the row loads, ilabel | min(nblocks, 255) << 24 per
  // state (4 B; labels below 2^24) and {the record of its block 1, nblocks} (read only for
  // states with more than one block)
  const uint32_t* rlab;
  const uint2* rxrec;
  uint32_t nrec;  // records (nblocks * kp)
  // [nblocks * kp] tier P's 4-B records (eager_pull.hip: the source as 8 * (target - source)
  // + rbias8 in the high half, the key bits and weight in the low half), else null
  const uint32_t* rrec4;
  uint32_t rbias8;
  // 2^-k: the compact records (rrec32 / rrec8 / rrec4) hold every weight times 2^k, the
  // smallest power of two that makes them all integers (DeviceFst::int_wmax); the kernels
  // multiply back what they output (exact).  1 for integer weights.  (The view's layout
  // steers tier P's register allocation: one more 8-B field here cost it 3 %, so the weight
  // table below has no pointer of its own.)
  double winv;
  // (weights no such scale makes integers, DeviceFst::widx: rrec4's low byte indexes a
  // table of the rhs's distinct arc weights stored after the records, rv_weight_table)
};
constexpr uint32_t kPullWt = 64;  // (a power of two: the kernels mask the index)
// rhs with 65..256 distinct weights: tier P's RK 5 (the same records, a 256-entry LDS
// table, 4 waves per SIMD instead of 5); the global copy always holds kPullWtMax entries
constexpr uint32_t kPullWtMax = 256;
// the weight table of an rhs with DeviceFst::widx: kPullWtMax doubles right after the
// rrec4 records (their count rounded up to 8-B alignment)
__host__ __device__ inline const double* rv_weight_table(const RevView& rv) {
  return reinterpret_cast<const double*>(rv.rrec4 + ((rv.nrec + 1u) & ~1u));
}
// tier P's packed-cell records (DeviceFst::pack; kernels/eager_pull.hpp): nrec words in that
// same place -- an rhs has either the weight table (weights no scale makes integers) or
// these (integer weights <= kRec8WMax), never both, and the view gains no field
__host__ __device__ inline const uint32_t* rv_packed(const RevView& rv) {
  return rv.rrec4 + ((rv.nrec + 1u) & ~1u);
}
constexpr double kRec8WMax = 7.0;

struct DeviceFst {
  int dev = 0;
  uint8_t* blob = nullptr;  // the frozen blob itself, byte-identical to the host copy
  size_t blob_size = 0;
  uint2* span = nullptr;
  double* final_w = nullptr;
  uint32_t* il = nullptr;
  ArcRec* rec = nullptr;
  uint4* sspan = nullptr;
  RhsView view{};
  bool has_eps = false;
  bool nonneg = true;        // every arc and final weight >= +0
  bool nan = false;          // some arc or final weight is NaN
  bool finite = true;        // every arc weight finite
  uint8_t weight_type = 0;
  // pull tier (kernels/eager_pull.hpp): reverse mirror, built when the rhs qualifies
  // (no input epsilon, weights >= +0, every same-ilabel run of a state <= 8 arcs)
  bool pull_ok = false;
  // lazy pull tier (kernels/lazy_pull.hpp) too: for arcs of one source into one target
  // within a same-ilabel run, candidate order = olabel order (relax's (id, il, ol) rule
  // then reduces to (id, candidate))
  bool lazy_pull_ok = false;
  double int_wmax = -1.0;    // largest arc weight times RevView::winv^-1 when every scaled
                             // weight is an integer >= 0 below 2^24, else -1
  bool widx = false;         // rrec4 holds weight-table indices (RK 4 / 5; rv_weight_table)
  uint32_t wt_n = 0;         // distinct arc weights in that table (<= kPullWtMax)
  // rrec4 is followed by the packed-cell records (rv_packed): integer weights <= kRec8WMax,
  // a jump span of at most 63 states, no in-label 0xFFFFFF.  Per launch pull_pack decides
  bool pack = false;
  // the direct layout with every in-arc group within 255 / kp blocks: a back record can be
  // one byte, the in-arc's position x * kp + m in its target's group (the chases re-derive
  // the record from the target state: tier P with rrec4, the lazy pull with any records)
  bool byte_back = false;
  // the host's copy of the RK 4 / 5 weight table (kPullWtMax entries, what rv_weight_table
  // holds on the device): the streamed batch expands weight codes with it
  std::vector<double> wtab_host;
  // Routing hints learnt from earlier batches on this rhs: a small-lattice (LDS) tier that
  // handed on nearly every string is skipped next time (config 3's lattices never fit).
  mutable std::atomic<int> skip_tiny_lazy{0}, skip_tiny_eager{0};
  // ... and one whose 128-tuple LDS size handed on over a third of a batch starts at 256
  mutable std::atomic<int> tiny_lazy_256{0}, tiny_eager_256{0};
  // ... counted over small batches too (coalesced single calls: batches of a few strings
  // never reach the per-batch thresholds): strings the 128-tuple LDS replay saw / handed on
  mutable std::atomic<uint64_t> tiny_lazy_seen{0}, tiny_lazy_over{0};
  RevView rev{};
  void* rev_bufs[9] = {};
  // band replay (kernels/lazy_band.hpp): the arcs at a fixed stride of 2^band_sh slots per
  // state (device numbering), built when the rhs takes the band replay (arcs forward, input
  // epsilon, <= 64 arcs per state) and the table stays small; padding slots: ilabel
  // 0xFFFFFFFF, a zero record
  uint32_t* band_il = nullptr;
  ArcRec* band_rec = nullptr;
  uint32_t band_sh = 0;
  // every state's arcs are non-decreasing in (ilabel, olabel) (fromMutable sorts them so; a
  // fromBytes blob need only be ilabel-sorted): the band's slot fold needs it, since it
  // breaks a tie between equal-distance arcs into one target by arc position
  bool band_ol_sorted = false;
  // The device's state numbering (old id -> new id; empty = the blob's own ids): a
  // breadth-first renumbering of an rhs with scattered ids (device_engine.hip
  // bfs_renumbering).  Every device view (RhsView, RevView) uses it; results do not.
  std::vector<uint32_t> perm;

  static DeviceFst* create(const FrozenFst& f, int dev);
  // Blob already in device memory on `dev` (e.g. after an RCCL broadcast).
  static DeviceFst* adopt(const void* d_blob, const FrozenFst& host_view, int dev);
  static void destroy(DeviceFst* d);
};

// Device pointers of one batch's outputs (mirrors FstDeviceBatch in fst_batch.h).
struct BatchOutDev {
  int32_t* status;
  uint32_t* path_len;
  uint64_t* path_off;
  double* final_w;
  uint32_t* out_il;
  uint32_t* out_ol;
  double* out_w;
  uint64_t arc_cap;
  unsigned long long* cursor;
  uint32_t* work;
  // The host batch's streamed mode (c_api.cpp run_streamed; rhs without input epsilons, so
  // every path has exactly L arcs):
  //   slots: string si's path sits at arena slot slots[si] (the batch's own label offsets:
  //     no cursor, no compaction);
  //   host_ol / host_w (pull tiers only): each finished path's olabels and weights are
  //     also copied into these host-mapped result arrays (whole lines per store), and the
  //     chase skips the ilabels (the host stages them: on an OK path il[k] = label k).
  const uint64_t* slots = nullptr;
  uint32_t* host_ol = nullptr;
  // (host_w is dead in the streamed text batch, which has no host_ol: `text`, below, shares
  // its place, so the kernels' argument block does not grow -- DESIGN.md §3.1: the layout of
  // the argument structs steers the pull tiers' register allocation)
  union {
    double* host_w = nullptr;
    const struct TextOutDev* text;
    // the lattice batch (fst_compose_frozen_batch; the emitting instances of eager_bfs_kernel,
    // lattice_batch.hip): where every item's lattice goes.  A third tenant of the same place:
    // the emitting instances write no path, so neither of the other two is theirs
    const struct LatticeOutDev* lattice;
  };
  // (host side, not read by kernels) when set, run_chain copies the statuses right after
  // the first tier here: which strings the pull tier finished (and copied out) itself
  int32_t* first_status = nullptr;
  // The streamed text batch (c_api.cpp, text mode of run_streamed; launch_pull_part with
  // text = true, `slots` set, host_ol null): after each batched chase the wave emits the
  // finished paths as text (kernels/device_common.hpp emit_text_paths).  One pointer to a
  // small device struct, not three fields.  Only the pull tiers' text instances read it;
  // every other caller leaves the place to host_w, which goes with host_ol.
};

// Text outputs of the streamed text batch.  String si's bytes go to its fixed text slot
// host_text[slots[si] ..]: its own input byte range (no input epsilon in the rhs: a path of
// a string of L bytes has L arcs and every arc emits at most one byte).
constexpr uint32_t kTextNotBytes = 0xFFFFFFFFu;
struct TextOutDev {
  uint8_t* host_text;  // host-mapped result bytes, indexed like the arena (BatchOutDev::slots)
  uint32_t* nbytes;    // [num] device: bytes written, kTextNotBytes for a path with an
                       // olabel > 256 (the host reports UNSUPPORTED; the device status stays
                       // OK: the later tiers take every UNSUPPORTED string for theirs)
  double* total_w;     // [num] device: the serial fold of the path's weights and the final
};

// Lattice outputs of the lattice batch.  An item that finished its compose
// reserves round4(N) states and round4(A) arcs in the arena with one atomicAdd on each cursor
// (so every item starts 16-B aligned in every array and the copies are whole 16-B stores),
// copies nfin / aoff (local offsets, N of them: the closing one is A) and the four arc arrays
// there, and records where.  The cursors keep counting past the capacities: such an item
// reports OUTPUT_FULL and the cursors end at what the batch needs.
struct LatItem {
  uint64_t spos, apos;  // first state / arc of the item in the arena
  uint32_t n, a;        // its states and arcs
  uint32_t pad[2];
};
static_assert(sizeof(LatItem) == 32, "two 16-B stores per item");
struct LatticeOutDev {
  LatItem* item;        // [num], defined for OK items
  double* fin;          // [state_cap]
  uint32_t* aoff;       // [state_cap] arc offsets local to the item
  uint32_t* il;         // [arc_cap]
  uint32_t* ol;
  double* w;
  uint32_t* next;
  uint64_t state_cap, arc_cap;  // multiples of 4
  unsigned long long* cursor;   // [2] states, arcs
  uint32_t project;             // 1: il := ol (FST_LATTICE_PROJECT_OUTPUT)
};
// The compacted batch, in FstLhsBatch's layout (device memory).
struct LatticeCsrDev {
  int32_t* status;          // [num]
  uint64_t* state_offsets;  // [num + 1]
  uint32_t* start;          // [num]
  double* final_w;          // [state_cap]
  uint64_t* arc_offsets;    // [state_cap + 1]
  uint32_t* il;             // [arc_cap]
  uint32_t* ol;
  double* w;
  uint32_t* next;
  uint64_t state_cap, arc_cap;
};
// The lattice trim's workspace (kernels/lattice_trim.hpp): connect of every item
// of an arena before its compaction.
enum : uint32_t { kTrimCtrList = 0, kTrimCtrSweep = 1, kTrimCtrLinear = 2, kTrimCtrWords = 4 };
struct LatTrimDev {
  uint32_t* mark;    // [state_cap] bit 0 coaccessible, bit 1 accessible; then the new ids
  uint32_t* queue;   // [state_cap] the frontier BFS's queue (accessibility, the linear tier)
  uint32_t* roff;    // [state_cap] the linear tier: the item's reverse CSR ...
  uint32_t* rcur;    // [state_cap]     ... its fill cursors ...
  uint32_t* rsrc;    // [arc_cap]       ... and the arcs' sources
  uint32_t* list;    // [num] items the sweep tier handed on
  uint32_t* ctr;     // [kTrimCtrWords] the list's length, items settled per tier
  unsigned long long* tot;  // [4] states before / after, arcs before / after
  const uint32_t* start;    // [num] the items' starts; null: 0 (compose output)
  uint32_t sweeps;          // the sweep budget (FSTAMD_TRIM_SWEEPS)
  uint32_t access;          // 1: mark holds the accessibility pass's result
  uint32_t aoff_skew;       // item i's arc offsets start at aoff[spos + aoff_skew * i]
};
// The lattice shortest path's inputs and workspace (kernels/lattice_sp.hpp):
// fst_shortest_path of every item of an lhs batch, the batch's CSR read in place.
enum : uint32_t { kSpCtrList = 0, kSpCtrWave = 1, kSpCtrFrontier = 2, kSpCtrReplay = 3,
                  kSpCtrWords = 4 };
struct SpHeapEnt;
struct LatSpDev {
  const struct LhsDesc* desc;  // [num]
  const uint32_t* state_off;   // the batch's arrays, as GraphInput holds them for a batch
  const double* final_w;
  const uint32_t* arc_next;
  const uint32_t* arc_il;
  const uint32_t* arc_ol;
  const double* arc_w;
  unsigned long long* key;     // [states] okey of the distance
  unsigned long long* back;    // [states] (source << 32) | arc index of the back-pointer
  uint32_t* mark;              // [states] the frontier tier: round stamps ...
  uint32_t* fa;                // [states]     ... and its two frontiers
  uint32_t* fb;
  SpHeapEnt* heap;             // [arcs + num] the replay tier: item i's heap at arc_base + i
  uint8_t* settled;            // [states]     ... and its settled flags
  uint32_t* list;              // [num] items the wave tier handed on
  uint32_t* ctr;               // [kSpCtrWords] the list's length, items finished per tier
  uint32_t sweeps;             // the wave tier's budget (FSTAMD_SP_SWEEPS)
  uint32_t n_best;
  unsigned long long wd_ticks;
};
// The lattice prune's inputs, workspace and outputs (kernels/lattice_prune.hpp):
// the beam cut of every item of an lhs batch, the batch's CSR read in place.  The outputs are a
// shadow view for the trim ladder: LatItem / status / start per item, the finals and the arcs'
// targets with what the cut drops taken out (indexed like the batch's own arrays).
enum : uint32_t { kPrCtrList = 0, kPrCtrWave = 1, kPrCtrFrontier = 2, kPrCtrWords = 4 };
constexpr uint32_t kPruneLdsStates = 256;  // the wave tier keeps both key arrays in LDS up to here
struct LatPruneDev {
  const struct LhsDesc* desc;  // [num]
  const uint32_t* state_off;   // the batch's arrays, as GraphInput holds them for a batch
  const double* final_w;
  const uint32_t* arc_next;
  const double* arc_w;
  unsigned long long* key;     // [2 * states] item at 2 * state_base: n keys of F, then n of B
  uint32_t* mark;              // [states] the frontier tier: round stamps ...
  uint32_t* fa;                // [states]     ... its two frontiers ...
  uint32_t* fb;
  uint32_t* roff;              // [states]     ... and the item's reverse CSR: offsets, cursors,
  uint32_t* rcur;
  uint32_t* rsrc;              // [arcs]       the arcs' sources and their indices
  uint32_t* rarc;
  uint32_t* list;              // [num] items the wave tier handed on
  uint32_t* ctr;               // [kPrCtrWords] the list's length, items finished per tier
  LatItem* item;               // [num] out
  int32_t* status;             // [num] out
  uint32_t* start;             // [num] out
  double* sfin;                // [states] out: the kept final weights, +inf elsewhere
  uint32_t* snext;             // [arcs] out: the kept arcs' targets, kNoState elsewhere
  double beam;
  uint32_t sweeps;             // the wave tier's budget per direction (FSTAMD_PRUNE_SWEEPS)
  unsigned long long wd_ticks;
};
// The lattice n-best's inputs and workspace (kernels/lattice_nbest.hpp): the n
// best distinct paths of every item of an lhs batch, the batch's CSR read in place.
constexpr uint32_t kNbestMax = 16;  // FST_NBEST_MAX
enum : uint32_t { kNbCtrList = 0, kNbCtrLds = 1, kNbCtrHbm = 2, kNbCtrWords = 4 };
struct LatNbestDev {
  const struct LhsDesc* desc;  // [num]
  const uint32_t* state_off;   // the batch's arrays, as GraphInput holds them for a batch
  const double* final_w;
  const uint32_t* arc_next;
  const uint32_t* arc_il;
  const uint32_t* arc_ol;
  const double* arc_w;
  // the HBM tier's tables (null while the LDS tier runs), an item's slice at its bases
  unsigned long long* eg;      // [states * n] list entries: the cost ...
  unsigned long long* ear;     // [states * n]     ... and (last arc << 32) | rank of the rest
  uint32_t* depth;             // [states] five words per state
  uint32_t* roff;
  uint32_t* cnt;
  uint32_t* lvl;
  uint32_t* order;
  uint32_t* rarc;              // [arcs] two words per arc
  uint32_t* asrc;
  uint32_t* list;              // [num] items the LDS tier handed on
  uint32_t* ctr;               // [kNbCtrWords] the list's length, items finished per tier
  uint32_t n_best;
  uint32_t lds_budget;         // bytes of dynamic LDS per workgroup of the LDS tier
  unsigned long long wd_ticks;
  // the unique instances alone (distinct output texts)
  unsigned long long* eh;      // [states * n] the HBM tier's text hashes, beside eg and ear
  unsigned long long hash_mask;  // ANDed onto every hash (FSTAMD_NBEST_HASH_MASK; all ones)
};
// The lattice posteriors' inputs, workspace and outputs (kernels/lattice_posterior.hpp, DESIGN.md
// §7l).  `nb` is the n-best's view of the batch (nb_item reads it), its list and counters, and
// the workgroup tier's tables: eg / ear hold alpha / beta (8 B per state), depth, roff, lvl,
// order and rarc, asrc as there; cnt, eh, n_best and hash_mask are not used.  The outputs are
// indexed by the items' own bases: alpha, beta like final_w, arc_cost like arc_w.
struct LatPostDev {
  LatNbestDev nb;
  int32_t* status;   // [num] out
  double* total;     // [num] out: -log Z, +inf unless OK
  double* alpha;     // [states] out, or null
  double* beta;      // [states] out, or null
  double* arc_cost;  // [arcs] out
};

// Chain inputs (batch API) or one general lhs FST (single-call C ABI).
struct ChainInput {
  // 4-B labels, or -- the streamed text batch alone (launch_pull_part with text = true: the
  // pull tiers' text instances, text_pull.hip) -- the strings as bytes, label = byte + 1.
  // One place for both, so the struct (a kernel argument) is the same for every kernel.
  // A batch of general lhs (run_lhs_batch: the kLhsBatch instances, lhs_batch.hip) has no
  // labels either: the place holds the items' descriptors.
  union {
    const uint32_t* labels;
    const uint8_t* text;
    const struct LhsDesc* lhs_desc;
  };
  const uint64_t* offsets;
  uint32_t num_strings;
  uint32_t max_len;
};
// The lhs kind of the two general kernels (eager_bfs_kernel, lazy_wave_kernel): chain strings,
// one general lhs (the single-call ABI), or a batch of general lhs.  false / true name the
// first two as before.
enum LhsKind : int { kLhsChain = 0, kLhsGraph = 1, kLhsBatch = 2 };
// One lhs of a batch (fst_compose_frozen_shortest_path_lhs_batch), 32 B.  The batch is one
// concatenated CSR on the device (a GraphInput of whole-batch arrays): item i's per-state
// arc offsets (u32, local to the item, num_states + 1 of them) start at state_off[state_base
// + i], its finals at final_w[state_base], its arcs at arc_*[arc_base]; start and nextstates
// are local to the item.
struct LhsDesc {
  uint64_t state_base;
  uint64_t arc_base;
  uint32_t num_states;
  uint32_t start;
  uint32_t num_arcs;
  uint32_t flags;   // kLhs* below
};
static_assert(sizeof(LhsDesc) == 32, "two 16-B loads per item");
constexpr uint32_t kLhsReplay = 1u;  // eager: a weight that is negative, -0.0 or an arc of +inf:
                                     // the exact heap replay (sp_replay), not the fixpoint
constexpr uint32_t kLhsNaN = 2u;     // a NaN weight (in the item or the rhs): UNSUPPORTED
constexpr uint32_t kLhsEpsOut = 4u;  // some arc has output epsilon
constexpr uint32_t kLhsInvalid = 8u; // the device-resident entry's prepare kernel: the item
                                     // failed validation (it also carries kLhsNaN, the bit the
                                     // kernels turn into UNSUPPORTED; this one is for the log)
struct GraphInput {       // CSR of a MutableFst lhs, arcs in insertion order
  const uint32_t* state_off;   // [ns + 1]
  const uint32_t* arc_il;
  const uint32_t* arc_ol;
  const double* arc_w;
  const uint32_t* arc_next;
  const double* final_w;   // [ns]
  uint32_t num_states;
  uint32_t start;
  uint32_t max_outdeg;     // largest lhs out-degree (sizes the per-pop table)
  uint32_t ncap;           // product-tuple capacity for this run (power of two)
  uint32_t eps_out;        // 1: some lhs arc has output epsilon (filter-2 tuples exist)
};

// Lattice of one fst_compose_frozen call, downloaded from the device (CSR by source id).
// Pooled pinned host memory (c_api.cpp): D2H / H2D of it is one DMA, without the
// runtime's staging copies.
void* pin_host_alloc(size_t bytes);
void pin_host_release(void* p);
// Frees the device block pool's cached blocks of `dev` (c_api.cpp), so that a free-HBM query
// sees them as free.
void device_pool_release(int dev);
template <class T>
struct PinnedAllocator {
  using value_type = T;
  PinnedAllocator() = default;
  template <class U>
  PinnedAllocator(const PinnedAllocator<U>&) {}
  T* allocate(size_t n) {
    void* p = pin_host_alloc(n * sizeof(T));
    if (!p) throw std::bad_alloc();
    return (T*)p;
  }
  void deallocate(T* p, size_t) { pin_host_release(p); }
  template <class U>
  bool operator==(const PinnedAllocator<U>&) const { return true; }
  template <class U>
  bool operator!=(const PinnedAllocator<U>&) const { return false; }
};
template <class T>
using PinnedVec = std::vector<T, PinnedAllocator<T>>;

struct HostLattice {
  int32_t status = 0;  // PathStatus of the compose (kPathOk or kPathOverflow/kPathInternal)
  uint32_t n_nodes = 0, n_arcs = 0;
  PinnedVec<uint32_t> aoff, anext, ail, aol;  // downloaded from the device (config 1: 10 M arcs)
  PinnedVec<double> aw, nfin;
};

struct LaunchStats {
  double kernel_ms = 0;
  uint32_t launches = 0;
  uint32_t engine = 0;
  uint32_t grid = 0;
  // set by the caller: run_chain records its events but does not wait for them; the caller
  // synchronises the stream itself and then calls DeviceEngine::finish_deferred
  bool defer = false;
};

// ---- pull tier (eager_pull.hip, kernels/eager_pull.hpp) ----
struct EagerLaunch;
// Window rows of the pull tier: W = 64 * kPullRows target states per layer.
constexpr int kPullRows = 5;
constexpr uint32_t kPullW = 64 * kPullRows;
// Builds d->rev from the host copy when the rhs qualifies (sets d->pull_ok); false only
// on a device allocation failure.
bool build_reverse_mirror(DeviceFst* d, const FrozenFst& f);
void free_reverse_mirror(DeviceFst* d);
// Resident waves per CU of the pull kernel for this rhs.
int pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len);
// f32 cells for the pull tiers: every distance of a string of <= max_len labels is an
// integer below 2^24 (exact in f32)
bool pull_f32(const DeviceFst& rhs, uint32_t max_len);
hipError_t launch_eager_pull(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                             unsigned int* next_item, const EagerLaunch& lp,
                             const BatchOutDev& out, uint32_t grid, hipStream_t stream);
// The streamed text batch's instances of the two pull kernels (text_pull.hip: byte labels,
// text emission; pull_kernel_dispatch.hpp picks the same variant as for labels): resident
// waves per CU and the launches.
int text_pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len, bool lazy);
hipError_t launch_eager_pull_text(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                  unsigned int* next_item, const EagerLaunch& lp,
                                  const BatchOutDev& out, uint32_t grid, hipStream_t stream);
hipError_t launch_lazy_pull_text(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                 unsigned int* next_item, const EagerLaunch& lp,
                                 const BatchOutDev& out, uint32_t grid, hipStream_t stream);
// Tier P's weight-code instances (code_pull.hip; the streamed label batch).  pull_codes_table:
// whether this rhs, these semantics and this max_len take them -- eager semantics and records
// that hold the weight as a byte (RK 2..6; it follows pull_rk / pull_pack, the single
// decision) -- and if so the 256 f64 values the codes stand for: (double)c * RevView::winv
// for the integer kinds, the rhs's weight table for RK 4 and 5.  They are the values the f64
// chase writes, bit for bit.  Then resident waves per CU and the launch: out.out_w holds the
// device byte arena and out.host_w the host's code staging block (both indexed like the
// path arena, 4-B aligned bases), out.host_ol the result's olabels.
bool pull_codes_table(const DeviceFst& rhs, int semantics, uint32_t max_len, double* table);
int code_pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len);
hipError_t launch_eager_pull_codes(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                                   unsigned int* next_item, const EagerLaunch& lp,
                                   const BatchOutDev& out, uint32_t grid, hipStream_t stream);
// Lazy pull tier (eager_pull.hip, kernels/lazy_pull.hpp): resident waves per CU, launch.
int lazy_pull_waves_per_cu(const DeviceFst& rhs, uint32_t max_len);
bool lazy_pull_f32(const DeviceFst& rhs, uint32_t max_len);
hipError_t launch_lazy_pull(const DeviceFst& rhs, const ChainInput& in, uint32_t n_best,
                            unsigned int* next_item, const EagerLaunch& lp,
                            const BatchOutDev& out, uint32_t grid, hipStream_t stream);

// ---- batch of general lhs (lhs_batch.hip: the kLhsBatch instances of eager_bfs_kernel and
// lazy_wave_kernel) ----
struct BfsWs;
struct LazyWs;
// The eager instances: tables in LDS for 128 / 256 tuples, then HBM slabs with one wavefront
// or one kLhsWG-thread workgroup per item.
enum LhsTier : int { kLhsTierWave = 0, kLhsTierTiny128 = 1, kLhsTierTiny256 = 2, kLhsTierWG = 3 };
constexpr int kLhsWG = 256;
// Resident workgroups per CU of an eager instance.
int lhs_eager_per_cu(int tier);
hipError_t launch_lhs_eager(int tier, const RhsView& rhs, const ChainInput& in,
                            const GraphInput& lhs, uint32_t n_best, unsigned int* next_item,
                            const uint32_t* items, const uint32_t* num_items_dev,
                            const BfsWs& ws, const BatchOutDev& out, uint32_t grid,
                            hipStream_t stream);
hipError_t launch_lhs_lazy(const RhsView& rhs, const ChainInput& in, const GraphInput& lhs,
                           uint32_t n_best, unsigned int* next_item, const uint32_t* items,
                           uint32_t num_items, const LazyWs& ws, const BatchOutDev& out,
                           uint32_t grid, hipStream_t stream);
// ---- lattice batch (lattice_batch.hip: the emitting instances of eager_bfs_kernel, chain and
// kLhsBatch at the four LhsTier shapes, and the compaction kernels) ----
int lattice_per_cu(int tier, bool chain);
hipError_t launch_lattice(int tier, bool chain, const RhsView& rhs, const ChainInput& in,
                          const GraphInput& lhs, unsigned int* next_item, const uint32_t* items,
                          const uint32_t* num_items_dev, const BfsWs& ws, const BatchOutDev& out,
                          uint32_t grid, hipStream_t stream);
hipError_t launch_lattice_count(const int32_t* status, const LatItem* item, uint32_t num,
                                int32_t* status_out, uint64_t* cnt_states, uint64_t* cnt_arcs,
                                hipStream_t stream);
hipError_t launch_lattice_gather(const LatticeOutDev& arena, const uint64_t* arc_base,
                                 const LatticeCsrDev& csr, uint32_t num, uint32_t grid,
                                 hipStream_t stream);
// ---- lattice trim (lattice_trim.hip, kernels/lattice_trim.hpp): connect on the arena ----
hipError_t launch_trim_stage(const LhsDesc* desc, uint32_t num, LatItem* item, int32_t* status,
                             uint32_t* start, hipStream_t stream);
hipError_t launch_trim_access(const LatticeOutDev& arena, const LatTrimDev& t,
                              const int32_t* status, uint32_t num, uint32_t grid,
                              hipStream_t stream);
hipError_t launch_trim_sweep(const LatticeOutDev& arena, const LatTrimDev& t,
                             const int32_t* status, uint32_t num, uint32_t grid,
                             hipStream_t stream);
hipError_t launch_trim_linear(const LatticeOutDev& arena, const LatTrimDev& t,
                              const int32_t* status, uint32_t grid, hipStream_t stream);
hipError_t launch_trim_finalize(const LatticeOutDev& arena, const LatTrimDev& t,
                                const int32_t* status, uint32_t num, uint32_t grid,
                                hipStream_t stream);
hipError_t launch_trim_gather(const LatticeOutDev& arena, const LatTrimDev& t,
                              const uint64_t* arc_base, const LatticeCsrDev& csr, uint32_t num,
                              uint32_t grid, hipStream_t stream);
// ---- lattice shortest path (lattice_sp.hip, kernels/lattice_sp.hpp) ----
hipError_t launch_sp_wave(const LatSpDev& p, const uint32_t* items, uint32_t count,
                          const BatchOutDev& out, uint32_t grid, hipStream_t stream);
hipError_t launch_sp_frontier(const LatSpDev& p, const BatchOutDev& out, uint32_t grid,
                              hipStream_t stream);
hipError_t launch_sp_replay(const LatSpDev& p, const uint32_t* items, uint32_t count,
                            const BatchOutDev& out, uint32_t grid, hipStream_t stream);
// ---- lattice prune (lattice_prune.hip, kernels/lattice_prune.hpp) ----
hipError_t launch_prune_wave(const LatPruneDev& p, uint32_t num, uint32_t grid,
                             hipStream_t stream);
hipError_t launch_prune_frontier(const LatPruneDev& p, uint32_t grid, hipStream_t stream);
// ---- input spans per output symbol (text_align.hip, kernels/text_align.hpp) ----
hipError_t launch_align_write(const BatchOutDev& s, uint32_t num, const uint64_t* offsets,
                              uint32_t* begin, uint32_t* end, uint64_t cap, uint32_t* consumed,
                              uint32_t grid, hipStream_t stream);
hipError_t launch_align_compose(uint32_t num, const uint64_t* outer_off, const uint32_t* b,
                                const uint32_t* e, const uint64_t* inner_off,
                                const uint32_t* in_begin, const uint32_t* in_end,
                                const uint32_t* n1, uint32_t* out_begin, uint32_t* out_end,
                                uint64_t cap, uint32_t grid, hipStream_t stream);
// ---- lattice n-best (lattice_nbest.hip, kernels/lattice_nbest.hpp) ----
// (unique: the instances that keep one path per output text)
hipError_t launch_nbest_lds(const LatNbestDev& p, bool unique, uint32_t count,
                            const BatchOutDev& out, uint32_t grid, hipStream_t stream);
hipError_t launch_nbest_hbm(const LatNbestDev& p, bool unique, const BatchOutDev& out,
                            uint32_t grid, hipStream_t stream);
// ---- lattice posteriors (lattice_posterior.hip, kernels/lattice_posterior.hpp) ----
hipError_t launch_posterior_lds(const LatPostDev& p, uint32_t count, uint32_t grid,
                                hipStream_t stream);
hipError_t launch_posterior_hbm(const LatPostDev& p, uint32_t grid, hipStream_t stream);
// On-device preparation of a device-resident batch (kernels/lhs_prepare.hpp; lhs_batch.hip
// holds the instances).  In: the caller's arrays in FstLhsBatch's layout, all device memory,
// and their two extents as the host read them.  Out: descriptors, local arc offsets
// (total_states + num words), the two eager item lists in ascending item order, and five
// totals: [0] non-negative items, [1] replay items, [2] largest out-degree, [3] invalid items,
// [4] items i with state_offsets[i] > state_offsets[i + 1] (not zero: the whole batch is
// invalid, kernels/lhs_prepare.hpp).
constexpr uint32_t kLhsPrepTotalsWords = 5;
struct LhsPrepIn {
  const uint64_t* state_offsets;  // [num + 1]
  const uint32_t* start;          // [num]
  const double* final_w;          // [total_states]
  const uint64_t* arc_offsets;    // [total_states + 1]
  const uint32_t* arc_ol;         // [total_arcs]
  const double* arc_w;
  const uint32_t* arc_next;
  uint64_t total_states;
  uint64_t total_arcs;
  uint32_t num;
  uint32_t base_flags;            // the rhs's share of every item's flags; with kLhsInvalid
                                  // every item is invalid and none is read
};
struct LhsPrepOut {
  LhsDesc* desc;
  uint32_t* state_off;
  uint32_t* totals;  // [kLhsPrepTotalsWords], zeroed before the launch
};
hipError_t launch_lhs_prepare(const LhsPrepIn& in, const LhsPrepOut& out, uint32_t grid,
                              hipStream_t stream);
hipError_t launch_lhs_lists(const LhsDesc* desc, uint32_t num, uint32_t* list_nonneg,
                            uint32_t* list_replay, uint32_t* totals, hipStream_t stream);
// A batch of general lhs in device memory, as run_lhs_batch, run_sp_batch and the lattice batch
// read it.  Both routes end up with one: the host route stages the caller's items into a block
// of its own (host::stage_lhs_items), the device-resident route derives it from the caller's
// arrays in place (DeviceEngine::prepare_lhs).
struct LhsBatchDev {
  ChainInput in{};    // lhs_desc = the items' descriptors, num_strings = their number
  GraphInput lhs{};   // the whole batch's concatenated CSR (start / num_states unused,
                      // max_outdeg = the batch's)
  const uint32_t* items_nonneg = nullptr;  // device lists of the items without / with
  const uint32_t* items_replay = nullptr;  // LhsDesc::flags & kLhsReplay ...
  uint32_t num_nonneg = 0, num_replay = 0;  // ... and their host counts
  uint64_t total_states = 0, total_arcs = 0;  // the batch's extents
};
// What else DeviceEngine::prepare_lhs reports.
struct LhsPrepared {
  uint32_t invalid = 0;   // items that failed validation
  uint32_t launches = 0;
};
// The rhs's share of every item's flags (no rhs: none; an item's flags are then its own).
inline uint32_t lhs_base_flags(const DeviceFst* rhs) {
  return rhs ? (rhs->nan ? kLhsNaN : 0u) | (rhs->nonneg ? 0u : kLhsReplay) : 0u;
}

// What a batch of general lhs took which way (FSTAMD_ROUTE_LOG, tests): items that entered
// each tier.  Eager: t[0..3] = tiny128, tiny256, tier 0, tiers 1+ (summed); replay = items on
// the heap-replay route (they appear in t[2..3] too).  Lazy: t[k] = items that entered the
// table tier of 1024 << 4k tuples.  run_sp_batch: t[0..1] = items the wave / frontier tier
// finished.
struct LhsRoute {
  uint32_t t[8] = {};
  uint32_t replay = 0;
  uint32_t tiers_run = 0;  // kernel launches of the tier ladders
};

// Per-device engine state: persistent workspaces (grown on demand), its own non-blocking
// HIP stream and events.  A device has a small pool of engines (FSTAMD_ENGINES, default
// 4): concurrent C-ABI calls each lease one, so they run side by side on separate streams
// and synchronise only their own stream (src/c-api.zig:776-787 runs compute outside its
// lock; include/fst.h:11-26).
class DeviceEngine {
 public:
  // Exclusive use of one engine of `dev` for the lifetime of the lease.  use(s) binds the
  // stream the call's work goes on (the engine's own stream for synchronous entries, the
  // caller's for the async device entries): a stream other than the previous user's first
  // waits for that user's work (an event), and the lease records the event when it ends,
  // so an engine's workspaces are never reused while earlier work on them still runs.
  class Lease {
   public:
    Lease() = default;
    Lease(Lease&& o) noexcept : e_(o.e_), s_(o.s_), used_(o.used_) { o.e_ = nullptr; }
    Lease& operator=(Lease&& o) noexcept {
      if (this != &o) {
        release();
        e_ = o.e_;
        s_ = o.s_;
        used_ = o.used_;
        o.e_ = nullptr;
      }
      return *this;
    }
    ~Lease() { release(); }
    DeviceEngine* operator->() const { return e_; }
    DeviceEngine& operator*() const { return *e_; }
    explicit operator bool() const { return e_ != nullptr; }
    hipStream_t use(hipStream_t s);
    hipStream_t stream() { return used_ ? s_ : use(own_stream()); }

   private:
    friend class DeviceEngine;
    explicit Lease(DeviceEngine* e) : e_(e) {}
    void release();  // records the end event, returns the engine to its pool
    hipStream_t own_stream() const;
    DeviceEngine* e_ = nullptr;
    hipStream_t s_ = nullptr;
    bool used_ = false;
  };
  // Blocks while every engine of the device is leased.  An empty lease on failure.
  static Lease acquire(int dev);
  // The same without blocking: an empty lease when every engine of the device is leased.
  static Lease try_acquire(int dev);

  // All launches are asynchronous on `stream`; stats are filled when `stats` is
  // non-null (this synchronises on the stream's end event).
  hipError_t run_chain(const DeviceFst& rhs, const ChainInput& in, uint32_t n, int semantics,
                       const BatchOutDev& out, hipStream_t stream, LaunchStats* stats);
  // Whether run_chain's first tier for these semantics is a pull tier (eager tier P, the
  // lazy pull): only those wait for streamed labels (ChainInput::ready) and copy their
  // paths out (BatchOutDev::host_ol), so the streamed host batch needs it.  run_chain
  // refuses streamed inputs otherwise.
  static bool pull_first(const DeviceFst& rhs, int semantics);
  // kernel_ms of a deferred LaunchStats, once the caller has synchronised the stream
  hipError_t finish_deferred(LaunchStats* stats);
  // The streamed host batch's parts (c_api.cpp run_streamed): the pull tier alone on `in`
  // (pull_first must hold), no fills or copies on `stream` (a fill or copy is a blit that
  // waits for CU slots behind the other engine's persistent kernel) and no host
  // synchronisation; item_ctr zeroed and statuses filled by the caller.  The later tiers
  // then run once over the whole batch: run_chain with set_after_pull(true).
  hipError_t launch_pull_part(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                              int semantics, const BatchOutDev& out, hipStream_t stream,
                              unsigned int* item_ctr, bool text = false, bool codes = false);
  // codes = true (the streamed label batch, pull_codes_table holds): tier P's weight-code
  // instance; out.out_w / out.host_w hold the byte arenas (launch_eager_pull_codes).
  // text = true (the streamed text batch): `in` holds bytes (ChainInput::text), `out` the
  // text outputs (BatchOutDev::text, with slots and without host_ol), and the pull tier's
  // text instance runs.  Otherwise host_w without host_ol is refused: it shares text's place.
  // run_chain after launch_pull_part: the statuses are the pull tier's (no INTERNAL fill,
  // no pull launch); the later tiers take the strings it handed on.
  void set_after_pull(bool v) { after_pull_ = v; }
  // Out of HBM: the workspaces of the device's idle engines (kept per engine between calls)
  // go back to the device (all but `except`'s; hipFree outside the pool lock).
  static void trim_idle(int dev, const DeviceEngine* except = nullptr);
  hipError_t run_graph(const DeviceFst& rhs, const GraphInput& in, uint32_t n, int semantics,
                       const BatchOutDev& out, hipStream_t stream, LaunchStats* stats);
  // A batch of general lhs (fst_compose_frozen_shortest_path_lhs_batch), `b` as LhsBatchDev
  // describes it.  Lazy (semantics 0): the hashed replay, one wave per item, table tiers 1024
  // tuples x16 up to 2^26.  Eager (1): the general BFS engine's tier ladder with the 1-best in
  // the kernel, over b's two item lists in turn.  Items no tier holds end OVERFLOW.
  // Synchronises on `stream` between tiers.
  hipError_t run_lhs_batch(const DeviceFst& rhs, const LhsBatchDev& b, uint32_t n, int semantics,
                           const BatchOutDev& out, hipStream_t stream, LaunchStats* stats,
                           LhsRoute* route);
  // The LhsBatchDev of a batch that is already in device memory (the device-resident lhs
  // entries): lhs_prepare_kernel validates every item against in.total_states / total_arcs and
  // writes descriptors, local arc offsets and flags into the engine's workspaces (kinds of
  // their own: run_lhs_batch uses the others in the same call); lhs_lists_kernel builds the two
  // eager item lists; one small D2H brings the totals back.  The batch's arc arrays are the
  // caller's, read in place (`arc_il`: the one the prepare kernel does not read).  A batch whose
  // state_offsets decrease somewhere is prepared a second time with every item invalid.
  // in.base_flags is set here, from the rhs (lhs_base_flags; null: no rhs,
  // fst_device_shortest_path_lhs).  Synchronises `stream`.
  hipError_t prepare_lhs(const DeviceFst* rhs, LhsPrepIn in, const uint32_t* arc_il,
                         hipStream_t stream, LhsBatchDev* batch, LhsPrepared* prepared);
  // fst_shortest_path of every item of an lhs batch (fst_shortest_path_lhs_batch; kernels/
  // lattice_sp.hpp); b's extents size the workspaces.  The wave tier takes the non-negative
  // items and hands what its sweep budget (FSTAMD_SP_SWEEPS) does not settle to the frontier
  // tier; the replay tier takes the others.  Items the arena cannot hold end OUTPUT_FULL, the
  // cursor at what the batch needs.  Synchronises `stream`.
  hipError_t run_sp_batch(const LhsBatchDev& b, uint32_t n, const BatchOutDev& out,
                          hipStream_t stream, LaunchStats* stats, LhsRoute* route);
  // The n best distinct paths of every item of an lhs batch (fst_nbest_lhs_batch; kernels/
  // lattice_nbest.hpp): item i's k-th best is string i * n + k of `out`, which has room for
  // num * n strings; 1 <= n <= kNbestMax.  The LDS tier (one wave per item, a budget of
  // 4 KiB + n KiB of LDS per workgroup, or FSTAMD_NBEST_LDS bytes; 0: no item fits) hands the
  // items whose tables do not fit to the HBM tier, whose workspace b's extents size (it is
  // allocated only when an item needs it).  Strings the arena cannot hold end OUTPUT_FULL, the
  // cursor at what the batch needs.  route: t[0..1] = items the LDS / HBM tier finished.
  // unique (fst_nbest_unique_lhs_batch, engine 14): the n best paths with pairwise different
  // output texts, by the instances that carry a text hash per list entry; their tables take
  // 24 B per entry against the same budget, and the workspace holds the hashes too.
  // Synchronises `stream`.
  hipError_t run_nbest_batch(const LhsBatchDev& b, uint32_t n, bool unique,
                             const BatchOutDev& out, hipStream_t stream, LaunchStats* stats,
                             LhsRoute* route);
  // The beam cut of every item of an lhs batch (fst_prune_lhs_batch; kernels/lattice_prune.hpp):
  // forward and backward distances, then the mark pass into v's outputs (the caller's: item,
  // status, start, sfin, snext; everything else of `v` is filled here, b's extents size the
  // workspaces).  The wave tier takes every item and hands what its sweep budget
  // (FSTAMD_PRUNE_SWEEPS) does not settle to the frontier tier.  The trim ladder on the shadow
  // view is the caller's next step (host::prune_lattices).  route: t[0..1] = items the wave /
  // frontier tier finished.  Synchronises `stream`.
  hipError_t run_prune_batch(const LhsBatchDev& b, double beam, LatPruneDev v, hipStream_t stream,
                             LaunchStats* stats, LhsRoute* route);
  // Arc posteriors of every item of an lhs batch (fst_posterior_lhs_batch; kernels/
  // lattice_posterior.hpp): v's outputs are the caller's (status, total, alpha, beta, arc_cost;
  // alpha and beta may be null), everything else of `v` is filled here.  The wave tier (one wave
  // per item, a budget of 8 KiB of LDS per workgroup, or FSTAMD_POSTERIOR_LDS bytes; 0: no item
  // fits) hands the items whose tables do not fit to the workgroup tier, whose workspace b's
  // extents size (it is allocated only when an item needs it).  route: t[0..1] = items the wave /
  // workgroup tier finished.  Synchronises `stream`.
  hipError_t run_posterior_batch(const LhsBatchDev& b, LatPostDev v, hipStream_t stream,
                                 LaunchStats* stats, LhsRoute* route);
  // fst_compose_frozen: the whole lattice of one general lhs (kernels/eager_bfs.hpp), on
  // `stream` (synchronised: the lattice is downloaded).
  hipError_t compose_lattice(const DeviceFst& rhs, const GraphInput& lhs, HostLattice* lat,
                             LaunchStats* stats, hipStream_t stream);
  // The lattice batch (fst_compose_frozen_batch / _lhs_batch): the tier ladder of run_lhs_eager
  // over every item, with the emitting instances of eager_bfs_kernel (chain: `lhs` null,
  // in.labels / offsets; else in.lhs_desc and *lhs as for run_lhs_batch).  `lat` is the host
  // copy of the arena's description; `out` carries statuses (its path arrays only take the
  // zeroes of non-OK items).  Resets the arena's cursors.  Items no tier holds end OVERFLOW,
  // items the arena cannot hold OUTPUT_FULL.  Synchronises `stream` between tiers.
  hipError_t run_lattice_batch(const DeviceFst& rhs, const ChainInput& in, const GraphInput* lhs,
                               const LatticeOutDev& lat, const BatchOutDev& out,
                               hipStream_t stream, LaunchStats* stats, LhsRoute* route);
  // The arena in item order, step 1: csr.status (non-OK items own nothing), csr.state_offsets
  // and the items' arc bases (a workspace) by two scans.  Synchronises; needed = {states, arcs}.
  hipError_t compact_lattices_count(const int32_t* status, const LatticeOutDev& lat, uint32_t num,
                                    const LatticeCsrDev& csr, uint64_t needed[2],
                                    hipStream_t stream);
  // Step 2 (after step 1 on the same engine; needed within csr's capacities): start, finals,
  // global arc offsets with the closing entry, and the arcs.  Asynchronous on `stream`.
  // `trim` (a trimmed arena: host::trim_lattices): the filtering gather instead.
  hipError_t compact_lattices(const LatticeOutDev& lat, uint32_t num, const LatticeCsrDev& csr,
                              hipStream_t stream, const LatTrimDev* trim = nullptr);
  // Output tape of each path of a finished stage as the next stage's chain inputs
  // (printOutputString + compileString on device): next_labels = the path's non-epsilon
  // olabels.  A string whose status is not OK, or whose output has a label > 256, gets
  // the single input label kDeadLabel (no rhs arc matches it: the next stage reports
  // EMPTY) and its reason in proj_status.  Synchronises on `stream` (returns max_len).
  hipError_t project_output(const BatchOutDev& stage, uint32_t num, uint32_t* next_labels,
                            uint64_t* next_offsets, int32_t* proj_status, uint32_t* max_len,
                            hipStream_t stream);
  // The batch result in CSR order, on the device: status (with `fail`, when given, taking
  // precedence: a pipeline's first failing stage), path offsets over the OK strings'
  // paths, the arcs gathered from the arena, final weights (+inf unless OK).  il / ol / w
  // hold out_cap arcs (the arena's used arcs); no path is written past them.  Synchronises
  // on `stream`; *total = arcs (> out_cap only if an engine broke its arena invariant).
  hipError_t compact_paths(const BatchOutDev& s, uint32_t num, const int32_t* fail,
                           int32_t* status, uint64_t* offsets, uint32_t* il, uint32_t* ol,
                           double* w, double* fin, uint64_t out_cap, uint64_t* total,
                           hipStream_t stream);
  // Text entries (kernels/text_io.hpp).  widen_text: labels[k] = text[k] + 1 over
  // [offsets[0], offsets[num]) (compileString for the batch), asynchronous on `stream`.
  hipError_t widen_text(const uint8_t* text, const uint64_t* offsets, uint32_t num,
                        uint32_t* labels, hipStream_t stream);
  // A finished (last) stage as text, step 1: per string its status (`fail` as in
  // compact_paths; UNSUPPORTED for an olabel > 256), its byte count scanned into
  // offsets[num + 1], and total_w = the serial fold of the path's weights and the final
  // weight (+inf unless OK).  Synchronises on `stream`; *total = the bytes of the batch.
  hipError_t text_count(const BatchOutDev& s, uint32_t num, const int32_t* fail, int32_t* status,
                        uint64_t* offsets, double* total_w, uint64_t* total, hipStream_t stream);
  // Step 2: the OK strings' bytes (non-epsilon olabels - 1) at their offsets; no byte at or
  // past `cap` is written.  Asynchronous on `stream`.
  hipError_t text_write(const BatchOutDev& s, uint32_t num, const int32_t* status,
                        const uint64_t* offsets, uint8_t* text, uint64_t cap, hipStream_t stream);
  // Input spans per output symbol (kernels/text_align.hpp).  align_write: a finished stage's
  // (b, e) per non-epsilon olabel at offsets[i] + rank -- `offsets` [num + 1] are text_count's
  // or project_output's for that stage -- and consumed[i] = the non-epsilon ilabels of the
  // path; a string whose entries are not its path's (no bytes, a dead label) gets [0, 0) and
  // 0.  No entry at or past `cap` is written.  align_compose: the gather of the outer stage's
  // (b, e) through the running map (in_begin, in_end at inner_off) of the stage before it;
  // out_* may be b and e themselves.  Both asynchronous on `stream`.
  hipError_t align_write(const BatchOutDev& s, uint32_t num, const uint64_t* offsets,
                         uint32_t* begin, uint32_t* end, uint64_t cap, uint32_t* consumed,
                         hipStream_t stream);
  hipError_t align_compose(uint32_t num, const uint64_t* outer_off, const uint32_t* b,
                           const uint32_t* e, const uint64_t* inner_off,
                           const uint32_t* in_begin, const uint32_t* in_end, const uint32_t* n1,
                           uint32_t* out_begin, uint32_t* out_end, uint64_t cap,
                           hipStream_t stream);
  // The streamed text batch's strings the pull tier handed on, once the later tiers have
  // written their paths to the arena's fixed slots: the same emission (emit_text_paths) for
  // every string whose `first` status is neither OK nor EMPTY.  Asynchronous on `stream`.
  hipError_t text_fixup(const BatchOutDev& s, const TextOutDev& tx, const int32_t* first,
                        uint32_t num, hipStream_t stream);
  // fail[i] = st[i] where fail[i] is still OK (the first failing stage wins).
  hipError_t merge_status(int32_t* fail, const int32_t* st, uint32_t num, hipStream_t stream);
  // fst_shortest_path on an explicit graph; `g` holds the FST itself (CSR, arcs in
  // insertion order).  nonneg: every weight >= +0 (parallel fixpoint); otherwise the exact
  // one-lane replay of the reference's heap order (sp_replay_kernel).  No NaN weights.
  // Runs on `stream` and synchronises it.
  hipError_t shortest_path_graph(const GraphInput& g, uint32_t n, const BatchOutDev& out,
                                 LaunchStats* stats, hipStream_t stream, bool nonneg = true);

  int dev() const { return dev_; }
  int num_cus() const { return num_cus_; }

 private:
  explicit DeviceEngine(int dev);
  // The stats bracket: ev0_, body() (a callable returning hipError_t), ev1_, kernel_ms.
  template <class F>
  hipError_t timed(LaunchStats* stats, hipStream_t stream, F&& body);
  // run_chain's routes (device_engine.hip chain_route): run_chain's arguments and the counter
  // block, its prologue words zeroed.  lazy_lds_sizes: the LDS replays at the head of the dense
  // route; (*todo, *todo_n) = the device list of the strings they left OVERFLOW and its length.
#define FSTAMD_ROUTE_ARGS                                                                      \
  const DeviceFst &rhs, const ChainInput &in, uint32_t n, const BatchOutDev &out,              \
      hipStream_t stream, LaunchStats *stats, unsigned int *counter
  hipError_t route_eager_tiers(FSTAMD_ROUTE_ARGS);
  hipError_t route_lazy_dense(FSTAMD_ROUTE_ARGS);
  hipError_t route_lazy_rounds(FSTAMD_ROUTE_ARGS);
  hipError_t route_lazy_hashed(FSTAMD_ROUTE_ARGS);
  hipError_t lazy_lds_sizes(FSTAMD_ROUTE_ARGS, const uint32_t** todo, uint32_t* todo_n);
#undef FSTAMD_ROUTE_ARGS
  hipStream_t stream_ = nullptr;   // the engine's own stream (non-blocking)
  bool after_pull_ = false;        // run_chain: the pull tier already ran (set_after_pull)
  void take_scratch(std::vector<void*>* out);  // an idle engine's workspaces, to be freed
  hipEvent_t done_ = nullptr;      // recorded when a lease ends (on the stream it used)
  hipStream_t done_stream_ = nullptr;
  bool done_valid_ = false;
  // General engine (kernels/eager_bfs.hpp) over the strings of `in` whose status is
  // UNSUPPORTED or OVERFLOW after the layered tiers (all strings when `all`); eager
  // shortestPath or, with `lazy`, composeShortestPath semantics (finite weights >= 0).
  // Grows its per-string workspace in tiers.  Synchronises on `stream` to size the tiers.
  hipError_t run_bfs_chain(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                           const BatchOutDev& out, hipStream_t stream, bool all,
                           bool lazy = false, bool replay = false);
  // composeShortestPath on layered lattices (kernels/lazy_layered.hpp); strings it does
  // not take end UNSUPPORTED / OVERFLOW for run_bfs_chain.
  hipError_t run_lazy_layered(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                              const BatchOutDev& out, hipStream_t stream,
                              const uint32_t* items = nullptr,
                              const uint32_t* num_items_dev = nullptr);
  // composeShortestPath on layered lattices by the layer-local pull (kernels/lazy_pull.hpp);
  // the strings it hands on (OVERFLOW) are listed in *list, their count at *count_dev.
  hipError_t run_lazy_pull(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                           const BatchOutDev& out, hipStream_t stream, uint32_t** list,
                           uint32_t** count_dev, bool launch = true);
  // composeShortestPath as a dense-indexed exact replay (kernels/lazy_dense.hpp), for rhs
  // with input epsilons; strings it does not take end UNSUPPORTED / OVERFLOW for
  // run_bfs_chain.  *ran = false: it took none (the lattice exceeds its dense index).
  // subset_dev (device, subset_n entries): only those strings (nullptr: all).
  hipError_t run_lazy_dense(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                            const BatchOutDev& out, hipStream_t stream, bool* ran,
                            const uint32_t* subset_dev = nullptr, uint32_t subset_n = 0);
  // composeShortestPath with the wave's tables in LDS (kernels/lazy_tiny.hpp, tier t holds
  // 64 << t tuples: 1 = 128 ... 4 = 1024) over a device list of strings (nullptr: all);
  // strings whose lattice outgrows it end OVERFLOW.
  // The band replay (kernels/lazy_band.hpp); *ran = false when the rhs or the batch is not
  // its (arcs going backwards, lengths > 4095); strings it hands on end OVERFLOW.  capped:
  // back pointers only for the first 2 x window states past the start (the early exit's
  // footprint), strings reaching beyond end OVERFLOW.
  hipError_t run_lazy_band(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                           const BatchOutDev& out, hipStream_t stream, bool* ran,
                           const uint32_t* subset_dev = nullptr, uint32_t subset_n = 0,
                           bool capped = false);
  hipError_t launch_lazy_hashed(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                                const BatchOutDev& out, hipStream_t stream, uint64_t want_nodes,
                                const uint32_t* items, uint32_t num_items, unsigned int* ctr,
                                uint32_t* grid_out, const GraphInput* lhs_batch = nullptr);
  // run_lhs_batch's eager ladder over one item list (replay: the heap-replay route).
  hipError_t run_lhs_eager(const DeviceFst& rhs, const ChainInput& in, const GraphInput& lhs,
                           uint32_t n, const uint32_t* items, uint32_t count, bool replay,
                           const BatchOutDev& out, hipStream_t stream, LhsRoute* route,
                           uint32_t* grid_out);
  // The tier ladder of the general BFS engine over a device item list (LDS 128, LDS 256, tier
  // 0, then 256-thread tiers x8; OVERFLOW items move on), shared by run_bfs_chain,
  // run_lhs_eager and run_lattice_batch, which differ in the kernel a tier launches (`kind`:
  // an LhsTier shape).
  struct BfsLadder {
    int first = -2;             // first tier: -2 / -1 (LDS 128 / 256 tuples) or 0 (HBM)
    bool replay = false;        // heap-replay workspaces
    bool lazy = false;          // BfsWs::lazy
    bool wg0 = false;           // tier 0 as kLhsTierWG (256 threads, 4 per CU), not one wave
    bool prof = false;          // FSTAMD_BFS_PROF: the phase profile, one line per tier
    uint32_t lattice_only = 0;  // BfsWs::lattice_only
    uint32_t grid_cap = 0xFFFFFFFFu;      // FSTAMD_GRAPH_GRID of the batches
    std::function<int(int kind)> per_cu;  // resident workgroups per CU of an LDS tier
    std::function<hipError_t(int kind, const BfsWs& ws, unsigned int* next_item,
                             const uint32_t* list, const uint32_t* count_dev, uint32_t grid)>
        launch;
    // optional, after a tier's hand-over: the items it took and those it handed on
    std::function<void(int tier, uint32_t count_in, uint32_t count_out)> after;
  };
  hipError_t run_bfs_ladder(uint32_t count, uint32_t* list, uint32_t* list2, uint32_t* cnt,
                            const int32_t* status, const BfsLadder& L, hipStream_t stream,
                            LhsRoute* route, uint32_t* grid_out);
  hipError_t run_lazy_tiny(const DeviceFst& rhs, const ChainInput& in, uint32_t n,
                           const BatchOutDev& out, hipStream_t stream, int tier,
                           const uint32_t* items, uint32_t num_items, unsigned int* ctr,
                           uint32_t* grid_out);
  void* scratch(size_t idx, size_t bytes);
  int dev_;
  int num_cus_ = 0;
  std::vector<void*> bufs_;
  std::vector<size_t> sizes_;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
  size_t lazy_hash_bytes_ = 0;   // hash table stamps are valid for this allocation
  uint32_t lazy_stamp_ = 0;      // next stamp base (bumped per launch)
  void* ll_clean_ = nullptr;     // lazy-layered dense arrays initialised for this allocation
  size_t ll_clean_bytes_ = 0;
  void* ld_clean_ = nullptr;     // lazy-dense rec / leaf arrays initialised for these allocations
  size_t ld_clean_bytes_ = 0;
  void* ld_leaf_ = nullptr;
  size_t ld_leaf_bytes_ = 0;
  void* lb_clean_ = nullptr;     // band-replay window initialised for this allocation
  size_t lb_clean_bytes_ = 0;
};

}  // namespace fstamd

/*
 * fst_batch.h -- batched entry points of libfst_amd (new; no libfst counterpart).
 *
 * A batch is N linear-chain acceptors given as CSR label sequences
 * (labels[offsets[i] .. offsets[i+1]) for string i).  Each string is the FST
 * `fst_compile_string` would build (src/string.zig:24-50): state k --l:l/One-->
 * k+1, final(L) = One; labels are used as given (fst_compile_string's byte+1
 * encoding is the caller's choice).  Every string is composed against ONE
 * frozen rhs FstHandle and reduced to its 1-best path with either
 *   FST_SEM_LAZY : the result fst_compose_frozen_shortest_path(a, b, n) returns
 *                  (src/ops/compose-shortest-path.zig:26-401), or
 *   FST_SEM_EAGER: the result fst_shortest_path(fst_compose_frozen(a, b), n)
 *                  returns (src/ops/compose.zig:29-198 then
 *                  src/ops/shortest-path.zig:18-139) -- what the reference bench
 *                  scenario compose_frozen_shortest_path_* measures.
 * The two agree on weight but may pick different equal-weight paths.
 *
 * Per-string results use the FST_PATH_* codes; a string with FST_PATH_OK has a
 * result chain of path_len arcs (states 0..path_len, start 0, final(path_len) =
 * final_weight), FST_PATH_EMPTY is the reference's empty FST.
 */
#ifndef LIBFST_AMD_FST_BATCH_H
#define LIBFST_AMD_FST_BATCH_H

#include "fst.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    FST_SEM_LAZY = 0,
    FST_SEM_EAGER = 1,
} FstSemantics;

typedef enum {
    FST_PATH_OK = 0,           /* a 1-best chain */
    FST_PATH_EMPTY = 1,        /* empty result FST (no path, n == 0, or rhs has no start) */
    FST_PATH_ERROR_N = 2,      /* n not in {0, 1}: the reference returns FST_INVALID_HANDLE */
    FST_PATH_CYCLE = 3,        /* back-pointer cycle; the reference would not terminate */
    FST_PATH_OVERFLOW = 4,     /* internal: engine capacity exceeded (retried internally) */
    FST_PATH_UNSUPPORTED = 5,  /* input outside every available engine's contract */
    FST_PATH_OUTPUT_FULL = 6,  /* device arc arena too small */
    FST_PATH_INTERNAL = 7,     /* engine invariant violated (a bug), reported, never silent */
} FstPathStatus;

/* Host-memory result of a batch, allocated by the library (pooled pinned host blocks the
 * device writes by DMA) and valid until fst_batch_result_free(), which returns them. */
typedef struct {
    uint32_t num_strings;
    int32_t* status;          /* [num_strings] FstPathStatus */
    uint64_t* path_offsets;   /* [num_strings + 1] CSR offsets into the arc arrays */
    uint32_t* ilabels;        /* [total_arcs] */
    uint32_t* olabels;        /* [total_arcs] */
    double* weights;          /* [total_arcs] */
    double* final_weights;    /* [num_strings] */
    uint64_t total_arcs;
} FstBatchResult;

/* Multi-GPU batches inside the library: with FST_BATCH_DEVICES in flags the
 * host entries (fst_compose_frozen_shortest_path_batch, fst_pipeline_batch) split the
 * strings into contiguous shards balanced by estimated work (sum over the string's input
 * positions of the rhs states a layer can hold) and run one shard per device of
 * device_mask (bit d = HIP device d), each on its own host thread, with the frozen rhs
 * replicated to every device on first use (one DMA from its pinned host copy).  Results
 * are gathered into one FstBatchResult in input order, identical to a one-device run.
 * num_shards > popcount(device_mask) runs several shards per device (round robin) on
 * separate engines and streams; 0 = one per device.  No collective runs on the data path. */
#define FST_BATCH_DEVICES 1u

/* The work estimate the shard planner uses for one chain string of `len` labels against
 * rhs b (product tuples: the sum over input positions of the rhs states a layer can hold),
 * for callers that shard batches over processes themselves (one rank per GPU); < 0 for an
 * invalid handle. */
double fst_chain_cost(FstHandle b, uint64_t len);

typedef struct {
    int32_t device;           /* HIP device ordinal (-1: current device); without
                                 FST_BATCH_DEVICES the whole batch runs there */
    uint32_t semantics;       /* FstSemantics */
    uint32_t flags;           /* FST_BATCH_DEVICES or 0 */
    uint32_t num_shards;      /* with FST_BATCH_DEVICES: shards (0 = one per device) */
    uint64_t device_mask;     /* with FST_BATCH_DEVICES: the devices (0 = `device` only) */
} FstBatchOptions;

/* Host arrays in, host result out (H2D, kernels, D2H).  Returns FST_INVALID_ARG for an
 * invalid handle or malformed offsets; per-string outcomes are in out->status.  Once the
 * arguments are checked, *out is zeroed before anything else: on any error return it holds
 * nothing (a result the caller still owned in that struct must be freed beforehand). */
FstError fst_compose_frozen_shortest_path_batch(FstHandle b, const uint32_t* labels,
                                                const uint64_t* offsets, uint32_t num_strings,
                                                uint32_t n, const FstBatchOptions* opts,
                                                FstBatchResult* out);
void fst_batch_result_free(FstBatchResult* r);

/* Batch of general lhs FSTs: word lattices, confusion networks, n-best unions -- anything
 * fst_compose_frozen_shortest_path takes as `a`, many at once.
 *
 * N lhs FSTs as one concatenated CSR (host memory).  lhs i owns the states
 * [state_offsets[i], state_offsets[i+1]) of the per-state arrays; state ids inside
 * an lhs (start, nextstates) are local to it.  Arcs of a state are in insertion
 * order (MutableFst order: it decides ties, compose.zig:95-194). */
typedef struct {
    uint32_t num_fsts;
    const uint64_t* state_offsets;  /* [num_fsts + 1] */
    const uint32_t* start;          /* [num_fsts], FST_NO_STATE: no start */
    const double*   final_weights;  /* [total_states], +inf: not final */
    const uint64_t* arc_offsets;    /* [total_states + 1] */
    const uint32_t* ilabels;        /* [total_arcs] */
    const uint32_t* olabels;
    const double*   weights;
    const uint32_t* nextstates;     /* local to the arc's lhs */
} FstLhsBatch;

/* Per item the result is, bit for bit (labels, arc weights times(w_lhs, w_rhs), final
 * times(fw1, fw2)),
 *   FST_SEM_LAZY : what fst_compose_frozen_shortest_path(a_i, b, n) returns,
 *   FST_SEM_EAGER: what fst_shortest_path(fst_compose_frozen(a_i, b), n) returns,
 * as a status and a 1-best chain in the FstBatchResult (fst_batch_result_free,
 * fst_batch_result_to_text work on it unchanged).  Statuses as for the chain entries: no
 * start in the lhs (an lhs of zero states has none) or the rhs, or n == 0: EMPTY (checked
 * before n, compose-shortest-path.zig:30-33); other n != 1: ERROR_N; a back-pointer cycle:
 * CYCLE; a NaN weight in the item (or the rhs): UNSUPPORTED.  OVERFLOW / OUTPUT_FULL are
 * retried internally.
 * Checked on the host before any device work, each FST_INVALID_ARG with *out zeroed: null
 * pointers, decreasing state_offsets or arc_offsets, arc_offsets[0] != 0, a start or
 * nextstate at or beyond the item's state count, an item of 2^30 or more states or 2^32 or
 * more arcs, unknown flags, an invalid rhs handle.  num_fsts == 0 gives an empty OK result.
 * FST_BATCH_DEVICES shards the items as for the label entries (balanced by arcs + 1 per
 * item); the result is in input order and byte-identical to a one-shard run. */
FstError fst_compose_frozen_shortest_path_lhs_batch(FstHandle b, const FstLhsBatch* lhs,
                                                    uint32_t n, const FstBatchOptions* opts,
                                                    FstBatchResult* out);
/* Same, from handles: each a[i] is snapshotted under its lock as the single call does
 * (c-api.zig:754); an invalid handle is FST_INVALID_ARG for the call. */
FstError fst_compose_frozen_shortest_path_handles_batch(FstHandle b, const FstMutableHandle* a,
                                                        uint32_t num, uint32_t n,
                                                        const FstBatchOptions* opts,
                                                        FstBatchResult* out);

/* Device-resident batch: every pointer is device memory on opts->device; the call is
 * asynchronous on `stream` (a hipStream_t, or NULL for the null stream).  Paths are
 * appended to the arc arena; *arc_cursor (device) is reset by the call.  `work`, if
 * non-NULL, receives two counters per string: product states and relaxations.
 * max_len (fst_device_compose_shortest_path) is the caller's bound on the strings'
 * lengths: it sizes workspaces and picks kernels (e.g. f32 cells when every distance
 * stays an exact integer below 2^24).  A string longer than max_len is still answered
 * exactly, by a slower tier.
 *
 * The stream contract of every fst_device_* entry that takes a `stream` (each comment says
 * which of the two it is; tests/test_gpu_device_streams.py pins it on a non-blocking stream):
 *   - inputs are read, and outputs written, in `stream` order, after the work the caller
 *     queued on `stream` before the call: buffers that earlier work on `stream` is still
 *     filling are valid arguments;
 *   - an entry that is asynchronous on `stream` may return with its work still queued: later
 *     work on `stream` sees the result, the host and other streams only after they have
 *     waited for `stream`.  It may also wait for `stream` on some routes; callers rely on
 *     neither;
 *   - an entry that synchronises `stream` returns with the result complete and its host
 *     outputs (needed, total_bytes, max_len) set;
 *   - no other stream of the caller is waited on, the null stream included when `stream` is
 *     non-blocking: what the call reads must be ordered before it on `stream` itself.
 * The library's own workspaces pass from one call to the next in order, whatever streams the
 * two calls use. */
typedef struct {
    int32_t* status;            /* [num_strings] */
    uint32_t* path_len;         /* [num_strings] */
    uint64_t* path_offset;      /* [num_strings] offset of the string's first arc */
    double* final_weight;       /* [num_strings] */
    uint32_t* ilabels;          /* [arc_capacity] */
    uint32_t* olabels;          /* [arc_capacity] */
    double* weights;            /* [arc_capacity] */
    uint64_t arc_capacity;
    uint64_t* arc_cursor;       /* [1] */
    uint32_t* work;             /* [2 * num_strings] or NULL */
} FstDeviceBatch;

FstError fst_device_compose_shortest_path(FstHandle b, const uint32_t* d_labels,
                                          const uint64_t* d_offsets, uint32_t num_strings,
                                          uint32_t max_len, uint32_t n,
                                          const FstBatchOptions* opts, const FstDeviceBatch* out,
                                          void* stream);

/* Multi-stage pipelines (tagger -> verbalizer, README.md:177-214) without host round
 * trips.  The reference app does, per utterance and stage:
 *   print_output_string(best) -> compile_string(bytes) -> compose_frozen_shortest_path.
 * On a 1-best chain that is: next input labels = the path's non-epsilon olabels
 * (src/string.zig:60-97 then :24-50; label = byte + 1 on both sides).
 * fst_device_project_output does that for a whole batch on the device.  A string whose
 * stage status is not OK, or whose output holds a label > 256 (not a byte: the
 * reference's @intCast would trap), gets one input label no rhs carries (the next stage
 * reports EMPTY) and its reason in d_proj_status (the stage's status, or
 * FST_PATH_UNSUPPORTED for a non-byte label).  d_next_labels needs room for the sum of
 * path_len plus num_strings; d_next_offsets for num_strings + 1.  The call
 * synchronises `stream` and returns the longest projected input in *max_len. */
FstError fst_device_project_output(const FstDeviceBatch* stage, uint32_t num_strings,
                                   uint32_t* d_next_labels, uint64_t* d_next_offsets,
                                   int32_t* d_proj_status, uint32_t* max_len, void* stream);

/* Host convenience: runs num_stages frozen FSTs in sequence on one device, each stage's
 * 1-best output tape feeding the next (fst_device_project_output in between).  The
 * result holds the last stage's paths; a string that failed at an earlier stage reports
 * that stage's status.  Semantics / device from opts (NULL: lazy, current device). */
FstError fst_pipeline_batch(const FstHandle* stages, uint32_t num_stages, const uint32_t* labels,
                            const uint64_t* offsets, uint32_t num_strings, uint32_t n,
                            const FstBatchOptions* opts, FstBatchResult* out);

/* Pipelines on a general first stage: lattices in, labels or text out (a recogniser's
 * confusion networks through tagger -> verbalizer without a host round trip in between).
 * Per item, bit for bit:
 *   - stage 1 is what fst_compose_frozen_shortest_path_lhs_batch(stages[0], lhs, n, opts)
 *     returns for the item, statuses and path;
 *   - each later stage takes the previous stage's 1-best output tape as a chain, exactly as
 *     fst_pipeline_batch does between its stages (fst_device_project_output: the non-epsilon
 *     olabels are the next input, an olabel above 256 makes the item FST_PATH_UNSUPPORTED, an
 *     item that failed earlier reports that stage's status).
 * fst_pipeline_lhs_batch returns the last stage's paths as an ordinary FstBatchResult
 * (fst_batch_result_free, fst_batch_result_to_text).  fst_normalize_lhs_batch (n is 1) returns
 * the text fst_normalize_text_batch documents below for every producer, emitted on the
 * device: no path arena is downloaded; with num_stages == 1 it equals
 * fst_batch_result_to_text of the lhs batch entry's result byte for byte.
 * Checked on the host before any device work, each FST_INVALID_ARG with *out zeroed:
 * everything fst_compose_frozen_shortest_path_lhs_batch checks (the same validator), a null
 * `stages`, num_stages == 0, an invalid stage handle.  num_fsts == 0 gives the empty OK
 * result.  FST_BATCH_DEVICES shards as the lhs batch entry does (arcs + 1 per item); the
 * result is in input order and byte-identical to a one-shard run.
 * (fst_normalize_lhs_batch is declared after FstTextResult, below.) */
FstError fst_pipeline_lhs_batch(const FstHandle* stages, uint32_t num_stages,
                                const FstLhsBatch* lhs, uint32_t n,
                                const FstBatchOptions* opts, FstBatchResult* out);

/* Device-resident batch of general lhs: the struct `d_lhs` is in host memory, every pointer
 * in it is device memory on opts->device, in FstLhsBatch's layout.  The finals and the four
 * arc arrays are used in place; a kernel derives what the host entry derives while it stages
 * a batch (per-item descriptors, arc offsets local to the item, the weight flags, the largest
 * out-degree) into workspaces of the library's own, O(items + states) bytes.
 *   - Trusted extents: total_states = state_offsets[num_fsts] and total_arcs =
 *     arc_offsets[total_states].  The host reads these two values and trusts them as the
 *     extents of the per-state arrays (total_states entries; arc_offsets one more) and of the
 *     arc arrays (total_arcs entries): the caller guarantees the arrays are that long.
 *     Nothing outside those extents is read.
 *   - The host cannot read the rest, so FST_INVALID_ARG is only: a null `out`, `d_lhs`, arc
 *     cursor or needed array, unknown flags or semantics, an invalid handle.  What the host
 *     entry rejects per item the kernel checks per item -- state_offsets[i] <=
 *     state_offsets[i + 1] <= total_states, fewer than 2^30 states, arc_offsets non-decreasing
 *     over the item's states and ending at or below total_arcs, fewer than 2^32 arcs, a start
 *     that is FST_NO_STATE or below the item's state count, every nextstate below it -- and
 *     an item that fails is never traversed and reports FST_PATH_UNSUPPORTED; the other items
 *     are unaffected.  One exception: state_offsets must be non-decreasing over the whole
 *     batch, as the host entry demands, because only then do the items own disjoint state
 *     ranges.  If state_offsets[i] > state_offsets[i + 1] for any i, no item is traversed and
 *     every item reports FST_PATH_UNSUPPORTED.
 *   - Statuses in the single call's order: no start in the lhs or the rhs, or n == 0: EMPTY;
 *     other n != 1: ERROR_N; then UNSUPPORTED (an invalid item, a NaN weight).
 *   - Output as for fst_device_compose_shortest_path, so the result chains into
 *     fst_device_project_output, fst_device_compose_shortest_path and fst_device_emit_text: a
 *     device-resident lattice -> text pipeline.  The arena is the caller's: items that do not
 *     fit report FST_PATH_OUTPUT_FULL and *arc_cursor ends at the arcs the batch needs; call
 *     again with that capacity.
 *   - Unlike fst_device_compose_shortest_path the call synchronises `stream` (the engine sizes
 *     its tiers from counts it reads back); it returns with the result complete.
 *   - fst_last_launch_stats reports engine 8 / 9 as for the host entry; `launches` counts
 *     the two preparation kernels too. */
FstError fst_device_compose_shortest_path_lhs(FstHandle b, const FstLhsBatch* d_lhs,
                                              uint32_t n, const FstBatchOptions* opts,
                                              const FstDeviceBatch* out, void* stream);

/* Lattices out: fst_compose_frozen for a whole batch.  Item i of the result is, bit for bit,
 * the MutableFst fst_compose_frozen(a_i, b) returns (src/ops/compose.zig:29-198): states in
 * the reference's BFS ids, arcs of a state in compose order, arc weights times(w_lhs, w_rhs),
 * final weights times(fw1, fw2) (+inf: not final), start 0 when the lattice has states, no
 * trimming.  For the chain entry a_i is the fst_compile_string-style chain of string i's
 * labels (zero labels: the one-state final acceptor).  The result is an FstLhsBatch: &r.fsts is
 * a valid argument of every lhs batch entry, so
 *   compose(project_output(compose(a, tagger)), verbalizer)
 * is two library calls on batches, and the optimum over both stages is kept.
 * With FST_LATTICE_PROJECT_OUTPUT the only difference is ilabels[k] = olabels[k]
 * (src/ops/project.zig, .output).
 * Statuses: FST_PATH_OK is a lattice, and also the reference's empty FST when the lhs or the
 * rhs has no start (zero states, start = FST_NO_STATE).  A NaN weight in the item or the rhs:
 * FST_PATH_UNSUPPORTED, as the lhs batch entry reports it (the single call composes NaNs; this
 * is a documented difference).  FST_PATH_OVERFLOW: no engine tier holds the item (the single
 * call returns FST_INVALID_HANDLE there).  FST_PATH_INTERNAL: the watchdog.  Every non-OK item
 * owns zero states and has start = FST_NO_STATE.  opts->semantics is ignored.
 * Checked on the host before any device work, each FST_INVALID_ARG with *out zeroed: what
 * fst_compose_frozen_shortest_path_lhs_batch checks of an lhs batch (the same validator) /
 * what fst_compose_frozen_shortest_path_batch checks of labels and offsets, unknown bits in
 * lattice_flags or opts->flags, an invalid handle.  Zero items give an empty OK result with
 * state_offsets = {0} and arc_offsets = {0}.  FST_BATCH_DEVICES shards as the 1-best entries
 * do (fst_chain_cost per chain, arcs + 1 per lhs); a sharded result is byte-identical to a
 * one-shard run.  The result lives in pooled pinned blocks until fst_lattice_batch_free. */
typedef struct {
    FstLhsBatch fsts;        /* the lattices; &r.fsts is a valid argument of every lhs batch entry */
    int32_t* status;         /* [fsts.num_fsts] FstPathStatus */
    uint64_t total_states, total_arcs;
} FstLatticeBatch;

#define FST_LATTICE_PROJECT_OUTPUT 1u   /* every arc's ilabel := its olabel (project.zig, .output) */
/* Item i is connect(fst_compose_frozen(a_i, b)) (src/ops/connect.zig:17-124), bit for bit: the
 * states that can reach a final state are kept (compose output is accessible by construction)
 * and renumbered in increasing old id, a kept state's arcs are its old arcs whose target is
 * kept, in their order, with labels and weights copied bit for bit; a final weight of -inf
 * comes out +inf (isFinal is !isInf).  An OK item whose start cannot reach a final state is the
 * reference's empty FST: zero states, start = FST_NO_STATE.  Non-OK items are as without the
 * flag; with FST_LATTICE_PROJECT_OUTPUT as well the only difference remains ilabels[k] =
 * olabels[k].  fst_device_compose_frozen reports the trimmed totals in `needed`.  The trim runs
 * on the device before the compaction, so what shrinks is the compacted result, its download
 * and everything downstream; peak device memory does not.  Opt-in: on lattices without dead
 * ends the pass costs time and removes nothing.
 * The value is 4, not 2: bit 1 is not assigned and stays an unknown flag (FST_INVALID_ARG). */
#define FST_LATTICE_CONNECT 4u

FstError fst_compose_frozen_batch(FstHandle b, const uint32_t* labels, const uint64_t* offsets,
                                  uint32_t num_strings, uint32_t lattice_flags,
                                  const FstBatchOptions* opts, FstLatticeBatch* out);
FstError fst_compose_frozen_lhs_batch(FstHandle b, const FstLhsBatch* lhs, uint32_t lattice_flags,
                                      const FstBatchOptions* opts, FstLatticeBatch* out);
void fst_lattice_batch_free(FstLatticeBatch* r);

/* Connect (trim) of every item of an lhs batch, with no compose: a recogniser's lattices before
 * they meet a grammar, or a lattice batch the caller has rescored.  Item i of the result is
 * connect(lhs_i) as src/ops/connect.zig:17-124 returns it, bit for bit: kept = reachable from
 * the start and able to reach a final state (final: the weight is not +-inf, so NaN is final);
 * new id = rank among the kept states in increasing old id; a kept state's final weight is
 * copied when final and +inf otherwise; its arcs are the old arcs whose target is kept, in the
 * old order.  The result's start is the renumbered old start (it need not be 0).  No start, no
 * states or a start that is not kept: zero states, start = FST_NO_STATE.
 * Every item is FST_PATH_OK: connect never compares weights, so NaN weights are copied, not
 * refused -- unlike the compose entries, which report FST_PATH_UNSUPPORTED for them.
 * The same validator as the other lhs entries runs first (a failed check: FST_INVALID_ARG with
 * *out zeroed; also a null lhs / out, unknown opts->flags).  num_fsts == 0 gives the empty OK
 * result.  There is no rhs and opts->semantics is ignored.  FST_BATCH_DEVICES shards by arcs + 1
 * per item; a sharded result is byte-identical to a one-shard run.  fst_last_launch_stats
 * reports engine 11 (the compose entries keep 10 and count the trim kernels in `launches`).
 * Free with fst_lattice_batch_free. */
FstError fst_connect_lhs_batch(const FstLhsBatch* lhs, const FstBatchOptions* opts,
                               FstLatticeBatch* out);

/* Shortest path of every item of an lhs batch, with no compose: the 1-best of a recogniser's
 * lattices, or of a lattice batch the caller has rescored (LM scores added to the arc weights, a
 * bias on some olabels, a penalty on finals).  Item i is fst_shortest_path(lhs_i, n)
 * (src/ops/shortest-path.zig:18-139), bit for bit, as a status and a 1-best chain in the
 * FstBatchResult.  Per item, in the single call's order (:21-24):
 *   no start (an item of zero states has none) or n == 0       FST_PATH_EMPTY
 *   any other n != 1                                           FST_PATH_ERROR_N
 *   a NaN arc or final weight in the item                      FST_PATH_UNSUPPORTED (the single
 *       call returns an invalid handle there; the compose entries' rule)
 *   no final state reachable, or the backtrace does not end
 *       at the start (:105, :120)                              FST_PATH_EMPTY
 *   a back-pointer cycle (the reference would not terminate)   FST_PATH_CYCLE
 *   otherwise                                                  FST_PATH_OK
 * An OK path's arcs are the item's own arcs, ilabel, olabel and weight copied bit for bit;
 * final_weights[i] is the final weight of the chosen final state, copied; a path of zero arcs
 * (the start is the best final) is FST_PATH_OK with a length of 0.
 * A non-OK item of an FstLatticeBatch owns zero states, so here it comes out FST_PATH_EMPTY:
 * callers feeding &r.fsts should read r.status first.
 * The same validator as the other lhs entries runs first (a failed check: FST_INVALID_ARG with
 * *out zeroed; also a null lhs / out, unknown opts->flags).  num_fsts == 0 gives the empty OK
 * result.  There is no rhs and opts->semantics is ignored.  FST_BATCH_DEVICES shards by arcs + 1
 * per item; a sharded result is byte-identical to a one-shard run.  The result is an ordinary
 * FstBatchResult (fst_batch_result_free, fst_batch_result_to_text).  fst_last_launch_stats
 * reports engine 12. */
FstError fst_shortest_path_lhs_batch(const FstLhsBatch* lhs, uint32_t n,
                                     const FstBatchOptions* opts, FstBatchResult* out);

/* Device-resident: d_lhs as for fst_device_compose_shortest_path_lhs (a host struct of device
 * pointers, trusted extents, per-item validation by the prepare kernel: an item that fails it
 * reports FST_PATH_UNSUPPORTED and is never traversed; state_offsets decreasing anywhere makes
 * every item FST_PATH_UNSUPPORTED), out as for every FstDeviceBatch producer: the arena is the
 * caller's, items that do not fit report FST_PATH_OUTPUT_FULL, *arc_cursor ends at what the
 * batch needs (the total states of the batch always suffice), and the result chains into
 * fst_device_project_output, fst_device_compose_shortest_path and fst_device_emit_text.  So
 * chains -> lattices (fst_device_compose_frozen) -> the caller's rescoring kernel -> 1-best ->
 * text never leaves the device.  The call synchronises `stream`.  Engine 12; `launches` counts
 * the two preparation kernels too. */
FstError fst_device_shortest_path_lhs(const FstLhsBatch* d_lhs, uint32_t n,
                                      const FstBatchOptions* opts, const FstDeviceBatch* out,
                                      void* stream);

/* The n best DISTINCT PATHS of every item of an lhs batch, for ACYCLIC items: what a caller asks
 * of a lattice before it picks a reading with a model of its own (an LM, a bias list, a UI with
 * alternatives).  The reference has no n-best (shortestPath returns UnsupportedNShortest for
 * n > 1, src/ops/shortest-path.zig:14-24), so the definition is this comment.  The result is an
 * ordinary FstBatchResult of num_fsts * n strings: item i's k-th best is string i * n + k, and
 * fst_batch_result_free, fst_batch_result_to_text and fst_batch_result_to_aligned_text work on
 * it unchanged.
 *
 * Per item: states 0 .. S-1, arcs in CSR.  An arc's INDEX a is its position in the item's own
 * arc range; it runs src(a) -> dst(a) with weight w(a).
 * Statuses.  All n strings of an item get the same one, tested in this order:
 *   1. no start, or zero states                                 FST_PATH_EMPTY
 *   2. a NaN arc or final weight anywhere in the item           FST_PATH_UNSUPPORTED
 *   3. a cycle among the states reachable from the start        FST_PATH_UNSUPPORTED
 *      (every arc counts, whatever its weight; a self-loop is a cycle.  Such an item may have
 *      infinitely many paths.  Compose of a chain with an rhs that has no input-epsilon cycle,
 *      confusion networks and recogniser lattices are acyclic.)
 *   4. (device entry) an item the prepare kernel refuses        FST_PATH_UNSUPPORTED
 * An arc of weight +inf is never part of a path (the reference's isZero, :93).
 * A PREFIX is a path from the start.  Its cost g is the f64 left fold ((0.0 + w_1) + w_2) + ...
 * (:72); a prefix whose g is +inf is dropped, by overflow as well.
 * The order of two prefixes that END IN THE SAME STATE, recursively:
 *   1. the smaller g first, compared as f64 values (-0.0 equals +0.0);
 *   2. then the smaller index of the last arc;
 *   3. then, with the same last arc, the order of the two prefixes without it (both end in its
 *      src);
 *   4. the empty prefix at the start has no last arc and sorts after any arc at equal g (it has
 *      no competitor in an acyclic item).
 * A COMPLETE PATH is a prefix that ends in a state t with final(t) != +inf.  Its total is
 * fl(g + final(t)); it is dropped if that is +inf.  Complete paths are ordered by total, then
 * by t, then by the prefix's rank among all prefixes ending in t.
 * String i * n + k is the k-th complete path in that order, FST_PATH_OK: its arcs are the item's
 * own arcs (ilabel, olabel and weight bits copied), its final_weights entry is final(t), copied;
 * the start being final gives a path of zero arcs.  An item of m < n complete paths leaves
 * strings i * n + m .. i * n + n - 1 FST_PATH_EMPTY.  Paths are distinct as arc sequences; two
 * may print the same text (removing those is determinisation, which is not built).
 * How it is computed: E(t), the at most n best prefixes ending in t, each (g, a, r) = cost, last
 * arc, rank of the rest in E(src(a)).  E(start) = [(0.0, none, 0)]; E(t) = the n smallest of
 * {(fl(E(src(a))[r].g + w(a)), a, r)} over the arcs a into t and all r, in (g, a, r)
 * lexicographic order.  f64 addition is monotone in either operand, so a prefix outside its
 * state's top n is never part of a later top n; on an acyclic item every order of evaluation
 * that finishes the predecessors first gives the same lists.
 *
 * The same validator as the other lhs entries runs; a failed check returns FST_INVALID_ARG
 * with *out zeroed, as do n == 0, n > FST_NBEST_MAX, num_fsts * n >= 2^32 (these three are
 * tested before lhs's arrays are read), a null lhs / out and unknown opts->flags.
 * num_fsts == 0 gives the empty OK result.  opts->semantics
 * is ignored.  FST_BATCH_DEVICES shards by arcs + 1 per item; a sharded result is in input order
 * and byte-identical to a one-shard run.  fst_last_launch_stats reports engine 13. */
#define FST_NBEST_MAX 16u
FstError fst_nbest_lhs_batch(const FstLhsBatch* lhs, uint32_t n, const FstBatchOptions* opts,
                             FstBatchResult* out);

/* Device-resident, as fst_device_shortest_path_lhs: d_lhs is a host struct of device pointers
 * with trusted extents, the prepare kernel validates the items, the call synchronises `stream`.
 * `out` has room for num_fsts * n strings; the arena is the caller's, strings that do not fit
 * report FST_PATH_OUTPUT_FULL and *arc_cursor ends at what the batch needs (n * the total
 * states of the batch always suffice: a path of an acyclic item has fewer arcs than the item has
 * states).  The result chains into fst_device_emit_text, fst_device_project_output and
 * fst_device_path_alignment on num_fsts * n strings.  Engine 13; `launches` counts the two
 * preparation kernels too. */
FstError fst_device_nbest_lhs(const FstLhsBatch* d_lhs, uint32_t n, const FstBatchOptions* opts,
                              const FstDeviceBatch* out, void* stream);

/* The n best paths WITH DISTINCT OUTPUT TEXT of every item of an lhs batch, for acyclic items:
 * what OpenFst and Pynini callers know as ShortestPath(nshortest = n, unique = true), without a
 * determinisation.  Everything fst_nbest_lhs_batch says about arguments, validation (the same
 * FST_INVALID_ARG cases, n <= FST_NBEST_MAX, num_fsts * n < 2^32), the result layout (string
 * i * n + k), the item statuses and their order, sharding and the empty batch holds here
 * unchanged; the plain entries and their results do not change.
 * Definition.
 *   The OUTPUT TEXT of a path is the sequence of its non-epsilon olabels (olabel != 0), as u32
 *   labels; a label above 256 is a label like any other here.
 *   Take all complete paths of the item in the order fst_nbest_lhs_batch defines: total, then
 *   final state t, then the prefix order at t.  That order does not depend on n.
 *   Drop every path whose output text equals that of an earlier path.
 *   String i * n + k is the k-th path that is left, FST_PATH_OK; its arcs, weights and final
 *   weight are copied as the plain entry copies them.  An item with m < n distinct texts leaves
 *   the rest FST_PATH_EMPTY.
 * So n = 1 equals fst_nbest_lhs_batch at n = 1 byte for byte, an item whose complete paths all
 * print different texts gives the plain entry's result, and the OK strings of one item have
 * pairwise different output texts.
 * How it is computed: Eu(t), the at most n least prefixes ending in t with pairwise different
 * output texts, each (g, a, r) with r the rank of the rest in Eu(src(a)).  Among the candidates
 * (fl(Eu(src(a))[r].g + w(a)), a, r) with the same text only the least in (g, a, r) order is
 * kept.  Nothing is lost: if n prefixes with other texts precede p at s, their extensions by
 * the same suffix are n complete paths with n other texts, none after p's; the order is strict
 * under extension by one arc, because equal g falls back to the order of the rests.  The final
 * selection applies the same rule across final states: candidates in (total, t, r) order, a
 * candidate whose text was already chosen is passed over.  Texts are compared label by label;
 * a 64-bit hash per prefix only spares comparisons.
 * fst_last_launch_stats reports engine 14. */
FstError fst_nbest_unique_lhs_batch(const FstLhsBatch* lhs, uint32_t n,
                                    const FstBatchOptions* opts, FstBatchResult* out);

/* Device-resident, exactly as fst_device_nbest_lhs: trusted extents, the prepare kernel (an item
 * it refuses is FST_PATH_UNSUPPORTED), the caller's arena with FST_PATH_OUTPUT_FULL and
 * *arc_cursor at what the batch needs, the call synchronises `stream`.  The result chains into
 * fst_device_emit_text: text in, n distinct readings out.  Engine 14. */
FstError fst_device_nbest_unique_lhs(const FstLhsBatch* d_lhs, uint32_t n,
                                     const FstBatchOptions* opts, const FstDeviceBatch* out,
                                     void* stream);

/* The device-resident form, chains in and lattices out, so that a cascade never leaves the
 * device.  Every pointer in `out` is device memory on opts->device, in FstLhsBatch's layout: a
 * host-side FstLhsBatch holding those pointers goes straight into
 * fst_device_compose_shortest_path_lhs.  The call synchronises `stream` (the tier ladder reads
 * counts back).  needed (host memory) receives the states and arcs the batch needs; when
 * either exceeds its capacity only `status` and `needed` are defined and nothing past a
 * capacity is written: call again with larger arrays (the pattern of fst_device_emit_text).
 * FST_INVALID_ARG: a null out / needed / d_offsets or array, unknown flags, an invalid
 * handle.  The host cannot read d_offsets (it reads the first and the last entry, to size its
 * arena): they are TRUSTED, as fst_device_compose_shortest_path trusts them -- the caller
 * guarantees d_offsets[0 .. num_strings] is non-decreasing and that d_labels holds
 * d_offsets[num_strings] labels; nothing is checked per string, and max_len is a hint, not
 * enforced.  num_strings == 0 is valid: needed = {0, 0}, state_offsets[0] = 0 and
 * arc_offsets[0] = 0 are written, status and start may then be NULL.
 * fst_last_launch_stats reports engine 10. */
typedef struct {
    int32_t* status; uint64_t* state_offsets; uint32_t* start;   /* [num], [num + 1], [num] */
    double* final_weights; uint64_t* arc_offsets;                /* [state_capacity], [state_capacity + 1] */
    uint32_t* ilabels; uint32_t* olabels; double* weights; uint32_t* nextstates;  /* [arc_capacity] */
    uint64_t state_capacity, arc_capacity;
} FstDeviceLattices;

FstError fst_device_compose_frozen(FstHandle b, const uint32_t* d_labels, const uint64_t* d_offsets,
                                   uint32_t num_strings, uint32_t max_len, uint32_t lattice_flags,
                                   const FstBatchOptions* opts, const FstDeviceLattices* out,
                                   uint64_t needed[2], void* stream);

/* Beam pruning of every item of an lhs batch: what OpenFst and Kaldi callers know as fstprune /
 * Prune(beam), run before a rescoring pass, a second grammar or an n-best.  Connect drops dead
 * ends; this drops what is alive but hopeless: arcs and final weights that lie only on paths
 * worse than the best one by more than `beam`.  The reference has no prune, so the definition is
 * this comment.
 *
 * Items and statuses.  An item has states 0 .. S-1, arcs in CSR and a start; arc a runs
 * src(a) -> dst(a) with weight w(a).  A state is final when its final weight is not +-inf
 * (connect's rule).  Tested in this order:
 *   1. no start, or zero states: FST_PATH_OK with the empty FST (zero states, start =
 *      FST_NO_STATE), as connect gives;
 *   2. a NaN arc or final weight anywhere in the item, or an arc weight w < 0.0 (-inf included;
 *      -0.0 is not < 0.0: it is accepted and acts as zero): FST_PATH_UNSUPPORTED with zero
 *      states and start = FST_NO_STATE.  Final weights may be negative.  An arc of weight +inf
 *      is accepted and is never part of a path;
 *   3. (device entry) an item the prepare kernel refuses: FST_PATH_UNSUPPORTED, the other items
 *      unaffected, exactly as for fst_device_shortest_path_lhs;
 *   4. otherwise FST_PATH_OK with the result below.
 * Distances.  Both are minima over f64 values and nothing else.
 *   F(s) = the minimum over paths from the start to s of the LEFT fold ((0.0 + w_1) + w_2) + ...;
 *     F(start) = 0.0, F(s) = +inf when s is not reachable (fst_shortest_path_lhs_batch's
 *     distance on items of non-negative weights).
 *   B(s) = the minimum over paths from s to a final state t of the RIGHT fold
 *     w_1 + (w_2 + (... + (w_k + final(t)))); the empty path gives final(s); B(s) = +inf when no
 *     final state is reachable.  As a recurrence:
 *     B(s) = min(final(s) if final, min over arcs a out of s of fl(w(a) + B(dst(a)))).
 *   With every arc weight >= 0, fl(x + w) >= x, so both are the fixpoints that any order of
 *   relaxations reaches from +inf; B is the same problem on the reversed arcs with several
 *   sources, because fl(a + b) = fl(b + a).  Cycles are therefore allowed.
 * The cut.
 *   best = min over final t of fl(F(t) + final(t)), a THIRD sum.  best = +inf: the result is the
 *     empty FST, status OK.
 *   limit = fl(best + beam).
 *   Arc a is kept iff T(a) = fl(fl(F(src(a)) + w(a)) + B(dst(a))) is not +inf and T(a) <= limit.
 *   State s keeps its final weight iff it is final and fl(F(s) + final(s)) is not +inf and is
 *     <= limit; otherwise its final weight becomes +inf.
 *   All comparisons are on f64 values: -0.0 equals +0.0.
 * The result is connect, by fst_connect_lhs_batch's definition word for word, of the item with
 * only the kept arcs and the kept finals: the kept states renumbered by increasing old id, arcs
 * in their old order, labels and weight bits copied; a start that is not kept gives the empty
 * FST.  (The connect step is needed: in exact arithmetic a kept arc's src is reachable over kept
 * arcs; under rounding that is not guaranteed.)
 * What this means.  F is a left fold, B a right fold and best a third sum.  When every sum is
 * exact -- integer or dyadic weights of bounded size -- the result is exactly the states and arcs
 * on some complete path of total <= best + beam, and the 1-best path survives at beam = 0.  With
 * arbitrary f64 weights T on the best path can exceed best by rounding: a caller who needs the
 * best path kept must give the beam that slack.  The final state that attains best always keeps
 * its final weight (beam >= 0 and fl is monotone).  beam = +inf keeps everything of finite
 * total: on an item without +inf arcs and without sums that overflow this is connect.
 *
 * Validation.  A beam that is NaN or < 0.0 returns FST_INVALID_ARG (tested before lhs's arrays
 * are read; -0.0 is valid).  Otherwise the same validator as every lhs entry: *out zeroed on
 * error, a null lhs / out and unknown opts->flags rejected.  num_fsts == 0 gives the empty OK
 * result.  opts->semantics is ignored.  FST_BATCH_DEVICES shards by arcs + 1 per item; a sharded
 * result is byte-identical to a one-shard run.  Free with fst_lattice_batch_free.
 * fst_last_launch_stats reports engine 15. */
FstError fst_prune_lhs_batch(const FstLhsBatch* lhs, double beam, const FstBatchOptions* opts,
                             FstLatticeBatch* out);

/* Device-resident: d_lhs as for fst_device_shortest_path_lhs (a host struct of device pointers,
 * trusted extents, per-item validation by the prepare kernel), out and needed as for
 * fst_device_compose_frozen: needed receives the pruned totals; when either exceeds its capacity
 * only `status` and `needed` are defined and nothing past a capacity is written.  num_fsts == 0:
 * needed = {0, 0}, state_offsets[0] = 0 and arc_offsets[0] = 0 are written.  The call
 * synchronises `stream`.  The result chains into every device lhs entry, so chains -> lattices ->
 * prune -> unique n-best -> text never leaves the device.  Engine 15; `launches` counts the
 * preparation kernels too. */
FstError fst_device_prune_lhs(const FstLhsBatch* d_lhs, double beam, const FstBatchOptions* opts,
                              const FstDeviceLattices* out, uint64_t needed[2], void* stream);

/* Arc posteriors of every item of an lhs batch, on the device: forward and backward sums in the
 * LOG semiring (src/weight.zig:67-91, LogWeight.plus), the total mass of the lattice, and for
 * every arc the share of that mass that runs through it, as -log.  The entries above work in the
 * tropical semiring and say which readings are best; this one says how sure the lattice is of
 * them (confidences beside alternatives, dropping low-confidence words, handing a lattice to a
 * downstream model).  The reference has no such operation, so this comment is the definition.
 *
 * An item has states 0 .. S-1, arcs in CSR order (arc index a within the item), a start state,
 * and src(a) -> dst(a) with weight w(a).  fl(.) is one rounding to f64.
 * Statuses, tested in this order:
 *   1. no start, or zero states: FST_PATH_EMPTY;
 *   2. a NaN, or a -inf, arc or final weight anywhere in the item: FST_PATH_UNSUPPORTED;
 *   3. a cycle among the states reachable from the start: FST_PATH_UNSUPPORTED
 *      (fst_nbest_lhs_batch's rule: every arc counts, whatever its weight; a self-loop is a cycle);
 *   4. device entry only: an item the prepare kernel refuses is FST_PATH_UNSUPPORTED;
 *   5. any forward or backward value that comes out -inf (or NaN, which only sums of -inf give),
 *      because finite weights overflowed: FST_PATH_UNSUPPORTED;
 *   6. total == +inf, no complete path of finite cost: FST_PATH_EMPTY;
 *   7. otherwise FST_PATH_OK.
 * The sums.
 *   logadd(x, y): if x == +inf return y; if y == +inf return x; otherwise, with m = min(x, y) and
 *     d = max(x, y) - m, return m - log1p(exp(-d)).  These are the reference's plus, isZero and
 *     times: a sum that is +inf is zero, an arc of weight +inf is never part of a path.
 *   alpha(start) = 0.0.  For every other reachable t, alpha(t) is the fold
 *     acc = +inf; acc = logadd(acc, fl(alpha(src(a)) + w(a)))
 *     over the arcs a into t whose source is reachable, IN INCREASING ARC INDEX.
 *     Unreachable states have alpha = +inf.
 *   beta(s), for reachable s: acc = final(s) (+inf for a non-final state), then
 *     acc = logadd(acc, fl(w(a) + beta(dst(a)))) over the arcs out of s IN INCREASING ARC INDEX.
 *     Unreachable states have beta = +inf.
 *   total = beta(start): -log Z, the log-sum over all complete paths.
 *   arc_cost(a) = fl(fl(fl(alpha(src) + w(a)) + beta(dst)) - total), the arc's -log posterior;
 *     +inf when any of the three terms is +inf.  It is not clamped: rounding may leave it a few
 *     ulps below zero.
 * Outputs, in the caller's own layout: alpha and beta are indexed like lhs->final_weights,
 * arc_cost like lhs->weights; nothing is compacted.  Every entry of a non-OK item is +inf, and so
 * is its total.
 * The fold order is part of the contract: log-add is not associative in f64, and with a fixed
 * order both tiers, every sharding and both entries give identical bytes.
 * Error.  With u = 2^-53, D the number of levels (the longest path's states), d the largest in-
 * or out-degree and M the largest finite magnitude among the weights, alpha and beta, every
 * alpha, beta and total lies within D (d + 1) (M + 8) u of the value of the same fold in exact
 * arithmetic, given exp and log1p within 2 ulp.
 *
 * Validation.  The same validator as every lhs entry: *out zeroed on error, a null lhs / out and
 * unknown opts->flags rejected.  num_fsts == 0 gives the empty OK result.  opts->semantics is
 * ignored.  The result lives in pooled pinned blocks until fst_posterior_result_free.
 * FST_BATCH_DEVICES shards by arcs + 1 per item; a shard's state and arc ranges are written at
 * the items' own offsets and a sharded result is byte-identical to a one-shard run.
 * fst_last_launch_stats reports engine 16. */
typedef struct {
    uint32_t num_fsts;
    int32_t* status;      /* [num_fsts] */
    double*  total;       /* [num_fsts]  -log Z */
    double*  alpha;       /* [total_states], as lhs->final_weights is indexed */
    double*  beta;        /* [total_states] */
    double*  arc_cost;    /* [total_arcs], as lhs->weights is indexed */
    uint64_t total_states, total_arcs;
} FstPosteriorResult;
FstError fst_posterior_lhs_batch(const FstLhsBatch* lhs, const FstBatchOptions* opts,
                                 FstPosteriorResult* out);
void fst_posterior_result_free(FstPosteriorResult* r);

/* Device-resident: d_lhs as for fst_device_shortest_path_lhs (a host struct of device pointers,
 * trusted extents, per-item validation by the prepare kernel); out's arrays are device memory of
 * the sizes above; alpha and beta may be NULL.  Only status and total are written for an item the
 * prepare kernel refuses (its ranges cannot be trusted); if state_offsets decrease anywhere every
 * item is FST_PATH_UNSUPPORTED and nothing else is written.  arc_cost lines up with d_lhs's
 * weights, so chains -> fst_device_compose_frozen -> posteriors -> the caller's own kernel ->
 * fst_device_prune_lhs or the n-best stays on the device.  The call synchronises `stream`.
 * Engine 16; `launches` counts the preparation kernels too. */
typedef struct {
    int32_t* status;      /* [num_fsts] */
    double*  total;       /* [num_fsts] */
    double*  alpha;       /* [total_states], or NULL */
    double*  beta;        /* [total_states], or NULL */
    double*  arc_cost;    /* [total_arcs] */
} FstDevicePosteriors;
FstError fst_device_posterior_lhs(const FstLhsBatch* d_lhs, const FstBatchOptions* opts,
                                  const FstDevicePosteriors* out, void* stream);

/* -log confidences of n-best paths (host only, no GPU): `paths` holds `per` strings per item
 * (fst_nbest_lhs_batch's result at n = per), total[i] is item i's -log Z.  For an OK string,
 * out[i * per + k] = fl(fl(c + final_weight) - total[i]) with c the left fold of the path's
 * weights from 0.0; +inf for every other string.  FST_INVALID_ARG for a null argument,
 * per == 0, or paths->num_strings != num_fsts * per. */
FstError fst_batch_result_path_costs(const FstBatchResult* paths, uint32_t per,
                                     const double* total, uint32_t num_fsts, double* out);

/* Text in, text out: the loop the reference application runs per utterance and stage,
 *   fst_compile_string(bytes) -> fst_compose_frozen_shortest_path -> fst_print_output_string
 * (README.md:177-214, src/string.zig:17-97), for a whole batch with bytes on both sides of
 * the bus: 1 B per input byte up instead of a 4-B label, and per string its status, offset,
 * total weight and output bytes down instead of 16 B per path arc.
 *
 * Input: string i is text[offsets[i] .. offsets[i+1]); its stage-1 labels are byte + 1
 * (compileString), every byte value is legal, an empty string is the one-state final
 * acceptor.  n is 1; one stage runs as fst_compose_frozen_shortest_path_batch does, several
 * as fst_pipeline_batch does.
 * Output, for every producer below (device emission, host conversion):
 *   - an OK string's bytes are the last stage's path olabels in path order, epsilons
 *     dropped, each minus 1 (printStringFromTape(.output));
 *   - an olabel above 256 is no byte: the string is FST_PATH_UNSUPPORTED;
 *   - every non-OK string has zero bytes and total_weight = +inf; a string that failed at
 *     an earlier stage reports that stage's status;
 *   - total_weight is the reference search's own best total, the f64 left fold
 *     ((0.0 + w_1) + w_2 ... + w_L) + final_weight over the path's arcs (dist of
 *     shortest-path.zig:72, then times(dist, final)), bit for bit. */
typedef struct {
    uint32_t num_strings;
    int32_t* status;          /* [num_strings] FstPathStatus */
    uint64_t* text_offsets;   /* [num_strings + 1] CSR offsets into text */
    uint8_t* text;            /* [total_bytes] */
    double* total_weight;     /* [num_strings] */
    uint64_t total_bytes;
} FstTextResult;

/* Host bytes in, host bytes out.  Arguments are checked as by fst_pipeline_batch
 * (FST_INVALID_ARG for a bad handle, decreasing offsets, num_stages == 0 or unknown flags;
 * *out is zeroed once they are checked); num_strings == 0 gives an empty OK result.
 * Semantics, device and FST_BATCH_DEVICES sharding from opts, as for the label entries
 * (shards balanced by fst_chain_cost of stage 1; the result is in input order and
 * byte-identical to a one-shard run).  Two routes, same result:
 *   - streamed (one stage whose rhs has no input epsilon and starts with a pull tier, as
 *     the streamed route of fst_compose_frozen_shortest_path_batch; FSTAMD_STREAM=0 turns it
 *     off): each shard uploads its bytes in a few parts under the pull kernels, which read
 *     the bytes themselves (label = byte + 1) and write every finished string's text
 *     straight into its fixed slot of the pinned result (its own input byte range: no path
 *     is longer than its input); 20 B per string come down, short slots are closed up on
 *     the host;
 *   - sharded (everything else): each shard uploads bytes and offsets, widens them to
 *     labels on the device, runs the stages, emits the text on the device and downloads
 *     only the four result arrays.
 * The result lives in pooled pinned blocks until fst_text_result_free. */
FstError fst_normalize_text_batch(const FstHandle* stages, uint32_t num_stages,
                                  const uint8_t* text, const uint64_t* offsets,
                                  uint32_t num_strings, const FstBatchOptions* opts,
                                  FstTextResult* out);
void fst_text_result_free(FstTextResult* r);
/* Lattices in, text out: the text form of fst_pipeline_lhs_batch (documented there). */
FstError fst_normalize_lhs_batch(const FstHandle* stages, uint32_t num_stages,
                                 const FstLhsBatch* lhs,
                                 const FstBatchOptions* opts, FstTextResult* out);

/* The device-resident pieces (every d_ pointer is device memory on the current device).
 * fst_device_compile_text: d_labels[k] = d_text[k] + 1 for k in [d_offsets[0],
 * d_offsets[num_strings]), so d_offsets serves the labels too; asynchronous on `stream`.
 * Nothing outside that range is read or written. */
FstError fst_device_compile_text(const uint8_t* d_text, const uint64_t* d_offsets,
                                 uint32_t num_strings, uint32_t* d_labels, void* stream);
/* fst_device_emit_text: a finished stage as text (d_text_offsets [num_strings + 1], d_status
 * and d_total_weight [num_strings]).  The call synchronises `stream`.  *total_bytes (host)
 * receives the bytes the batch needs; no byte at or past text_capacity is written, so when
 * *total_bytes > text_capacity the text is incomplete (offsets, statuses and weights are
 * not): call again with a buffer of *total_bytes. */
FstError fst_device_emit_text(const FstDeviceBatch* stage, uint32_t num_strings,
                              uint8_t* d_text, uint64_t text_capacity,
                              uint64_t* d_text_offsets, int32_t* d_status,
                              double* d_total_weight, uint64_t* total_bytes, void* stream);

/* Host conversion of a label result to text, same semantics, no GPU needed (the result is
 * freed with fst_text_result_free all the same).  FST_INVALID_ARG for a null argument or
 * decreasing path offsets. */
FstError fst_batch_result_to_text(const FstBatchResult* in, FstTextResult* out);

/* Text in, text out, with the input span of every output byte: which bytes of string i became
 * which bytes of its normalised text (SSML marks and word boundaries across "7" -> "seven", a
 * recogniser's word timestamps through ITN, an editor's highlights).
 *
 * For an OK string, output byte j gets the half-open interval [in_begin[j], in_end[j]) of the
 * string's own input bytes; indices are relative to the string, 0 <= begin <= end <= length,
 * and j runs over text_offsets as the text does.
 *   One stage.  Along the path's arcs a_0 .. a_{L-1}, with nz(x) = (x != 0): the arc a_k that
 *     emits the q-th non-epsilon olabel gives b[q] = sum_{t<k} nz(il_t) and
 *     e[q] = b[q] + nz(il_k).  An x:y arc gives a one-byte interval, an eps:y arc the empty
 *     interval at the boundary where it was taken, a deleted input (x:eps) belongs to no output
 *     byte.  N = sum_t nz(il_t) is what the path consumed: the string's length.
 *   Several stages.  Stage s consumes stage s-1's projected output (fst_device_project_output).
 *     With (B, E) the running map of stage s-1's M output symbols into the original input and
 *     (b, e) stage s's own,  B'[q] = b < M ? B[b] : N_1,  E'[q] = e > b ? E[b] : B'[q];
 *     (B_1, E_1) = (b_1, e_1).  The result is the last stage's map: the text's bytes and its
 *     projected symbols are the same sequence, the non-epsilon olabels.
 * So begin[j] <= end[j] <= begin[j+1] and end <= length.  Non-OK strings have no bytes and no
 * entries. */
typedef struct {
    uint32_t num_strings;
    int32_t* status;          /* as FstTextResult */
    uint64_t* text_offsets;
    uint8_t* text;
    double* total_weight;
    uint64_t total_bytes;
    uint32_t* in_begin;       /* [total_bytes] */
    uint32_t* in_end;         /* [total_bytes] */
} FstAlignedTextResult;

/* fst_normalize_text_batch plus the two maps.  The same argument checks and zeroing of *out,
 * the same FST_BATCH_DEVICES sharding (a sharded result is byte-identical to a one-shard run);
 * text, offsets, statuses and total weights are byte-identical to fst_normalize_text_batch on
 * the same call.  Always the sharded route: every stage's paths stay on the device, each
 * finished stage's map is composed into a running one (8 B per projected symbol), and two
 * more arrays come down.  Freed with fst_aligned_text_result_free. */
FstError fst_normalize_text_aligned_batch(const FstHandle* stages, uint32_t num_stages,
                                          const uint8_t* text, const uint64_t* offsets,
                                          uint32_t num_strings, const FstBatchOptions* opts,
                                          FstAlignedTextResult* out);
void fst_aligned_text_result_free(FstAlignedTextResult* r);

/* The device-resident pieces (every d_ pointer is device memory on the current device; both
 * asynchronous on `stream`).
 * fst_device_path_alignment: one stage's (b, e) per output symbol.  d_offsets [num_strings + 1]
 * are those fst_device_emit_text or fst_device_project_output wrote for the same stage: string
 * i owns the entries [d_offsets[i], d_offsets[i+1]) of d_begin and d_end, and d_consumed[i]
 * receives N.  A string whose entries are not its path's symbols (not OK, an olabel above 256:
 * no bytes in a text, the one dead label in a projection) gets [0, 0) on its entries and N = 0.
 * d_offsets must come from that call on this same `stage`, as it wrote them: the kernel reads
 * the stage's own statuses and takes any string whose entry count is not the count of its
 * path's non-epsilon olabels (offsets of another stage, or changed by a status mask of the
 * caller's) for a failed one, whose map is zeroed without an error.
 * No entry at or past `capacity` is written.  The call is asynchronous on `stream`.
 * fst_device_compose_alignment: the gather above.  String i's outer entries
 * [d_outer_offsets[i], d_outer_offsets[i+1]) of (d_b, d_e) index its inner symbols, whose map
 * (d_inner_begin, d_inner_end; d_inner_offsets[num_strings] entries) sits at
 * d_inner_offsets[i]; d_consumed is stage 1's.  The result goes to d_out_begin / d_out_end at
 * the outer offsets; they may be d_b and d_e themselves.  No entry at or past `capacity` is
 * read or written.  The call is asynchronous on `stream`. */
FstError fst_device_path_alignment(const FstDeviceBatch* stage, uint32_t num_strings,
                                   const uint64_t* d_offsets, uint32_t* d_begin,
                                   uint32_t* d_end, uint64_t capacity, uint32_t* d_consumed,
                                   void* stream);
FstError fst_device_compose_alignment(uint32_t num_strings, const uint64_t* d_outer_offsets,
                                      const uint32_t* d_b, const uint32_t* d_e,
                                      const uint64_t* d_inner_offsets,
                                      const uint32_t* d_inner_begin,
                                      const uint32_t* d_inner_end, const uint32_t* d_consumed,
                                      uint32_t* d_out_begin, uint32_t* d_out_end,
                                      uint64_t capacity, void* stream);

/* Host conversion of a one-stage label result to aligned text: fst_batch_result_to_text plus
 * the one-stage map from the result's ilabels, same semantics, no GPU needed (freed with
 * fst_aligned_text_result_free).  FST_INVALID_ARG for a null argument or decreasing path
 * offsets. */
FstError fst_batch_result_to_aligned_text(const FstBatchResult* in, FstAlignedTextResult* out);

/* Bring a frozen FST's device copy up on `device` (blob H2D + on-device SoA mirror).  Takes no
 * stream: it works on the null stream and returns with the copy complete.  A device entry
 * whose rhs has no copy on its device yet does the same in the middle of the call, whatever
 * `stream` it was given. */
FstError fst_device_prepare(FstHandle b, int32_t device);
/* Adopt a blob that already sits in device memory on `device` (e.g. received by an
 * RCCL broadcast): validates the header, builds the SoA mirror, returns a new handle.
 * `host_copy` must hold the same bytes (used for host-side queries); may be NULL, in
 * which case the bytes are copied back from the device.  Takes no stream and works on the null
 * stream, which a non-blocking stream does not wait for: a blob that was produced
 * asynchronously (a copy or a collective on a stream of the caller's) must be complete --
 * that stream waited for -- before this call. */
FstHandle fst_device_adopt_blob(const void* d_blob, uint64_t len, int32_t device,
                                const void* host_copy);

/* Engine introspection for benchmarks (last device launch on this thread). */
typedef struct {
    double kernel_ms;           /* sum of kernel durations, HIP events on the launch stream */
    uint32_t launches;          /* kernel launches in the call */
    uint32_t engine;            /* 0 = eager-layered, 1 = lazy replay, 2 = eager-general,
                                   3 = lazy rounds, 4 = lazy layered (+ rounds for the rest),
                                   5 = lazy dense replay, 6 = shortest-path heap replay,
                                   7 = lazy pull tier,
                                   8 = lhs batch, lazy (hashed replay, one wave per lhs),
                                   9 = lhs batch, eager (general BFS tiers, 1-best in kernel),
                                   10 = lattice batch (general BFS tiers, lattice emission;
                                        with FST_LATTICE_CONNECT the trim kernels too),
                                   11 = fst_connect_lhs_batch (the lattice trim alone),
                                   12 = fst_shortest_path_lhs_batch and
                                        fst_device_shortest_path_lhs (one wave per lattice,
                                        frontier and heap-replay tiers behind it),
                                   13 = fst_nbest_lhs_batch and fst_device_nbest_lhs (one wave
                                        per lattice with its tables in LDS, a workgroup per
                                        lattice with them in HBM behind it),
                                   14 = fst_nbest_unique_lhs_batch and
                                        fst_device_nbest_unique_lhs (engine 13's two tiers with
                                        a text hash per list entry),
                                   15 = fst_prune_lhs_batch and fst_device_prune_lhs (one wave
                                        per lattice for both distances and the cut, a workgroup
                                        per lattice behind it, then the trim kernels),
                                   16 = fst_posterior_lhs_batch and fst_device_posterior_lhs
                                        (one wave per lattice with its tables in LDS, a workgroup
                                        per lattice with them in HBM behind it) */
    uint32_t grid;              /* workgroups of the dominant kernel */
} FstLaunchStats;
FstError fst_last_launch_stats(FstLaunchStats* out);

/* Generators of the reference bench's synthetic rhs (bench/optimize-bench.zig:219-306),
 * built host-side and frozen: 0 = ambiguous chain, 1 = epsilon dense, 2 = branching. */
FstHandle fst_bench_transducer(uint32_t kind, uint32_t transducer_len, uint32_t branches);
/* Same, frozen with the given weight type (0 = tropical, 1 = log; src/fst.zig:43-47). */
FstHandle fst_bench_transducer_wt(uint32_t kind, uint32_t transducer_len, uint32_t branches,
                                  uint32_t weight_type);

/* Frozen blobs of either weight type for the batch entries ("weight_type
 * taken from the blob header").  fst_load stays Tropical-only like the reference c-api
 * (src/c-api.zig:601, W = TropicalWeight); these accept header weight_type 0 (tropical)
 * or 1 (log) and otherwise validate exactly like Fst.fromBytes (src/fst.zig:227-273).
 * On this path LogWeight's times / compare / isZero equal TropicalWeight's
 * (src/weight.zig:15-37 vs :88-104; log-add `plus` is never used), so both run through
 * the same engines. */
FstHandle fst_batch_load(const char* path);
FstHandle fst_batch_load_bytes(const void* bytes, uint64_t len);
/* OpenFst AT&T text -> frozen FST in one call: readText (src/io/text.zig:20-115; files up
 * to 256 MiB, src/tools/att2lfst.zig:40-45), then with FST_ATT_SHIFT_BYTE_LABELS every
 * non-epsilon ilabel / olabel + 1 (att2lfst.zig:54-60: OpenFst byte labels -> libfst's
 * byte + 1, so the asset matches fst_compile_string input), then fromMutable (Tropical).
 * tools/att2lfst (libfst_amd/att2lfst) is this plus fst_save. */
#define FST_ATT_SHIFT_BYTE_LABELS 1u
FstHandle fst_load_att(const char* path, uint32_t flags);

/* Header weight type of a frozen FST: 0 tropical, 1 log, -1 invalid handle. */
int32_t fst_weight_type(FstHandle b);

/* Diagnostics: the coalescer of single fst_compose_frozen_shortest_path calls on `device`
 * (leader slots in use, calls waiting in its queue).  Both are 0 when no call is in
 * flight; tests check that no slot leaks.  Returns -1 for a negative device. */
int32_t fst_debug_coalescer_state(int32_t device, uint32_t* queued);

/* Diagnostics / tests, no GPU needed: the host step that closes the streamed text route's
 * fixed slots up into the CSR result.  In: offsets[0 .. num_strings] = the slots (string i's
 * bytes start at offsets[i], its slot ends at offsets[i + 1]), nbytes[i] = bytes the device
 * wrote there (0xFFFFFFFF: the path has an olabel above 256), status[i].  Out: offsets = the
 * CSR offsets, text compacted in place moving left in input order, status[i] =
 * FST_PATH_UNSUPPORTED for the 0xFFFFFFFF strings (FST_PATH_INTERNAL should a count exceed
 * its slot), total_weight[i] = +inf for every non-OK string.  Returns the total bytes.
 * Nothing at or past offsets[num_strings] is read or written. */
uint64_t fst_debug_text_compact(uint32_t num_strings, uint64_t* offsets, const uint32_t* nbytes,
                                int32_t* status, double* total_weight, uint8_t* text);

/* Diagnostics / tests, no GPU needed: the host step of the streamed batch's weight codes.
 * dst[i] = table[codes[i]] for i < n; table has 256 entries, dst is 8-byte aligned and is
 * written with non-temporal stores where whole 64-byte lines allow.  Nothing outside
 * codes[0 .. n), table[0 .. 256) and dst[0 .. n) is read or written. */
void fst_debug_expand_weight_codes(const uint8_t* codes, uint64_t n, const double* table,
                                   double* dst);

/* Diagnostics / tests, no GPU needed: the streamed batch's part planner.  offsets[0 ..
 * num_strings] = a shard's label offsets (any first offset), per_mille[0 .. num_per_mille) =
 * the fractions of its labels to cut at (each in 1..999, as FSTAMD_STREAM_CUTS gives them).
 * Writes the parts' string boundaries 0, .., num_strings into cuts (room for num_per_mille + 2)
 * and returns how many it wrote: 2 (one part) for a shard under 2^15 strings or 2^22 labels;
 * a cut is kept only past the previous one and before num_strings.  0 on a null argument. */
uint32_t fst_debug_stream_part_cuts(const uint64_t* offsets, uint32_t num_strings,
                                    const uint64_t* per_mille, uint32_t num_per_mille,
                                    uint32_t* cuts);

#ifdef __cplusplus
}
#endif

#endif /* LIBFST_AMD_FST_BATCH_H */

"""libfst_amd: MI355X-native (gfx950) batched frozen-FST compose + 1-best engine.

Drop-in for ontypehq/libfst's fst_compose_frozen_shortest_path / fst_compose_frozen
hot path; see include/fst.h, include/fst_batch.h and DESIGN.md.
"""
from .fst import (  # noqa: F401
    BENCH_AMBIGUOUS, BENCH_BRANCHING, BENCH_EPS_DENSE, FST_EPSILON, FST_INVALID_HANDLE,
    FST_NO_STATE, FST_PATH_CYCLE, FST_PATH_EMPTY, FST_PATH_ERROR_N, FST_PATH_OK,
    FST_PATH_OUTPUT_FULL, FST_PATH_OVERFLOW, FST_PATH_UNSUPPORTED, FST_SEM_EAGER, FST_SEM_LAZY,
    BatchResult, Fst, FstTextResult, MutableFst, TextResult, batch_result_to_text, compose_frozen,
    compose_frozen_shortest_path, coalescer_state, compose_frozen_shortest_path_batch,
    last_launch_stats, lib, normalize_text_batch, pipeline_batch, shortest_path,
    FstLhsBatch, LhsBatch, compose_frozen_shortest_path_lhs_batch,
    compose_frozen_shortest_path_handles_batch, normalize_lhs_batch, pipeline_lhs_batch,
    FST_LATTICE_PROJECT_OUTPUT, FST_PATH_INTERNAL, FstDeviceLattices, FstLatticeBatch,
    LatticeBatch, compose_frozen_batch, compose_frozen_lhs_batch,
    FST_LATTICE_CONNECT, connect_lhs_batch, shortest_path_lhs_batch,
    AlignedTextResult, FstAlignedTextResult, batch_result_to_aligned_text,
    normalize_text_aligned_batch, FST_NBEST_MAX, nbest_lhs_batch,
    nbest_unique_lhs_batch, prune_lhs_batch,
    FstDevicePosteriors, FstPosteriorResult, PosteriorResult, batch_result_path_costs,
    posterior_lhs_batch)

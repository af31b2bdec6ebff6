"""What FST_LATTICE_CONNECT and fst_connect_lhs_batch cost and save, in one process, on one GPU.

Workloads (--workload):
  wetext     libfst_amd/wetext_standin.py: its utterances against its tagger (stage 1), the
             projected lattices against its verbalizer (stage 2) -- dead ends to trim
  synthetic  synthetic.utterances against synthetic.tagger(), stage 2 synthetic.verbalizer():
             nothing to trim, so the cost of the pass alone

Legs, alternating in every round after the warm-up:
  compose          fst_compose_frozen_batch, FST_LATTICE_PROJECT_OUTPUT
  compose_connect  the same with FST_LATTICE_CONNECT
  compose_linear   the same with FSTAMD_TRIM_SWEEPS=0: every item through the linear tier (what
                   a single-tier trim would cost)
  stage2_<sem>_full / _trim   fst_compose_frozen_shortest_path_lhs_batch (lazy, eager) on the
                   untrimmed / the trimmed stage-1 lattices (made once, before the timing)
  connect_alone    fst_connect_lhs_batch on the untrimmed stage-1 lattices
Per leg: wall time per round, median and spread (max - min), kernel time by the launch stats
(median).  Also the result bytes derived from the counts, the share of states and arcs kept,
the trim kernels' own time (compose_connect's kernel time minus compose's: both cover the tier
ladder, the first the trim too), and whether stage 2 gives every item the same status and total
weight on both inputs.

usage: python scripts/lattice_trim_bench.py [--workload both] [--items 16384] [--rounds 5]
           [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import libfst_amd as F  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402
from libfst_amd import wetext_standin as W  # noqa: E402


def workload(name, items):
    rng = np.random.default_rng(44)
    if name == "wetext":
        tag = W.tagger()
        rhs1 = F.Fst.from_bytes(W.freeze_blob(tag))
        rhs2 = F.Fst.from_bytes(W.freeze_blob(W.verbalizer()))
        labels, offsets = W.utterances(rng, items, tag)
        return "wetext_standin utterances vs tagger, then verbalizer", rhs1, rhs2, labels, offsets
    rhs1 = SY.to_mutable(SY.tagger()).freeze()
    rhs2 = SY.to_mutable(SY.verbalizer()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, items))
    return "synthetic.utterances vs synthetic.tagger(), then verbalizer()", rhs1, rhs2, labels, offsets


def result_bytes(r):
    """What the result sink copies down, from the counts: status, start and state offset per
    item; final and arc offset per state; the four arc arrays."""
    ns, na = int(r.state_offsets[-1]), int(r.arc_offsets[-1])
    return 16 * len(r) + 8 + 16 * ns + 8 + 20 * na


def totals(res):
    """Per item the serial total of its path, NaN where it has none."""
    out = np.full(len(res.status), np.nan)
    off = res.offsets.astype(np.int64)
    for i in np.flatnonzero(res.status == F.FST_PATH_OK):
        out[i] = float(np.sum(res.weights[off[i]:off[i + 1]])) + float(res.finals[i])
    return out


def run(name, a):
    what, rhs1, rhs2, labels, offsets = workload(name, a.items)
    sems = (("lazy", F.FST_SEM_LAZY), ("eager", F.FST_SEM_EAGER))

    def compose(connect):
        return F.compose_frozen_batch(rhs1, labels, offsets, project_output=True, connect=connect)

    def linear():
        os.environ["FSTAMD_TRIM_SWEEPS"] = "0"
        try:
            return compose(True)
        finally:
            del os.environ["FSTAMD_TRIM_SWEEPS"]

    os.environ["FSTAMD_ROUTE_LOG"] = "1"  # these two calls' tier counts, on stderr
    full, trim = compose(False), compose(True)
    del os.environ["FSTAMD_ROUTE_LOG"]
    alone = F.connect_lhs_batch(full.as_lhs())
    names = ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
             "olabels", "weights", "nextstates")
    ns0, na0 = int(full.state_offsets[-1]), int(full.arc_offsets[-1])
    ns1, na1 = int(trim.state_offsets[-1]), int(trim.arc_offsets[-1])
    check = {"ok_items": int((full.status == F.FST_PATH_OK).sum()),
             "states": [ns0, ns1], "arcs": [na0, na1],
             "states_kept": ns1 / max(ns0, 1), "arcs_kept": na1 / max(na0, 1),
             "items_trimmed_to_empty": int(np.sum((np.diff(trim.state_offsets.astype(np.int64)) == 0)
                                                  & (np.diff(full.state_offsets.astype(np.int64)) > 0))),
             "result_bytes_derived": [result_bytes(full), result_bytes(trim)],
             # (compose output is accessible, so the stand-alone entry must agree with the flag
             # on every array but the statuses of items that were not OK)
             "connect_alone_equals_flag": all(
                 getattr(alone, k).tobytes() == getattr(trim, k).tobytes() for k in names[1:])}
    lhs_full, lhs_trim = full.as_lhs(), trim.as_lhs()
    for sem_name, sem in sems:
        r0 = F.compose_frozen_shortest_path_lhs_batch(rhs2, lhs_full, 1, sem)
        r1 = F.compose_frozen_shortest_path_lhs_batch(rhs2, lhs_trim, 1, sem)
        t0, t1 = totals(r0), totals(r1)
        check["stage2_%s_same_status_and_total" % sem_name] = bool(
            np.array_equal(r0.status, r1.status) and
            np.array_equal(t0.view(np.uint64), t1.view(np.uint64)))
        both = ~np.isnan(t0) & ~np.isnan(t1)
        # (equal-weight alternatives may be summed in another order: the difference, too)
        check["stage2_%s_max_total_diff" % sem_name] = float(
            np.max(np.abs(t0[both] - t1[both]))) if both.any() else 0.0
        check["stage2_%s_ok_items" % sem_name] = int((r0.status == F.FST_PATH_OK).sum())
    legs = [("compose", lambda: compose(False)), ("compose_connect", lambda: compose(True)),
            ("compose_linear", linear)]
    for sem_name, sem in sems:
        for tag, lhs in (("full", lhs_full), ("trim", lhs_trim)):
            legs.append(("stage2_%s_%s" % (sem_name, tag),
                         lambda lhs=lhs, sem=sem: F.compose_frozen_shortest_path_lhs_batch(
                             rhs2, lhs, 1, sem)))
    legs.append(("connect_alone", lambda: F.connect_lhs_batch(lhs_full)))
    for _ in range(a.warmup):
        for _, call in legs:
            call()
    walls = {leg: [] for leg, _ in legs}
    kms = {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, call in legs:
            t0 = time.perf_counter()
            r = call()
            walls[leg].append(time.perf_counter() - t0)
            kms[leg].append(float(F.last_launch_stats().kernel_ms))
            del r
    out = {"workload": what, "items": a.items, "labels": int(offsets[-1]), "rounds": a.rounds,
           "warmup": a.warmup, "check": check, "devices": 1,
           "more_than_one_device": "not measured", "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3,
                            "kernel_ms_median": float(np.median(kms[leg])),
                            "us_per_item": med / a.items * 1e6}
    L = out["legs"]
    out["trim_kernel_ms"] = L["compose_connect"]["kernel_ms_median"] - L["compose"]["kernel_ms_median"]
    out["trim_kernel_ms_linear_tier_only"] = (L["compose_linear"]["kernel_ms_median"] -
                                              L["compose"]["kernel_ms_median"])
    out["compose_connect_over_compose_wall"] = L["compose_connect"]["median_ms"] / L["compose"]["median_ms"]
    for sem_name, _ in sems:
        out["stage2_%s_trim_over_full_wall" % sem_name] = (
            L["stage2_%s_trim" % sem_name]["median_ms"] / L["stage2_%s_full" % sem_name]["median_ms"])
        out["cascade_%s_trim_over_full_wall" % sem_name] = (
            (L["compose_connect"]["median_ms"] + L["stage2_%s_trim" % sem_name]["median_ms"]) /
            (L["compose"]["median_ms"] + L["stage2_%s_full" % sem_name]["median_ms"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=("both", "wetext", "synthetic"))
    ap.add_argument("--items", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_trim",
                                                  "lattice_trim_bench.json"))
    a = ap.parse_args()
    out = {}
    for name in (("wetext", "synthetic") if a.workload == "both" else (a.workload,)):
        out[name] = run(name, a)
        print(json.dumps({name: out[name]}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

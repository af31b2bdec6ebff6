"""The lhs batch entry against single calls, in one process, on one GPU.

Workload: confusion networks (synthetic.confusion_network) over synthetic.utterances against
synthetic.tagger() -- what a dictation caller's recogniser hands an ITN tagger.

Legs, alternating in every round after the warm-up:
  batch_lazy    fst_compose_frozen_shortest_path_lhs_batch, FST_SEM_LAZY, all items in one call
  batch_eager   the same, FST_SEM_EAGER
  single_lazy   fst_compose_frozen_shortest_path per item, from --threads host threads
  single_eager  fst_shortest_path(fst_compose_frozen(a, b)) per item, from --threads threads
The single legs are what a build without the batch entry offers for these inputs; they run on
MutableFst handles built once before the timing (the batch legs' CSR arrays are built once
too).  Per leg: wall time per round, its median and its spread (max - min over the rounds),
items per second at the median.  Before the timing the batch results are compared with the
single calls' on the first --check items, bit for bit.

usage: python scripts/lhs_batch_bench.py [--items 65536] [--rounds 5] [--warmup 1]
           [--threads 16] [--single-items N] [--check 256] [--out FILE]
--single-items N times the single legs on the first N items only (their rate is per item;
the JSON says so); 0 = all.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import libfst_amd as F  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402


def to_mutable(it):
    start, finals, arcs = it
    return SY.to_mutable((len(finals), start, finals, arcs))


def chain_of(m):
    """(ilabels, olabels, weight bits, final bits) of a result chain, None for the empty FST."""
    if m is None:
        return "error"
    start, finals, arcs = m.to_lists()
    if start == F.FST_NO_STATE:
        return None
    il, ol, w, s = [], [], [], start
    while arcs[s]:
        a = arcs[s][0]
        il.append(a[0]); ol.append(a[1]); w.append(a[2]); s = a[3]
    return il, ol, np.array(w, np.float64).view(np.uint64).tolist(), \
        int(np.array([finals[s]]).view(np.uint64)[0])


def batch_item(r, i):
    if int(r.status[i]) == F.FST_PATH_EMPTY:
        return None
    if int(r.status[i]) != F.FST_PATH_OK:
        return "error"
    a0, a1 = int(r.offsets[i]), int(r.offsets[i + 1])
    return (r.ilabels[a0:a1].tolist(), r.olabels[a0:a1].tolist(),
            r.weights[a0:a1].view(np.uint64).tolist(), int(r.finals[i:i + 1].view(np.uint64)[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--single-items", type=int, default=0)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lhs_batch",
                                                  "lhs_batch_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(44)
    rhs = SY.to_mutable(SY.tagger()).freeze()
    texts = SY.utterances(rng, a.items)
    items = [SY.confusion_network(rng, t, 3, 0.1) for t in texts]
    lhs = F.LhsBatch.from_fsts(items)
    n_single = a.single_items or a.items
    t0 = time.perf_counter()
    handles = [to_mutable(it) for it in items[:n_single]]
    build_s = time.perf_counter() - t0
    pool = ThreadPoolExecutor(a.threads)

    def single_lazy_one(m):
        return F.compose_frozen_shortest_path(m, rhs, 1)

    def single_eager_one(m):
        lat = F.compose_frozen(m, rhs)
        return None if lat is None else F.shortest_path(lat, 1)

    def single(fn):
        def run():
            ok = 0
            for r in pool.map(fn, handles, chunksize=64):
                ok += r is not None
            return ok
        return run

    legs = (("batch_lazy", lambda: F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, F.FST_SEM_LAZY)),
            ("single_lazy", single(single_lazy_one)),
            ("batch_eager", lambda: F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, F.FST_SEM_EAGER)),
            ("single_eager", single(single_eager_one)))
    # the same answers from both routes, on the first items
    nchk = min(a.check, n_single)
    same = {}
    for sem, name, one in ((F.FST_SEM_LAZY, "lazy", single_lazy_one),
                           (F.FST_SEM_EAGER, "eager", single_eager_one)):
        os.environ["FSTAMD_ROUTE_LOG"] = "1"  # this one call's tier counts, on stderr
        r = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, sem)
        del os.environ["FSTAMD_ROUTE_LOG"]
        st = F.last_launch_stats()  # (the batch call's: the single calls below set their own)
        same[name + "_engine"] = int(st.engine)
        same[name + "_grid"] = int(st.grid)
        same[name + "_launches"] = int(st.launches)
        same[name + "_kernel_ms"] = float(st.kernel_ms)
        same[name] = all(batch_item(r, i) == chain_of(one(handles[i])) for i in range(nchk))
        same[name + "_ok_items"] = int((r.status == F.FST_PATH_OK).sum())
        same[name + "_path_arcs"] = int(r.offsets[-1])
        del r
    for _ in range(a.warmup):
        for _, call in legs:
            call()
    walls = {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, call in legs:
            t0 = time.perf_counter()
            r = call()
            walls[leg].append(time.perf_counter() - t0)
            del r
    count = {"batch_lazy": a.items, "batch_eager": a.items, "single_lazy": n_single,
             "single_eager": n_single}
    out = {"workload": "confusion networks over synthetic.utterances vs synthetic.tagger()",
           "items": a.items, "single_items": n_single, "threads": a.threads, "rounds": a.rounds,
           "warmup": a.warmup, "lhs_states": int(lhs.state_offsets[-1]),
           "lhs_arcs": int(lhs.arc_offsets[-1]), "handles_build_s": build_s,
           "checked_items": nchk, "check": same, "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3, "items": count[leg],
                            "items_per_s": count[leg] / med,
                            "us_per_item": med / count[leg] * 1e6}
    for sem in ("lazy", "eager"):
        b, s = out["legs"]["batch_" + sem], out["legs"]["single_" + sem]
        out[sem + "_speedup_per_item"] = b["items_per_s"] / s["items_per_s"]
        # the bar: faster per item than the single-call leg by more than that leg's own spread
        out[sem + "_beats_single_by_more_than_its_spread"] = bool(
            b["us_per_item"] < s["us_per_item"] - s["spread_ms"] * 1e3 / s["items"])
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()

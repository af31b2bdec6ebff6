"""The lattice batch entry against single fst_compose_frozen calls and against the 1-best
batch entry, in one process, on one GPU.

Workload: synthetic.utterances against synthetic.tagger() -- the lattices a caller would
rescore, take an n-best of, or hand to the verbalizer with the tagger's ambiguity kept.

Legs, alternating in every round after the warm-up:
  batch    (a) fst_compose_frozen_batch, all items in one call: N lattices in FstLhsBatch's
           layout
  single   (b) fst_compose_frozen per item, from --threads host threads, on MutableFst handles
           built once before the timing; the first --single-items items (its rate is per item)
  onebest  (c) fst_compose_frozen_shortest_path_batch, FST_SEM_EAGER, same items: the same
           compose with a 1-best instead of the emission, and paths instead of lattices coming
           down -- the floor
Per leg: wall time per round, its median and its spread (max - min over the rounds), items per
second at the median.  Also the bytes of (a)'s result (derived from its item, state and arc
counts, not measured) and the kernel time of its tier ladder (launch stats).  Before
the timing (a)'s items are compared with the single calls' on the first --check items, bit
for bit.

usage: python scripts/lattice_batch_bench.py [--items 65536] [--rounds 5] [--warmup 1]
           [--threads 16] [--single-items 4096] [--check 256] [--out FILE]
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


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist()


def lists_key(start, finals, arcs):
    return (start if finals else F.FST_NO_STATE, bits(finals),
            [[(a, b, bits([w])[0], d) for (a, b, w, d) in al] for al in arcs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--single-items", type=int, default=4096)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_batch",
                                                  "lattice_batch_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(44)
    rhs = SY.to_mutable(SY.tagger()).freeze()
    texts = SY.utterances(rng, a.items)
    labels, offsets = SY.to_labels(texts)
    n_single = min(a.single_items or a.items, a.items)
    handles = [F.MutableFst.compile_string(t.encode()) for t in texts[:n_single]]
    pool = ThreadPoolExecutor(a.threads)

    def single_one(m):
        return F.compose_frozen(m, rhs)

    def single():
        ok = 0
        for r in pool.map(single_one, handles, chunksize=64):
            ok += r is not None
        return ok

    legs = (("batch", lambda: F.compose_frozen_batch(rhs, labels, offsets)),
            ("single", single),
            ("onebest", lambda: F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1,
                                                                     F.FST_SEM_EAGER)))
    # the same lattices from both routes, on the first items
    os.environ["FSTAMD_ROUTE_LOG"] = "1"  # this one call's tier counts, on stderr
    r = F.compose_frozen_batch(rhs, labels, offsets)
    del os.environ["FSTAMD_ROUTE_LOG"]
    st = F.last_launch_stats()  # (the batch call's: the single calls below set their own)
    nchk = min(a.check, n_single)
    ns, na = int(r.state_offsets[-1]), int(r.arc_offsets[-1])
    check = {"engine": int(st.engine), "grid": int(st.grid), "launches": int(st.launches),
             "kernel_ms": float(st.kernel_ms),
             "ok_items": int((r.status == F.FST_PATH_OK).sum()), "states": ns, "arcs": na,
             # derived from the counts, not measured: what the result sink copies down --
             # status, start and state offset per item; final and arc offset per state; the
             # four arc arrays
             "result_bytes_derived": 16 * a.items + 8 + 16 * ns + 8 + 20 * na,
             "kernel_ms_covers": "the tier ladder's launches (not the compaction kernels and scans)",
             "equal_to_single_calls": all(
                 lists_key(*r.item(i)) == lists_key(*single_one(handles[i]).to_lists())
                 for i in range(nchk))}
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
    count = {"batch": a.items, "single": n_single, "onebest": a.items}
    out = {"workload": "synthetic.utterances vs synthetic.tagger()", "items": a.items,
           "single_items": n_single, "threads": a.threads, "rounds": a.rounds,
           "warmup": a.warmup, "labels": int(offsets[-1]), "checked_items": nchk,
           "check": check, "devices": 1, "more_than_one_device": "not measured", "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3, "items": count[leg],
                            "items_per_s": count[leg] / med,
                            "us_per_item": med / count[leg] * 1e6}
    b, s, o = (out["legs"][k] for k in ("batch", "single", "onebest"))
    out["batch_over_single_per_item"] = b["items_per_s"] / s["items_per_s"]
    out["batch_over_onebest_wall"] = b["median_ms"] / o["median_ms"]
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()

"""What fst_device_posterior_lhs (engine 16) costs beside the two engines that share its depth and
sweep phases, in one process, on one GPU, on one device-resident lattice batch.

The batch: the lattices fst_compose_frozen_batch (project output) returns for
synthetic.utterances against synthetic.tagger() (--items, default 65,536), uploaded once.

Legs, alternating in every round after the warm-up (host clock around calls that end in a
synchronise; kernel time by the launch stats' events):
  posterior           fst_device_posterior_lhs, alpha and beta asked for
  posterior_again     the same once more in the same round: the spread of identical legs
  posterior_arcs      ... with alpha and beta NULL
  nbest_n1            fst_device_nbest_lhs at n = 1 (engine 13: the same depth, reverse and level
                      phases, a min where the posteriors add in the log semiring)
  prune_binf          fst_device_prune_lhs at beam = +inf (engine 15: a forward and a backward
                      sweep with a min per arc; its kernel time includes the trim kernels and its
                      wall time the compaction)
Then the wave tier's LDS budget, FSTAMD_POSTERIOR_LDS from 4 to 60 KiB: kernel time per budget
(median of the same number of rounds, the budgets alternating inside a round) and the items per
tier.  Before the timing: the statuses, and that what leaves every start state sums to one.
No ratio is fixed in advance.  More than one device: not measured.

usage: python scripts/lattice_posterior_bench.py [--items 65536] [--rounds 5] [--warmup 1]
           [--out FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import libfst_amd as F  # noqa: E402
import libfst_amd.fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402
from lattice_nbest_bench import FIELDS, DeviceOut, dev_tensor  # noqa: E402
from lattice_prune_bench import DeviceLattices  # noqa: E402

BUDGETS_KIB = (4, 6, 8, 12, 16, 24, 32, 48, 60)


def route_of(call):
    """(lds, hbm): the items per tier from the route line the call writes to stderr."""
    os.environ["FSTAMD_ROUTE_LOG"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    try:
        with tempfile.TemporaryFile() as tmp:
            os.dup2(tmp.fileno(), 2)
            try:
                call()
            finally:
                os.dup2(saved, 2)
            tmp.seek(0)
            err = tmp.read().decode()
    finally:
        os.close(saved)
        del os.environ["FSTAMD_ROUTE_LOG"]
    m = re.findall(r"lattice posterior: items \d+ \| lds (\d+) hbm (\d+)", err)
    assert m, err
    return {"lds": int(m[-1][0]), "hbm": int(m[-1][1])}


def stats(w, k, num):
    med = float(np.median(w))
    return {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
            "spread_ms": (max(w) - min(w)) * 1e3, "kernel_ms_median": float(np.median(k)),
            "kernel_ms_spread": max(k) - min(k), "us_per_item": med / max(num, 1) * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_posterior",
                                                  "lattice_posterior_bench.json"))
    a = ap.parse_args()
    os.environ.pop("FSTAMD_POSTERIOR_LDS", None)
    rng = np.random.default_rng(44)
    rhs1 = SY.to_mutable(SY.tagger()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, a.items))
    lat = F.compose_frozen_batch(rhs1, labels, offsets, project_output=True)
    lhs = lat.as_lhs()
    num = len(lhs)
    ns, na = int(lat.state_offsets[-1]), int(lat.arc_offsets[-1])
    src = {k: dev_tensor(getattr(lhs, k)) for k in FIELDS}
    cs = FF.FstLhsBatch(num, *[src[k].data_ptr() if src[k].numel() else None for k in FIELDS])
    opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda:0")
    status, total = z(num, torch.int32), z(num, torch.float64)
    alpha, beta, cost = z(ns, torch.float64), z(ns, torch.float64), z(na, torch.float64)
    full = FF.FstDevicePosteriors(status.data_ptr(), total.data_ptr(), alpha.data_ptr(),
                                  beta.data_ptr(), cost.data_ptr())
    arcs_only = FF.FstDevicePosteriors(status.data_ptr(), total.data_ptr(), None, None,
                                       cost.data_ptr())
    nb = DeviceOut(num, max(ns, 1))
    pruned = DeviceLattices(num, ns, na)
    needed = (C.c_uint64 * 2)(0, 0)

    def posterior(desc=full):
        rc = F.lib().fst_device_posterior_lhs(C.byref(cs), C.byref(opts), C.byref(desc), None)
        assert rc == FF.FST_OK, rc

    def nbest():
        rc = F.lib().fst_device_nbest_lhs(C.byref(cs), 1, C.byref(opts), C.byref(nb.desc), None)
        assert rc == FF.FST_OK, rc

    def prune():
        rc = F.lib().fst_device_prune_lhs(C.byref(cs), math.inf, C.byref(opts),
                                          C.byref(pruned.desc), needed, None)
        assert rc == FF.FST_OK, rc

    tiers = route_of(posterior)
    st = status.cpu().numpy()
    so, ao = lhs.state_offsets.astype(np.int64), lhs.arc_offsets.astype(np.int64)
    c, t = cost.cpu().numpy(), total.cpu().numpy()
    worst = 0.0
    for i in np.flatnonzero(st == F.FST_PATH_OK)[:2048]:
        s = so[i] + int(lhs.start[i])
        mass = float(np.sum(np.exp(-c[ao[s]:ao[s + 1]])))
        if lhs.final_weights[s] != math.inf:
            mass += math.exp(-(float(lhs.final_weights[s]) - float(t[i])))
        worst = max(worst, abs(mass - 1.0))
    sizes = 32 * np.diff(so) + 8 * (ao[so[1:]] - ao[so[:-1]])
    check = {"items": num, "states": ns, "arcs": na,
             "all_lattices_ok": bool((lat.status == F.FST_PATH_OK).all()),
             "posterior_ok_items": int((st == F.FST_PATH_OK).sum()),
             "start_mass_max_abs_error_first_2048": worst, "tiers_default_budget": tiers,
             "table_bytes_per_item": {"median": float(np.median(sizes)),
                                      "p99": float(np.percentile(sizes, 99)),
                                      "max": int(sizes.max())}}
    legs = [("posterior", posterior), ("posterior_again", posterior),
            ("posterior_arcs", lambda: posterior(arcs_only)), ("nbest_n1", nbest),
            ("prune_binf", prune)]
    for _ in range(a.warmup):
        for _, call in legs:
            call()
    walls = {leg: [] for leg, _ in legs}
    kms = {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, call in legs:
            t0 = time.perf_counter()
            call()
            walls[leg].append(time.perf_counter() - t0)
            kms[leg].append(float(F.last_launch_stats().kernel_ms))
    out = {"rounds": a.rounds, "warmup": a.warmup, "devices": 1,
           "more_than_one_device": "not measured",
           "batch": "synthetic.utterances vs synthetic.tagger(), project output", "check": check,
           "legs": {leg: stats(walls[leg], kms[leg], num) for leg, _ in legs}}
    k16 = out["legs"]["posterior"]["kernel_ms_median"]
    out["kernel_ratio_vs_engine13_n1"] = k16 / max(out["legs"]["nbest_n1"]["kernel_ms_median"], 1e-9)
    out["kernel_ratio_vs_engine15_binf"] = k16 / max(out["legs"]["prune_binf"]["kernel_ms_median"],
                                                     1e-9)
    # the wave tier's budget
    sweep = {}
    for kib in BUDGETS_KIB:
        os.environ["FSTAMD_POSTERIOR_LDS"] = str(kib * 1024)
        sweep[kib] = {"tiers": route_of(posterior), "kernel_ms": []}
    for _ in range(a.warmup + a.rounds):
        for kib in BUDGETS_KIB:
            os.environ["FSTAMD_POSTERIOR_LDS"] = str(kib * 1024)
            posterior()
            sweep[kib]["kernel_ms"].append(float(F.last_launch_stats().kernel_ms))
    del os.environ["FSTAMD_POSTERIOR_LDS"]
    for kib in BUDGETS_KIB:
        k = sweep[kib]["kernel_ms"][a.warmup:]
        sweep[kib] = {"tiers": sweep[kib]["tiers"], "kernel_ms": k,
                      "kernel_ms_median": float(np.median(k))}
    out["lds_budget_sweep_kib"] = sweep
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

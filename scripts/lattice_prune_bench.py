"""What fst_device_prune_lhs (engine 15) costs and what it saves downstream, in one process, on one
GPU, on device-resident lattice batches.

Two batches, each the lattices fst_compose_frozen_batch (project output) returns, uploaded once:
  A  synthetic.utterances against synthetic.tagger() (--items, default 65,536); stage 2 is
     synthetic.verbalizer().  Beams 0, 0.5, 1.0, +inf: the tagger's weights are 0.5 and 1.0.
  B  the WeText-scale stand-in (libfst_amd/wetext_standin.py): its utterances against its tagger
     (--items-b, default 16,384); stage 2 is its verbalizer.  Beams 0, 0.4, 2.0, +inf: its
     weights are 0.3, 0.4 and 2.0.

Legs, alternating in every round after the warm-up (host clock around calls that end in a
synchronise; kernel time by the launch stats' events):
  prune_b<beam>          fst_device_prune_lhs into a result of the input's size
  prune_b0_again         the first of them once more in the same round: the spread of identical
                         legs, the noise floor
  connect_host           fst_connect_lhs_batch on the same batch from host memory (there is no
                         device-resident connect: its wall time carries the upload and the
                         download, its kernel time is the comparable figure; prune at +inf is the
                         resident connect)
  unique_n<n>_b<beam>    fst_device_nbest_unique_lhs, n = 4 and 16, on the pruned batch; the
                         beam +inf batch is the connected one
  stage2_<sem>_b<beam>   fst_device_compose_shortest_path_lhs against the stage-2 rhs on the
                         pruned batch, lazy and eager; +inf again the connected one
Per leg: wall time per round, median and spread (max - min), kernel time median and spread.
Before the timing: per beam the states and arcs kept, the items per tier (from the route line),
and that the 1-best total of stage 2 at beam 0 equals the one on the connected batch wherever
both are OK.  No ratio is fixed in advance.  More than one device: not measured.

usage: python scripts/lattice_prune_bench.py [--items 65536] [--items-b 16384] [--rounds 5]
           [--warmup 1] [--out FILE]
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
from libfst_amd import wetext_standin as W  # noqa: E402
from lattice_nbest_bench import FIELDS, DeviceOut, dev_tensor  # noqa: E402

NS = (4, 16)
SEMS = (("lazy", F.FST_SEM_LAZY), ("eager", F.FST_SEM_EAGER))


def tag(beam):
    return "inf" if math.isinf(beam) else ("%g" % beam)


class DeviceLattices:
    """A device lattice batch of the given capacities: the prune's result, the next entry's lhs."""

    def __init__(self, num, scap, acap):
        z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda:0")
        self.num = num
        self.status, self.soff, self.start = z(num, torch.int32), z(num + 1, torch.int64), z(num, torch.int32)
        self.fin, self.aoff = z(scap, torch.float64), z(scap + 1, torch.int64)
        self.il, self.ol, self.nx = z(acap, torch.int32), z(acap, torch.int32), z(acap, torch.int32)
        self.w = z(acap, torch.float64)
        self.desc = FF.FstDeviceLattices(
            self.status.data_ptr(), self.soff.data_ptr(), self.start.data_ptr(),
            self.fin.data_ptr(), self.aoff.data_ptr(), self.il.data_ptr(), self.ol.data_ptr(),
            self.w.data_ptr(), self.nx.data_ptr(), scap, acap)
        self.cs = FF.FstLhsBatch(num, self.soff.data_ptr(), self.start.data_ptr(),
                                 self.fin.data_ptr(), self.aoff.data_ptr(), self.il.data_ptr(),
                                 self.ol.data_ptr(), self.w.data_ptr(), self.nx.data_ptr())


def route_of(call):
    """(wave, frontier): the items per tier from the route line the call writes to stderr."""
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
    m = re.findall(r"lattice prune: items \d+ \| wave (\d+) frontier (\d+)", err)
    assert m, err
    return {"wave": int(m[-1][0]), "frontier": int(m[-1][1])}


def totals(out: DeviceOut, num):
    """Per item the serial total of its path, NaN where it has none."""
    st = out.status.cpu().numpy()[:num]
    ln, off = out.plen.cpu().numpy(), out.poff.cpu().numpy()
    w, fin = out.w.cpu().numpy(), out.fin.cpu().numpy()
    t = np.full(num, np.nan)
    for i in np.flatnonzero(st == F.FST_PATH_OK):
        t[i] = float(np.sum(w[int(off[i]):int(off[i]) + int(ln[i])])) + float(fin[i])
    return st, t


def measure(name, lat, rhs2, beams, a):
    lhs = lat.as_lhs()
    num = len(lhs)
    ns, na = int(lat.state_offsets[-1]), int(lat.arc_offsets[-1])
    src = {k: dev_tensor(getattr(lhs, k)) for k in FIELDS}
    cs = FF.FstLhsBatch(num, *[src[k].data_ptr() if src[k].numel() else None for k in FIELDS])
    opts = {s: FF.FstBatchOptions(0, sem, 0, 0, 0) for s, sem in SEMS}
    pruned = {b: DeviceLattices(num, ns, na) for b in beams}
    needed = (C.c_uint64 * 2)(0, 0)

    def prune(b):
        rc = F.lib().fst_device_prune_lhs(C.byref(cs), b, C.byref(opts["lazy"]),
                                          C.byref(pruned[b].desc), needed, None)
        assert rc == FF.FST_OK, rc
        return int(needed[0]), int(needed[1])

    check = {"items": num, "states": ns, "arcs": na,
             "all_lattices_ok": bool((lat.status == F.FST_PATH_OK).all()), "beams": {}}
    for b in beams:
        tiers = route_of(lambda: prune(b))
        ks, ka = prune(b)
        check["beams"][tag(b)] = {"states_kept": ks, "arcs_kept": ka,
                                  "states_share": ks / max(ns, 1), "arcs_share": ka / max(na, 1),
                                  "tiers": tiers}
    uniq = {(n, b): DeviceOut(num * n, max(ns, 1) * n) for n in NS for b in beams}
    st2 = {(s, b): DeviceOut(num, 4 * na + 1024) for s, _ in SEMS for b in beams}

    def unique(n, b):
        rc = F.lib().fst_device_nbest_unique_lhs(C.byref(pruned[b].cs), n, C.byref(opts["lazy"]),
                                                 C.byref(uniq[n, b].desc), None)
        assert rc == FF.FST_OK, rc

    def stage2(s, b):
        rc = F.lib().fst_device_compose_shortest_path_lhs(rhs2.h, C.byref(pruned[b].cs), 1,
                                                          C.byref(opts[s]), C.byref(st2[s, b].desc),
                                                          None)
        assert rc == FF.FST_OK, rc

    for s, _ in SEMS:
        stage2(s, beams[0])
        stage2(s, beams[-1])
        s0, t0 = totals(st2[s, beams[0]], num)
        s1, t1 = totals(st2[s, beams[-1]], num)
        both = ~np.isnan(t0) & ~np.isnan(t1)
        check["stage2_%s_ok_items_pruned_connected" % s] = [int((s0 == 0).sum()), int((s1 == 0).sum())]
        # (with weights that do not add exactly a small beam can cut the 1-best: fst_batch.h)
        ok = {}
        for b in beams:
            stage2(s, b)
            ok[tag(b)] = int((st2[s, b].status.cpu().numpy()[:num] == F.FST_PATH_OK).sum())
        check["stage2_%s_ok_items_per_beam" % s] = ok
        check["stage2_%s_max_total_diff" % s] = float(np.max(np.abs(t0[both] - t1[both]))) \
            if both.any() else 0.0
    legs = [("prune_b%s" % tag(b), lambda b=b: prune(b)) for b in beams]
    legs.append(("prune_b%s_again" % tag(beams[0]), lambda: prune(beams[0])))
    legs.append(("connect_host", lambda: F.connect_lhs_batch(lhs)))
    for n in NS:
        legs += [("unique_n%d_b%s" % (n, tag(b)), lambda n=n, b=b: unique(n, b)) for b in beams]
    for s, _ in SEMS:
        legs += [("stage2_%s_b%s" % (s, tag(b)), lambda s=s, b=b: stage2(s, b)) for b in beams]
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
    out = {"batch": name, "check": check, "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3,
                            "kernel_ms_median": float(np.median(kms[leg])),
                            "kernel_ms_spread": max(kms[leg]) - min(kms[leg]),
                            "us_per_item": med / max(num, 1) * 1e6}
    return out


def batch_a(items):
    rng = np.random.default_rng(44)
    rhs1 = SY.to_mutable(SY.tagger()).freeze()
    rhs2 = SY.to_mutable(SY.verbalizer()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, items))
    return F.compose_frozen_batch(rhs1, labels, offsets, project_output=True), rhs2


def batch_b(items):
    rng = np.random.default_rng(44)
    tagger = W.tagger()
    rhs1 = F.Fst.from_bytes(W.freeze_blob(tagger))
    rhs2 = F.Fst.from_bytes(W.freeze_blob(W.verbalizer()))
    labels, offsets = W.utterances(rng, items, tagger)
    return F.compose_frozen_batch(rhs1, labels, offsets, project_output=True), rhs2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--items-b", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_prune",
                                                  "lattice_prune_bench.json"))
    a = ap.parse_args()
    out = {"rounds": a.rounds, "warmup": a.warmup, "devices": 1,
           "more_than_one_device": "not measured"}
    for key, name, make, beams in (
            ("A", "A: synthetic.utterances vs synthetic.tagger(), project output",
             lambda: batch_a(a.items), (0.0, 0.5, 1.0, math.inf)),
            ("B", "B: wetext_standin utterances vs its tagger, project output",
             lambda: batch_b(a.items_b), (0.0, 0.4, 2.0, math.inf))):
        lat, rhs2 = make()
        out[key] = measure(name, lat, rhs2, beams, a)
        print(json.dumps({key: out[key]}), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""What fst_shortest_path_lhs_batch and fst_device_shortest_path_lhs cost, in one process, on one
GPU: the 1-best of a batch of lattices that are given, not composed.

Workloads (--workload), each with and without FST_LATTICE_CONNECT on the producing call:
  synthetic  the lattices fst_compose_frozen_batch returns for synthetic.utterances against
             synthetic.tagger() (--items, default 65,536)
  wetext     the same for libfst_amd/wetext_standin.py (--wetext-items, default 16,384)

Legs, alternating in every round after the warm-up (host clock around calls that end in a
synchronise):
  batch        (a) fst_shortest_path_lhs_batch on the downloaded batch
  batch_s0     the same with FSTAMD_SP_SWEEPS=0: every item through the frontier tier (the kernel
               A/B: kernel time by the launch stats' events, default budget against it)
  batch_again  (a) once more in the same round: the spread between identical legs
  single       (b) the first --single items as single fst_shortest_path calls from 16 threads,
               checked bit-identical to (a) on those items before the timing
  device       (c) fst_device_shortest_path_lhs on the device-resident lattices
  eager_chain  (d) for context, the eager chain 1-best entry on the same utterances: the same
               answer, but it includes the compose
Per leg: wall time per round, median and spread (max - min), kernel time by the launch stats
(median; they are the calling thread's, so the `single` leg, whose calls the pool's threads make,
repeats the leg before it there and says nothing).  More than one device: not measured.

usage: python scripts/lattice_sp_bench.py [--workload both] [--items 65536] [--wetext-items 16384]
           [--single 4096] [--rounds 5] [--warmup 1] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import libfst_amd as F  # noqa: E402
import libfst_amd.fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402
from libfst_amd import wetext_standin as W  # noqa: E402

FIELDS = ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels", "weights",
          "nextstates")


def workload(name, items):
    rng = np.random.default_rng(44)
    if name == "wetext":
        tag = W.tagger()
        rhs = F.Fst.from_bytes(W.freeze_blob(tag))
        labels, offsets = W.utterances(rng, items, tag)
        return "wetext_standin utterances vs its tagger", rhs, labels, offsets
    rhs = SY.to_mutable(SY.tagger()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, items))
    return "synthetic.utterances vs synthetic.tagger()", rhs, labels, offsets


def dev_tensor(a):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.as_tensor(np.ascontiguousarray(a).view(signed) if signed else a, device="cuda:0")


class DeviceSide:
    """The lattice batch uploaded once, and an arena of its total states."""

    def __init__(self, lhs):
        self.num = len(lhs)
        self.t = {k: dev_tensor(getattr(lhs, k)) for k in FIELDS}
        self.cs = FF.FstLhsBatch(self.num, *[self.t[k].data_ptr() if self.t[k].numel() else None
                                             for k in FIELDS])
        cap = max(int(lhs.state_offsets[-1]), 1)
        z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda:0")
        self.status, self.plen = z(self.num, torch.int32), z(self.num, torch.int32)
        self.poff, self.fin = z(self.num, torch.int64), z(self.num, torch.float64)
        self.il, self.ol, self.w = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.float64)
        self.cur = z(1, torch.int64)
        self.desc = FF.FstDeviceBatch(self.status.data_ptr(), self.plen.data_ptr(),
                                      self.poff.data_ptr(), self.fin.data_ptr(),
                                      self.il.data_ptr(), self.ol.data_ptr(), self.w.data_ptr(),
                                      cap, self.cur.data_ptr(), 0)
        self.opts = FF.FstBatchOptions(0, 0, 0, 0, 0)

    def run(self):
        rc = F.lib().fst_device_shortest_path_lhs(C.byref(self.cs), 1, C.byref(self.opts),
                                                  C.byref(self.desc), None)
        assert rc == FF.FST_OK, rc
        return self

    def equals(self, host):
        st = self.status.cpu().numpy()
        if not np.array_equal(st, host.status):
            return False
        ln, off = self.plen.cpu().numpy(), self.poff.cpu().numpy()
        il, ol = self.il.cpu().numpy().view(np.uint32), self.ol.cpu().numpy().view(np.uint32)
        w, fin = self.w.cpu().numpy().view(np.uint64), self.fin.cpu().numpy().view(np.uint64)
        ho = host.offsets.astype(np.int64)
        for i in np.flatnonzero(st == F.FST_PATH_OK):
            a, z = int(off[i]), int(off[i]) + int(ln[i])
            b, y = int(ho[i]), int(ho[i + 1])
            if not (np.array_equal(il[a:z], host.ilabels[b:y]) and
                    np.array_equal(ol[a:z], host.olabels[b:y]) and
                    np.array_equal(w[a:z], host.weights[b:y].view(np.uint64)) and
                    fin[i] == host.finals[i:i + 1].view(np.uint64)[0]):
                return False
        return True


def mutable_items(lat, count):
    """The first `count` items as MutableFst handles (the single call's inputs)."""
    out = []
    for i in range(count):
        start, finals, arcs = lat.item(i)
        m = F.MutableFst()
        for f in finals:
            m.set_final(m.add_state(), f)
        if finals and start != F.FST_NO_STATE:
            m.set_start(start)
        for s, al in enumerate(arcs):
            for il, ol, w, nx in al:
                m.add_arc(s, il, ol, w, nx)
        out.append(m)
    return out


def single_equals(ms, host):
    """Every single call's chain against the batch's item, bit for bit."""
    ho = host.offsets.astype(np.int64)
    for i, m in enumerate(ms):
        r = F.shortest_path(m, 1)
        ok = int(host.status[i]) == F.FST_PATH_OK
        if r is None or (r.num_states == 0) != (not ok):
            return False
        if not ok:
            continue
        _, off, arcs, fin = r.to_arrays()
        b, y = int(ho[i]), int(ho[i + 1])
        if not (len(arcs) == y - b and
                np.array_equal(arcs["il"], host.ilabels[b:y]) and
                np.array_equal(arcs["ol"], host.olabels[b:y]) and
                np.array_equal(arcs["w"].view(np.uint64), host.weights[b:y].view(np.uint64)) and
                fin[-1:].view(np.uint64)[0] == host.finals[i:i + 1].view(np.uint64)[0]):
            return False
    return True


def run(name, items, connect, a):
    what, rhs, labels, offsets = workload(name, items)
    lat = F.compose_frozen_batch(rhs, labels, offsets, connect=connect)
    lhs = lat.as_lhs()
    os.environ["FSTAMD_ROUTE_LOG"] = "1"  # this call's tier counts, on stderr
    host = F.shortest_path_lhs_batch(lhs)
    del os.environ["FSTAMD_ROUTE_LOG"]
    eager = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, F.FST_SEM_EAGER)
    dev = DeviceSide(lhs)
    nsingle = min(a.single, items)
    ms = mutable_items(lat, nsingle)

    def budget0():
        os.environ["FSTAMD_SP_SWEEPS"] = "0"
        try:
            return F.shortest_path_lhs_batch(lhs)
        finally:
            del os.environ["FSTAMD_SP_SWEEPS"]

    def single():
        with ThreadPoolExecutor(16) as pool:
            return list(pool.map(lambda m: F.shortest_path(m, 1), ms))

    names = ("status", "offsets", "ilabels", "olabels", "weights", "finals")
    same = lambda x, y: all(getattr(x, k).tobytes() == getattr(y, k).tobytes() for k in names)
    ok_lat = lat.status == F.FST_PATH_OK
    check = {"items": items, "ok_items": int((host.status == F.FST_PATH_OK).sum()),
             "states": int(lat.state_offsets[-1]), "arcs": int(lat.arc_offsets[-1]),
             "path_arcs": int(host.offsets[-1]),
             "budget0_equals_default": same(host, budget0()),
             "device_equals_batch": dev.run().equals(host),
             "single_calls_equal_batch": single_equals(ms, host),
             "all_lattices_ok": bool(ok_lat.all()),
             "eager_chain_equals_batch": same(host, eager)}
    legs = [("batch", lambda: F.shortest_path_lhs_batch(lhs)), ("batch_s0", budget0),
            ("batch_again", lambda: F.shortest_path_lhs_batch(lhs)), ("single", single),
            ("device", dev.run),
            ("eager_chain", lambda: F.compose_frozen_shortest_path_batch(
                rhs, labels, offsets, 1, F.FST_SEM_EAGER))]
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
    out = {"workload": what, "connect": connect, "rounds": a.rounds, "warmup": a.warmup,
           "check": check, "devices": 1, "more_than_one_device": "not measured", "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        n = nsingle if leg == "single" else items
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3,
                            "kernel_ms": kms[leg], "kernel_ms_median": float(np.median(kms[leg])),
                            "items": n, "us_per_item": med / n * 1e6}
    L = out["legs"]
    out["single_over_batch_per_item"] = L["single"]["us_per_item"] / L["batch"]["us_per_item"]
    # the kernel A/B: the frontier tier alone against the default budget, and the spread two
    # identical legs show in the same rounds
    out["kernel_ms_s0_over_default"] = (L["batch_s0"]["kernel_ms_median"] /
                                        max(L["batch"]["kernel_ms_median"], 1e-9))
    out["kernel_ms_again_over_default"] = (L["batch_again"]["kernel_ms_median"] /
                                           max(L["batch"]["kernel_ms_median"], 1e-9))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=("both", "wetext", "synthetic"))
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--wetext-items", type=int, default=16384)
    ap.add_argument("--single", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_sp",
                                                  "lattice_sp_bench.json"))
    a = ap.parse_args()
    out = {}
    for name in (("synthetic", "wetext") if a.workload == "both" else (a.workload,)):
        for connect in (False, True):
            key = name + ("_connect" if connect else "")
            out[key] = run(name, a.items if name == "synthetic" else a.wetext_items, connect, a)
            print(json.dumps({key: out[key]}), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

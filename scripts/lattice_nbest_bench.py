"""What fst_device_nbest_lhs and fst_nbest_lhs_batch cost, in one process, on one GPU: the n best
paths of a batch of lattices that are given, not composed.

Input: the lattices fst_compose_frozen_batch returns for synthetic.utterances against
synthetic.tagger() (--items, default 65,536), uploaded once for the device legs.

Legs, alternating in every round after the warm-up (host clock around calls that end in a
synchronise; kernel time by the launch stats' events):
  device_n1 / _n4 / _n8 / _n16  (a) fst_device_nbest_lhs on the device-resident lattices
  device_sp                     (b) fst_device_shortest_path_lhs, the engine built for n = 1
  device_sp_again               (b) once more in the same round: the spread of identical legs
  host_n4                       (c) fst_nbest_lhs_batch at n = 4 on the downloaded batch
  download                      (d) the lattice batch copied to pinned host memory: what a caller
                                    who enumerates on the host has to do first
Per leg: wall time per round, median and spread (max - min), kernel time (median).  The checks
before the timing: the device entry equals the host entry at n = 4, and at n = 1 engine 13 and
engine 12 agree on every status.  More than one device: not measured.
--budgets B1,B2,...: after the legs, the device entry's kernel time per n under
FSTAMD_NBEST_LDS = each budget in bytes (0: the library's default), alternating per round: the
record the default budget was chosen from.

usage: python scripts/lattice_nbest_bench.py [--items 65536] [--rounds 5] [--warmup 1]
           [--budgets 0,8192,12288,16384,24576,32768,49152,61440] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import libfst_amd as F  # noqa: E402
import libfst_amd.fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402

FIELDS = ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels", "weights",
          "nextstates")
NS = (1, 4, 8, 16)


def dev_tensor(a):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.as_tensor(np.ascontiguousarray(a).view(signed) if signed else a, device="cuda:0")


class DeviceOut:
    """Room for `strings` paths in an arena of `cap` arcs."""

    def __init__(self, strings, cap):
        z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda:0")
        self.status, self.plen = z(strings, torch.int32), z(strings, torch.int32)
        self.poff, self.fin = z(strings, torch.int64), z(strings, torch.float64)
        self.il, self.ol, self.w = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.float64)
        self.cur = z(1, torch.int64)
        self.desc = FF.FstDeviceBatch(self.status.data_ptr(), self.plen.data_ptr(),
                                      self.poff.data_ptr(), self.fin.data_ptr(),
                                      self.il.data_ptr(), self.ol.data_ptr(), self.w.data_ptr(),
                                      cap, self.cur.data_ptr(), 0)

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


class DeviceSide:
    """The lattice batch uploaded once, an arena per n, and pinned room for its download."""

    def __init__(self, lhs):
        self.num = len(lhs)
        self.t = {k: dev_tensor(getattr(lhs, k)) for k in FIELDS}
        self.cs = FF.FstLhsBatch(self.num, *[self.t[k].data_ptr() if self.t[k].numel() else None
                                             for k in FIELDS])
        states = max(int(lhs.state_offsets[-1]), 1)
        self.out = {n: DeviceOut(self.num * n, states * n) for n in NS}
        self.sp_out = DeviceOut(self.num, states)
        self.opts = FF.FstBatchOptions(0, 0, 0, 0, 0)
        self.pinned = {k: torch.empty_like(v, device="cpu").pin_memory()
                       for k, v in self.t.items()}
        self.bytes = sum(v.numel() * v.element_size() for v in self.t.values())

    def nbest(self, n):
        rc = F.lib().fst_device_nbest_lhs(C.byref(self.cs), n, C.byref(self.opts),
                                          C.byref(self.out[n].desc), None)
        assert rc == FF.FST_OK, rc
        return self.out[n]

    def sp(self):
        rc = F.lib().fst_device_shortest_path_lhs(C.byref(self.cs), 1, C.byref(self.opts),
                                                  C.byref(self.sp_out.desc), None)
        assert rc == FF.FST_OK, rc
        return self.sp_out

    def download(self):
        for k, v in self.t.items():
            self.pinned[k].copy_(v, non_blocking=True)
        torch.cuda.synchronize()


def run(a):
    rng = np.random.default_rng(44)
    rhs = SY.to_mutable(SY.tagger()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, a.items))
    lat = F.compose_frozen_batch(rhs, labels, offsets)
    lhs = lat.as_lhs()
    dev = DeviceSide(lhs)
    os.environ["FSTAMD_ROUTE_LOG"] = "1"  # the tier counts per n, on stderr
    paths = {n: int(dev.nbest(n).cur.cpu()[0]) for n in NS}
    ok = {n: int((dev.out[n].status.cpu().numpy() == F.FST_PATH_OK).sum()) for n in NS}
    del os.environ["FSTAMD_ROUTE_LOG"]
    host4 = F.nbest_lhs_batch(lhs, 4)
    check = {"items": a.items, "states": int(lat.state_offsets[-1]),
             "arcs": int(lat.arc_offsets[-1]), "lattice_bytes": dev.bytes,
             "all_lattices_ok": bool((lat.status == F.FST_PATH_OK).all()),
             "path_arcs_per_n": paths, "ok_strings_per_n": ok,
             "device_n4_equals_host_n4": dev.nbest(4).equals(host4),
             "n1_statuses_equal_engine_12": bool(np.array_equal(
                 dev.nbest(1).status.cpu().numpy(), dev.sp().status.cpu().numpy()))}
    legs = [(f"device_n{n}", (lambda n=n: dev.nbest(n))) for n in NS]
    legs += [("device_sp", dev.sp), ("device_sp_again", dev.sp),
             ("host_n4", lambda: F.nbest_lhs_batch(lhs, 4)), ("download", dev.download)]
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
            kms[leg].append(float(F.last_launch_stats().kernel_ms) if leg != "download" else 0.0)
            del r
    out = {"workload": "synthetic.utterances vs synthetic.tagger()", "rounds": a.rounds,
           "warmup": a.warmup, "check": check, "devices": 1,
           "more_than_one_device": "not measured", "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3, "kernel_ms": kms[leg],
                            "kernel_ms_median": float(np.median(kms[leg])),
                            "kernel_ms_spread": max(kms[leg]) - min(kms[leg]),
                            "us_per_item": med / a.items * 1e6}
    L = out["legs"]
    out["kernel_ms_n1_over_engine_12"] = (L["device_n1"]["kernel_ms_median"] /
                                          max(L["device_sp"]["kernel_ms_median"], 1e-9))
    out["kernel_ms_engine_12_again_over_engine_12"] = (
        L["device_sp_again"]["kernel_ms_median"] / max(L["device_sp"]["kernel_ms_median"], 1e-9))
    out["wall_device_n4_over_download"] = (L["device_n4"]["median_ms"] /
                                           max(L["download"]["median_ms"], 1e-9))
    if a.budgets:
        out["lds_budget_sweep"] = budget_sweep(dev, [int(b) for b in a.budgets.split(",")],
                                               a.rounds)
    return out


def budget_sweep(dev, budgets, rounds):
    """Kernel time of the device entry per n under FSTAMD_NBEST_LDS = each budget (0: the
    library's own), the budgets alternating inside every round."""
    ms = {n: {b: [] for b in budgets} for n in NS}
    for _ in range(rounds + 1):  # (the first round warms up)
        for n in NS:
            for b in budgets:
                if b:
                    os.environ["FSTAMD_NBEST_LDS"] = str(b)
                try:
                    dev.nbest(n)
                finally:
                    os.environ.pop("FSTAMD_NBEST_LDS", None)
                ms[n][b].append(float(F.last_launch_stats().kernel_ms))
    return {f"n{n}": {("default" if b == 0 else str(b)): float(np.median(v[1:]))
                      for b, v in per.items()} for n, per in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budgets", default="",
                    help="comma-separated LDS budgets in bytes to sweep (0: the default)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_nbest",
                                                  "lattice_nbest_bench.json"))
    a = ap.parse_args()
    out = run(a)
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Lattices in, text out: the lhs pipeline entry and the device-resident lhs entry against what
a build without them offers, in one process, on one GPU.

Workload: scripts/lhs_batch_bench.py's confusion networks (same generator, same seed) through
synthetic.tagger() -> synthetic.verbalizer(), both semantics.

Legs, alternating in every round after the warm-up:
  a_normalize_lhs   fst_normalize_lhs_batch([tagger, verbalizer]): one call
  b_two_entries     the same job through the entries that existed before it:
                    fst_compose_frozen_shortest_path_lhs_batch(tagger), a vectorised numpy
                    projection of the result (mask of non-zero olabels, minus 1, cumsum
                    offsets), fst_normalize_text_batch([verbalizer]).  Its three parts are
                    timed separately (b_lhs_batch_ms, b_numpy_ms, b_text_batch_ms), so the
                    numpy step can be discounted.
  c_device_lhs      fst_device_compose_shortest_path_lhs(tagger) on tensors that are already
                    on the device, results left there
  c_host_lhs        fst_compose_frozen_shortest_path_lhs_batch(tagger) on the same items: the
                    difference to c_device_lhs is staging, upload and download
Before the timing (a) and (b) are compared byte for byte on every item, and (c) with the host
entry on statuses, paths and weight bits.  Per leg: wall time per round, its median and its
spread (max - min); a difference between two legs is reported as one only when it exceeds
both spreads.  No GPU: the script fails.

usage: python scripts/lhs_pipeline_bench.py [--items 65536] [--rounds 5] [--warmup 1] [--out FILE]
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

SEMS = (("lazy", F.FST_SEM_LAZY), ("eager", F.FST_SEM_EAGER))


def project(r):
    """The next stage's bytes and offsets from a label result, vectorised."""
    keep = r.olabels != 0
    data = (r.olabels[keep] - 1).astype(np.uint8)
    before = np.zeros(len(keep) + 1, np.uint64)
    np.cumsum(keep, dtype=np.uint64, out=before[1:])
    return data, before[r.offsets.astype(np.int64)]


def two_entries(tagger, verbalizer, lhs, sem, parts=None):
    t0 = time.perf_counter()
    r = F.compose_frozen_shortest_path_lhs_batch(tagger, lhs, 1, sem)
    t1 = time.perf_counter()
    text = project(r)
    t2 = time.perf_counter()
    out = F.normalize_text_batch([verbalizer], text, sem)
    t3 = time.perf_counter()
    if parts is not None:
        for k, v in (("b_lhs_batch_ms", t1 - t0), ("b_numpy_ms", t2 - t1),
                     ("b_text_batch_ms", t3 - t2)):
            parts.setdefault(k, []).append(v * 1e3)
    return out


class Resident:
    """The batch as device tensors, and a path arena of `cap` arcs, all allocated once."""

    FIELDS = ("state_offsets", "start", "final_weights", "arc_offsets", "ilabels", "olabels",
              "weights", "nextstates")

    def __init__(self, lhs, cap):
        dev = "cuda:0"
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
        self.t = {k: torch.as_tensor(getattr(lhs, k).view(signed.get(getattr(lhs, k).dtype,
                                                                     getattr(lhs, k).dtype)),
                                     device=dev) for k in self.FIELDS}
        self.cs = FF.FstLhsBatch(len(lhs), *[self.t[k].data_ptr() for k in self.FIELDS])
        n = len(lhs)
        self.o = dict(status=torch.zeros(n, dtype=torch.int32, device=dev),
                      plen=torch.zeros(n, dtype=torch.int32, device=dev),
                      poff=torch.zeros(n, dtype=torch.int64, device=dev),
                      fin=torch.zeros(n, dtype=torch.float64, device=dev),
                      il=torch.zeros(cap, dtype=torch.int32, device=dev),
                      ol=torch.zeros(cap, dtype=torch.int32, device=dev),
                      w=torch.zeros(cap, dtype=torch.float64, device=dev),
                      cur=torch.zeros(1, dtype=torch.int64, device=dev))
        o = self.o
        self.desc = FF.FstDeviceBatch(o["status"].data_ptr(), o["plen"].data_ptr(),
                                      o["poff"].data_ptr(), o["fin"].data_ptr(),
                                      o["il"].data_ptr(), o["ol"].data_ptr(), o["w"].data_ptr(),
                                      cap, o["cur"].data_ptr(), 0)

    def run(self, rhs, sem):
        opts = FF.FstBatchOptions(0, sem, 0, 0, 0)
        rc = F.lib().fst_device_compose_shortest_path_lhs(rhs.h, C.byref(self.cs), 1,
                                                          C.byref(opts), C.byref(self.desc), None)
        if rc != FF.FST_OK:
            raise RuntimeError(f"fst_device_compose_shortest_path_lhs failed: {rc}")

    def equals(self, host):
        """Statuses, paths and weight bits against a host label result."""
        o = {k: v.cpu().numpy() for k, v in self.o.items()}
        ok = host.status == F.FST_PATH_OK
        if not np.array_equal(o["status"], host.status):
            return False
        lens = np.diff(host.offsets.astype(np.int64))
        if not np.array_equal(o["plen"][ok].astype(np.int64), lens[ok]):
            return False
        # arena index of every arc of the host's CSR order
        idx = np.repeat(o["poff"] - host.offsets[:-1].astype(np.int64), lens) + \
            np.arange(int(host.offsets[-1]), dtype=np.int64)
        return (np.array_equal(o["il"].view(np.uint32)[idx], host.ilabels) and
                np.array_equal(o["ol"].view(np.uint32)[idx], host.olabels) and
                np.array_equal(o["w"][idx].view(np.uint64), host.weights.view(np.uint64)) and
                np.array_equal(o["fin"][ok].view(np.uint64), host.finals[ok].view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lhs_pipeline",
                                                  "lhs_pipeline_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lhs_pipeline_bench.py needs a GPU")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(44)
    tagger = SY.to_mutable(SY.tagger()).freeze()
    verbalizer = SY.to_mutable(SY.verbalizer()).freeze()
    texts = SY.utterances(rng, a.items)
    lhs = F.LhsBatch.from_fsts([SY.confusion_network(rng, t, 3, 0.1) for t in texts])
    out = {"workload": "confusion networks over synthetic.utterances through synthetic.tagger() "
                       "-> synthetic.verbalizer()",
           "items": a.items, "rounds": a.rounds, "warmup": a.warmup, "devices": 1,
           "lhs_states": int(lhs.state_offsets[-1]), "lhs_arcs": int(lhs.arc_offsets[-1]),
           "semantics": {}}
    for name, sem in SEMS:
        # the same answers first
        ra = F.normalize_lhs_batch([tagger, verbalizer], lhs, sem)
        rb = two_entries(tagger, verbalizer, lhs, sem)
        for k in ("status", "offsets", "text", "total_weight"):
            assert getattr(ra, k).tobytes() == getattr(rb, k).tobytes(), (name, k)
        host = F.compose_frozen_shortest_path_lhs_batch(tagger, lhs, 1, sem)
        res = Resident(lhs, int(host.offsets[-1]) + 1024)
        res.run(tagger, sem)
        st = F.last_launch_stats()
        assert res.equals(host), name
        check = {"a_equals_b_bytes": True, "c_equals_host_entry": True,
                 "ok_items": int((ra.status == F.FST_PATH_OK).sum()),
                 "text_bytes": int(ra.offsets[-1]), "stage1_path_arcs": int(host.offsets[-1]),
                 "c_engine": int(st.engine), "c_launches": int(st.launches),
                 "c_kernel_ms": float(st.kernel_ms)}
        del ra, rb, host
        parts = {}
        legs = (("a_normalize_lhs", lambda: F.normalize_lhs_batch([tagger, verbalizer], lhs, sem)),
                ("b_two_entries", lambda: two_entries(tagger, verbalizer, lhs, sem, parts)),
                ("c_device_lhs", lambda: res.run(tagger, sem)),
                ("c_host_lhs", lambda: F.compose_frozen_shortest_path_lhs_batch(tagger, lhs, 1, sem)))
        for _ in range(a.warmup):
            for _, call in legs:
                call()
        parts.clear()
        walls = {leg: [] for leg, _ in legs}
        for _ in range(a.rounds):
            for leg, call in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = call()
                walls[leg].append((time.perf_counter() - t0) * 1e3)
                del r
        walls.update(parts)
        rep = {"check": check, "legs": {}}
        for leg, w in walls.items():
            med = float(np.median(w))
            rep["legs"][leg] = {"wall_ms": w, "median_ms": med, "spread_ms": max(w) - min(w),
                                "items_per_s": a.items / med * 1e3}
        for new, base in (("a_normalize_lhs", "b_two_entries"), ("c_device_lhs", "c_host_lhs")):
            n, b = rep["legs"][new], rep["legs"][base]
            diff = b["median_ms"] - n["median_ms"]
            rep[new + "_vs_" + base] = {
                "baseline_minus_new_ms": diff, "baseline_over_new": b["median_ms"] / n["median_ms"],
                "exceeds_both_spreads": bool(abs(diff) > max(n["spread_ms"], b["spread_ms"]))}
        out["semantics"][name] = rep
        del res
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

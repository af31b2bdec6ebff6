"""What the rule "one path per output text" costs, in one process, on one GPU:
fst_device_nbest_unique_lhs (engine 14) against fst_device_nbest_lhs (engine 13) at the same n on
the same device-resident batch.

Two batches:
  A  the lattices fst_compose_frozen_batch returns for synthetic.utterances against
     synthetic.tagger() (--items, default 65,536; the batch of lattice_nbest_bench.py).  No two
     paths of an item print the same text, so the rule removes nothing: what it costs then.
  B  repeat-rich: synthetic.respelled_union items (--items-b, default 16,384; 4 hypotheses of a
     text of 4 .. 10 characters) -> compose_frozen_lhs_batch(tagger, project output, connect)
     -> compose_frozen_lhs_batch(verbalizer, connect).

Legs per batch and n in (4, 16), alternating in every round after the warm-up (host clock around
calls that end in a synchronise; kernel time by the launch stats' events):
  unique        (a) fst_device_nbest_unique_lhs
  plain         (b) fst_device_nbest_lhs
  plain_again   (b) once more in the same round: the spread of identical legs, the noise floor
Before the timing, per batch and n: the items each tier of either entry took (from the route
line), the OK strings of either entry, for (b) the strings that repeat an earlier text of their
item (the reason for the feature), and that (a) has none.  No ratio is fixed in advance; the
record reports (a) over (b) beside (b)-again over (b).  More than one device: not measured.
--budgets B1,B2,...: after the legs of batch A, (a)'s kernel time per n under FSTAMD_NBEST_LDS =
each budget in bytes (0: the library's default), alternating per round.

usage: python scripts/lattice_nbest_unique_bench.py [--items 65536] [--items-b 16384]
           [--rounds 5] [--warmup 1] [--budgets 0,8192,12288,...] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import libfst_amd as F  # noqa: E402
import libfst_amd.fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402
from lattice_nbest_bench import FIELDS, DeviceOut, dev_tensor  # noqa: E402

NS = (4, 16)


class DeviceSide:
    """A lattice batch uploaded once, and an arena per entry and n."""

    def __init__(self, lhs):
        self.num = len(lhs)
        self.t = {k: dev_tensor(getattr(lhs, k)) for k in FIELDS}
        self.cs = FF.FstLhsBatch(self.num, *[self.t[k].data_ptr() if self.t[k].numel() else None
                                             for k in FIELDS])
        states = max(int(lhs.state_offsets[-1]), 1)
        self.out = {(u, n): DeviceOut(self.num * n, states * n) for u in (False, True) for n in NS}
        self.opts = FF.FstBatchOptions(0, 0, 0, 0, 0)

    def nbest(self, unique, n):
        fn = F.lib().fst_device_nbest_unique_lhs if unique else F.lib().fst_device_nbest_lhs
        rc = fn(C.byref(self.cs), n, C.byref(self.opts), C.byref(self.out[unique, n].desc), None)
        assert rc == FF.FST_OK, rc
        return self.out[unique, n]


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
    m = re.findall(r"lattice nbest(?:-unique)?: items \d+ \| lds (\d+) hbm (\d+)", err)
    assert m, err
    return {"lds": int(m[-1][0]), "hbm": int(m[-1][1])}


def repeats(out, num, n):
    """(OK strings, strings whose output text an earlier string of their item printed)."""
    st = out.status.cpu().numpy()[:num * n]
    ln, off = out.plen.cpu().numpy(), out.poff.cpu().numpy()
    ol = out.ol.cpu().numpy()
    ok = rep = 0
    for i in range(num):
        seen = set()
        for k in range(i * n, (i + 1) * n):
            if int(st[k]) != F.FST_PATH_OK:
                continue
            ok += 1
            row = ol[int(off[k]):int(off[k]) + int(ln[k])]
            text = row[row != 0].tobytes()
            rep += text in seen
            seen.add(text)
    return ok, rep


def batch_a(items):
    rng = np.random.default_rng(44)
    rhs = SY.to_mutable(SY.tagger()).freeze()
    labels, offsets = SY.to_labels(SY.utterances(rng, items))
    return F.compose_frozen_batch(rhs, labels, offsets)


def batch_b(items):
    rng = np.random.default_rng(45)
    unions = [SY.respelled_union(rng, t, 4) for t in SY.utterances(rng, items, 4, 10)]
    tagged = F.compose_frozen_lhs_batch(SY.to_mutable(SY.tagger()).freeze(),
                                        F.LhsBatch.from_fsts(unions), project_output=True,
                                        connect=True)
    return F.compose_frozen_lhs_batch(SY.to_mutable(SY.verbalizer()).freeze(), tagged.as_lhs(),
                                      connect=True)


def budget_sweep(dev, budgets, rounds):
    """Kernel time of the unique device entry per n under FSTAMD_NBEST_LDS = each budget (0: the
    library's own), the budgets alternating inside every round."""
    ms = {n: {b: [] for b in budgets} for n in NS}
    for _ in range(rounds + 1):  # (the first round warms up)
        for n in NS:
            for b in budgets:
                if b:
                    os.environ["FSTAMD_NBEST_LDS"] = str(b)
                try:
                    dev.nbest(True, n)
                finally:
                    os.environ.pop("FSTAMD_NBEST_LDS", None)
                ms[n][b].append(float(F.last_launch_stats().kernel_ms))
    return {f"n{n}": {("default" if b == 0 else str(b)): float(np.median(v[1:]))
                      for b, v in per.items()} for n, per in ms.items()}


def measure(name, lat, a, budgets=()):
    lhs = lat.as_lhs()
    dev = DeviceSide(lhs)
    check = {"items": len(lhs), "states": int(lat.state_offsets[-1]),
             "arcs": int(lat.arc_offsets[-1]),
             "all_lattices_ok": bool((lat.status == F.FST_PATH_OK).all())}
    for n in NS:
        per = {}
        for unique, key in ((True, "unique"), (False, "plain")):
            per[key + "_tiers"] = route_of(lambda: dev.nbest(unique, n))
            ok, rep = repeats(dev.out[unique, n], dev.num, n)
            per[key + "_ok_strings"], per[key + "_repeated_texts"] = ok, rep
        assert per["unique_repeated_texts"] == 0, per
        check[f"n{n}"] = per
    legs = []
    for n in NS:
        legs += [(f"unique_n{n}", (lambda n=n: dev.nbest(True, n))),
                 (f"plain_n{n}", (lambda n=n: dev.nbest(False, n))),
                 (f"plain_again_n{n}", (lambda n=n: dev.nbest(False, n)))]
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
    out = {"batch": name, "check": check, "legs": {}}
    for leg, w in walls.items():
        med = float(np.median(w))
        out["legs"][leg] = {"wall_ms": [x * 1e3 for x in w], "median_ms": med * 1e3,
                            "spread_ms": (max(w) - min(w)) * 1e3, "kernel_ms": kms[leg],
                            "kernel_ms_median": float(np.median(kms[leg])),
                            "kernel_ms_spread": max(kms[leg]) - min(kms[leg]),
                            "us_per_item": med / max(len(lhs), 1) * 1e6}
    L = out["legs"]
    for n in NS:
        base = max(L[f"plain_n{n}"]["kernel_ms_median"], 1e-9)
        out[f"kernel_ms_unique_over_plain_n{n}"] = L[f"unique_n{n}"]["kernel_ms_median"] / base
        out[f"kernel_ms_plain_again_over_plain_n{n}"] = \
            L[f"plain_again_n{n}"]["kernel_ms_median"] / base
    out["lds_budget_sweep"] = budget_sweep(dev, budgets, a.rounds) if budgets else "not measured"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--items-b", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budgets", default="",
                    help="comma-separated LDS budgets in bytes to sweep on batch A (0: the default)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lattice_nbest_unique",
                                                  "lattice_nbest_unique_bench.json"))
    a = ap.parse_args()
    out = {"rounds": a.rounds, "warmup": a.warmup, "devices": 1,
           "more_than_one_device": "not measured",
           "A": measure("A: synthetic.utterances vs synthetic.tagger()", batch_a(a.items), a,
                        [int(b) for b in a.budgets.split(",")] if a.budgets else ()),
           "B": measure("B: respelled_union -> tagger (project output) -> verbalizer",
                        batch_b(a.items_b), a)}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

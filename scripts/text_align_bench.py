"""What the input spans cost: the aligned text entry against the text entry on the same route,
and against what a caller had to do before it existed.  One process, one GPU.

Workload: SY.tagger() -> SY.verbalizer() on 65,536 utterances (scripts/bench_configs.py's
config 4), lazy and eager.  Legs, alternating after warm-up:

  a          fst_normalize_text_aligned_batch
  b_1, b_2   fst_normalize_text_batch with FSTAMD_STREAM=0: the same (sharded) route without
             the map, twice per round -- their difference is the run-to-run spread of (b)
  c          on the first 4,096 utterances: the per-stage label entries
             (fst_compose_frozen_shortest_path_batch, the projection between the stages on the
             host) and the definition in Python over the downloaded paths

Reported: medians and spreads per leg, (a) - (b) against the spread of (b), and where (a)'s
extra time goes -- the alignment kernels timed by events on the same paths held on the device
(the device pieces fst_device_path_alignment / fst_device_compose_alignment: stage 1 at its
projection offsets, stage 2 at its text offsets, the gather), against a pinned download of
the two extra arrays (8 B per output byte).  (a)'s text, offsets, statuses and weights are
compared with (b)'s at the timed size, and its maps with leg (c)'s on the 4,096.

usage: python scripts/text_align_bench.py [--rounds 7] [--warmup 3] [--strings N]
           [--model-strings N] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import libfst_amd as F  # noqa: E402
from libfst_amd import fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402

DEAD = 0xFFFFFFFF


def no_stream(call):
    """`call` with FSTAMD_STREAM=0 (the library reads it per call)."""
    def run():
        before = os.environ.get("FSTAMD_STREAM")
        os.environ["FSTAMD_STREAM"] = "0"
        try:
            return call()
        finally:
            if before is None:
                del os.environ["FSTAMD_STREAM"]
            else:
                os.environ["FSTAMD_STREAM"] = before
    return run


def project(r):
    """The next stage's chain inputs from a label result, on the host: the non-epsilon
    olabels of every OK path, one dead label for every other string."""
    n = len(r.status)
    lens = np.diff(r.offsets.astype(np.int64))
    sid = np.repeat(np.arange(n), lens)
    ok = r.status == F.FST_PATH_OK
    keep = (r.olabels != 0) & ok[sid]
    counts = np.bincount(sid[keep], minlength=n)
    counts[~ok] = 1
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    labels = np.full(int(off[-1]), DEAD, np.uint32)
    ks = sid[keep]
    first = np.concatenate([[0], np.cumsum(np.bincount(ks, minlength=n))])[:-1]
    labels[off[:-1].astype(np.int64)[ks] + np.arange(len(ks)) - first[ks]] = r.olabels[keep]
    return labels, off


def stage_map(il, ol):
    b, e, n = [], [], 0
    for i, o in zip(il, ol):
        step = int(i != 0)
        if o != 0:
            b.append(n)
            e.append(n + step)
        n += step
    return b, e, n


def per_stage(stages, labels, offsets, sem):
    """Leg (c)'s device part: every stage through the label entry, projected on the host."""
    out = []
    for s in stages:
        r = F.compose_frozen_shortest_path_batch(s, labels, offsets, 1, sem)
        out.append(r)
        labels, offsets = project(r)
    return out


def model_maps(results):
    """Leg (c)'s host part: the definition of include/fst_batch.h over the downloaded paths;
    (begin, end) per string, empty for a string that is not OK at the last stage."""
    n = len(results[0].status)
    paths = [(r.offsets.astype(np.int64), r.ilabels.tolist(), r.olabels.tolist()) for r in results]
    ok = np.all([r.status == F.FST_PATH_OK for r in results], axis=0)
    maps = []
    for i in range(n):
        if not ok[i]:
            maps.append(([], []))
            continue
        B = E = None
        for off, il, ol in paths:
            b, e, cons = stage_map(il[off[i]:off[i + 1]], ol[off[i]:off[i + 1]])
            if B is None:
                B, E, n1 = b, e, cons
            else:
                M = len(B)
                lo = [B[x] if x < M else n1 for x in b]
                E = [E[x] if y > x else l for x, y, l in zip(b, e, lo)]
                B = lo
        maps.append((B, E))
    return maps


def device_stage(r, torch, dev):
    """A label result as an FstDeviceBatch (the paths back to back, as they came down)."""
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt), device=dev)
    n = len(r.status)
    arcs = max(int(r.offsets[-1]), 1)
    pad = lambda a, dt: np.concatenate([a, np.zeros(arcs - len(a), a.dtype)]).view(dt) \
        if len(a) < arcs else a.view(dt)
    keep = [t(r.status, np.int32), t(np.diff(r.offsets.astype(np.int64)), np.int32),
            t(r.offsets[:-1], np.int64), t(r.finals, np.float64), t(pad(r.ilabels, np.int32), np.int32),
            t(pad(r.olabels, np.int32), np.int32), t(pad(r.weights, np.float64), np.float64),
            torch.zeros(1, dtype=torch.int64, device=dev)]
    desc = FF.FstDeviceBatch(*[k.data_ptr() for k in keep[:7]], arcs, keep[7].data_ptr(), 0)
    return desc, keep, n


def kernel_events(results, rounds):
    """The alignment kernels alone, by events: both stages' paths on the device, stage 1's map
    at its projection offsets, stage 2's at its text offsets, then the gather; and a pinned
    download of the two result arrays."""
    import torch
    dev = torch.device("cuda", 0)
    L = F.lib()
    d1, keep1, n = device_stage(results[0], torch, dev)
    d2, keep2, _ = device_stage(results[1], torch, dev)
    P = lambda x: C.c_void_p(x.data_ptr())
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
    i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)
    poff, pst, ml = i64(n + 1), i32(n), FF._u32(0)
    plab = i32(int(results[0].offsets[-1]) + n)
    assert L.fst_device_project_output(C.byref(d1), n, P(plab), P(poff), P(pst), C.byref(ml),
                                       None) == FF.FST_OK
    toff, tst, ttw, tot = i64(n + 1), i32(n), torch.zeros(n, dtype=torch.float64, device=dev), FF._u64(0)
    assert L.fst_device_emit_text(C.byref(d2), n, None, 0, P(toff), P(tst), P(ttw), C.byref(tot),
                                  None) == FF.FST_OK
    torch.cuda.synchronize()
    m1, m2 = int(poff[-1].item()), int(tot.value)
    b1, e1, c1 = i32(m1), i32(m1), i32(n)
    b2, e2, c2 = i32(m2), i32(m2), i32(n)
    host_b = torch.empty(max(m2, 1), dtype=torch.int32).pin_memory()
    host_e = torch.empty(max(m2, 1), dtype=torch.int32).pin_memory()
    stream = torch.cuda.Stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    times = {"path_alignment_stage1_ms": [], "path_alignment_stage2_ms": [], "compose_ms": [],
             "download_ms": []}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        for k in range(rounds + 2):
            marks = [ev() for _ in range(5)]
            marks[0].record(stream)
            assert L.fst_device_path_alignment(C.byref(d1), n, P(poff), P(b1), P(e1), m1, P(c1),
                                               sp) == FF.FST_OK
            marks[1].record(stream)
            assert L.fst_device_path_alignment(C.byref(d2), n, P(toff), P(b2), P(e2), m2, P(c2),
                                               sp) == FF.FST_OK
            marks[2].record(stream)
            assert L.fst_device_compose_alignment(n, P(toff), P(b2), P(e2), P(poff), P(b1), P(e1),
                                                  P(c1), P(b2), P(e2), m2, sp) == FF.FST_OK
            marks[3].record(stream)
            host_b.copy_(b2[:max(m2, 1)], non_blocking=True)
            host_e.copy_(e2[:max(m2, 1)], non_blocking=True)
            marks[4].record(stream)
            stream.synchronize()
            if k >= 2:   # (two warm-up rounds)
                for name, x, y in zip(times, marks, marks[1:]):
                    times[name].append(x.elapsed_time(y))
    del keep1, keep2
    out = {k: float(np.median(v)) for k, v in times.items()}
    out["kernels_ms"] = (out["path_alignment_stage1_ms"] + out["path_alignment_stage2_ms"] +
                         out["compose_ms"])
    out["projected_symbols"], out["output_bytes"] = m1, m2
    out["download_bytes"] = 8 * m2
    return out, host_b.numpy()[:m2].view(np.uint32).copy(), host_e.numpy()[:m2].view(np.uint32).copy()


def run(n, n_model, sem, rounds, warmup):
    stages = [SY.to_mutable(SY.tagger()).freeze(), SY.to_mutable(SY.verbalizer()).freeze()]
    texts = SY.utterances(np.random.default_rng(44), n)
    data, toff = FF.text_csr([t.encode() for t in texts])
    labels, offsets = SY.to_labels(texts[:n_model])
    aligned = lambda: F.normalize_text_aligned_batch(stages, (data, toff), sem)
    plain = no_stream(lambda: F.normalize_text_batch(stages, (data, toff), sem))
    model = lambda: model_maps(per_stage(stages, labels, offsets, sem))
    legs = (("b_1", plain), ("a", aligned), ("c", model), ("b_2", plain))
    for _ in range(warmup):
        aligned()
        plain()
    model()
    walls = {leg: [] for leg, _ in legs}
    for _ in range(rounds):
        for leg, call in legs:
            t0 = time.perf_counter()
            r = call()
            walls[leg].append(time.perf_counter() - t0)
            del r
    # results compared at the timed sizes
    a, b = aligned(), plain()
    same_text = all(x.tobytes() == y.tobytes() for x, y in (
        (a.status, b.status), (a.offsets, b.offsets), (a.text, b.text),
        (a.total_weight, b.total_weight)))
    maps = model()
    same_maps = True
    for i, (mb, me) in enumerate(maps):
        lo, hi = int(a.offsets[i]), int(a.offsets[i + 1])
        same_maps &= a.in_begin[lo:hi].tolist() == mb and a.in_end[lo:hi].tolist() == me
    full = [F.compose_frozen_shortest_path_batch(stages[0], *SY.to_labels(texts), 1, sem)]
    full.append(F.compose_frozen_shortest_path_batch(stages[1], *project(full[0]), 1, sem))
    events, dev_b, dev_e = kernel_events(full, rounds)
    same_device = bool(np.array_equal(dev_b, a.in_begin) and np.array_equal(dev_e, a.in_end))
    out_bytes, ok = int(a.offsets[-1]), int((a.status == 0).sum())
    del a, b
    ms = {k: [x * 1e3 for x in v] for k, v in walls.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread_b = abs(med["b_1"] - med["b_2"])
    range_b = max(ms["b_1"] + ms["b_2"]) - min(ms["b_1"] + ms["b_2"])
    b_ms = float(np.median(ms["b_1"] + ms["b_2"]))
    return {
        "workload": f"config4 tagger -> verbalizer, {'lazy' if sem == F.FST_SEM_LAZY else 'eager'}",
        "strings": n, "ok": ok, "input_bytes": int(toff[-1]), "output_bytes": out_bytes,
        "rounds": rounds, "warmup": warmup,
        "a_aligned_wall_ms": med["a"], "a_range_ms": max(ms["a"]) - min(ms["a"]),
        "b_text_sharded_wall_ms": b_ms, "b_1_wall_ms": med["b_1"], "b_2_wall_ms": med["b_2"],
        "b_spread_ms": spread_b, "b_range_ms": range_b,
        "a_minus_b_ms": med["a"] - b_ms,
        "a_minus_b_within_b_spread": bool(med["a"] - b_ms <= spread_b),
        "a_minus_b_within_b_range": bool(med["a"] - b_ms <= range_b),
        "c_model_strings": n_model, "c_per_stage_plus_model_wall_ms": med["c"],
        "c_us_per_string": med["c"] * 1e3 / max(n_model, 1),
        "a_us_per_string": med["a"] * 1e3 / n, "b_us_per_string": b_ms * 1e3 / n,
        "alignment_by_events": events,
        "extra_d2h_bytes_per_string": 8.0 * out_bytes / n,
        "aligned_text_equals_text_entry": bool(same_text),
        "aligned_maps_equal_model_on_c": bool(same_maps),
        "device_pieces_equal_host_entry": same_device,
        "walls_ms": ms,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--strings", type=int, default=65536)
    ap.add_argument("--model-strings", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for sem in (F.FST_SEM_LAZY, F.FST_SEM_EAGER):
        rows.append(run(a.strings, min(a.model_strings, a.strings), sem, a.rounds, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"what": "scripts/text_align_bench.py, one process, one MI355X; more than "
                               "one device: not measured", "rows": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

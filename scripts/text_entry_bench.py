"""Label entry vs text entry of the host batch API, in one process, on one GPU.

Two workloads, each with four legs alternating after warm-up -- the label entry twice (A and
B: their difference is the run-to-run spread), the text entry, and the text entry with
FSTAMD_STREAM=0 (its sharded route):

  config4  SY.tagger() -> SY.verbalizer(), 65,536 utterances (scripts/bench_configs.py's
           config 4): fst_pipeline_batch vs fst_normalize_text_batch, lazy and eager (two
           stages: the text entry takes the sharded route either way)
  metric   ambiguous T=4096 B=12, 1M strings of 64 labels, eager (bench.py's shape):
           fst_compose_frozen_shortest_path_batch (the streamed label route) vs
           fst_normalize_text_batch (the streamed text route; sharded with FSTAMD_STREAM=0)

Per leg: host wall time (the calls return host memory, so they are synchronised), the
engine's kernel_ms (fst_last_launch_stats: the last stage's engine kernels, for the streamed
routes the wall time of the overlapped parts; the sharded route's emission and widen kernels
are not in it) and the H2D / D2H bytes of the call computed from the shapes.
Both text legs' results are compared with batch_result_to_text of the label leg's result at
the timed size.  One JSON line per workload; --out also writes them to a file.

usage: python scripts/text_entry_bench.py [--rounds 7] [--warmup 3] [--only config4,metric]
           [--config4-strings N] [--metric-strings N] [--out FILE]
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
from libfst_amd import fst as FF  # noqa: E402
from libfst_amd import synthetic as SY  # noqa: E402


def label_bytes(n, total_in, arcs):
    return {"h2d": 4 * total_in + 8 * (n + 1), "d2h": 16 * arcs + 4 * n + 8 * (n + 1) + 8 * n}


def text_bytes(n, total_in, out_bytes):
    return {"h2d": total_in + 8 * (n + 1), "d2h": out_bytes + 4 * n + 8 * (n + 1) + 8 * n}


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


def same_text(a, b):
    return all(np.array_equal(x, y) for x, y in (
        (a.status, b.status), (a.offsets, b.offsets), (a.text, b.text),
        (a.total_weight.view(np.uint64), b.total_weight.view(np.uint64))))


def run_legs(name, label_call, text_call, n, total_in, rounds, warmup):
    """label_call() -> BatchResult, text_call() -> TextResult; results are dropped right after
    each call so that the pinned blocks go back to the pool, as a caller's loop would."""
    sharded_call = no_stream(text_call)
    legs = (("label_a", label_call), ("text", text_call), ("text_sharded", sharded_call),
            ("label_b", label_call))
    for _ in range(warmup):
        label_call()
        text_call()
        sharded_call()
    walls = {leg: [] for leg, _ in legs}
    kms = {leg: [] for leg, _ in legs}
    for _ in range(rounds):
        for leg, call in legs:
            t0 = time.perf_counter()
            r = call()
            walls[leg].append(time.perf_counter() - t0)
            kms[leg].append(F.last_launch_stats().kernel_ms)
            del r
    # the same strings through both entries, compared at the timed size
    lab, txt, sh = label_call(), text_call(), sharded_call()
    conv = F.batch_result_to_text(lab)
    identical = same_text(conv, txt)
    identical_sharded = same_text(conv, sh)
    arcs, out_bytes = int(lab.offsets[-1]), int(txt.offsets[-1])
    ok = int((txt.status == 0).sum())
    del lab, txt, sh, conv
    med = {k: float(np.median(v)) for k, v in walls.items()}
    label = float(np.median(walls["label_a"] + walls["label_b"]))
    spread = abs(med["label_a"] - med["label_b"])
    lb, tb = label_bytes(n, total_in, arcs), text_bytes(n, total_in, out_bytes)
    return {
        "workload": name, "strings": n, "ok": ok, "rounds": rounds, "warmup": warmup,
        "label_wall_ms": label * 1e3, "label_a_wall_ms": med["label_a"] * 1e3,
        "label_b_wall_ms": med["label_b"] * 1e3, "label_spread_ms": spread * 1e3,
        "text_wall_ms": med["text"] * 1e3,
        "text_sharded_wall_ms": med["text_sharded"] * 1e3,
        "text_within_spread_or_faster": bool(med["text"] <= label + spread),
        "text_beats_sharded_by_more_than_spread": bool(
            med["text"] + spread < med["text_sharded"]),
        "label_kernel_ms": float(np.median(kms["label_a"] + kms["label_b"])),
        "text_kernel_ms": float(np.median(kms["text"])),
        "text_sharded_kernel_ms": float(np.median(kms["text_sharded"])),
        "label_bytes": lb, "text_bytes": tb,
        "label_bytes_per_string": {k: v / n for k, v in lb.items()},
        "text_bytes_per_string": {k: v / n for k, v in tb.items()},
        "text_equals_converted_label_result": bool(identical),
        "text_sharded_equals_converted_label_result": bool(identical_sharded),
        "walls_ms": {k: [x * 1e3 for x in v] for k, v in walls.items()},
    }


def config4(n, sem, rounds, warmup):
    stages = [SY.to_mutable(SY.tagger()).freeze(), SY.to_mutable(SY.verbalizer()).freeze()]
    texts = SY.utterances(np.random.default_rng(44), n)
    labels, offsets = SY.to_labels(texts)
    data, toff = FF.text_csr([t.encode() for t in texts])
    name = f"config4 tagger -> verbalizer, {'lazy' if sem == F.FST_SEM_LAZY else 'eager'}"
    return run_legs(name, lambda: F.pipeline_batch(stages, labels, offsets, 1, sem),
                    lambda: F.normalize_text_batch(stages, (data, toff), sem),
                    n, int(offsets[-1]), rounds, warmup)


def metric(n, rounds, warmup):
    rhs = F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 4096, 12)
    L = 64
    labels = np.ones(n * L, np.uint32)
    offsets = (np.arange(n + 1, dtype=np.uint64) * L)
    data = np.zeros(n * L, np.uint8)   # byte 0 is label 1
    sem = F.FST_SEM_EAGER
    return run_legs("metric ambiguous T=4096 B=12, 64 labels, eager",
                    lambda: F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem),
                    lambda: F.normalize_text_batch([rhs], (data, offsets), sem),
                    n, n * L, rounds, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="config4,metric")
    ap.add_argument("--config4-strings", type=int, default=65536)
    ap.add_argument("--metric-strings", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    only = a.only.split(",")
    if "config4" in only:
        for sem in (F.FST_SEM_LAZY, F.FST_SEM_EAGER):
            rows.append(config4(a.config4_strings, sem, a.rounds, a.warmup))
            print(json.dumps(rows[-1]), flush=True)
    if "metric" in only:
        rows.append(metric(a.metric_strings, a.rounds, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

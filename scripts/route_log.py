"""Which way small fixed batches go through the engine's host layer: the route record.

One case per route of DeviceEngine::run_chain (device_engine.hip chain_route), eager and lazy,
then the knobs that move strings between tiers, then an lhs batch and a lattice batch.  Each
case runs in a fresh child process (the per-rhs adaptive flags start equal) with
FSTAMD_ROUTE_LOG=1, and its record is the library's "[libfst_amd route]" lines plus the
LaunchStats of the call (engine, grid, launches) and a checksum of the statuses.  Two builds
of the library route alike exactly when their records are the same file:

  python scripts/route_log.py --out a.txt                      # this tree's build
  LIBFST_AMD_LIB=/path/to/other/libfst_amd.so python scripts/route_log.py --out b.txt
  diff a.txt b.txt

Band plans print the free HBM of the moment; no case here reaches the band replay.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KNOBS = ("FSTAMD_BFS_TINY", "FSTAMD_BFS_TINY_START", "FSTAMD_EAGER_CTINY", "FSTAMD_LAZY_TINY",
         "FSTAMD_LAZY_TINY_START", "FSTAMD_EAGER_TIER1", "FSTAMD_LAZY_ENGINE", "FSTAMD_BFS_WG0")

# name -> (workload, semantics, environment)
CASES = [
    ("eager-nan", "nan", "eager", {}),
    ("eager-replay", "negative", "eager", {}),
    ("eager-general", "tagger", "eager", {}),
    ("eager-tiers", "ambiguous", "eager", {}),
    ("lazy-dense", "tagger", "lazy", {}),
    ("lazy-rounds", "ambiguous", "lazy", {}),
    ("lazy-hashed", "negative", "lazy", {}),
    ("lazy-hashed-forced", "tagger", "lazy", {"FSTAMD_LAZY_ENGINE": "replay"}),
    ("lazy-rounds-forced", "tagger", "lazy", {"FSTAMD_LAZY_ENGINE": "rounds"}),
    ("bfs-tiny-0", "tagger", "eager", {"FSTAMD_BFS_TINY": "0"}),
    ("bfs-tiny-0-replay", "negative", "eager", {"FSTAMD_BFS_TINY": "0"}),
    ("bfs-tiny-start-2", "tagger", "eager", {"FSTAMD_BFS_TINY_START": "2"}),
    ("eager-ctiny-0", "tagger", "eager", {"FSTAMD_EAGER_CTINY": "0"}),
    ("bfs-wg0-256", "tagger", "eager", {"FSTAMD_BFS_WG0": "256", "FSTAMD_BFS_TINY": "0"}),
    ("lazy-tiny-0", "tagger", "lazy", {"FSTAMD_LAZY_TINY": "0"}),
    ("lazy-tiny-0-hashed", "negative", "lazy", {"FSTAMD_LAZY_TINY": "0"}),
    ("lazy-tiny-start-2", "tagger", "lazy", {"FSTAMD_LAZY_TINY_START": "2"}),
    ("lazy-many", "tagger-many", "lazy", {}),
    ("eager-tier1-window", "ambiguous", "eager", {"FSTAMD_EAGER_TIER1": "window"}),
    ("eager-tier1-wave", "ambiguous", "eager", {"FSTAMD_EAGER_TIER1": "wave"}),
    ("eager-tier1-wg", "ambiguous", "eager", {"FSTAMD_EAGER_TIER1": "wg"}),
    ("lhs-batch-eager", "lhs", "eager", {}),
    ("lhs-batch-lazy", "lhs", "lazy", {}),
    ("lattice-batch", "lattice", "eager", {}),
]


def small_rhs(F, weight):
    """Five states in a ring over labels 1..3, one arc carrying `weight` (NaN or negative)."""
    m = F.MutableFst()
    for _ in range(5):
        m.add_state()
    m.set_start(0)
    m.set_final(4, 0.0)
    for s in range(5):
        for lab in (1, 2, 3):
            m.add_arc(s, lab, lab, float(lab), (s + lab) % 5)
    m.add_arc(0, 1, 2, weight, 3)
    return m.freeze()


def run_case(workload, sem_name):
    import libfst_amd as F
    from libfst_amd import synthetic as SY
    sem = F.FST_SEM_EAGER if sem_name == "eager" else F.FST_SEM_LAZY
    rng = np.random.default_rng(2024)
    if workload in ("nan", "negative"):
        rhs = small_rhs(F, float("nan") if workload == "nan" else -1.5)
        lens = rng.integers(0, 12, 64)
        labels = np.concatenate([rng.integers(1, 4, n) for n in lens]).astype(np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        r = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    elif workload == "ambiguous":
        rhs = F.Fst.bench_transducer(F.BENCH_AMBIGUOUS, 256, 12)
        lens = rng.integers(0, 40, 96)
        labels = np.concatenate([np.where(rng.random(n) < 0.9, 1, 2) for n in lens]).astype(np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        r = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    elif workload in ("tagger", "tagger-many"):
        rhs = SY.to_mutable(SY.tagger()).freeze()
        texts = SY.utterances(rng, 4096 if workload == "tagger-many" else 200)
        if workload == "tagger-many":  # a few lattices past every LDS size
            texts[::512] = [t * 12 for t in texts[::512]]
        labels, offsets = SY.to_labels(texts)
        r = F.compose_frozen_shortest_path_batch(rhs, labels, offsets, 1, sem)
    else:
        rhs = SY.to_mutable(SY.tagger()).freeze()
        texts = SY.utterances(rng, 128)
        if workload == "lhs":
            lhs = F.LhsBatch.from_fsts([SY.confusion_network(rng, t, 3, 0.1) for t in texts])
            r = F.compose_frozen_shortest_path_lhs_batch(rhs, lhs, 1, sem)
        else:
            r = F.compose_frozen_batch(rhs, *SY.to_labels(texts))
    st = F.last_launch_stats()
    status = np.asarray(r.status, np.int64)
    print(f"stats: engine {int(st.engine)} grid {int(st.grid)} launches {int(st.launches)} | "
          f"statuses {len(status)} sum {int(status.sum())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process")
    a = ap.parse_args()
    if a.case:
        name, workload, sem, _ = next(c for c in CASES if c[0] == a.case)
        run_case(workload, sem)
        return 0
    lines, bad = [], 0
    for name, _, _, env in CASES:
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env, FSTAMD_ROUTE_LOG="1")
        knobs = " ".join(f"{k}={v}" for k, v in sorted(env.items())) or "-"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], env=e,
                               capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:  # a hang: recorded, and nothing more runs on this GPU
            lines.append(f"== {name} ({knobs}) hung: no answer in 120 s")
            bad += 1
            break
        lines.append(f"== {name} ({knobs}) rc {p.returncode}")
        lines += [x for x in p.stderr.splitlines() if x.startswith("[libfst_amd route]")]
        lines += [x for x in p.stdout.splitlines() if x.startswith("stats:")]
        if p.returncode != 0:
            bad += 1
            lines += ["!! " + x for x in p.stderr.splitlines()[-5:]]
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                break  # a fault or a hang: nothing more runs on this GPU
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""bench.py's rank topology (CPU): `--gpus N` without a launcher starts torchrun with N ranks
as a child process (the driver's 1/2/4/8-GPU runs call `python bench.py --gpus N` directly),
and a WORLD_SIZE that disagrees with --gpus is refused before anything touches a GPU.
Also on the CPU: --no-e2e needs --full, and the files --dump-outputs writes (dump_outputs on
a made-up result: whole batch, sampled batch, the size bound)."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BENCH = os.path.join(os.path.dirname(HERE), "bench.py")


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True,
                          text=True, timeout=120)


def test_gpus_n_launches_n_ranks():
    r = _run(["--gpus", "4", "--steps", "3", "--warmup", "1"], {"FSTAMD_BENCH_DRY_LAUNCH": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    cmd = json.loads(r.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert os.path.samefile(cmd[-7], BENCH)


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and "WORLD_SIZE=3 but --gpus 2" in r.stderr
    r = _run(["--gpus", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2


def test_no_e2e_needs_full():
    # --no-e2e swaps the headline for the kernel-resident leg, which only --full runs; and
    # --dump-outputs writes the host entry's result, which --no-e2e drops
    r = _run(["--gpus", "1", "--no-e2e"], {})
    assert r.returncode == 2 and "--full" in r.stderr
    r = _run(["--gpus", "1", "--full", "--no-e2e", "--dump-outputs", "x"], {})
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


class _Result:
    """A host BatchResult as dump_outputs reads it: string i has i % 4 arcs, arc k of the
    batch carries ilabel k, olabel 2 k, weight k / 4; strings 5, 10, ... have no path."""

    def __init__(self, num):
        plen = np.arange(num) % 4
        self.status = np.where((np.arange(num) % 5 == 0) & (plen == 0), 1, 0).astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
        arcs = int(self.offsets[-1])
        self.ilabels = np.arange(arcs, dtype=np.uint32)
        self.olabels = 2 * np.arange(arcs, dtype=np.uint32)
        self.weights = np.arange(arcs) / 4.0
        self.finals = np.where(self.status == 0, np.arange(num) + 0.5, np.nan)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_whole_batch(tmp_path):
    import bench
    r = _Result(37)
    bench.dump_outputs(r, str(tmp_path / "a"))
    bench.dump_outputs(_Result(37), str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["finals", "ilabels", "offsets", "olabels", "path_strings", "status",
                         "strings", "weights"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)          # NaN-free, run to run
    assert np.array_equal(a["status"], r.status) and np.array_equal(a["offsets"], r.offsets)
    assert np.array_equal(a["ilabels"], r.ilabels) and np.array_equal(a["olabels"], r.olabels)
    assert np.array_equal(a["weights"], r.weights)
    assert np.array_equal(a["finals"], np.where(r.status == 0, r.finals, 0.0))


def test_dump_outputs_samples_a_large_batch(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_STRINGS", 64)
    monkeypatch.setattr(bench, "DUMP_PATHS", 16)
    monkeypatch.setattr(bench, "DUMP_ARCS", 20)
    r = _Result(1000)
    bench.dump_outputs(r, str(tmp_path))
    a = _load(tmp_path)
    s, p = a["strings"].astype(np.int64), a["path_strings"].astype(np.int64)
    assert len(s) == 32 and len(p) == 16
    assert np.all(np.diff(s) > 0) and np.all(np.diff(p) > 0) and s[-1] < 1000 and p[-1] < 1000
    assert np.array_equal(a["status"], r.status[s])
    assert np.array_equal(a["offsets_begin"], r.offsets[s])
    assert np.array_equal(a["offsets"], r.offsets[s + 1])
    want = np.concatenate([np.arange(r.offsets[i], r.offsets[i + 1]) for i in p])[:20]
    assert len(want) == 20 and np.array_equal(a["ilabels"], want)
    assert np.array_equal(a["olabels"], 2 * want) and np.array_equal(a["weights"], want / 4.0)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total < 20 * 8 * 3 + 32 * 8 * 5 + 16 * 8 + 10 * 128   # arrays + .npy headers


def test_dump_outputs_fits_the_budget():
    # the bounds at their real values: per-string arrays whole up to 1M strings
    # (strings, offsets + 1, finals in f64, status in f32), 16K paths' ids, 1M arcs x 3
    import bench
    n, a = bench.DUMP_STRINGS, bench.DUMP_ARCS
    assert (3 * 8 + 4) * n + 8 + 8 * bench.DUMP_PATHS + 3 * 8 * a + 8 * 128 <= 64 * 10**6

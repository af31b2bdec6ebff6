"""A plain `bench.py --gpus 1 --steps K --warmup W` run on the GPU: the headline alone (none
of --full's legs in the line), `ms_per_step` consistent with `value`, and --dump-outputs
writing the last timed step's host result, checked here against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import libfst_amd as F
import oracle_ffi as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BENCH = os.path.join(os.path.dirname(HERE), "bench.py")
FULL_ONLY = ("roofline", "cpu_baseline", "checked_vs_oracle", "value_kernel", "kernel_resident",
             "end_to_end", "varied", "lazy", "f64_cells", "fractional_weights",
             "non_dyadic_weights", "wide_weight_table")


def test_plain_run_and_dump(tmp_path):
    # 20,000 strings: more than the dump's sample of paths (16,384 strings), fewer than its
    # bound on the per-string arrays
    num, L, T, B = 20000, 16, 256, 12
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", str(num), "--len", str(L), "--transducer-len", str(T),
                        "--branches", str(B), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "strings/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["metric"].startswith("strings/sec")
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(num * 1e3 / line["ms_per_step"], rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]

    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sorted(d) == ["finals", "ilabels", "offsets", "olabels", "path_strings", "status",
                         "strings", "weights"]
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    # every string is 1^L: one oracle run gives every string's expected path
    blob = O.freeze(O.gen("ambiguous", T, B))
    ref = O.batch_run(blob, np.ones(L, np.uint32), np.array([0, L], np.uint64), 1)
    assert ref.empty[0] == 0 and int(ref.offsets[1]) == L
    assert np.array_equal(d["strings"], np.arange(num))
    assert np.array_equal(d["status"], np.full(num, F.FST_PATH_OK))
    assert np.array_equal(d["offsets"], np.arange(num + 1) * L)
    assert np.array_equal(d["finals"], np.full(num, ref.finals[0]))
    p = d["path_strings"]
    assert len(p) == 16384 and np.all(np.diff(p) > 0) and 0 <= p[0] and p[-1] < num
    for name in ("ilabels", "olabels", "weights"):
        assert np.array_equal(d[name], np.tile(getattr(ref, name).astype(np.float64), len(p)))

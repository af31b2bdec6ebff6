"""The lhs and lattice batch host layer on one small fixed batch: routes, shard plans, host
profile lines and a digest of every result array, for comparing two builds of the library.

Every host entry on general lhs and every lattice entry runs on synthetic.edge_networks() -- 48
confusion networks of 3 to 10 positions with up to 3 alternatives each, two of them with a
negative weight (the replay list), one with a NaN, one without states, one of one state, one
with a dead end -- and the chain entries on 48 strings of 0 to 12 labels.  Each case runs in
four layouts: one shard, 2 and 3 shards on one GPU, and one shard with a first arena too small
for the batch (the rerun path).
A layout is one fresh child process with FSTAMD_ROUTE_LOG, FSTAMD_SHARD_LOG and FSTAMD_HOST_PROF
set; its record is the library's "[libfst_amd route|shard|host]" lines with the times masked
(sorted per call when the call has several shards: they print from threads), the LaunchStats of
the call and a SHA-256 of every result array.  Two builds agree exactly when their records are
the same file:

  python scripts/lhs_host_routes.py --out a.txt                 # this tree's build
  LIBFST_AMD_LIB=/path/to/other/libfst_amd.so python scripts/lhs_host_routes.py --out b.txt
  diff a.txt b.txt
"""
import argparse
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name -> (shards, environment)
LAYOUTS = [
    ("one-shard", 0, {}),
    ("two-shards", 2, {}),
    ("three-shards", 3, {}),
    ("small-arena", 0, {"FSTAMD_ARENA_ARCS": "8", "FSTAMD_LATTICE_ARENA": "8,8"}),
]
KNOBS = ("FSTAMD_ARENA_ARCS", "FSTAMD_LATTICE_ARENA", "FSTAMD_STREAM", "FSTAMD_PIPELINE",
         "FSTAMD_GRAPH_GRID", "FSTAMD_TRIM_SWEEPS", "FSTAMD_SP_SWEEPS")
MARK = "== case "


def strings(SY):
    return SY.utterances(np.random.default_rng(1212), 48, 0, 12)


def digest(**arrays):
    return " ".join(f"{k} {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]}"
                    for k, v in arrays.items())


def digest_of(r):
    names = [n for n in ("status", "offsets", "state_offsets", "start", "final_weights",
                         "arc_offsets", "ilabels", "olabels", "weights", "nextstates", "finals",
                         "text", "total_weight") if hasattr(r, n)]
    return digest(**{n: getattr(r, n) for n in names})


def run_layout(shards):
    import torch

    import libfst_amd as F
    from libfst_amd import fst as FF
    from libfst_amd import synthetic as SY

    torch.cuda.set_device(0)
    tagger = SY.to_mutable(SY.tagger()).freeze()
    stages = [tagger, SY.to_mutable(SY.verbalizer()).freeze()]
    fsts = SY.edge_networks()
    lhs = F.LhsBatch.from_fsts(fsts)
    texts = strings(SY)
    labels, offsets = SY.to_labels(texts)
    kw = {"devices": [0], "shards": shards} if shards else {}

    def handles():
        ms = []
        for st, fin, arcs in fsts:
            m = F.MutableFst()
            for _ in fin:
                m.add_state()
            if st is not None:
                m.set_start(st)
            for s, fw in enumerate(fin):
                if fw != SY.INF:
                    m.set_final(s, fw)
            for s, al in enumerate(arcs):
                for il, ol, w, nx in al:
                    m.add_arc(s, il, ol, w, nx)
            ms.append(m)
        return F.compose_frozen_shortest_path_handles_batch(tagger, ms, 1, F.FST_SEM_EAGER, **kw)

    def text_sharded():
        os.environ["FSTAMD_STREAM"] = "0"
        try:
            return F.normalize_text_batch(stages, [t.encode() for t in texts], **kw)
        finally:
            del os.environ["FSTAMD_STREAM"]

    def dev(a):
        signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
        return torch.as_tensor(a.view(signed) if signed else a, device="cuda:0")

    def zeros(n, dt):
        return torch.zeros(max(int(n), 1), dtype=dt, device="cuda:0")

    opts = FF.FstBatchOptions(0, F.FST_SEM_EAGER, 0, 0, 0)

    def device_paths(call, num, cap):
        """A device 1-best entry into an arena of `cap` arcs; the digest is of the items in item
        order (the order of the paths in the arena is the kernels' own)."""
        st, ln, off = zeros(num, torch.int32), zeros(num, torch.int32), zeros(num, torch.int64)
        fin, w = zeros(num, torch.float64), zeros(cap, torch.float64)
        il, ol, cur = zeros(cap, torch.int32), zeros(cap, torch.int32), zeros(1, torch.int64)
        desc = FF.FstDeviceBatch(st.data_ptr(), ln.data_ptr(), off.data_ptr(), fin.data_ptr(),
                                 il.data_ptr(), ol.data_ptr(), w.data_ptr(), cap, cur.data_ptr(), 0)
        rc = call(C.byref(desc))
        assert rc == FF.FST_OK, rc
        torch.cuda.synchronize()
        st, ln, off = st.cpu().numpy()[:num], ln.cpu().numpy()[:num], off.cpu().numpy()[:num]
        il, ol, w = il.cpu().numpy(), ol.cpu().numpy(), w.cpu().numpy()
        ok = st == F.FST_PATH_OK
        rows = [np.arange(int(a), int(a) + int(n)) for a, n, k in zip(off, ln, ok) if k]
        idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        return digest(status=st, lengths=np.where(ok, ln, 0), ilabels=il[idx], olabels=ol[idx],
                      weights=w[idx], finals=np.where(ok, fin.cpu().numpy()[:num], 0.0),
                      cursor=cur.cpu().numpy())

    d_lhs = {k: dev(getattr(lhs, k)) for k in ("state_offsets", "start", "final_weights",
                                               "arc_offsets", "ilabels", "olabels", "weights",
                                               "nextstates")}
    cs = FF.FstLhsBatch(len(lhs), *[t.data_ptr() for t in d_lhs.values()])

    def device_lattices():
        num = len(texts)
        host = F.compose_frozen_batch(tagger, labels, offsets, connect=True)
        ns, na = int(host.state_offsets[-1]), int(host.arc_offsets[-1])
        t = {"status": zeros(num, torch.int32), "state_offsets": zeros(num + 1, torch.int64),
             "start": zeros(num, torch.int32), "final_weights": zeros(ns, torch.float64),
             "arc_offsets": zeros(ns + 1, torch.int64), "ilabels": zeros(na, torch.int32),
             "olabels": zeros(na, torch.int32), "weights": zeros(na, torch.float64),
             "nextstates": zeros(na, torch.int32)}
        desc = FF.FstDeviceLattices(*[x.data_ptr() for x in t.values()], ns, na)
        needed = (C.c_uint64 * 2)(0, 0)
        d_lab, d_off = dev(labels), dev(offsets)
        rc = F.lib().fst_device_compose_frozen(tagger.h, d_lab.data_ptr(), d_off.data_ptr(), num,
                                               12, F.FST_LATTICE_CONNECT, C.byref(opts),
                                               C.byref(desc), needed, None)
        assert rc == FF.FST_OK, rc
        torch.cuda.synchronize()
        sizes = {"status": num, "state_offsets": num + 1, "start": num, "final_weights": ns,
                 "arc_offsets": ns + 1, "ilabels": na, "olabels": na, "weights": na,
                 "nextstates": na}
        return digest(needed=np.array(list(needed), np.uint64),
                      **{k: v.cpu().numpy()[:sizes[k]] for k, v in t.items()})

    L = F.lib()
    cap = 16 * len(lhs.ilabels) + 1024
    cases = [
        ("lhs-batch-lazy", lambda: F.compose_frozen_shortest_path_lhs_batch(
            tagger, lhs, 1, F.FST_SEM_LAZY, **kw)),
        ("lhs-batch-eager", lambda: F.compose_frozen_shortest_path_lhs_batch(
            tagger, lhs, 1, F.FST_SEM_EAGER, **kw)),
        ("handles-batch", handles),
        ("pipeline-lhs", lambda: F.pipeline_lhs_batch(stages, lhs, 1, F.FST_SEM_EAGER, **kw)),
        ("normalize-lhs", lambda: F.normalize_lhs_batch(stages, lhs, F.FST_SEM_EAGER, **kw)),
        ("lattice-chain", lambda: F.compose_frozen_batch(tagger, labels, offsets, **kw)),
        ("lattice-chain-project-connect", lambda: F.compose_frozen_batch(
            tagger, labels, offsets, project_output=True, connect=True, **kw)),
        ("lattice-lhs", lambda: F.compose_frozen_lhs_batch(tagger, lhs, **kw)),
        ("lattice-lhs-project-connect", lambda: F.compose_frozen_lhs_batch(
            tagger, lhs, project_output=True, connect=True, **kw)),
        ("connect-lhs", lambda: F.connect_lhs_batch(lhs, **kw)),
        ("shortest-path-lhs", lambda: F.shortest_path_lhs_batch(lhs, 1, **kw)),
        ("pipeline-batch", lambda: F.pipeline_batch(stages, labels, offsets, 1, F.FST_SEM_EAGER,
                                                    **kw)),
        ("normalize-text-sharded", text_sharded),
        ("device-compose-shortest-path-lhs", lambda: device_paths(
            lambda o: L.fst_device_compose_shortest_path_lhs(tagger.h, C.byref(cs), 1,
                                                             C.byref(opts), o, None),
            len(lhs), cap)),
        ("device-shortest-path-lhs", lambda: device_paths(
            lambda o: L.fst_device_shortest_path_lhs(C.byref(cs), 1, C.byref(opts), o, None),
            len(lhs), int(lhs.state_offsets[-1]))),
        ("device-compose-frozen", device_lattices),
    ]
    for name, fn in cases:
        sys.stderr.write(f"{MARK}{name}\n")
        sys.stderr.flush()
        r = fn()
        st = F.last_launch_stats()
        sys.stderr.write(f"stats: engine {int(st.engine)} grid {int(st.grid)} launches "
                         f"{int(st.launches)}\n")
        sys.stderr.write(f"sha256: {r if isinstance(r, str) else digest_of(r)}\n")
        sys.stderr.flush()


def masked(line):
    """A log line without its times: every 'x.yz ms' and, in a host profile line, every figure."""
    if line.startswith("[libfst_amd host]"):
        head, _, tail = line.partition(": inputs ")
        return head + ": inputs " + re.sub(r"\d+\.\d+", "T", tail)
    return re.sub(r"\d+\.\d+ ms", "T ms", line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layout", default=None, help="(internal) run one layout in this process")
    a = ap.parse_args()
    if a.layout:
        run_layout(next(s for n, s, _ in LAYOUTS if n == a.layout))
        return 0
    keep = ("[libfst_amd route]", "[libfst_amd shard]", "[libfst_amd host]", "stats:", "sha256:")
    lines, bad = [], 0
    for name, shards, env in LAYOUTS:
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env, FSTAMD_ROUTE_LOG="1", FSTAMD_SHARD_LOG="1", FSTAMD_HOST_PROF="1")
        knobs = " ".join(f"{k}={v}" for k, v in sorted(env.items())) or "-"
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--layout", name],
                               env=e, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:  # a hang: recorded, and nothing more runs on this GPU
            lines.append(f"==== {name} ({knobs}) hung: no answer in 240 s")
            bad += 1
            break
        lines.append(f"==== {name} ({knobs}) rc {p.returncode}")
        call = []

        def flush():
            lines.extend(sorted(call) if shards > 1 else call)
            call.clear()

        for x in p.stderr.splitlines():
            if x.startswith(MARK):
                flush()
                lines.append(x)
            elif x.startswith(keep):
                call.append(masked(x))
        flush()
        if p.returncode != 0:
            bad += 1
            lines += ["!! " + x for x in p.stderr.splitlines()[-8:]]
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

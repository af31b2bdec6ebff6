"""GPU: the stream contract of the fst_device_* entries on a caller-owned, non-blocking stream.

Every other suite (and bench.py) passes the null stream, the one stream on which the contract
cannot fail: it serialises with every blocking stream whether the library orders anything or
not.  Here the caller's stream S is a torch.cuda.Stream (non-blocking) and R is a second one,
used for read-back.

Late inputs.  The input buffers of a call hold a DECOY (another valid input over the same offset
arrays, so that extents, nextstates and capacities are those of the real input and a premature
read stays in bounds); S then gets a sleep and device-to-device copies of the real input into the
same buffers, and the entry is called with S.  A call that reads its inputs before S reaches them
gives the decoy's result.  Outputs are pre-filled with a sentinel.  An entry documented as
synchronising is read back on R, with no wait on S, once it returns; an asynchronous one is
snapshotted on S, its outputs overwritten on S, and the snapshot compared after S is drained.

Expected: the same entry on the real input on the null stream (what the other suites pin to the
oracle and the models), plus direct comparisons with the oracle (compose_shortest_path,
compose_frozen) and the posterior model.  Path arenas are filled through an atomic cursor, so
where a string's arcs lie is not fixed run to run: FstDeviceBatch results are compared per string
(status, arcs, weights and final weight bit for bit), by the cursor, and by the arena behind the
cursor still holding the sentinel.  Everything else is compared as whole arrays, byte for byte.

Intermediate buffers of the chains are pre-filled so that a premature read of them stays in
bounds too (offsets and lengths 0, statuses not OK): the tests look for wrong results, none is
meant to fault.
"""
import contextlib
import ctypes as C
import json
import os
import time
import types

import numpy as np
import pytest
import torch

import libfst_amd as F
import libfst_amd.fst as FF
import oracle_ffi as O
import posterior_model as PM
from libfst_amd import synthetic as SY
from test_gpu_concurrency import run_threads
from test_gpu_lattice_batch import DeviceLattices, assert_item, chain_fst, oracle
from test_gpu_lattice_posterior import RATIOS, DevicePost, compare
from test_gpu_lattice_sp import emit_text, tagger_blob, verbalizer_blob
from test_gpu_lhs_device import DeviceLhs, DeviceOut, dev_tensor
from test_gpu_multidevice import run_py
from test_gpu_parity import check as check_host_against_oracle
from test_gpu_parity import expected_status, load_blob
from test_posterior_model import random_item

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAZY, EAGER = F.FST_SEM_LAZY, F.FST_SEM_EAGER
OK, EMPTY, UNSUPPORTED = F.FST_PATH_OK, F.FST_PATH_EMPTY, F.FST_PATH_UNSUPPORTED
SENT32, SENT64, SENT8, SENTF = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0x5A, DevicePost.SENTINEL
WRONG = 0xDEAD                   # what the host outputs hold before a call
NBEST = 4
BEAM = 0.5
TIER_ENV = {"FSTAMD_NBEST_LDS": "0", "FSTAMD_PRUNE_SWEEPS": "0", "FSTAMD_POSTERIOR_LDS": "0"}


def P(t):
    return C.c_void_p(t.data_ptr())


def SP(stream):
    return C.c_void_p(stream) if stream else None


def prefill(tensors):
    for t in tensors:
        t.fill_(SENTF if t.dtype.is_floating_point else
                {torch.uint8: SENT8, torch.int32: SENT32, torch.int64: SENT64}[t.dtype])


def opts_of(sem=LAZY):
    return FF.FstBatchOptions(0, sem, 0, 0, 0)


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


# ---- buffers ---------------------------------------------------------------------------------------

class Late:
    """Input buffers with their two contents: `load("decoy")` / `load("real")` copy in place,
    on the current stream, so the pointers the entry was given do not move."""

    def __init__(self, buf, real, decoy):
        assert len(buf) == len(real) == len(decoy)
        for b, r, d in zip(buf, real, decoy):
            assert b.shape == r.shape == d.shape and b.dtype == r.dtype == d.dtype
        self.buf, self.real, self.decoy = list(buf), [t.clone() for t in real], \
            [t.clone() for t in decoy]

    def load(self, which):
        for b, s in zip(self.buf, getattr(self, which)):
            b.copy_(s)


def paths_tensors(o: DeviceOut):
    return [o.status, o.plen, o.poff, o.fin, o.il, o.ol, o.w, o.cur]


def lattice_tensors(o: DeviceLattices):
    return [o.status, o.soff, o.start, o.fin, o.aoff, o.il, o.ol, o.w, o.nx]


def post_tensors(o: DevicePost):
    return [o.status, o.total, o.alpha, o.beta, o.arc_cost]


def quiet_paths(o: DeviceOut):
    """An FstDeviceBatch between two stages of a chain: no string is OK, so a consumer that ran
    early would read no arc of it."""
    prefill([o.fin, o.il, o.ol, o.w, o.cur])
    o.status.fill_(-1)
    o.plen.zero_()
    o.poff.zero_()


def quiet_lattices(o: DeviceLattices):
    """An FstDeviceLattices between two stages: every item has zero states."""
    prefill([o.status, o.fin, o.il, o.ol, o.w, o.nx])
    o.soff.zero_()
    o.aoff.zero_()
    o.start.zero_()


def canon_paths(arrs, num, cap):
    """An FstDeviceBatch result without the placement of the strings in the arena."""
    st, ln, off, fin, il, ol, w, cur = arrs
    cursor = int(cur.view(np.uint64)[0])
    items = []
    for i in range(num):
        if int(st[i]) != OK:
            items.append((int(st[i]),))
            continue
        a0, a1 = int(off[i]), int(off[i]) + int(ln[i])
        assert 0 <= a0 <= a1 <= cap, (i, a0, a1, cap)
        items.append((OK, il[a0:a1].tobytes(), ol[a0:a1].tobytes(), w[a0:a1].tobytes(),
                      fin[i:i + 1].tobytes()))
    c = min(cursor, cap)
    untouched = bool(np.all(il[c:] == SENT32) and np.all(ol[c:] == SENT32) and
                     np.all(w[c:] == SENTF))
    return cursor, items, untouched


def canon_bytes(arrs):
    return [a.tobytes() for a in arrs]


# ---- the inputs ------------------------------------------------------------------------------------

def text_front():
    """96 strings of 0..40 bytes for the tagger, among them an empty and a dead one, and a decoy
    of other bytes over the same offsets."""
    rng = np.random.default_rng(2024)
    texts = SY.utterances(rng, 96, 0, 40)
    texts[0], texts[1], texts[2] = "", "ab#c", SY.utterances(rng, 1, 40, 40)[0]
    rng = np.random.default_rng(2025)
    decoy = [SY.utterances(rng, 1, len(t), len(t))[0] for t in texts]
    assert sum(a != b for a, b in zip(texts, decoy)) > 80
    return texts, decoy


def label_front():
    """96 label strings of 0..40 labels for the ambiguous rhs (every arc reads label 1; a 2 is
    dead), and a decoy with the dead strings elsewhere."""
    rng = np.random.default_rng(2026)
    real, decoy = [], []
    for i in range(96):
        L = int(rng.integers(0, 41)) if i else 0
        a, b = [1] * L, [1] * L
        if L and i % 5 == 1:
            a[int(rng.integers(L))] = 2
        if L and i % 5 == 3:
            b[int(rng.integers(L))] = 2
        real.append(a)
        decoy.append(b)
    return real, decoy


def csr_labels(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.array([l for s in seqs for l in s], np.uint32), off


def lattice_front(tag):
    rng = np.random.default_rng(2027)
    lat = F.compose_frozen_batch(tag, *SY.to_labels(SY.utterances(rng, 96, 4, 12)))
    assert np.all(lat.status == OK)
    fsts = [lat.item(i) for i in range(96)] + [random_item(rng, 1, 40, 0.08) for _ in range(60)]
    return fsts, F.LhsBatch.from_fsts(fsts)


def decoy_of_lhs(lhs: F.LhsBatch) -> F.LhsBatch:
    """The same state_offsets, arc_offsets and nextstates; other weights, finals, olabels, starts."""
    ns = np.diff(lhs.state_offsets.astype(np.int64))
    start = lhs.start.copy()
    for i in range(len(start)):
        if i % 3 == 0 and ns[i] > 1 and start[i] != F.FST_NO_STATE:
            start[i] = (int(start[i]) + 1) % int(ns[i])
    w = np.where(np.isfinite(lhs.weights), np.abs(lhs.weights) * 0.5 + 0.25, lhs.weights)
    fin = np.where(np.isfinite(lhs.final_weights), lhs.final_weights + 1.25, lhs.final_weights)
    ol = np.where(lhs.olabels != 0, (lhs.olabels * 7 + 3) % 200 + 1, 0).astype(np.uint32)
    return F.LhsBatch(lhs.state_offsets, start, fin, lhs.arc_offsets, lhs.ilabels, ol, w,
                      lhs.nextstates)


LHS_LATE = ("start", "final_weights", "olabels", "weights")


# ---- one entry, one case ---------------------------------------------------------------------------

class Case:
    """One call of one entry: `lates` its late inputs, `outs` its device outputs, call(stream) ->
    the host outputs, `sync` what the header says about the entry, canon(arrays) what is compared."""

    def __init__(self, name, lates, outs, call, sync, engine=None, canon=canon_bytes, env=None):
        self.name, self.lates, self.outs, self.call, self.sync = name, lates, outs, call, sync
        self.engine, self.canon, self.env = engine, canon, env or {}
        self.want = self.decoy = None
        self.warm_ms = 0.0

    def on_null_stream(self, which):
        for l in self.lates:
            l.load(which)
        prefill(self.outs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hostout = self.call(None)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        eng = F.last_launch_stats().engine if self.engine is not None else None
        return (self.canon(host(self.outs)), hostout, eng), ms

    def reference(self):
        with environ(self.env):
            self.on_null_stream("real")
            self.want, self.warm_ms = self.on_null_stream("real")
            self.decoy, _ = self.on_null_stream("decoy")
        if self.engine is not None and self.engine >= 0:      # (-1: compared, whatever it is)
            assert self.want[2] == self.engine, (self.name, self.want[2])

    def late(self, W, call_stream=None):
        """The late-input sequence on W.S; the entry gets call_stream (default W.S)."""
        S, R = W.S, W.R
        for l in self.lates:
            l.load("decoy")
        prefill(self.outs)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            torch.cuda._sleep(W.cycles)
            for l in self.lates:
                l.load("real")
        use = call_stream or S
        hostout = self.call(use.cuda_stream)
        eng = F.last_launch_stats().engine if self.engine is not None else None
        if self.sync:
            with torch.cuda.stream(R):            # no wait on S: the entry said it had finished
                got = host(self.outs)
        else:
            with torch.cuda.stream(use):
                snap = [t.clone() for t in self.outs]
                prefill(self.outs)
            use.synchronize()
            got = host(snap)
        torch.cuda.synchronize()
        return self.canon(got), hostout, eng


class World:
    """Everything the module shares: streams, inputs, the cases with their null-stream results."""

    def __init__(self):
        torch.cuda.set_device(0)
        self.S, self.R = torch.cuda.Stream(), torch.cuda.Stream()
        assert self.S.cuda_stream != 0 and self.R.cuda_stream != 0
        assert self.S.cuda_stream != self.R.cuda_stream
        self.tag_blob, self.verb_blob = tagger_blob(), verbalizer_blob()
        self.amb_blob = O.freeze(O.gen("ambiguous", 64, 12))
        self.tag, self.verb = load_blob(self.tag_blob), load_blob(self.verb_blob)
        self.amb = load_blob(self.amb_blob)
        self.cases = {}
        self.cycles = 0
        self.build_text_cases()
        self.build_lattice_cases()
        for c in self.cases.values():
            c.reference()
        self.calibrate()

    def add(self, case):
        assert case.name not in self.cases
        self.cases[case.name] = case
        return case

    # -- chains in: labels and text ------------------------------------------------------------------

    def compose_case(self, name, rhs, real, decoy, sem):
        lab_r, off = csr_labels(real)
        lab_d, off_d = csr_labels(decoy)
        assert off.tobytes() == off_d.tobytes()
        num, max_len = len(real), int(np.diff(off.astype(np.int64)).max())
        d_off = dev_tensor(off)
        lab = Late([dev_tensor(lab_d)], [dev_tensor(lab_r)], [dev_tensor(lab_d)])
        out = DeviceOut(num, 16 * len(lab_r) + 1024)
        opts = opts_of(sem)

        def call(stream):
            rc = F.lib().fst_device_compose_shortest_path(
                rhs.h, P(lab.buf[0]), P(d_off), num, max_len, 1, C.byref(opts), C.byref(out.desc),
                SP(stream))
            assert rc == FF.FST_OK
            return ()
        c = Case(name, [lab], paths_tensors(out), call, sync=False, engine=-1,
                 canon=lambda a: canon_paths(a, num, out.cap))
        c.num, c.out, c.labels, c.offsets, c.lab, c.d_off = num, out, lab_r, off, lab, d_off
        c.max_len = max_len
        return c

    def build_text_cases(self):
        L = F.lib()
        texts, decoy = text_front()
        self.texts, self.decoy_texts = texts, decoy
        num = len(texts)
        data, off = FF.text_csr([t.encode() for t in texts])
        data_d, _ = FF.text_csr([t.encode() for t in decoy])
        nbytes = len(data)
        self.text_off = off
        d_off = dev_tensor(off)
        # fst_device_compile_text
        txt = Late([dev_tensor(data_d.copy())], [dev_tensor(data.copy())], [dev_tensor(data_d.copy())])
        labels = torch.zeros(nbytes + 16, dtype=torch.int32, device="cuda:0")

        def compile_text(stream):
            assert L.fst_device_compile_text(P(txt.buf[0]), P(d_off), num, P(labels),
                                             SP(stream)) == FF.FST_OK
            return ()
        self.add(Case("compile_text", [txt], [labels], compile_text, sync=False))
        # fst_device_compose_shortest_path: both rhs, both semantics
        lab_real = [[ord(ch) + 1 for ch in t] for t in texts]
        lab_decoy = [[ord(ch) + 1 for ch in t] for t in decoy]
        amb_real, amb_decoy = label_front()
        for sem, sname in ((LAZY, "lazy"), (EAGER, "eager")):
            c = self.add(self.compose_case(f"compose_shortest_path-tagger-{sname}", self.tag,
                                           lab_real, lab_decoy, sem))
            c.blob, c.sem = self.tag_blob, sem
            c = self.add(self.compose_case(f"compose_shortest_path-ambiguous-{sname}", self.amb,
                                           amb_real, amb_decoy, sem))
            c.blob, c.sem = self.amb_blob, sem
        # two finished stages as inputs: the tagger's paths of the real and of the decoy texts, the
        # real one with an output label that is no byte
        base = self.cases["compose_shortest_path-tagger-lazy"]
        stages = {}
        for which in ("real", "decoy"):
            base.lab.load(which)
            o = DeviceOut(num, base.out.cap)
            prefill(paths_tensors(o))
            opts = opts_of(LAZY)
            assert L.fst_device_compose_shortest_path(
                self.tag.h, P(base.lab.buf[0]), P(base.d_off), num, base.max_len, 1,
                C.byref(opts), C.byref(o.desc), None) == FF.FST_OK
            torch.cuda.synchronize()
            stages[which] = o
        st, ln, po = (t.cpu().numpy() for t in (stages["real"].status, stages["real"].plen,
                                                stages["real"].poff))
        k = next(i for i in range(num) if st[i] == OK and ln[i] >= 3)
        stages["real"].ol[int(po[k]) + 1] = 300
        self.non_byte = k
        cap = base.out.cap
        stage = DeviceOut(num, cap)
        stage_late = Late(paths_tensors(stage), paths_tensors(stages["real"]),
                          paths_tensors(stages["decoy"]))
        # fst_device_project_output
        nlab = torch.zeros(cap + num, dtype=torch.int32, device="cuda:0")
        noff = torch.zeros(num + 1, dtype=torch.int64, device="cuda:0")
        pst = torch.zeros(num, dtype=torch.int32, device="cuda:0")

        def project(stream):
            ml = C.c_uint32(WRONG)
            assert L.fst_device_project_output(C.byref(stage.desc), num, P(nlab), P(noff), P(pst),
                                               C.byref(ml), SP(stream)) == FF.FST_OK
            return (ml.value,)
        self.add(Case("project_output", [stage_late], [nlab, noff, pst], project, sync=True))
        # fst_device_emit_text
        text = torch.zeros(2 * cap, dtype=torch.uint8, device="cuda:0")
        toff = torch.zeros(num + 1, dtype=torch.int64, device="cuda:0")
        tst = torch.zeros(num, dtype=torch.int32, device="cuda:0")
        tw = torch.zeros(num, dtype=torch.float64, device="cuda:0")

        def emit(stream):
            tot = C.c_uint64(WRONG)
            assert L.fst_device_emit_text(C.byref(stage.desc), num, P(text), 2 * cap, P(toff), P(tst),
                                          P(tw), C.byref(tot), SP(stream)) == FF.FST_OK
            return (tot.value,)
        self.add(Case("emit_text", [stage_late], [text, toff, tst, tw], emit, sync=True))
        # fst_device_path_alignment at the text offsets of either stage
        offs = {}
        for which in ("real", "decoy"):
            stage_late.load(which)
            torch.cuda.synchronize()
            emit(None)
            torch.cuda.synchronize()
            offs[which] = toff.clone()
        aoff = torch.zeros(num + 1, dtype=torch.int64, device="cuda:0")
        aoff_late = Late([aoff], [offs["real"]], [offs["decoy"]])
        mcap = 2 * cap
        mb = torch.zeros(mcap + 16, dtype=torch.int32, device="cuda:0")
        me = torch.zeros(mcap + 16, dtype=torch.int32, device="cuda:0")
        cons = torch.zeros(num, dtype=torch.int32, device="cuda:0")

        def path_alignment(stream):
            assert L.fst_device_path_alignment(C.byref(stage.desc), num, P(aoff), P(mb), P(me), mcap,
                                               P(cons), SP(stream)) == FF.FST_OK
            return ()
        self.add(Case("path_alignment", [stage_late, aoff_late], [mb, me, cons], path_alignment,
                      sync=False))
        # fst_device_compose_alignment: the seven inputs of the last step of the two-stage chain
        self.chain_bufs = ChainBufs(num, nbytes)
        sets = {}
        for which, tx in (("real", data), ("decoy", data_d)):
            cb = self.chain_bufs
            cb.quiet()
            cb.text_in[:nbytes].copy_(dev_tensor(tx.copy()))
            cb.off_in.copy_(d_off)
            torch.cuda.synchronize()
            chain_a(cb, self.tag, self.verb, LAZY, None, last=False)
            torch.cuda.synchronize()
            sets[which] = [t.clone() for t in (cb.toff, cb.b, cb.e, cb.off2, cb.B, cb.E, cb.n1)]
        ins = [t.clone() for t in sets["decoy"]]
        ca_late = Late(ins, sets["real"], sets["decoy"])
        ob, oe = torch.zeros_like(ins[1]), torch.zeros_like(ins[2])
        tcap = self.chain_bufs.tcap

        def compose_alignment(stream):
            assert L.fst_device_compose_alignment(num, P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]),
                                                  P(ins[4]), P(ins[5]), P(ins[6]), P(ob), P(oe),
                                                  tcap, SP(stream)) == FF.FST_OK
            return ()
        self.add(Case("compose_alignment", [ca_late], [ob, oe], compose_alignment, sync=False))
        # fst_device_compose_frozen, with and without the trim
        lab = base.lab
        host_lat = F.compose_frozen_batch(self.tag, base.labels, base.offsets)
        ns, na = int(host_lat.state_offsets[-1]), int(host_lat.arc_offsets[-1])
        lat_d = F.compose_frozen_batch(self.tag, *csr_labels(lab_decoy))
        scap = max(ns, int(lat_d.state_offsets[-1])) + 64
        acap = max(na, int(lat_d.arc_offsets[-1])) + 64
        for flags, fname in ((0, "plain"), (FF.FST_LATTICE_CONNECT, "connect")):
            out = DeviceLattices(num, scap, acap)
            opts = opts_of()

            def compose_frozen(stream, out=out, flags=flags, opts=opts):
                needed = (C.c_uint64 * 2)(WRONG, WRONG)
                assert L.fst_device_compose_frozen(
                    self.tag.h, P(lab.buf[0]), P(base.d_off), num, base.max_len, flags,
                    C.byref(opts), C.byref(out.desc), needed, SP(stream)) == FF.FST_OK
                return (int(needed[0]), int(needed[1]))
            c = self.add(Case(f"compose_frozen-{fname}", [lab], lattice_tensors(out), compose_frozen,
                              sync=True, engine=10))
            c.out = out

    # -- lattices in ---------------------------------------------------------------------------------

    def build_lattice_cases(self):
        L = F.lib()
        self.fsts, self.lhs = lattice_front(self.tag)
        lhs, dlhs = self.lhs, decoy_of_lhs(self.lhs)
        num = len(lhs)
        ns, na = len(lhs.final_weights), len(lhs.weights)
        d, real = DeviceLhs(dlhs), DeviceLhs(lhs)
        self.dlhs, self.real_lhs = d, real
        late = Late([d.t[k] for k in LHS_LATE], [real.t[k] for k in LHS_LATE],
                    [d.t[k].clone() for k in LHS_LATE])
        self.lhs_late = late
        opts = opts_of()

        def paths_case(name, fn, per, cap, engine, env=None, sem=None):
            out = DeviceOut(num * per, cap)
            o = opts_of(sem) if sem is not None else opts

            def call(stream):
                assert fn(o, out, stream) == FF.FST_OK
                return ()
            c = self.add(Case(name, [late], paths_tensors(out), call, sync=True, engine=engine,
                              canon=lambda a: canon_paths(a, num * per, cap), env=env))
            c.out = out
            return c

        for sem, sname, eng in ((LAZY, "lazy", 8), (EAGER, "eager", 9)):
            paths_case(f"compose_shortest_path_lhs-{sname}",
                       lambda o, out, s: L.fst_device_compose_shortest_path_lhs(
                           self.verb.h, C.byref(d.cs), 1, C.byref(o), C.byref(out.desc), SP(s)),
                       1, 16 * na + 1024, eng, sem=sem)
        paths_case("shortest_path_lhs",
                   lambda o, out, s: L.fst_device_shortest_path_lhs(
                       C.byref(d.cs), 1, C.byref(o), C.byref(out.desc), SP(s)), 1, ns + 64, 12)
        for tier, env in (("default", None), ("workspace", TIER_ENV)):
            paths_case(f"nbest_lhs-{tier}",
                       lambda o, out, s: L.fst_device_nbest_lhs(
                           C.byref(d.cs), NBEST, C.byref(o), C.byref(out.desc), SP(s)),
                       NBEST, NBEST * ns + 64, 13, env)
            paths_case(f"nbest_unique_lhs-{tier}",
                       lambda o, out, s: L.fst_device_nbest_unique_lhs(
                           C.byref(d.cs), NBEST, C.byref(o), C.byref(out.desc), SP(s)),
                       NBEST, NBEST * ns + 64, 14, env)
            pruned = DeviceLattices(num, ns + 64, na + 64)

            def prune(stream, pruned=pruned):
                needed = (C.c_uint64 * 2)(WRONG, WRONG)
                assert L.fst_device_prune_lhs(C.byref(d.cs), BEAM, C.byref(opts),
                                              C.byref(pruned.desc), needed,
                                              SP(stream)) == FF.FST_OK
                return (int(needed[0]), int(needed[1]))
            self.add(Case(f"prune_lhs-{tier}", [late], lattice_tensors(pruned), prune, sync=True,
                          engine=15, env=env))
            for with_ab in (True, False):
                post = DevicePost(num, ns, na, with_ab=with_ab)

                def posterior(stream, post=post):
                    assert L.fst_device_posterior_lhs(C.byref(d.cs), C.byref(opts),
                                                      C.byref(post.desc), SP(stream)) == FF.FST_OK
                    return ()
                c = self.add(Case(f"posterior_lhs-{'ab' if with_ab else 'null'}-{tier}", [late],
                                  post_tensors(post), posterior, sync=True, engine=16, env=env))
                c.post = post

    # -- the delay -----------------------------------------------------------------------------------

    def time_sleep(self, cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.S):
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
        self.S.synchronize()
        return a.elapsed_time(b)

    def calibrate(self):
        """The sleep is at least 10 times the warm wall time of the slowest entry and at least
        5 ms: the host gets through all of a call's launches while the inputs are the decoy."""
        self.time_sleep(1000)
        probe = 2_000_000
        per_ms = probe / max(self.time_sleep(probe), 1e-3)
        slowest = max(self.cases.values(), key=lambda c: c.warm_ms)
        target = max(5.0, 10.0 * slowest.warm_ms)
        self.cycles = int(1.3 * target * per_ms)
        self.sleep_ms = min(self.time_sleep(self.cycles) for _ in range(3))
        self.short_cycles = max(int(0.5 * per_ms), 1)
        rec = {"what": "the delay in front of the late inputs (tests/test_gpu_device_streams.py): "
                       "torch.cuda._sleep(cycles) timed with events on the caller's stream, against "
                       "the warm null-stream wall time of the slowest entry at the test shapes",
               "cycles": self.cycles, "sleep_ms": float("%.4g" % self.sleep_ms),
               "slowest_entry": slowest.name, "slowest_entry_ms": float("%.4g" % slowest.warm_ms),
               "entry_ms": {c.name: float("%.4g" % c.warm_ms) for c in self.cases.values()}}
        print("calibration:", json.dumps(rec, sort_keys=True))
        path = os.path.join(REPO, "profiles", "device_streams", "calibration.json")
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(rec, fh, indent=1, sort_keys=True)
                fh.write("\n")
        except OSError:
            pass
        self.slowest = slowest


# ---- the aligned two-stage text chain of INTEGRATION.md --------------------------------------------

class ChainBufs:
    """Every buffer of compile_text -> compose -> project_output -> path_alignment -> compose ->
    emit_text -> path_alignment -> compose_alignment for `num` strings of `nbytes` bytes."""

    def __init__(self, num, nbytes):
        dev = "cuda:0"
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
        self.num, self.nbytes = num, nbytes
        self.text_in, self.off_in = z(nbytes + 16, torch.uint8), z(num + 1, torch.int64)
        self.lab1 = z(nbytes + 16, torch.int32)
        cap1 = 4 * nbytes + 4 * num + 64                  # the tagger: at most two arcs per byte
        self.s1 = DeviceOut(num, cap1)
        self.lab2, self.off2 = z(cap1 + num, torch.int32), z(num + 1, torch.int64)
        self.pst = z(num, torch.int32)
        self.mcap = cap1 + num + 64
        self.B, self.E, self.n1 = z(self.mcap, torch.int32), z(self.mcap, torch.int32), \
            z(num, torch.int32)
        self.s2 = DeviceOut(num, 8 * (cap1 + num) + 64)   # the verbalizer: a word per "#x"
        self.tcap = self.s2.cap
        self.text, self.toff = z(self.tcap, torch.uint8), z(num + 1, torch.int64)
        self.tst, self.tw = z(num, torch.int32), z(num, torch.float64)
        self.b, self.e, self.n2 = z(self.tcap, torch.int32), z(self.tcap, torch.int32), \
            z(num, torch.int32)
        self.max_len, self.total = C.c_uint32(WRONG), C.c_uint64(WRONG)

    def quiet(self):
        """Pre-fill everything a stage writes.  What a later stage reads as an offset, a length
        or an index is 0 and every status is not OK, so a stage that ran early stays in bounds."""
        prefill([self.lab1, self.lab2, self.pst, self.B, self.E, self.text, self.tst, self.tw,
                 self.n2])
        for t in (self.off2, self.n1, self.toff, self.b, self.e):
            t.zero_()
        quiet_paths(self.s1)
        quiet_paths(self.s2)
        self.max_len.value = self.total.value = WRONG

    def outputs(self):
        return [self.text, self.toff, self.tst, self.tw, self.b, self.e]


def chain_a(cb: ChainBufs, rhs1, rhs2, sem, stream, last=True):
    L, num, s = F.lib(), cb.num, SP(stream)
    opts = opts_of(sem)
    ok = FF.FST_OK
    assert L.fst_device_compile_text(P(cb.text_in), P(cb.off_in), num, P(cb.lab1), s) == ok
    assert L.fst_device_compose_shortest_path(rhs1.h, P(cb.lab1), P(cb.off_in), num, 40, 1,
                                              C.byref(opts), C.byref(cb.s1.desc), s) == ok
    assert L.fst_device_project_output(C.byref(cb.s1.desc), num, P(cb.lab2), P(cb.off2), P(cb.pst),
                                       C.byref(cb.max_len), s) == ok
    assert L.fst_device_path_alignment(C.byref(cb.s1.desc), num, P(cb.off2), P(cb.B), P(cb.E),
                                       cb.mcap, P(cb.n1), s) == ok
    assert L.fst_device_compose_shortest_path(rhs2.h, P(cb.lab2), P(cb.off2), num,
                                              cb.max_len.value, 1, C.byref(opts),
                                              C.byref(cb.s2.desc), s) == ok
    assert L.fst_device_emit_text(C.byref(cb.s2.desc), num, P(cb.text), cb.tcap, P(cb.toff),
                                  P(cb.tst), P(cb.tw), C.byref(cb.total), s) == ok
    assert L.fst_device_path_alignment(C.byref(cb.s2.desc), num, P(cb.toff), P(cb.b), P(cb.e),
                                       cb.tcap, P(cb.n2), s) == ok
    if last:
        assert L.fst_device_compose_alignment(num, P(cb.toff), P(cb.b), P(cb.e), P(cb.off2),
                                              P(cb.B), P(cb.E), P(cb.n1), P(cb.b), P(cb.e),
                                              cb.tcap, s) == ok


def assert_chain_a(got, total, want, what):
    """The chain's snapshot [text, toff, tst, tw, b, e] against the host entry's aligned result."""
    text, toff, tst, tw, b, e = got
    assert total == int(want.offsets[-1]), what
    assert tst.tobytes() == want.status.tobytes(), what
    assert toff.view(np.uint64).tobytes() == want.offsets.tobytes(), what
    assert text[:total].tobytes() == want.text.tobytes(), what
    assert tw.tobytes() == want.total_weight.tobytes(), what
    assert b[:total].view(np.uint32).tobytes() == want.in_begin.tobytes(), what
    assert e[:total].view(np.uint32).tobytes() == want.in_end.tobytes(), what


def chain_a_on_stream(cb, rhs1, rhs2, stream, cycles, data_decoy, data_real, off):
    """One iteration on `stream`: buffers pre-filled, decoy text, a sleep, the real text, the chain,
    a snapshot -- all in stream order, no host wait but the entries' own.  Returns the snapshot."""
    with torch.cuda.stream(stream):
        cb.quiet()
        cb.off_in.copy_(off)
        cb.text_in[:cb.nbytes].copy_(data_decoy)
        torch.cuda._sleep(cycles)
        cb.text_in[:cb.nbytes].copy_(data_real)
    chain_a(cb, rhs1, rhs2, LAZY, stream.cuda_stream)
    with torch.cuda.stream(stream):
        snap = [t.clone() for t in cb.outputs()]
    stream.synchronize()
    with torch.cuda.stream(stream):
        return host(snap), int(cb.total.value)


def two_streams(stages, batches, cycles, iterations=20, extra=None):
    """Two threads, each with its own stream, buffers and batch, run chain (a) `iterations` times
    and compare every iteration with the host entry's bytes; `extra` is a third thread's body."""
    tag, verb = stages
    jobs = []
    for texts, decoy in batches:
        data, off = FF.text_csr([t.encode() for t in texts])
        data_d, _ = FF.text_csr([t.encode() for t in decoy])
        want = F.normalize_text_aligned_batch([tag, verb], [t.encode() for t in texts], LAZY)
        jobs.append((ChainBufs(len(texts), len(data)), dev_tensor(data_d.copy()),
                     dev_tensor(data.copy()), dev_tensor(off), want, torch.cuda.Stream()))
    torch.cuda.synchronize()
    assert jobs[0][5].cuda_stream != jobs[1][5].cuda_stream != 0

    def work(t):
        torch.cuda.set_device(0)
        if t == 2:
            return extra()
        cb, dd, dr, off, want, stream = jobs[t]
        for it in range(iterations):
            got, total = chain_a_on_stream(cb, tag, verb, stream, cycles, dd, dr, off)
            assert_chain_a(got, total, want, (t, it))
    run_threads(3 if extra else 2, work)
    torch.cuda.synchronize()


def thread_batches():
    out = []
    for seed in (31, 32):
        rng = np.random.default_rng(seed)
        texts = SY.utterances(rng, 64, 0, 40) + ["", "7", "a#"]
        decoy = [SY.utterances(rng, 1, len(t), len(t))[0] for t in texts]
        out.append((texts, decoy))
    return out


def one_engine_main():
    """Case 6, run in a child process with FSTAMD_ENGINES=1: every lease passes between the two
    caller streams and the engine's own stream (a third thread's host-entry calls)."""
    torch.cuda.set_device(0)
    tag, verb = load_blob(tagger_blob()), load_blob(verbalizer_blob())
    amb_blob = O.freeze(O.gen("ambiguous", 64, 12))
    amb = load_blob(amb_blob)
    labels, offsets = csr_labels(label_front()[0])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    a.record()
    torch.cuda._sleep(2_000_000)
    b.record()
    torch.cuda.synchronize()
    cycles = max(int(0.5 * 2_000_000 / max(a.elapsed_time(b), 1e-3)), 1)

    def host_calls():
        for it in range(10):
            check_host_against_oracle(amb_blob, labels, offsets, (LAZY, EAGER)[it % 2], rhs=amb)
    two_streams((tag, verb), thread_batches(), cycles, extra=host_calls)
    print("one engine: ok")


# ---- fixtures --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def W():
    w = World()
    yield w
    torch.cuda.synchronize()


def entry_names():
    names = ["compile_text"]
    for rhs in ("tagger", "ambiguous"):
        names += [f"compose_shortest_path-{rhs}-{s}" for s in ("lazy", "eager")]
    names += ["project_output", "emit_text", "path_alignment", "compose_alignment",
              "compose_frozen-plain", "compose_frozen-connect",
              "compose_shortest_path_lhs-lazy", "compose_shortest_path_lhs-eager",
              "shortest_path_lhs"]
    for tier in ("default", "workspace"):
        names += [f"nbest_lhs-{tier}", f"nbest_unique_lhs-{tier}", f"prune_lhs-{tier}",
                  f"posterior_lhs-ab-{tier}", f"posterior_lhs-null-{tier}"]
    return names


# ---- 0. the harness itself -------------------------------------------------------------------------

def test_the_delay_is_long_enough(W):
    """The calibration (profiles/device_streams/calibration.json): asserted, not skipped."""
    assert set(W.cases) == set(entry_names())
    assert W.sleep_ms >= 5.0 and W.sleep_ms >= 10.0 * W.slowest.warm_ms, \
        (W.sleep_ms, W.slowest.name, W.slowest.warm_ms)
    assert W.sleep_ms < 50.0, W.sleep_ms


@pytest.mark.parametrize("name", entry_names())
def test_the_decoy_differs(W, name):
    """Teeth: the decoy's null-stream result differs from the real one, so the comparisons below
    can tell a call that read its inputs early."""
    c = W.cases[name]
    assert c.decoy[0] != c.want[0], name


def test_control_a_call_on_another_stream_sees_the_decoy(W):
    """The harness sees a call that is not ordered behind S: the entry gets R while the real
    inputs arrive on S behind the sleep, and answers for the decoy (same topology: in bounds)."""
    c = W.cases["shortest_path_lhs"]
    got = c.late(W, call_stream=W.R)
    assert got == c.decoy and got != c.want


# ---- 1. each entry alone ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", entry_names())
def test_entry_with_late_inputs(W, name, monkeypatch):
    c = W.cases[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    got = c.late(W)
    assert got[1] == c.want[1], (name, "host outputs", got[1], c.want[1])
    assert got[2] == c.want[2], (name, "engine", got[2], c.want[2])
    assert got[0] == c.want[0], name
    assert WRONG not in got[1]


@pytest.mark.parametrize("name", [f"compose_shortest_path-{r}-{s}" for r in ("tagger", "ambiguous")
                                  for s in ("lazy", "eager")])
def test_compose_shortest_path_against_the_oracle(W, name):
    c = W.cases[name]
    got = c.late(W)[0]
    ref = O.batch_run(c.blob, c.labels, c.offsets, 0 if c.sem == LAZY else 1, 1)
    exp = expected_status(ref)
    assert [e[0] for e in got[1]] == exp.tolist()
    assert {OK, EMPTY} <= set(exp.tolist())
    for i, e in enumerate(got[1]):
        if e[0] != OK:
            continue
        a0, a1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert e[1:] == (ref.ilabels[a0:a1].tobytes(), ref.olabels[a0:a1].tobytes(),
                         ref.weights[a0:a1].tobytes(), ref.finals[i:i + 1].tobytes()), (name, i)


def test_compose_frozen_against_the_oracle(W):
    c = W.cases["compose_frozen-plain"]
    got, needed, _ = c.late(W)
    base = W.cases["compose_shortest_path-tagger-lazy"]
    names = ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
             "olabels", "weights", "nextstates")
    dts = (np.int32, np.uint64, np.uint32, np.float64, np.uint64, np.uint32, np.uint32, np.float64,
           np.uint32)
    lat = types.SimpleNamespace(**{n: np.frombuffer(b, dt) for n, b, dt in zip(names, got, dts)})
    off = base.offsets.astype(np.int64)
    ns = na = 0
    for i in range(base.num):
        seq = base.labels[off[i]:off[i + 1]].tolist()
        item = oracle(chain_fst(seq), W.tag_blob)
        assert_item(lat, i, item)
        ns, na = ns + len(item.finals), na + len(item.arcs)
    assert needed == (ns, na)


def test_posterior_against_the_model(W):
    c = W.cases["posterior_lhs-ab-default"]
    got = c.late(W)[0]
    arrs = {"status": np.frombuffer(got[0], np.int32),
            **{k: np.frombuffer(b, np.float64) for k, b in zip(("total", "alpha", "beta", "arc_cost"),
                                                               got[1:])}}
    model = PM.posterior_batch(W.fsts)
    assert {OK, EMPTY} <= {m[0] for m in model}
    try:
        compare("device-streams", W.fsts, W.lhs, arrs, model, tier="S")
    finally:
        RATIOS.pop("device-streams[S]", None)     # (that module's own record stays its own)


# ---- 2. first use on the caller's stream -----------------------------------------------------------

def test_first_call_of_a_fresh_rhs_handle(W):
    """The handle's device copy and mirror are built on the null stream in the middle of the call."""
    base = W.cases["compose_shortest_path-tagger-eager"]
    fresh = load_blob(W.tag_blob)
    assert fresh.h != W.tag.h
    opts = opts_of(EAGER)

    def call(stream):
        assert F.lib().fst_device_compose_shortest_path(
            fresh.h, P(base.lab.buf[0]), P(base.d_off), base.num, base.max_len, 1, C.byref(opts),
            C.byref(base.out.desc), SP(stream)) == FF.FST_OK
        return ()
    c = Case("fresh-rhs", base.lates, base.outs, call, sync=False, engine=-1, canon=base.canon)
    got = c.late(W)
    assert got == base.want


def test_first_call_that_regrows_the_workspaces(W):
    """A batch larger than any this module ran before: scratch() frees and allocates while the
    sleep is still queued on S.  The expected result is computed afterwards, and checked against
    the oracle."""
    rng = np.random.default_rng(77)
    real = [[1] * int(rng.integers(0, 65)) for _ in range(1536)]
    decoy = [list(s) for s in real]
    for i in range(0, len(real), 3):
        if real[i]:
            decoy[i][len(decoy[i]) // 2] = 2
    c = W.compose_case("regrow", W.amb, real, decoy, EAGER)
    got = c.late(W)
    c.reference()
    assert got == c.want and c.decoy[0] != c.want[0]
    ref = O.batch_run(W.amb_blob, c.labels, c.offsets, 1, 1)
    assert [e[0] for e in got[0][1]] == expected_status(ref).tolist()
    for i, e in enumerate(got[0][1]):
        a0, a1 = int(ref.offsets[i]), int(ref.offsets[i + 1])
        assert e[0] == OK and e[2] == ref.olabels[a0:a1].tobytes(), i


# ---- 3. the early returns of run_chain -------------------------------------------------------------

def early_return(W, first_call):
    """first_call(stream) returns early with work queued; at once a compose on S (late inputs)
    and a shortest path on R follow on the same engine.  Returns (compose on S, shortest path)."""
    second, third = W.cases["compose_shortest_path-tagger-lazy"], W.cases["shortest_path_lhs"]
    S, R = W.S, W.R
    for l in second.lates:
        l.load("decoy")
    W.lhs_late.load("real")
    prefill(second.outs + third.outs)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(W.cycles)
        for l in second.lates:
            l.load("real")
    snap0 = first_call(S)
    second.call(S.cuda_stream)
    third.call(R.cuda_stream)
    with torch.cuda.stream(R):
        got3 = third.canon(host(third.outs))
    with torch.cuda.stream(S):
        snap = [t.clone() for t in second.outs]
        first = [t.clone() for t in snap0]
    S.synchronize()
    got2 = second.canon(host(snap))
    first = host(first)
    torch.cuda.synchronize()
    assert got2 == second.want[0]
    assert got3 == third.want[0]
    return first


def test_early_return_of_an_empty_batch(W):
    base = W.cases["compose_shortest_path-tagger-lazy"]
    out = DeviceOut(0, 64)
    prefill(paths_tensors(out))
    opts = opts_of(LAZY)

    def first(S):
        assert F.lib().fst_device_compose_shortest_path(
            W.tag.h, P(base.lab.buf[0]), P(base.d_off), 0, 0, 1, C.byref(opts), C.byref(out.desc),
            SP(S.cuda_stream)) == FF.FST_OK
        return [out.cur, out.status]
    cur, status = early_return(W, first)
    assert int(cur.view(np.uint64)[0]) == 0          # as seen from S
    assert int(status[0]) == SENT32                   # nothing else was written


def test_early_return_of_the_nan_route(W):
    """An rhs with a NaN weight, eager: run_chain marks the statuses and returns with the kernel
    queued behind the sleep."""
    nan_rhs = O.Fst(start=0, finals=[0.0], arcs=[[(2, 2, 0.5, 0), (3, 3, float("nan"), 0)]])
    rhs = load_blob(O.freeze(nan_rhs))
    base = W.cases["compose_shortest_path-tagger-lazy"]
    out = DeviceOut(base.num, 64)
    opts = opts_of(EAGER)

    def call(stream):
        assert F.lib().fst_device_compose_shortest_path(
            rhs.h, P(base.lab.buf[0]), P(base.d_off), base.num, base.max_len, 1, C.byref(opts),
            C.byref(out.desc), SP(stream)) == FF.FST_OK
    prefill(paths_tensors(out))
    torch.cuda.synchronize()
    call(None)
    torch.cuda.synchronize()
    want = host([out.status, out.cur])
    assert set(want[0].tolist()) == {UNSUPPORTED}
    prefill(paths_tensors(out))

    def first(S):
        call(S.cuda_stream)
        return [out.status, out.cur]
    got = early_return(W, first)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- 4. the documented chains, end to end on S -----------------------------------------------------

def test_chain_text_to_aligned_text(W):
    """INTEGRATION.md's aligned two-stage chain with one sleep and late text at its head."""
    cb = W.chain_bufs
    texts = [t.encode() for t in W.texts]
    data, off = FF.text_csr(texts)
    data_d, _ = FF.text_csr([t.encode() for t in W.decoy_texts])
    d_real, d_decoy, d_off = dev_tensor(data.copy()), dev_tensor(data_d.copy()), dev_tensor(off)
    want = F.normalize_text_aligned_batch([W.tag, W.verb], texts, LAZY)
    assert {OK, EMPTY} <= set(want.status.tolist())
    # the same chain on the null stream: byte for byte, padding included
    cb.quiet()
    cb.off_in.copy_(d_off)
    cb.text_in[:cb.nbytes].copy_(d_real)
    torch.cuda.synchronize()
    chain_a(cb, W.tag, W.verb, LAZY, None)
    torch.cuda.synchronize()
    null, null_total = host(cb.outputs()), int(cb.total.value)
    assert_chain_a(null, null_total, want, "null stream")
    torch.cuda.synchronize()
    got, total = chain_a_on_stream(cb, W.tag, W.verb, W.S, W.cycles, d_decoy, d_real, d_off)
    assert_chain_a(got, total, want, "S")
    assert total == null_total and canon_bytes(got) == canon_bytes(null)
    # teeth: the decoy's text is another
    other = F.normalize_text_aligned_batch([W.tag, W.verb], [t.encode() for t in W.decoy_texts], LAZY)
    assert other.text.tobytes() != want.text.tobytes()


def test_chain_lattices_prune_posterior_nbest_text(W):
    """compose_frozen with connect -> prune -> posterior and unique n-best -> text on S: the first
    run of engine 15 into engine 16.  Expected: the host entries on the host's pruned batch."""
    L = F.lib()
    base = W.cases["compose_shortest_path-tagger-lazy"]
    num, S = base.num, W.S
    host_lat = F.compose_frozen_batch(W.tag, base.labels, base.offsets, connect=True)
    pruned = F.prune_lhs_batch(host_lat.as_lhs(), BEAM)
    plhs = pruned.as_lhs()
    ns1, na1 = int(host_lat.state_offsets[-1]), int(host_lat.arc_offsets[-1])
    ns2, na2 = int(pruned.state_offsets[-1]), int(pruned.arc_offsets[-1])
    assert 0 < ns2 <= ns1      # (on the tagger's lattices a beam of 0.5 keeps every state)
    want_post = F.posterior_lhs_batch(plhs)
    want_nb = F.nbest_unique_lhs_batch(plhs, NBEST)
    want_text = F.batch_result_to_text(want_nb)
    lat, cut = DeviceLattices(num, ns1, na1), DeviceLattices(num, ns2, na2)
    post = DevicePost(num, ns2, na2)
    paths = DeviceOut(num * NBEST, NBEST * ns2 + 64)
    tcap = 8 * NBEST * max(na2, 1) + 64
    text = torch.zeros(tcap, dtype=torch.uint8, device="cuda:0")
    toff = torch.zeros(num * NBEST + 1, dtype=torch.int64, device="cuda:0")
    tst = torch.zeros(num * NBEST, dtype=torch.int32, device="cuda:0")
    tw = torch.zeros(num * NBEST, dtype=torch.float64, device="cuda:0")
    opts = opts_of()
    for l in base.lates:
        l.load("decoy")
    quiet_lattices(lat)
    quiet_lattices(cut)
    quiet_paths(paths)
    prefill(post_tensors(post) + [text, tst, tw])
    toff.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(W.cycles)
        for l in base.lates:
            l.load("real")
    s = SP(S.cuda_stream)
    need1, need2 = (C.c_uint64 * 2)(WRONG, WRONG), (C.c_uint64 * 2)(WRONG, WRONG)
    total = C.c_uint64(WRONG)
    assert L.fst_device_compose_frozen(W.tag.h, P(base.lab.buf[0]), P(base.d_off), num, base.max_len,
                                       FF.FST_LATTICE_CONNECT, C.byref(opts), C.byref(lat.desc),
                                       need1, s) == FF.FST_OK
    cs1 = lat.as_device_lhs()
    assert L.fst_device_prune_lhs(C.byref(cs1), BEAM, C.byref(opts), C.byref(cut.desc), need2,
                                  s) == FF.FST_OK
    assert F.last_launch_stats().engine == 15
    cs2 = cut.as_device_lhs()
    assert L.fst_device_posterior_lhs(C.byref(cs2), C.byref(opts), C.byref(post.desc),
                                      s) == FF.FST_OK
    assert F.last_launch_stats().engine == 16
    assert L.fst_device_nbest_unique_lhs(C.byref(cs2), NBEST, C.byref(opts), C.byref(paths.desc),
                                         s) == FF.FST_OK
    assert L.fst_device_emit_text(C.byref(paths.desc), num * NBEST, P(text), tcap, P(toff), P(tst),
                                  P(tw), C.byref(total), s) == FF.FST_OK
    with torch.cuda.stream(W.R):                       # every entry of this chain synchronises
        g_cut = cut.arrays(ns2, na2)
        g_post = post.arrays()
        g_text, g_toff, g_tst, g_tw = host([text, toff, tst, tw])
    torch.cuda.synchronize()
    assert (need1[0], need1[1]) == (ns1, na1) and (need2[0], need2[1]) == (ns2, na2)
    for name in ("status", "state_offsets", "start", "final_weights", "arc_offsets", "ilabels",
                 "olabels", "weights", "nextstates"):
        assert g_cut[name].tobytes() == getattr(pruned, name).tobytes(), name
    for name in ("status", "total", "alpha", "beta", "arc_cost"):
        assert g_post[name].tobytes() == getattr(want_post, name).tobytes(), name
    assert total.value == int(want_text.offsets[-1])
    assert g_tst.tobytes() == want_text.status.tobytes()
    assert g_toff.view(np.uint64).tobytes() == want_text.offsets.tobytes()
    assert g_text[:total.value].tobytes() == want_text.text.tobytes()
    assert g_tw.tobytes() == want_text.total_weight.tobytes()
    assert sum(x == OK for x in g_tst.tolist()) > num
    # the posteriors against the model on the pruned items
    fsts = [pruned.item(i) for i in range(num)]
    try:
        compare("device-streams-pruned", fsts, plhs, g_post, PM.posterior_batch(fsts), tier="S")
    finally:
        RATIOS.pop("device-streams-pruned[S]", None)
    # the null-stream helper of the shortest-path suite prints the same texts from these paths
    texts, status = emit_text(paths, num * NBEST, tcap)
    assert texts == want_text.texts() and status == want_text.status.tolist()
    torch.cuda.synchronize()


# ---- 5, 6. two caller streams ----------------------------------------------------------------------

def test_two_streams_two_threads(W):
    two_streams((W.tag, W.verb), thread_batches(), W.short_cycles)


def test_one_engine_hands_over_between_streams():
    """FSTAMD_ENGINES is read once per process: one child, no retry."""
    r = run_py("import test_gpu_device_streams as T; T.one_engine_main()", {"FSTAMD_ENGINES": "1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "one engine: ok" in r.stdout

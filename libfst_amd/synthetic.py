"""Synthetic stand-ins for config 4 (WeTextProcessing tagger -> verbalizer).

The real zh_tagger.fst / zh_verbalizer.fst are not available offline, so
bench and tests use two small byte-level transducers with the same shape of work: label =
byte + 1 (compileString, src/string.zig:24-50), epsilon-input arcs for multi-symbol
outputs (rhs epsilons), and an ambiguous choice resolved by weight.

  tagger      copies letters and spaces; a digit d is either copied (weight 1.0) or
              tagged as "#" + chr(ord('a') + d) (weight 0.5, via an epsilon-input arc);
  verbalizer  copies letters, spaces and digits; "#x" becomes the English word of digit
              x, written with an epsilon-input chain.

Builders return plain lists (num_states, start, finals, arcs per state as (il, ol, w,
next)); tests wrap them for the oracle, bench freezes them through the C ABI.
"""
INF = float("inf")
LETTERS = "abcdefghijklmnopqrstuvwxyz "
DIGITS = "0123456789"
WORDS = ["zero", "one", "two", "three", "four", "five", "six", "seven", "eight", "nine"]


def lab(ch: str) -> int:
    return ord(ch) + 1


class _Builder:
    def __init__(self):
        self.finals = []
        self.arcs = []

    def state(self, final=INF):
        self.finals.append(final)
        self.arcs.append([])
        return len(self.finals) - 1

    def arc(self, s, il, ol, w, nx):
        self.arcs[s].append((il, ol, float(w), nx))

    def lists(self):
        return len(self.finals), 0, list(self.finals), [list(a) for a in self.arcs]


def tagger():
    b = _Builder()
    s0 = b.state(0.0)
    for ch in LETTERS:
        b.arc(s0, lab(ch), lab(ch), 0.0, s0)
    for d, ch in enumerate(DIGITS):
        b.arc(s0, lab(ch), lab(ch), 1.0, s0)          # keep the digit
        mid = b.state()
        b.arc(s0, lab(ch), lab("#"), 0.5, mid)        # tag it ...
        b.arc(mid, 0, lab(chr(ord("a") + d)), 0.0, s0)  # ... as "#" + letter
    return b.lists()


def verbalizer():
    b = _Builder()
    s0 = b.state(0.0)
    for ch in LETTERS + DIGITS:
        b.arc(s0, lab(ch), lab(ch), 0.0, s0)
    hs = b.state()
    b.arc(s0, lab("#"), 0, 0.0, hs)
    for d, word in enumerate(WORDS):
        cur = b.state()
        b.arc(hs, lab(chr(ord("a") + d)), 0, 0.0, cur)
        for k, ch in enumerate(word):
            nxt = s0 if k == len(word) - 1 else b.state()
            b.arc(cur, 0, lab(ch), 0.0, nxt)
            cur = nxt
    return b.lists()


def utterances(rng, n, min_len=5, max_len=40):
    """Random texts of letters, spaces and digit runs (numpy Generator `rng`)."""
    alphabet = LETTERS + DIGITS * 2
    out = []
    for _ in range(n):
        L = int(rng.integers(min_len, max_len + 1))
        out.append("".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), L)))
    return out


def to_labels(texts):
    """CSR (labels u32, offsets u64) of compileString label sequences."""
    import numpy as np
    lens = [len(t) for t in texts]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    labels = np.fromiter((ord(c) + 1 for t in texts for c in t), dtype=np.uint32,
                         count=int(offsets[-1]))
    return labels, offsets


def to_mutable(spec):
    """A libfst_amd.MutableFst from builder lists (C ABI)."""
    from .fst import MutableFst
    ns, start, finals, arcs = spec
    m = MutableFst()
    for _ in range(ns):
        m.add_state()
    m.set_start(start)
    for s, fw in enumerate(finals):
        if fw != INF:
            m.set_final(s, fw)
    for s, al in enumerate(arcs):
        for (il, ol, w, nx) in al:
            m.add_arc(s, il, ol, w, nx)
    return m


# ---- general lhs: what a recogniser emits instead of one string ------------------------
# Both return (start, finals, arcs per state), the item form of LhsBatch.from_fsts.

def confusion_network(rng, text, max_alts=3, skip_prob=0.1):
    """A confusion network ("sausage") over `text`: state k -> k + 1 per position, carrying
    the position's own byte and up to max_alts - 1 other alternatives as byte labels
    (byte + 1 on both tapes) with weights -log p (p a random distribution over the
    alternatives: non-dyadic), and with probability skip_prob an epsilon:epsilon skip arc.
    The last state is final with weight One."""
    import math
    alphabet = LETTERS + DIGITS
    L = len(text)
    finals = [INF] * L + [0.0]
    arcs = [[] for _ in range(L + 1)]
    for k, ch in enumerate(text):
        n_alt = int(rng.integers(1, max_alts + 1))
        alts = [ch]
        while len(alts) < n_alt:
            c = alphabet[int(rng.integers(0, len(alphabet)))]
            if c not in alts:
                alts.append(c)
        skip = bool(rng.random() < skip_prob)
        p = rng.random(len(alts) + (1 if skip else 0)) + 0.05
        p = p / p.sum()
        # (+ 0.0: a lone alternative has p = 1 and -log 1 is -0.0, which is not One; a negative
        # zero would also send the item down the library's negative-weight route)
        for c, pc in zip(alts, p):
            arcs[k].append((lab(c), lab(c), -math.log(float(pc)) + 0.0, k + 1))
        if skip:
            arcs[k].append((0, 0, -math.log(float(p[-1])) + 0.0, k + 1))
    return 0, finals, arcs


def edge_networks():
    """One small fixed batch for the lhs batch entries' host layer: 48 confusion networks of 3 to
    10 positions with up to 3 alternatives each, among them two with a negative weight (items 5
    and 17: the replay list), one with a NaN (9), one without states (13), one of one state (21)
    and one with a dead end (29: a state that reaches no final state, for connect)."""
    import numpy as np
    rng = np.random.default_rng(4848)
    fsts = [confusion_network(rng, t, 3, 0.1) for t in utterances(rng, 48, 3, 10)]
    for i, w in ((5, -0.5), (17, -0.5), (9, float("nan"))):
        il, ol, _, nx = fsts[i][2][1][0]
        fsts[i][2][1][0] = (il, ol, w, nx)
    fsts[13] = (None, [], [])
    fsts[21] = (0, [0.0], [[]])
    _, finals, arcs = fsts[29]
    arcs[0].append((lab("a"), lab("a"), 0.25, len(finals)))
    finals.append(INF)
    arcs.append([])
    return fsts


def nbest_union(rng, texts):
    """The union of n-best hypotheses as a prefix tree: one arc per byte (byte + 1 on both
    tapes) with a random per-arc cost, one final state per distinct hypothesis with a random
    final cost."""
    finals, arcs = [INF], [[]]
    child = [{}]
    for t in texts:
        s = 0
        for ch in t:
            nx = child[s].get(ch)
            if nx is None:
                nx = len(finals)
                finals.append(INF)
                arcs.append([])
                child.append({})
                child[s][ch] = nx
                arcs[s].append((lab(ch), lab(ch), float(rng.random()) * 2.0, nx))
            s = nx
        if finals[s] == INF:
            finals[s] = float(rng.random())
    return 0, finals, arcs


def respelled_union(rng, text, k):
    """An nbest_union of up to k hypotheses of `text` that differ in how its digits are written:
    the first is `text`, every other spells each digit as its WORDS entry with probability 1/2
    (equal hypotheses fall together).  After tagger -> verbalizer a kept digit can come out as
    its word too, so paths of different hypotheses print equal texts: the repeats that
    fst_nbest_unique_lhs_batch removes."""
    hyps = [text]
    for _ in range(k - 1):
        hyps.append("".join(WORDS[int(c)] if c in DIGITS and rng.random() < 0.5 else c
                            for c in text))
    return nbest_union(rng, hyps)

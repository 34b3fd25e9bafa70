"""Reference and helpers of the beam search tests (tests/test_beam_cpu.py, tests/test_gpu_beam.py): a plain-Python float64
beam search with exactly the rules include/ivl_hip.h states for ivl_beam_select_fwd / ivl_beam_commit_fwd, a brute-force
enumeration for it to be checked against, and the seeded synthetic cases of the select / commit tests."""
import itertools
import math
import random
import struct

NEG_INF = float("-inf")
TIE_REL = 2.0 ** -40         # two hypothesis scores this close (relative) may be ordered either way when pow() is involved


def hyp_score(s, n, lp):
    """sum / n^lp in float64: lp == 1 a plain division, lp == 0 the sum itself."""
    if lp == 0.0:
        return s
    if lp == 1.0:
        return s / float(n)
    return s / math.pow(float(n), lp)


def close(a, b):
    if a == b:
        return True
    if math.isinf(a) or math.isinf(b):
        return False
    return abs(a - b) <= TIE_REL * max(abs(a), abs(b))


class BeamGroup:
    """One group of B beams.  State: cum[B] (float, -inf = no beam), n_new[B], history[B] (token lists), token[B], the
    hypotheses (dicts tokens / score / sum, in insertion order) and done (0 running, 1 stopping rule, 2 budget).
    `contested`: a comparison of hypothesis scores that went through pow() came out within TIE_REL."""

    def __init__(self, B, length_penalty=1.0, early_stopping=False, budget=-1, stop_ids=()):
        self.B, self.lp, self.early, self.budget = B, float(length_penalty), bool(early_stopping), budget
        self.stop = [int(t) for t in stop_ids if t >= 0]
        self.cum = [0.0] + [NEG_INF] * (B - 1)
        self.n_new = [0] * B
        self.history = [[] for _ in range(B)]
        self.token = [0] * B
        self.hyps = []
        self.done = 0
        self.contested = False
        self.parent, self.next_token, self.next_score = list(range(B)), [0] * B, [NEG_INF] * B

    def _cmp(self, a, b):
        if self.lp not in (0.0, 1.0) and close(a, b):
            self.contested = True

    def insert(self, tokens, s, n):
        score = hyp_score(s, n, self.lp)
        if len(self.hyps) >= self.B:
            w = min(range(len(self.hyps)), key=lambda i: (self.hyps[i]["score"], i))
            self._cmp(score, self.hyps[w]["score"])
            for i, h in enumerate(self.hyps):
                if i != w:
                    self._cmp(h["score"], self.hyps[w]["score"])
            if not score > self.hyps[w]["score"]:
                return
            del self.hyps[w]
        self.hyps.append({"tokens": list(tokens), "score": score, "sum": s})

    def select(self, top_ids, top_lp, K=None):
        """top_ids / top_lp: per beam, its candidates most likely first (id < 0: none).  Sets parent / next_token / next_score
        (and the hypotheses, done); returns False for a group that was already done."""
        if self.done:
            return False
        B = self.B
        K = len(top_ids[0]) if K is None else K
        cands = []
        for b in range(B):
            if not math.isfinite(self.cum[b]):
                continue
            for j, (t, l) in enumerate(zip(top_ids[b], top_lp[b])):
                if t >= 0:
                    cands.append((self.cum[b] + float(l), b, j, int(t)))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        parent, ntok, nsc = [], [], []
        for r, (sc, b, j, t) in enumerate(cands[:K]):
            if t in self.stop:
                if r >= B:
                    continue
                self.insert(self.history[b] + [t], sc, self.n_new[b] + 1)
            else:
                parent.append(b)
                ntok.append(t)
                nsc.append(sc)
                if len(parent) == B:
                    break
        for d in range(len(parent), B):
            parent.append(d)
            ntok.append(0)
            nsc.append(NEG_INF)
        done = False
        if len(self.hyps) >= B:
            if self.early:
                done = True
            else:
                worst = min(h["score"] for h in self.hyps)
                best = hyp_score(cands[0][0] if cands else NEG_INF, self.n_new[0] + 1, self.lp)
                self._cmp(worst, best)
                done = worst >= best
        if done:
            self.done = 1
            parent = list(range(B))
        self.parent, self.next_token, self.next_score = parent, ntok, nsc
        return True

    def gather(self):
        if self.done:
            return
        p = self.parent
        self.cum = [self.cum[i] for i in p]
        self.n_new = [self.n_new[i] for i in p]
        self.history = [list(self.history[i]) for i in p]
        self.token = [self.token[i] for i in p]

    def commit(self):
        if self.done:
            return
        for d in range(self.B):
            self.token[d] = self.next_token[d]
            self.history[d].append(self.next_token[d])
            self.n_new[d] += 1
            self.cum[d] = self.next_score[d]
        if self.budget >= 0 and self.n_new[0] >= self.budget:
            for d in range(self.B):
                if math.isfinite(self.cum[d]):
                    self.insert(self.history[d], self.cum[d], self.n_new[d])
            self.done = 2
            self.parent = list(range(self.B))

    def step(self, top_ids, top_lp, K=None):
        if self.select(top_ids, top_lp, K):
            self.gather()
            self.commit()

    def result(self, n=1):
        """The n best hypotheses as (tokens, score, sum), best first, ties to the earlier insertion."""
        order = sorted(range(len(self.hyps)), key=lambda i: (-self.hyps[i]["score"], i))
        return [(self.hyps[i]["tokens"], self.hyps[i]["score"], self.hyps[i]["sum"]) for i in order[:n]]


# ---- a toy Markov model: log-probabilities of the next token given the last one ---------------------------------------------
def markov_table(V, seed):
    rng = random.Random(seed)
    rows = []
    for _ in range(V + 1):                         # row V: the start
        w = [rng.random() + 0.05 for _ in range(V)]
        z = sum(w)
        rows.append([math.log(x / z) for x in w])
    return rows


def markov_beam(table, V, length, B, length_penalty=0.0, stop_ids=(), early_stopping=False):
    g = BeamGroup(B, length_penalty=length_penalty, early_stopping=early_stopping, budget=length, stop_ids=stop_ids)
    K = max(2, 1 + len(g.stop)) * B
    while not g.done:
        ids, lps = [], []
        for b in range(B):
            row = table[g.history[b][-1] if g.history[b] else V]
            order = sorted(range(V), key=lambda i: (-row[i], i))[:K]
            ids.append(order)
            lps.append([row[i] for i in order])
        g.step(ids, lps, K=K)
    return g


def markov_brute(table, V, length):
    """Every sequence of `length` tokens with its sum (added left to right, as a beam adds it), best first."""
    out = []
    for seq in itertools.product(range(V), repeat=length):
        s, last = 0.0, V
        for t in seq:
            s += table[last][t]
            last = t
        out.append((list(seq), s))
    out.sort(key=lambda x: (-x[1], x[0]))
    return out


# ---- seeded synthetic cases of one select + gather + commit -----------------------------------------------------------------
HIST = 16          # L of the synthetic cases
CASE_SHAPES = [(2, 0), (2, 1), (3, 1), (4, 0), (4, 2), (4, 4), (8, 0)]       # (B, n_stop): K = max(2, 1 + n_stop) B <= 20
CASES_PER_SHAPE = 30
VOCAB = 50


def synthetic_case(B, n_stop, seed):
    """A group in the middle of a search with random candidate lists.  Returns a dict of plain lists; `kind` names what the
    seed forces: ties (scores on a coarse grid of exactly representable values), stop ids in the lists, -inf beams, a group
    that is already done."""
    rng = random.Random(seed * 7919 + B * 131 + n_stop)
    K = max(2, 1 + n_stop) * B
    kind = seed % 6
    n = rng.randint(1, HIST - 2)
    grid = kind in (0, 3)                          # forced ties: lps and sums are multiples of 1/4 (never with pow())
    lp = [0.0, 1.0, 2.0, 1.0, 0.7, 0.0][kind] if seed % 5 or grid else rng.choice([0.5, 1.5, 2.0])
    early = bool(rng.getrandbits(1))
    budget = rng.choice([-1, n + 1, n + 3])
    stop = rng.sample(range(VOCAB), n_stop)
    cum = []
    for b in range(B):
        v = -rng.randint(0, 12) / 4.0 if grid else -rng.random() * 6.0
        cum.append(v)
    if kind == 1 and B > 1:
        for b in rng.sample(range(B), rng.randint(1, B - 1)):
            cum[b] = NEG_INF
    ids, lps = [], []
    for b in range(B):
        toks = rng.sample(range(VOCAB), K)
        if n_stop and kind in (2, 3, 4):           # stop ids inside and beyond rank B
            for t in stop:
                if t not in toks:
                    toks[rng.randrange(K)] = t
            if len(set(toks)) != K:
                toks = stop + [t for t in range(VOCAB) if t not in stop][:K - n_stop]
                rng.shuffle(toks)
        if grid:
            vals = sorted((-rng.randint(0, 6) / 4.0 for _ in range(K)), reverse=True)
        else:
            vals = sorted((-rng.random() * 5.0 for _ in range(K)), reverse=True)
        vals = [struct.unpack("f", struct.pack("f", v))[0] for v in vals]        # fp32 values
        if kind == 5 and b == 0:
            toks[-1], vals[-1] = -1, NEG_INF       # a list shorter than K
        ids.append(toks)
        lps.append(vals)
    history = [[rng.randrange(VOCAB) for _ in range(n)] for _ in range(B)]
    hyps = []
    for _ in range(rng.randint(0, B)):
        m = rng.randint(1, n)
        s = -rng.randint(0, 40) / 4.0 if grid else -rng.random() * 10.0
        hyps.append({"tokens": [rng.randrange(VOCAB) for _ in range(m)], "score": hyp_score(s, m, lp), "sum": s})
    done = 1 if seed % 17 == 11 else 0
    return dict(B=B, K=K, n_stop=n_stop, stop=stop, lp=lp, early=early, budget=budget, cum=cum, n=n, ids=ids, lps=lps,
                history=history, hyps=hyps, done=done, kind=kind)


def reference_group(case):
    g = BeamGroup(case["B"], length_penalty=case["lp"], early_stopping=case["early"], budget=case["budget"],
                  stop_ids=case["stop"])
    g.cum = list(case["cum"])
    g.n_new = [case["n"]] * case["B"]
    g.history = [list(h) for h in case["history"]]
    g.token = [h[-1] for h in case["history"]]
    g.hyps = [dict(h, tokens=list(h["tokens"])) for h in case["hyps"]]
    g.done = case["done"]
    return g


def all_cases():
    return [(B, n_stop, [synthetic_case(B, n_stop, seed) for seed in range(CASES_PER_SHAPE)]) for B, n_stop in CASE_SHAPES]

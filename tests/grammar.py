"""Reference, input builders and the judge for constrained decoding: ivl_sample_rows_fwd / ops.sample_tokens(fsm_state=, fsm=)
(CPU only, numpy / torch).

A constrained row IS its allowed sub-vocabulary A (F1 of the header), so nothing new is judged by a new rule: `gather` takes
x[A] and the seen bits of A, and the float64 references of tests/sampling.py, tests/generation.py and tests/logprobs.py are
asked about that shorter row with their own bounds; ids are mapped through A (`to_row` / `to_vocab`).  The kernel's sums are
integers and its draw is the first index in vocabulary order, so the GPU test also asks for MORE than the references can: every
output bit-equal to the unconstrained scoring launch on the gathered row (F3).  The state is integer: `TokenFsm.step` is its
host model, compared exactly.  The builders walk seeds with sampling.with_margin on the gathered, penalised row, so every
sampled case carries the top-p margin (sampling.judge asserts it; no case is excused).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

import generation
import logprobs
import sampling

INF = float("inf")


def gather(x: torch.Tensor, seen, allow):
    """(x[A] bf16, seen[A] bool, A int64 ascending) of a row; allow None = a free row: everything"""
    V = x.shape[0]
    A = np.arange(V, dtype=np.int64) if allow is None else np.nonzero(np.asarray(allow, dtype=bool))[0].astype(np.int64)
    return x.detach().cpu()[torch.from_numpy(A)], np.asarray(seen, dtype=bool)[A], A


def to_vocab(ids, A: np.ndarray) -> np.ndarray:
    """indices into the gathered row -> token ids; -1 stays -1"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.where(ids >= 0, A[np.clip(ids, 0, max(A.shape[0] - 1, 0))] if A.shape[0] else -1, -1)


def to_row(ids, A: np.ndarray, where: str = "") -> np.ndarray:
    """token ids -> indices into the gathered row; an id outside A (a disallowed token emitted or listed) fails here"""
    ids = np.asarray(ids, dtype=np.int64)
    at = np.searchsorted(A, np.where(ids >= 0, ids, A[0] if A.shape[0] else 0))
    ok = (ids < 0) | ((at < A.shape[0]) & (A[np.minimum(at, A.shape[0] - 1)] == ids))
    assert ok.all(), f"{where}: tokens outside the allowed set: {ids[~ok][:4].tolist()}"
    return np.where(ids >= 0, at, -1)


def judge(case: Dict, ctr, token, n_kept=None, prob=None, logprob=None, top_ids=None, top_lps=None, seen_bool=None,
          where: str = "") -> None:
    """The float64 judges on the gathered row of `case`: sampling.judge (token, n_kept, prob) and logprobs.judge (scores)."""
    where = where or case["name"]
    seen = case["seen"] if seen_bool is None else seen_bool
    xg, sg, A = gather(case["x"], seen, case["allow"])
    assert A.shape[0] > 0, f"{where}: a dead end is not judged here"
    pen = generation.penalise(xg, sg, case["r"])
    tg = int(to_row([token], A, where)[0])
    sampling.judge(pen, case, ctr, tg, n_kept, prob, where=where)
    if logprob is not None:
        ids = None if top_ids is None else to_row(top_ids, A, where)
        logprobs.judge(pen, tg, logprob, ids, top_lps, where=where)


# =============================================================================================================================
# allowed sets and cases: {"name", "x" (the RAW bf16 row), "allow" (bool [V] or None), "seen", "r", "tau", "k", "p", "seed", "done"}
# =============================================================================================================================
def every(V: int, n: int, first: int = 0) -> np.ndarray:
    a = np.zeros(V, dtype=bool)
    a[first % V::n] = True
    return a


def only(V: int, ids) -> np.ndarray:
    """the ids that lie below V; token V - 1 where none does"""
    a = np.zeros(V, dtype=bool)
    ids = [i for i in ids if 0 <= i < V]
    a[ids if ids else [V - 1]] = True
    return a


def case(name, x, allow, tau=0.0, k=0, p=1.0, seed=1, r=1.0, seen=None, done=0) -> Dict:
    V = x.shape[0]
    return {"name": name, "x": x, "allow": allow, "tau": tau, "k": k, "p": p, "seed": seed, "r": r,
            "seen": np.zeros(V, dtype=bool) if seen is None else seen, "done": done}


def sampled(name, V, allow, tau, k, p, seed0, r=1.0, seen=None, scale=3.0) -> Dict:
    """a random row, the first seed from seed0 on whose GATHERED, penalised row has the top-p margin"""
    sn = np.zeros(V, dtype=bool) if seen is None else seen

    def make(s):
        xg, sg, _ = gather(sampling.random_row(V, s, scale=scale), sn, allow)
        return generation.penalise(xg, sg, r)
    _, s = sampling.with_margin(make, tau, k, p, seed0)
    return case(f"{name}-s{s}", sampling.random_row(V, s, scale=scale), allow, tau, k, p, seed=seed0 * 7 + 1, r=r, seen=sn)


def hostile(V: int, allow: np.ndarray, inside: float) -> torch.Tensor:
    """every allowed logit = `inside`; the disallowed ones +inf, NaN and the row's finite maximum in turn"""
    x = torch.full((V,), inside, dtype=torch.float32)
    out = np.nonzero(~allow)[0]
    x[torch.from_numpy(out[0::3])] = INF
    x[torch.from_numpy(out[1::3])] = float("nan")
    x[torch.from_numpy(out[2::3])] = 3.0e38
    return x.to(torch.bfloat16)


def operator_cases(V: int) -> List[Dict]:
    """every kind of constrained row at one V; the test adds a free and a finished row to its calls"""
    full = np.ones(V, dtype=bool)
    e7 = every(V, 7, 3)
    nA = int(e7.sum())
    half = np.random.default_rng(V).random(V) < 0.5
    half[V - 1] = True
    q = generation.random_seen(V, 60 + V, frac=0.5)
    edge = only(V, [31, 32, V - 1])
    rows = [case("all-greedy", sampling.random_row(V, 11), full),
            sampled("all-sampled", V, full, 0.7, 50, 0.9, 100 + V),
            sampled("one-token", V, only(V, [V // 2]), 0.7, 0, 1.0, 110 + V),
            case("one-token-greedy", sampling.random_row(V, 12), only(V, [V // 3])),
            sampled("bits-31-32-last", V, edge, 1.5, 0, 1.0, 120 + V),
            case("bits-31-32-last-greedy", sampling.random_row(V, 13), edge),
            case("ninf-inside-sampled", hostile(V, e7, -INF), e7, tau=1.0, seed=5),
            case("ninf-inside-greedy", hostile(V, e7, -INF), e7),
            case("nan-inside-topk", hostile(V, e7, float("nan")), e7, tau=0.7, k=2, seed=6),
            case("finite-inside-hostile-outside", hostile(V, half, -2.5), half, tau=0.7, seed=7),
            sampled("every7-topp", V, e7, 0.7, 0, 0.5, 130 + V),
            sampled("half-pen-1.3", V, half, 0.7, 50, 0.9, 140 + V, r=1.3, seen=q),
            case("half-pen-0.8-greedy", sampling.random_row(V, 14), half, r=0.8, seen=q),
            sampled("every7-pen-all-seen", V, e7, 1.5, 0, 1.0, 150 + V, r=0.8, seen=np.ones(V, dtype=bool), scale=5.0)]
    for k in sorted({nA - 1, nA, nA + 1, V - 1}):                      # top_k around |A| and just below V
        if k >= 1:
            rows.append(sampled(f"every7-k{k}", V, e7, 1.5, k, 1.0, 160 + V + k))
            rows.append(sampled(f"every7-k{k}-topp", V, e7, 0.7, k, 0.9, 170 + V + k))
    return [dict(c, name=f"V{V}-{c['name']}") for c in rows]


def grammars_for(cases: List[Dict], V: int):
    """Two TokenFsm over V tokens that hold the allowed sets of `cases` as states (even cases in the first, odd in the second; a
    case without a set gets none) plus, in each, one state that allows nothing (unreachable, so legal).  A token with an even id
    leads to the grammar's state 0, one with an odd id makes the row unconstrained: the class lookup decides.
    Returns (fsm_a, fsm_b, where) with where[i] = (0 | 1, local state) or None; the empty state is the last of each grammar."""
    from infinitevl_amd.grammar import TokenFsm
    sets = ([], [])
    where: List[Optional[tuple]] = []
    for i, c in enumerate(cases):
        if c["allow"] is None:
            where.append(None)
            continue
        g = i % 2
        if not sets[g]:                                               # state 0 must allow something: it is reachable
            assert c["allow"].any()
        where.append((g, len(sets[g])))
        sets[g].append(np.asarray(c["allow"], dtype=bool))
    fsms = []
    for g in (0, 1):
        own = sets[g] or [np.ones(V, dtype=bool)]
        edges = []
        for q, a in enumerate(own):
            ids = np.nonzero(a)[0]
            edges.append((q, ids[ids % 2 == 0].tolist(), 0))
            edges.append((q, ids[ids % 2 == 1].tolist(), TokenFsm.FREE))
        fsms.append(TokenFsm.from_edges(V, len(own) + 1, edges))
    return fsms[0], fsms[1], where

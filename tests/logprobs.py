"""Reference and judge for the scores of ivl_sample_rows_fwd / ops.sample_tokens(logprob=, top_ids=, ...) (CPU only, numpy /
torch): the log-probability of the emitted token and the N most likely alternatives.

The scored distribution is the row as the kernel keys it: the bf16 row after generation.penalise (where a penalty applies), NaN as
-inf, before temperature, top-k and top-p.  `reference` is its log-softmax in float64; `top_list` orders the exact bf16 values by
(value descending, index ascending).  The judge asks for
  * ids equal to the reference list, exactly: keys are exact, no case is skipped or given a margin;
  * |lp - lp_ref| <= 2^-18 max(1, |lp_ref|).  The kernel's Z1 = sum floor(exp2f((x - m) log2e) 2^40) has a relative error below
    (log2 V + 2) 2^-24 (the fp32 exponent argument of a weight that matters, one ulp of exp2f) + V 2^-40 (the floor); three fp32
    roundings follow (the conversion of Z1, logf, the subtraction); for V < 2^18 the total is below the bound;
  * +-inf exactly;
  * a top_logprobs entry bit-equal to `logprob` where it is the emitted token.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

import sampling

TOL = 2.0 ** -18
N_TOP_MAX = 20


def reference(x: torch.Tensor) -> np.ndarray:
    """bf16 [V] (already penalised) -> float64 [V] log-probabilities.  A row whose maximum is +inf puts all mass on its +inf
    tokens, equally; a row of nothing but -inf / NaN is uniform."""
    v = sampling.logits64(x)
    V = v.shape[0]
    m = v.max()
    if m == np.inf:
        top = v == np.inf
        return np.where(top, -np.log(float(top.sum())), -np.inf)
    if m == -np.inf:
        return np.full(V, -np.log(float(V)))
    with np.errstate(divide="ignore"):
        d = v - m
        return d - np.log(np.exp(d).sum())


def top_list(x: torch.Tensor, n: int) -> np.ndarray:
    """the min(n, V) indices with the largest values, by (value descending, index ascending); -0 ties with +0"""
    v = sampling.logits64(x) + 0.0
    order = np.lexsort((np.arange(v.shape[0]), -v))
    return order[:n].astype(np.int64)


def close(lp, ref) -> bool:
    lp, ref = float(lp), float(ref)
    if np.isinf(ref) or np.isinf(lp) or np.isnan(lp):
        return lp == ref
    return abs(lp - ref) <= TOL * max(1.0, abs(ref))


def judge(x: torch.Tensor, token: int, logprob, top_ids=None, top_lps=None, where: str = "") -> None:
    """x: the (penalised) bf16 row; logprob fp32 scalar; top_ids int64 [N] / top_lps fp32 [N] or None"""
    ref = reference(x)
    V = ref.shape[0]
    assert 0 <= int(token) < V, (where, token)
    lp = np.float32(logprob)
    assert close(lp, ref[int(token)]), f"{where}: logprob {float(lp)!r} of token {int(token)}, reference {ref[int(token)]!r}"
    if top_ids is None:
        return
    ids, lps = np.asarray(top_ids, dtype=np.int64), np.asarray(top_lps, dtype=np.float32)
    n = ids.shape[0]
    want = top_list(x, n)
    assert ids[:want.shape[0]].tolist() == want.tolist(), f"{where}: top ids {ids.tolist()}, reference {want.tolist()}"
    assert (ids[want.shape[0]:] == -1).all() and (lps[want.shape[0]:] == -np.inf).all(), f"{where}: the tail past V"
    for j, i in enumerate(want):
        assert close(lps[j], ref[i]), f"{where}: top_logprobs[{j}] = {float(lps[j])!r} of token {int(i)}, reference {ref[i]!r}"
        if int(i) == int(token):
            assert lps[j].tobytes() == lp.tobytes(), f"{where}: top_logprobs[{j}] {float(lps[j])!r} != logprob {float(lp)!r}"


# =============================================================================================================================
# rows
# =============================================================================================================================
def all_equal(V: int, value: float = 1.5) -> torch.Tensor:
    return torch.full((V,), value, dtype=torch.bfloat16)


def ties_across(V: int, n: int, seed: int = 0) -> torch.Tensor:
    """n - 1 distinct larger values at scattered places, then the (n)-th value shared by many indices on both sides of them: the
    N-th place falls inside a tie for every N >= n"""
    x = (sampling.random_row(V, 500 + seed, scale=1.0).float().clamp(max=2.0)).to(torch.bfloat16).float()
    g = np.random.default_rng(seed)
    idx = g.permutation(V)
    big = idx[:max(0, min(n - 1, V - 1))]
    tie = idx[len(big):len(big) + max(1, min(V - len(big), 40))]
    x[torch.from_numpy(tie)] = 4.0
    x[torch.from_numpy(big)] = torch.tensor([5.0 + 0.5 * i for i in range(len(big))])
    return x.to(torch.bfloat16)


def specials(V: int, kind: str) -> torch.Tensor:
    """NaN, +-inf and -0 among random values"""
    x = sampling.random_row(V, 77).float()
    at = lambda i: i % V
    if kind == "nan":                       # NaN = -inf; finite maximum
        x[[at(0), at(5), at(V - 1)]] = float("nan")
        x[at(3)] = -float("inf")
        x[at(7)] = -0.0
    elif kind == "pinf":                    # the maximum is +inf, twice where the row is long enough
        x[[at(2), at(V - 2)]] = float("inf")
        x[at(4)] = float("nan") if V > 4 else float("inf")
    elif kind == "ninf":                    # nothing but -inf and NaN
        x[:] = -float("inf")
        x[at(1)] = float("nan")
    else:
        raise ValueError(kind)
    return x.to(torch.bfloat16)


def deep(V: int, seed: int = 0) -> torch.Tensor:
    """a wide row: a handful of tokens near the maximum, everything else 30 .. 60 nats below it (weight 0 in Q40)"""
    g = torch.Generator().manual_seed(900 + seed)
    x = -40.0 + 6.0 * torch.randn(V, generator=g).clamp(-3.0, 1.5)
    top = torch.randperm(V, generator=g)[:min(V, 6)]
    x[top] = 8.0 - torch.arange(top.shape[0], dtype=torch.float32)
    return x.to(torch.bfloat16)

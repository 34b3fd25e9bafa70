"""Reference, input builders and the judge for the generation controls of ivl_sample_rows_fwd / ops.sample_tokens (CPU only,
numpy / torch): repetition penalty, stop ids, token budget.

The penalty is evaluated with exactly the header's arithmetic: fp32 on the widened bf16 logit, x < 0 ? x * r : x / r, one
round-to-nearest-even back to bf16 (`penalise`).  The penalised row is a bf16 row again, so the float64 reference and the judge of
tests/sampling.py apply to it unchanged: `reference` / `judge` here ARE sampling.reference / sampling.judge on penalise(x), with
sampling's bounds and sampling's top-p margin -- no new tolerance.  The builders walk seeds with sampling.with_margin on the
PENALISED row, so every case carries the margin (test_generation_cpu.py asserts it from the reference alone; no case is excused).
The stop / budget bookkeeping is integer state: `Book` is its host model, compared exactly.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

import sampling

RS = (1.3, 0.8)
FIXED_VS = (1, 97, 4099)
KS = (0, 50)


def penalise(x_bf16: torch.Tensor, seen_bool, r: float) -> torch.Tensor:
    """bf16 [V] -> bf16 [V]: bf16_rne(x < 0 ? x * r : x / r) in float32 where `seen_bool`, x elsewhere; r as the fp32 the kernel
    receives.  r == 1 leaves the row as it is (the kernel does not look at the bitmap then)."""
    assert x_bf16.dtype == torch.bfloat16 and x_bf16.dim() == 1
    seen = np.asarray(seen_bool, dtype=bool)
    assert seen.shape == (x_bf16.shape[0],)
    r32 = np.float32(r)
    if r32 == np.float32(1.0):
        return x_bf16.clone()
    x = x_bf16.detach().cpu().float().numpy()
    with np.errstate(all="ignore"):
        y = np.where(x < 0, (x * r32).astype(np.float32), (x / r32).astype(np.float32)).astype(np.float32)
    pen = torch.from_numpy(y).to(torch.bfloat16)                       # round to nearest even; NaN stays NaN
    return torch.where(torch.from_numpy(seen), pen, x_bf16.detach().cpu())


def reference(x: torch.Tensor, seen_bool, r: float, tau: float, k: int, p: float) -> sampling.Ref:
    return sampling.reference(penalise(x, seen_bool, r), tau, k, p)


def judge(case: Dict, ctr, token, n_kept=None, prob=None, seen_bool=None, where: str = "") -> None:
    """sampling.judge on the penalised row of `case` (its own bitmap, or `seen_bool` for an evolving one)"""
    seen = case["seen"] if seen_bool is None else seen_bool
    sampling.judge(penalise(case["x"], seen, case["r"]), case, ctr, token, n_kept, prob, where=where or case["name"])


# =============================================================================================================================
# bitmaps: bit (i & 31) of word (i >> 5)
# =============================================================================================================================
def words_for(V: int) -> int:
    return (V + 31) // 32


def pack(seen_bool, n_words: int, beyond: bool) -> np.ndarray:
    """bool [V] -> uint32 [n_words]; the bits at or above V (the tail of the last word and every further word) are `beyond`"""
    seen = np.asarray(seen_bool, dtype=bool)
    bits = np.full(n_words * 32, bool(beyond))
    assert seen.shape[0] <= bits.shape[0]
    bits[:seen.shape[0]] = seen
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u4").copy()


def unpack(words: np.ndarray) -> np.ndarray:
    """uint32 [n_words] -> bool [n_words * 32]"""
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)


def to_i32(words: np.ndarray) -> torch.Tensor:
    """uint32 words as the int32 tensor ops.sample_tokens takes"""
    return torch.from_numpy(np.ascontiguousarray(words, dtype="<u4").view(np.int32).copy())


def random_seen(V: int, seed: int, frac: float = 0.25) -> np.ndarray:
    return np.random.default_rng(seed).random(V) < frac


# =============================================================================================================================
# builders: {"name", "x" (the RAW bf16 row), "seen" (bool [V]), "r", "tau", "k", "p", "seed"}; every case has the top-p margin
# =============================================================================================================================
def fixed_cases(V: int) -> List[Dict]:
    """r in RS x (one greedy row + TAUS x KS x PS), a quarter of the bits set, then the all-seen and the none-seen bitmap"""
    cases, n = [], 0

    def add(tag, seen, r, tau, k, p, scale=3.0):
        nonlocal n
        n += 1
        x, s = sampling.with_margin(lambda s_: penalise(sampling.random_row(V, s_, scale=scale), seen, r), tau, k, p, 50 * n + V)
        cases.append({"name": f"V{V}-{tag}-r{r}-tau{tau}-k{k}-p{p}-s{s}", "x": sampling.random_row(V, s, scale=scale), "seen": seen,
                      "r": r, "tau": tau, "k": k, "p": p, "seed": (n * 0x2545F49 + V) * (-1 if n % 2 else 1)})

    for r in RS:
        add("quarter", random_seen(V, 7000 + n), r, 0.0, 7, 0.8)
        for tau in sampling.TAUS:
            for k in KS:
                for p in sampling.PS:
                    add("quarter", random_seen(V, 7000 + n), r, tau, k, p, scale=(2.0, 3.0, 5.0)[n % 3])
    for r in RS:
        for tag, seen in (("all", np.ones(V, dtype=bool)), ("none", np.zeros(V, dtype=bool))):
            add(tag, seen, r, 0.0, 0, 1.0)
            add(tag, seen, r, 0.7, 50, 0.9)
            add(tag, seen, r, 1.5, 0, 0.5)
    return cases


def special_row(V: int = 97) -> Dict:
    """NaN, +-inf, +-0 and a subnormal among seen and unseen tokens: what the penalty must leave in its class"""
    x = sampling.random_row(V, 31).float()
    x[[0, 1]] = float("nan")
    x[[2, 3]] = float("inf")
    x[[4, 5]] = -float("inf")
    x[[6, 7]] = torch.tensor([0.0, -0.0])
    x[8] = 2.0 ** -130
    seen = np.zeros(V, dtype=bool)
    seen[[0, 2, 4, 6, 7, 8]] = True
    seen[20:60:3] = True
    return {"name": "special", "x": x.to(torch.bfloat16), "seen": seen, "r": 1.3, "tau": 0.7, "k": 0, "p": 1.0, "seed": 9}


def greedy_chain(x: torch.Tensor, r: float, n: int, seen0=None) -> List[int]:
    """the tokens of n greedy calls on one row whose bitmap evolves: each token is penalised from the next call on"""
    seen = np.zeros(x.shape[0], dtype=bool) if seen0 is None else np.array(seen0, dtype=bool)
    out = []
    for _ in range(n):
        t = reference(x, seen, r, 0.0, 0, 1.0).argmax
        out.append(t)
        seen[t] = True
    return out


# =============================================================================================================================
# the bookkeeping of one row (step C of the header), on the host
# =============================================================================================================================
class Book:
    def __init__(self, V: int, stop_ids: Sequence[int] = (), budget: int = -1, fill: int = 0, hist_ld: int = 0,
                 seen0: Optional[np.ndarray] = None):
        self.seen = np.zeros(V, dtype=bool) if seen0 is None else np.array(seen0, dtype=bool)
        self.stop, self.budget, self.fill = [int(t) for t in stop_ids], int(budget), int(fill)
        self.n_new, self.done = 0, 0
        self.history = [0] * hist_ld

    def push(self, token: int) -> None:
        """a live row drew `token`"""
        assert self.done == 0
        self.seen[token] = True
        if self.history:
            self.history[self.n_new % len(self.history)] = int(token)
        self.n_new += 1
        if any(t >= 0 and t == token for t in self.stop):
            self.done = 1
        elif self.budget >= 0 and self.n_new >= self.budget:
            self.done = 2

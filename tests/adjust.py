"""Reference, input builders and the judge for the adjustment group of ivl_sample_rows_adj_fwd / ops.sample_tokens (CPU only,
numpy / torch): frequency / presence penalties, logit bias, min-p.

The additive adjustment is evaluated with exactly the header's arithmetic (ADJ-1): numpy float32 on the widened bf16 logit
x' (the row AFTER the repetition penalty, generation.penalise), every operation rounded once, in the header's order --
RN(f * (float)c), RN(. + p), RN(x' - .), RN(. + bias) -- and one round-to-nearest-even back to bf16 (`adjust`).  The adjusted
row x'' is a bf16 row again, so everything behind it is judged by what exists: the composition rule ADJ-2 is checked EXACTLY,
against ivl_sample_rows_fwd on x'' with r = 1, and the float64 reference and judge of tests/sampling.py apply to x'' unchanged.

min-p (ADJ-3) extends sampling.reference: P' = {i in P : w_i >= f32(min_p)}, w the float64 weight (1 at the maximum).  The kernel
compares integer weights, floor(w 2^40) >= floor(min_p 2^40), and its w carries the relative weight error derived in
tests/sampling.py (about 32 * 2^-23 = 3.8e-6, from three fp32 roundings of an exponent of at most 40 and a 2-ulp exp2f; the two
floors add 2^-40 / min_p, below 2^-35 for the min_p >= 0.05 used here).  So a case is only judged when every class of P other
than the maximum's satisfies |w - f32(min_p)| / f32(min_p) >= MINP_MARGIN = 2^-15 (`minp_margin`; the same 4 x margin over the
same error).  The maximum's class is exempt because its weight is exactly 2^40 on the device and exactly 1 here: it survives
every min_p <= 1 on both sides, with no rounding involved.  The builders walk seeds (as sampling.with_margin does) to the
first row with BOTH margins; test_adjust_cpu.py asserts both for every case from the reference alone.  No case is excused.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

import generation
import sampling

MINP_MARGIN = 2.0 ** -15
MIN_PS = (0.05, 0.3, 1.0)
KPS = ((0, 1.0), (50, 1.0), (0, 0.9), (50, 0.5))
FIXED_VS = (1, 97, 4099)
INF = float("inf")


# =============================================================================================================================
# ADJ-1 on the host
# =============================================================================================================================
def bits(x_bf16: torch.Tensor) -> np.ndarray:
    """bf16 [V] -> its uint16 bit patterns"""
    return x_bf16.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def adjust(x_bf16: torch.Tensor, seen_bool, count, f: float, p: float, bias_mask=None, bias_val=None) -> torch.Tensor:
    """bf16 [V] (x', the row after the repetition penalty) -> bf16 [V] (x''), in float32 with the operation order of ADJ-1:
         seen, count > 0, (f, p) != (0, 0):   t = x' - RN(RN(f * (float)count) + p)
         bias_mask:                           t = RN(t + bias_val)
         touched by either:                   x'' = bf16_rne(t); else the bits of x'.
    f, p as the fp32 values the kernel receives; count int32 [V]; bias_mask bool [V] and bias_val float32 [V], or None."""
    assert x_bf16.dtype == torch.bfloat16 and x_bf16.dim() == 1
    V = x_bf16.shape[0]
    seen, cnt = np.asarray(seen_bool, dtype=bool), np.asarray(count, dtype=np.int32)
    assert seen.shape == cnt.shape == (V,)
    f32_, p32 = np.float32(f), np.float32(p)
    x = x_bf16.detach().cpu().float().numpy()
    t = x.copy()
    with np.errstate(all="ignore"):
        pen = seen & (cnt > 0) & bool((f32_ != 0) or (p32 != 0))
        a = (f32_ * cnt.astype(np.float32)).astype(np.float32)
        b = (a + p32).astype(np.float32)
        t = np.where(pen, (x - b).astype(np.float32), t).astype(np.float32)
        touched = pen.copy()
        if bias_mask is not None:
            bm = np.asarray(bias_mask, dtype=bool)
            bv = np.asarray(bias_val, dtype=np.float32)
            assert bm.shape == bv.shape == (V,)
            t = np.where(bm, (t + bv).astype(np.float32), t).astype(np.float32)
            touched |= bm
    out = torch.from_numpy(t).to(torch.bfloat16)                       # round to nearest even; NaN stays NaN
    return torch.where(torch.from_numpy(touched), out, x_bf16.detach().cpu())


def adjusted_row(c: Dict, seen_bool=None, count=None) -> torch.Tensor:
    """x'' of a case: the repetition penalty (step B), then ADJ-1; `seen_bool` / `count` for evolving ones"""
    seen = c["seen"] if seen_bool is None else seen_bool
    cnt = c["count"] if count is None else count
    return adjust(generation.penalise(c["x"], seen, c["r"]), seen, cnt, c["f"], c["pp"], c["bias_mask"], c["bias_val"])


# =============================================================================================================================
# the reference with min-p
# =============================================================================================================================
@dataclass
class AdjRef(sampling.Ref):
    min_p: float = 0.0
    minp_margin: float = float("inf")     # min over the classes of P below the maximum of |w - min_p| / min_p


def reference(x2: torch.Tensor, tau: float, k: int, p: float, min_p: float = 0.0) -> AdjRef:
    """sampling.reference on the (adjusted) bf16 row x2, then ADJ-3: P' = {i in P : w_i >= f32(min_p)}"""
    base = sampling.reference(x2, tau, k, p)
    mp = sampling.f32(min_p)
    if base.greedy or not mp > 0:
        return AdjRef(**vars(base), min_p=mp)
    v = sampling.logits64(x2)
    top = v == v.max()
    below = base.P & ~top
    margin = float((np.abs(base.w[below] - mp) / mp).min()) if below.any() else float("inf")
    P = base.P & (top | (base.w >= mp))
    w = np.where(P, base.w, 0.0)
    C = np.cumsum(w)
    return AdjRef(base.V, base.tau, base.k, base.p, False, base.argmax, P, w, C, float(C[-1]), int(P.sum()), base.margin,
                  min_p=mp, minp_margin=margin)


def has_margins(ref: AdjRef) -> bool:
    return ref.greedy or (ref.margin >= sampling.MARGIN and ref.minp_margin >= MINP_MARGIN)


def judge(c: Dict, ctr, token, n_kept=None, prob=None, seen_bool=None, count=None, where: str = "") -> None:
    """sampling.judge on P' of the adjusted row of `c`"""
    ref = reference(adjusted_row(c, seen_bool, count), c["tau"], c["k"], c["p"], c["min_p"])
    assert has_margins(ref), f"{where or c['name']}: builder bug: margins {ref.margin:.3e} / {ref.minp_margin:.3e}"
    sampling.judge(ref, c, ctr, token, n_kept, prob, where=where or c["name"])


# =============================================================================================================================
# builders: {"name", "x" (the RAW bf16 row), "seen" (bool [V]), "count" (int32 [V]), "r", "f", "pp", "bias_mask" (bool [V] or
# None), "bias_val" (float32 [V] or None), "tau", "k", "p", "min_p", "seed"}; every case has both margins
# =============================================================================================================================
def random_count(V: int, seen, seed: int, hi: int = 6) -> np.ndarray:
    """counts 1 .. hi - 1 on about half of the seen tokens (the generated ones), 0 on the rest of them (a prompt's tokens) and
    on every unseen token"""
    g = np.random.default_rng(seed)
    c = g.integers(1, hi, size=V).astype(np.int32)
    return np.where(np.asarray(seen, dtype=bool) & (g.random(V) < 0.5), c, 0).astype(np.int32)


def random_bias(V: int, seed: int, frac: float = 0.1, scale: float = 3.0, ban: int = 0):
    """(mask bool [V], val float32 [V]): a bias on about `frac` of the tokens, the first `ban` of them -inf; val is 0 elsewhere"""
    g = np.random.default_rng(seed)
    mask = g.random(V) < frac
    if V <= 8:
        mask[:] = True
    val = np.where(mask, (g.standard_normal(V) * scale), 0.0).astype(np.float32)
    idx = np.nonzero(mask)[0]
    if V > 8:
        val[idx[:ban]] = -INF
    return mask, val


def bias_dict(mask, val) -> Dict[int, float]:
    return {int(i): float(val[i]) for i in np.nonzero(mask)[0]}


def case(name: str, x: torch.Tensor, seen=None, count=None, r: float = 1.0, f: float = 0.0, pp: float = 0.0, bias=None,
         tau: float = 0.0, k: int = 0, p: float = 1.0, min_p: float = 0.0, seed: int = 1) -> Dict:
    V = x.shape[0]
    seen = np.zeros(V, dtype=bool) if seen is None else np.asarray(seen, dtype=bool)
    count = np.zeros(V, dtype=np.int32) if count is None else np.asarray(count, dtype=np.int32)
    bm, bv = (None, None) if bias is None else bias
    return {"name": name, "x": x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16), "seen": seen, "count": count, "r": r, "f": f,
            "pp": pp, "bias_mask": bm, "bias_val": bv, "tau": tau, "k": k, "p": p, "min_p": min_p, "seed": seed}


def with_margins(make, seed0: int, tries: int = 96) -> Dict:
    """make(seed) -> case; the first seed of seed0, seed0 + 1, ... whose adjusted row has both margins (from the reference)"""
    for s in range(seed0, seed0 + tries):
        c = make(s)
        if has_margins(reference(adjusted_row(c), c["tau"], c["k"], c["p"], c["min_p"])):
            return c
    raise AssertionError(f"no seed in [{seed0}, {seed0 + tries}) gives both margins")


PENS = ((0.5, 0.25), (-0.3, 0.0), (0.0, 0.7), (0.0, 0.0))


def operator_cases(V: int) -> List[Dict]:
    """the rows of the composition test: every (f, p) of PENS with and without a bias table and a repetition penalty, greedy and
    sampled, top-k / top-p / min-p on and off"""
    cases = []
    combos = [(0.0, 0, 1.0, 0.0), (0.7, 0, 1.0, 0.0), (1.5, 50, 0.9, 0.05), (0.7, 50, 1.0, 0.3), (0.05, 0, 0.5, 0.0), (1.5, 0, 1.0, 1.0)]
    n = 0
    for i, (f, pp) in enumerate(PENS):
        for with_bias in (False, True):
            if (f, pp) == (0.0, 0.0) and not with_bias:
                continue                                               # (the all-off row is the identity test's)
            for j in range(2):
                tau, k, p, min_p = combos[n % len(combos)]
                r = (1.0, 1.3, 0.8)[n % 3]
                n += 1

                def make(s, n=n, f=f, pp=pp, with_bias=with_bias, tau=tau, k=k, p=p, min_p=min_p, r=r):
                    seen = generation.random_seen(V, 9000 + s, frac=0.3)
                    return case(f"V{V}-f{f}-pp{pp}-{'bias' if with_bias else 'nobias'}-r{r}-tau{tau}-k{k}-p{p}-minp{min_p}-s{s}",
                                sampling.random_row(V, s, scale=(2.0, 3.0, 5.0)[n % 3]), seen, random_count(V, seen, 9100 + s), r, f, pp,
                                random_bias(V, 9200 + s, ban=2) if with_bias else None, tau, k, p, min_p,
                                seed=(n * 0x3C6EF35 + V) * (-1 if n % 2 else 1))
                cases.append(with_margins(make, 70 * n + V))
    return cases


def minp_cases(V: int) -> List[Dict]:
    """sampling.TAUS x MIN_PS x KPS on random rows of their own, no other adjustment: what the min-p test draws from"""
    cases, n = [], 0
    for tau in sampling.TAUS:
        for min_p in MIN_PS:
            for k, p in KPS:
                n += 1

                def make(s, n=n, tau=tau, min_p=min_p, k=k, p=p):
                    return case(f"V{V}-minp{min_p}-tau{tau}-k{k}-p{p}-s{s}", sampling.random_row(V, s, scale=(2.0, 3.0, 5.0)[n % 3]),
                                tau=tau, k=k, p=p, min_p=min_p, seed=(n * 0x51ED27 + V) * (-1 if n % 2 else 1))
                cases.append(with_margins(make, 130 * n + V))
    return cases


def special_row(V: int = 97) -> Dict:
    """NaN, +-inf, +-0 and a subnormal among penalised, biased and untouched tokens"""
    x = sampling.random_row(V, 41).float()
    x[[0, 1, 2]] = float("nan")
    x[[3, 4]] = INF
    x[[5, 6]] = -INF
    x[[7, 8, 9]] = torch.tensor([0.0, -0.0, -0.0])
    x[10] = 2.0 ** -130
    seen = np.zeros(V, dtype=bool)
    seen[[0, 3, 5, 7, 8, 10]] = True
    seen[20:60:3] = True
    count = np.where(seen, 2, 0).astype(np.int32)
    bm = np.zeros(V, dtype=bool)
    bm[[1, 4, 6, 9, 11, 12, 13]] = True
    bm[21:60:6] = True
    bv = np.where(bm, 1.25, 0.0).astype(np.float32)
    bv[[4, 11]] = -INF                                                 # +inf - inf = NaN = -inf; a banned token
    bv[12] = INF
    bv[9] = 0.0                                                        # -0 + 0 = +0: the class of zero
    return case("special", x.to(torch.bfloat16), seen, count, 1.0, 0.5, -0.25, (bm, bv), 0.7, 0, 1.0, 0.0, seed=9)


def frequency_chain(x: torch.Tensor, f: float, pp: float, n: int, r: float = 1.0) -> List[int]:
    """the tokens of n greedy calls on one row whose bitmap and counts evolve: exact, the arithmetic is exact and greedy"""
    V = x.shape[0]
    seen, count, out = np.zeros(V, dtype=bool), np.zeros(V, dtype=np.int32), []
    for _ in range(n):
        x2 = adjust(generation.penalise(x, seen, r), seen, count, f, pp)
        t = sampling.reference(x2, 0.0, 0, 1.0).argmax
        out.append(t)
        seen[t] = True
        count[t] += 1
    return out


# ---------------------------------------------------------------------------------------------
# the C entry point on pointers that are never dereferenced (validation fails first)
# ---------------------------------------------------------------------------------------------
ONE = sampling.ONE
NAME = "ivl_sample_rows_adj_fwd"
ADJ_FIELDS = "min_p freq_penalty pres_penalty count count_ld bias_idx bias_mask bias_mask_ld bias_val bias_ld n_bias".split()


def c_call(lib, adj: Optional[Dict], V: int = 64, **fields) -> int:
    """ivl_sample_rows_adj_fwd on an ivl_sample_args that holds what the control-free call requires (as sampling.c_call) with
    `fields` on top, and an ivl_sample_adj_args of `adj` (None: a NULL group)"""
    from infinitevl_amd import _lib
    base = dict(logits=ONE, ld=V, S=1, V=V, temperature=ONE, top_k=ONE, top_p=ONE, seed=ONE, counter=ONE, token=ONE, token_stride=1)
    a = _lib.SampleArgs(**{**base, **fields})
    j = None if adj is None else ctypes.byref(_lib.GROUP_STRUCTS["ivl_sample_adj_args"](**adj))
    return lib.ivl_sample_rows_adj_fwd(ctypes.byref(a), j, None)


def c_refused(lib, code: int, word: bytes, adj: Optional[Dict], **fields) -> bool:
    """c_call returns `code` and ivl_last_error() names the entry point and `word`"""
    rc, err = c_call(lib, adj, **fields), lib.ivl_last_error()
    return rc == code and NAME.encode() in err and word in err

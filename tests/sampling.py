"""Float64 reference, input builders and the judge for ivl_sample_rows_fwd / ops.sample_tokens (CPU only, numpy / torch).

The reference evaluates the header's semantics in float64 on the bf16 logits: NaN = -inf; temperature <= 0 = the lowest-index
arg-max; top-k keeps ties at the threshold; w_i = exp((x_i - m) / tau), exactly 1 at the maximum, 0 at -inf below it; top-p keeps a
class of equal logits while the mass strictly above it is below p; the draw is the first index of P, in vocabulary order, whose
inclusive cumulative weight exceeds u Z_P, u = u64(seed, ctr) / 2^64 from the splitmix64 finaliser.  tau and p are taken as the
fp32 values the kernel receives.

What is judged, and why the bounds are what they are (none is fitted to the kernel):

  token   must lie in P, and with F_lo = C_{token-1} / Z_P, F_hi = C_token / Z_P (float64 cumulative weights over P in index
          order):  F_lo - EPS <= u < F_hi + EPS,  EPS = 2^-15.
          The kernel draws with integer weights q_i = floor(exp2f((x_i - m) * (log2e / tau)) * 2^40).  Only weights of at least
          2^-40 matter, so the exponent argument is at most 27.7 nats = 40 in base 2: its fp32 rounding (the difference, the
          factor log2e / tau, the product: 3 roundings of 2^-24 relative on a value of at most 40, i.e. about 30 * 2^-23
          absolute in the exponent at worst) plus a 2-ulp exp2f gives a relative weight error of at most about 32 * 2^-23; it
          enters the numerator and the denominator of F: 7.6e-6.  The floor adds at most V * 2^-40 = 1.4e-7 at V = 151936 (the
          weights dropped below 2^-40 are inside that figure).  Total about 7.8e-6; 2^-15 = 3.05e-5 is a 4 x margin.
  greedy  rows are exact: token = the lowest index of the maximum, n_kept = 1, prob = 1, the counter does not move.
  n_kept  is exact.  Top-k is exact by construction (an order statistic of bf16 values).  Top-p compares A(v) with p, and the
          kernel's A carries the weight error above, so a case is only judged when EVERY class boundary of the row satisfies
          |A(v) - f32(p)| >= MARGIN = 2^-15 (`margin`); the builders only emit such cases (random rows walk a fixed seed sequence
          to the first seed with the margin: on random rows about 1 seed in 25 lacks it), and test_sampling_cpu.py asserts it for
          every case of every builder from the reference alone.  No case is excused: one without the margin is a builder bug.
  prob    |prob - w_token / Z_P| <= 2^-15 * ref + 2^-39  (the same relative weight error; 2^-39: the floor of q_token, doubled).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

EPS = 2.0 ** -15
MARGIN = 2.0 ** -15
G = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
U64_VECTORS = (((0, 0), 0xE220A8397B1DCDAF), ((0, 1), 0x6E789E6AA1B965F4), ((1, 0), 0xBFEF8030DDC2D772),
               ((-1, 0), 0xA577782BC52A9F5A), ((1234567890123, 41), 0x83BE0D88B4416917))


def f32(v: float) -> float:
    """a Python float as the kernel receives it"""
    return float(np.float32(v))


# =============================================================================================================================
# the random stream
# =============================================================================================================================
def mix(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u64(seed: int, ctr: int) -> int:
    """the 64 random bits of draw number `ctr` (0-based: the counter BEFORE the draw) of the stream `seed`"""
    return mix(mix(seed) + (ctr + 1) * G)


def u64_array(seed: int, ctrs: Sequence[int]) -> np.ndarray:
    """u64 for many counters (numpy uint64 arithmetic wraps like the kernel's)"""
    def mixv(z):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        c = (np.asarray(ctrs, dtype=np.int64).astype(np.uint64) + np.uint64(1)) * np.uint64(G)
        return mixv(np.uint64(mix(seed)) + c)


# =============================================================================================================================
# the reference
# =============================================================================================================================
@dataclass
class Ref:
    V: int
    tau: float
    k: int
    p: float
    greedy: bool
    argmax: int                      # the lowest index of the maximum
    P: np.ndarray                    # bool [V]
    w: np.ndarray                    # float64 [V], 0 outside P
    C: np.ndarray                    # inclusive cumulative weight over P in index order
    Z: float
    n_kept: int
    margin: float                    # min over the classes of K of |A(v) - p| (inf when top-p is off)


def logits64(x: torch.Tensor) -> np.ndarray:
    """bf16 logits [V] -> float64 with NaN as -inf"""
    assert x.dtype == torch.bfloat16 and x.dim() == 1, (x.dtype, tuple(x.shape))
    v = x.detach().cpu().double().numpy().copy()
    v[np.isnan(v)] = -np.inf
    return v


def reference(x: torch.Tensor, tau: float, k: int, p: float) -> Ref:
    v = logits64(x)
    V = v.shape[0]
    tau, p, k = f32(tau), f32(p), int(k)
    m = v.max()
    argmax = int(np.argmax(v == m))
    if not tau > 0:
        P = np.zeros(V, dtype=bool)
        P[argmax] = True
        w = P.astype(np.float64)
        return Ref(V, tau, k, p, True, argmax, P, w, np.cumsum(w), 1.0, 1, float("inf"))
    K = np.ones(V, dtype=bool)
    if 0 < k < V:
        K = v >= np.sort(v)[V - k]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((v - m) / tau)
    w = np.where(v == m, 1.0, w)
    w = np.where(np.isneginf(v) & (v < m), 0.0, w)
    w = np.where(K, w, 0.0)
    P, margin = K, float("inf")
    if p < 1:
        vals, inv = np.unique(v[K], return_inverse=True)                 # ascending classes of K
        cm = np.bincount(inv, weights=w[K], minlength=vals.shape[0])
        above = np.concatenate([np.cumsum(cm[::-1])[::-1][1:], [0.0]])   # mass strictly above each class
        A = above / cm.sum()
        keep = A < p
        margin = float(np.abs(A - p).min())
        P = K.copy()
        P[K] = keep[inv]
    w = np.where(P, w, 0.0)
    C = np.cumsum(w)
    return Ref(V, tau, k, p, False, argmax, P, w, C, float(C[-1]), int(P.sum()), margin)


def draw(ref: Ref, seed: int, ctr: int) -> int:
    """the reference's own token of draw `ctr`"""
    if ref.greedy:
        return ref.argmax
    u = u64(seed, ctr) / 2.0 ** 64
    return int(np.searchsorted(ref.C, u * ref.Z, side="right"))


def judge(x, params: Dict, ctr, token, n_kept=None, prob=None, where: str = "") -> None:
    """Assert the kernel's outputs for draws `ctr` (counter before each draw; scalars or equal-length sequences) of ONE row.
    x: the bf16 logits [V] or their Ref; params: {"tau", "k", "p", "seed"}."""
    ref = x if isinstance(x, Ref) else reference(x, params["tau"], params["k"], params["p"])
    assert ref.greedy or ref.margin >= MARGIN, f"{where}: builder bug: a top-p boundary within {ref.margin:.3e} of p"
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.int64))
    token = np.atleast_1d(np.asarray(token, dtype=np.int64))
    assert token.shape == ctr.shape, (token.shape, ctr.shape)
    assert ((token >= 0) & (token < ref.V)).all(), f"{where}: token outside [0, {ref.V}): {token[(token < 0) | (token >= ref.V)][:4]}"
    if n_kept is not None:
        n_kept = np.atleast_1d(np.asarray(n_kept, dtype=np.int64))
        assert (n_kept == ref.n_kept).all(), f"{where}: n_kept {np.unique(n_kept)[:4]} != {ref.n_kept}"
    if ref.greedy:
        assert (token == ref.argmax).all(), f"{where}: greedy token {np.unique(token)[:4]} != lowest arg-max {ref.argmax}"
        if prob is not None:
            assert (np.atleast_1d(np.asarray(prob, dtype=np.float64)) == 1.0).all(), f"{where}: greedy prob != 1"
        return
    assert ref.P[token].all(), f"{where}: token outside P: {token[~ref.P[token]][:4]}"
    u = u64_array(params["seed"], ctr).astype(np.float64) / 2.0 ** 64
    F_hi = ref.C[token] / ref.Z
    F_lo = np.where(token > 0, ref.C[np.maximum(token - 1, 0)], 0.0) / ref.Z
    bad = ~((F_lo - EPS <= u) & (u < F_hi + EPS))
    assert not bad.any(), (f"{where}: {int(bad.sum())} of {bad.size} draws outside [F_lo - EPS, F_hi + EPS): first at ctr "
                           f"{ctr[bad][0]}: token {token[bad][0]} F_lo {F_lo[bad][0]:.9f} u {u[bad][0]:.9f} F_hi {F_hi[bad][0]:.9f}")
    if prob is not None:
        prob = np.atleast_1d(np.asarray(prob, dtype=np.float64))
        want = ref.w[token] / ref.Z
        err = np.abs(prob - want) - (2.0 ** -15 * want + 2.0 ** -39)
        assert (err <= 0).all(), f"{where}: prob off by {np.abs(prob - want).max():.3e} (first want {want[err > 0][0]:.6e})"


# =============================================================================================================================
# input builders: {"name", "x" (bf16 [V]), "tau", "k", "p", "seed"}; every case has the top-p margin
# =============================================================================================================================
TAUS = (0.05, 0.7, 1.5)
PS = (1.0, 0.9, 0.5)
OPERATOR_VS = (1, 97, 512, 4099, 151936)


def ks_for(V: int):
    return (0, 1, 50, V, V + 5)


def _bf(a) -> torch.Tensor:
    return torch.as_tensor(a, dtype=torch.float32).to(torch.bfloat16)


def random_row(V: int, seed: int, scale: float = 3.0) -> torch.Tensor:
    return _bf(torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale)


def with_margin(make, tau: float, k: int, p: float, seed0: int, tries: int = 64):
    """make(seed) -> bf16 row; the first seed of seed0, seed0 + 1, ... whose row has the top-p margin (decided by the reference)"""
    for s in range(seed0, seed0 + tries):
        x = make(s)
        if not tau > 0 or reference(x, tau, k, p).margin >= MARGIN:
            return x, s
    raise AssertionError(f"no seed in [{seed0}, {seed0 + tries}) gives the top-p margin (tau {tau} k {k} p {p})")


def operator_cases(V: int) -> List[Dict]:
    """one greedy row + every (tau, k, p) of the operator test, each on random logits of its own"""
    cases = [{"name": f"V{V}-greedy", "x": random_row(V, 1000 + V), "tau": 0.0, "k": 7, "p": 0.8, "seed": 5}]
    n = 0
    for tau in TAUS:
        for k in ks_for(V):
            for p in PS:
                n += 1
                x, s = with_margin(lambda s_: random_row(V, s_, scale=(2.0, 3.0, 5.0)[n % 3]), tau, k, p, 100 * n + V)
                cases.append({"name": f"V{V}-tau{tau}-k{k}-p{p}-s{s}", "x": x, "tau": tau, "k": k, "p": p,
                              "seed": (n * 0x1234567 + V) * (-1 if n % 2 else 1)})
    return cases


def adversarial_cases(V: int = 4099) -> List[Dict]:
    assert V >= 4099, "the cases place values at fixed indices up to 3000"
    inf = float("inf")
    out = []

    def add(name, x, tau, k, p, seed=11):
        out.append({"name": f"adv-{name}", "x": x if x.dtype == torch.bfloat16 else _bf(x), "tau": tau, "k": k, "p": p, "seed": seed})

    base = random_row(V, 77).float()
    add("all-equal", torch.full((V,), 1.5), 0.7, 0, 1.0)
    add("all-equal-topk-topp", torch.full((V,), -2.25), 0.7, 50, 0.9)
    x = base.clone()
    x[torch.arange(0, V, 7)] = float("nan")                                 # index 0 included
    add("nan-mixed", x, 0.7, 0, 1.0)
    add("nan-mixed-topk-topp", x, 1.5, 50, 0.5)
    add("nan-mixed-greedy", x, 0.0, 0, 1.0)
    add("all-ninf", torch.full((V,), -inf), 0.7, 0, 1.0)
    add("all-ninf-topk-topp", torch.full((V,), -inf), 0.7, 50, 0.9)
    add("all-nan-greedy", torch.full((V,), float("nan")), 0.0, 0, 1.0)
    x = base.clone()
    x[V // 3] = inf
    add("one-pinf", x, 0.7, 0, 1.0)
    add("one-pinf-topk-topp", x, 1.5, 50, 0.9)
    x = base.clone()
    x[V // 3], x[V // 2] = inf, -inf
    add("pinf-and-ninf", x, 0.7, 0, 0.9)
    x = (base * 0.25).clone()                                               # k-th largest value five times: k = 3 keeps 2 + 5
    x[[5, 900]] = torch.tensor([9.0, 8.5])
    x[[17, 18, 2000, 3000, V - 1]] = 8.0
    add("ties-at-topk", x, 1.5, 3, 1.0)
    add("ties-at-topk-topp", x, 1.5, 3, 0.9)
    x = base.clone()
    x[0] = 12.0
    add("max-at-0", x, 1.5, 0, 1.0)
    add("max-at-0-greedy", x, 0.0, 0, 1.0)
    x = base.clone()
    x[V - 1] = 12.0
    add("max-at-last", x, 1.5, 0, 1.0)
    add("max-at-last-greedy", x, 0.0, 0, 1.0)
    x = base.clone()
    x[[V - 2, 41, 1234]] = 14.0
    add("dup-max-greedy", x, 0.0, 0, 1.0)
    add("dup-max", x, 0.7, 0, 0.5)
    x = base.clone()
    x[3], x[4] = 0.0, -0.0                                                  # -0 and +0 are one class
    x[:3] = -1.0
    x[5:] = torch.where(x[5:] > 0, -x[5:], x[5:]) - 0.5
    add("signed-zero-max", x, 0.7, 2, 1.0)
    add("signed-zero-max-greedy", x, 0.0, 0, 1.0)
    x = (base * 40.0).clone()                                               # most of the row more than 27.7 nats below the maximum
    add("deep-tail", x, 0.05, 0, 1.0)
    add("deep-tail-topp", x, 0.7, 0, 0.9)
    return out


def hf_kept(x: torch.Tensor, tau: float, k: int, p: float) -> np.ndarray:
    """The kept set of HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper, by sorting (float64; for tie-free
    rows, where HF's cut does not depend on the sort order)."""
    s = torch.from_numpy(logits64(x)) / f32(tau)
    V = s.shape[0]
    if 0 < k < V:
        s = s.masked_fill(s < torch.topk(s, k)[0][-1], -float("inf"))
    if f32(p) < 1:
        srt, idx = torch.sort(s, descending=False)
        cum = srt.softmax(-1).cumsum(-1)
        remove = cum <= (1 - f32(p))
        remove[-1:] = False
        s = s.masked_fill(torch.zeros(V, dtype=torch.bool).scatter(0, idx, remove), -float("inf"))
    return (s > -float("inf")).numpy()


# ---------------------------------------------------------------------------------------------
# the C entry point on pointers that are never dereferenced (validation fails first)
# ---------------------------------------------------------------------------------------------
ONE = 0x1000
ARG_FIELDS = ("logits ld S V "
              "temperature top_k top_p seed counter token token_stride n_kept prob "
              "rep_penalty seen seen_ld stop_ids n_stop budget fill n_new done history hist_ld "
              "logprob n_top top_ids top_logprobs cum_logprob lp_history top_hist_ids top_hist_lp "
              "fsm_state fsm_mask mask_ld n_states fsm_desc fsm_cls fsm_trans score_only").split()


def c_call(lib, V: int = 64, **fields) -> int:
    """ivl_sample_rows_fwd on an ivl_sample_args that holds what the control-free call requires (S = 1, ld = V, token_stride = 1,
    every required pointer ONE) with `fields` on top (None = NULL); everything else is 0 / NULL."""
    from infinitevl_amd import _lib
    base = dict(logits=ONE, ld=V, S=1, V=V, temperature=ONE, top_k=ONE, top_p=ONE, seed=ONE, counter=ONE, token=ONE, token_stride=1)
    return lib.ivl_sample_rows_fwd(ctypes.byref(_lib.SampleArgs(**{**base, **fields})), None)


def c_refused(lib, code: int, word: bytes, **fields) -> bool:
    """c_call(**fields) returns `code` and ivl_last_error() names the entry point and `word`"""
    rc, err = c_call(lib, **fields), lib.ivl_last_error()
    return rc == code and b"ivl_sample_rows_fwd" in err and word in err

"""Builders of ADVERSARIAL probe inputs and their expected results (CPU only, pure torch / numpy + the oracle).

The numerical tests of the suite feed the kernels i.i.d. randn data, under which the softmax is diffuse (one key in a 4096-key
window carries 1/4096 of a row) and the GDN gates sit in the gentle middle.  The probes here make a one-key, one-tile or
one-chunk mistake catastrophic instead:

  A  band_probe / vision_band_probe     q = 0, V = one-hot residues of the key's position: round(out * n_visible) is an integer
                                        histogram of the keys a row saw.
  B  needle_probe / vision_needle_probe one key outweighs all others by e^42 or more: the row IS v[target], bit for bit
                                        ("inside"), or must ignore a dominant key just outside its band ("outside").
  C  peaked_probe / vision_peaked_probe randn q scaled by 8 (scores ~ N(0, 64)): a handful of keys own a row, the running
                                        maximum jumps by tens between tiles; reference in float64, judged per row.
  D  gdn_case                           GDN gates at the edges (wipe token, model-range decay, saturated beta, repeated key,
                                        large values), reference = the token-by-token rule in float64, judged per
                                        (batch, head, 64-token chunk).

tests/test_adversarial_cpu.py shows that every probe is satisfied by the oracle and violated by a deliberately wrong one;
tests/test_gpu_adversarial.py drives the HIP kernels with them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gdn as ogdn
from oracle import swa as oswa
from oracle import vision as ovis

BF = torch.bfloat16
ROW_BOUND_CAP = 4e-2          # the suite's existing per-row bound (test_ring256_random_shapes_vs_128_row_path_and_oracle_rows)


def bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF)


def row_bound(model_row_err_max: float) -> float:
    """Probe C's rule: the kernel gets twice the largest per-row distance of the oracle's own bf16 model from the float64 result
    on the same inputs (tile order and split-KV legitimately change which probabilities round up or down), never more than the
    suite's existing per-row bound."""
    return min(2.0 * model_row_err_max, ROW_BOUND_CAP)


def row_err(ref: torch.Tensor, got: torch.Tensor) -> torch.Tensor:
    """||got - ref|| / ||ref|| over the last dimension, float64."""
    ref, got = ref.double(), got.double()
    return (got - ref).norm(dim=-1) / (ref.norm(dim=-1) + 1e-30)


# =============================================================================================================================
# sliding-window attention over a ring
# =============================================================================================================================
@dataclass
class SwaCase:
    """One call of ops.swa_forward: batch row b has seen `seens[b]` tokens (all equal unless the call goes through pos_rows).
    k_loc / v_loc[b]: [n_prev_b + T, Hkv, d] = the keys the row's call can see, cached ones first (the oracle's layout);
    local key j of row b sits at ABSOLUTE position first[b] + j."""
    T: int
    Hq: int
    Hkv: int
    W: int
    seens: List[int]
    q: torch.Tensor                      # [B, T, Hq, d] bf16
    k_loc: List[torch.Tensor]            # bf16
    v_loc: List[torch.Tensor]
    d: int = 128
    extra: Dict = field(default_factory=dict)

    @property
    def B(self) -> int:
        return len(self.seens)

    @property
    def C(self) -> int:
        return self.W - 1

    def n_prev(self, b: int) -> int:
        return oswa.n_prev_keys(self.W, self.seens[b])

    def first(self, b: int) -> int:
        return self.seens[b] - self.n_prev(b)

    def new(self, which: str) -> torch.Tensor:
        """the call's own tokens [B, T, Hkv, d]"""
        src = self.k_loc if which == "k" else self.v_loc
        return torch.stack([src[b][self.n_prev(b):] for b in range(self.B)])

    def ring(self, which: str, fill: float) -> torch.Tensor:
        """[B, Hkv, C, d]: position p in slot p % C; slots no token has reached hold `fill` (a row that reads one shows it)."""
        src = self.k_loc if which == "k" else self.v_loc
        out = torch.full((self.B, self.Hkv, self.C, self.d), fill, dtype=BF)
        for b in range(self.B):
            n = self.n_prev(b)
            if n:
                slots = torch.arange(self.first(b), self.seens[b]) % self.C
                out[b, :, slots] = src[b][:n].transpose(0, 1)
        return out

    def ring_after(self, which: str, fill: float) -> torch.Tensor:
        """the ring after the call's tokens were appended at (seen + t) % C (std:146-172: the last C tokens survive)"""
        out = self.ring(which, fill)
        new = self.new(which)
        for b in range(self.B):
            for t in range(max(0, self.T - self.C), self.T):
                out[b, :, (self.seens[b] + t) % self.C] = new[b, t]
        return out

    def bounds_abs(self, b: int) -> Tuple[np.ndarray, np.ndarray]:
        """absolute inclusive key range of every row"""
        lo, hi = oswa.window_bounds(self.n_prev(b), self.T, self.W)
        return lo + self.first(b), hi + self.first(b)


def _swa_slab(case: SwaCase, b: int, h: int, t0: int, t1: int):
    """rows [t0, t1) of query head h with exactly the keys they can see, in the oracle's layout:
    q [1,1,t,d], k / v [1,1,S',d], n_prev' -- keys in front of the first row's band are dropped (the band would mask them)."""
    n_prev = case.n_prev(b)
    lo, _ = oswa.window_bounds(n_prev, case.T, case.W)
    # keep one key in front of the band where there is one, so that a mask that opens too early has something to admit
    j0 = max(0, int(lo[t0]) - 1)
    hk = h // (case.Hq // case.Hkv)
    q = case.q[b, t0:t1, h][None, None]
    k = case.k_loc[b][j0:n_prev + t1, hk][None, None]
    v = case.v_loc[b][j0:n_prev + t1, hk][None, None]
    return q, k, v, n_prev + t0 - j0


def swa_oracle(case: SwaCase, b: int, h: int, t0: int, t1: int, **kw) -> torch.Tensor:
    """oracle.swa.swa_attention on a slab -> [t, d] fp32"""
    q, k, v, n_prev = _swa_slab(case, b, h, t0, t1)
    return oswa.swa_attention(q.float(), k.float(), v.float(), n_prev, case.W, case.d ** -0.5, **kw)[0, :, 0]


def swa_f64(case: SwaCase, b: int, h: int, t0: int, t1: int) -> torch.Tensor:
    """softmax attention on the band, softmax and both products in float64 on the same bf16 inputs -> [t, d] float64"""
    q, k, v, n_prev = _swa_slab(case, b, h, t0, t1)
    q, k, v = q[0, 0].double(), k[0, 0].double(), v[0, 0].double()
    s = (q @ k.T) * (case.d ** -0.5)
    mask = torch.from_numpy(oswa.band_mask(n_prev, t1 - t0, case.W))
    p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
    return p @ v


def slabs(T: int) -> List[Tuple[int, int]]:
    """the rows the float64 references are computed for: all of a short call, else the first, a middle (unaligned) and the last 64"""
    if T <= 256:
        return [(0, T)]
    m = (T // 2) // 64 * 64 + 17
    return [(0, 64), (m, m + 64), (T - 64, T)]


def heads_checked(Hq: int) -> List[int]:
    return sorted({0, Hq // 2, Hq - 1})


# ---- probe A ----------------------------------------------------------------------------------------------------------------
BAND_ENCODINGS = ("fine", "coarse")
BAND_MAX_COUNT = 127      # count * 2^-8 < 0.5: the bf16 rounding of the output (and of a split-KV partial row) cannot move an integer


def _band_code(p: np.ndarray, enc: str) -> np.ndarray:
    """fine: p % 128; coarse: (p // 32) % 128 -- together they pin a contiguous range of up to 4096 positions"""
    return p % 128 if enc == "fine" else (p // 32) % 128


def band_probe(T: int, Hq: int, Hkv: int, W: int, seens: Sequence[int], enc: str, seed: int = 0) -> SwaCase:
    """q = 0 (uniform softmax over whatever the row sees), random keys, V = one-hot of the code of the key's ABSOLUTE position.
    extra["counts"][b]: int64 [T, 128] expected histogram, extra["n_vis"][b]: [T]."""
    assert W <= 4096 + 1
    g_ = torch.Generator().manual_seed(seed)
    seens = [int(s) for s in seens]
    case = SwaCase(T, Hq, Hkv, W, seens, torch.zeros(len(seens), T, Hq, 128, dtype=BF), [], [])
    counts, n_vis = [], []
    for b in range(case.B):
        S = case.n_prev(b) + T
        p = np.arange(case.first(b), case.first(b) + S)
        case.k_loc.append(bf(torch.randn(S, Hkv, 128, generator=g_)))
        oh = F.one_hot(torch.from_numpy(_band_code(p, enc)), 128).to(BF)
        case.v_loc.append(oh[:, None].expand(S, Hkv, 128).contiguous())
        lo, hi = case.bounds_abs(b)
        c = np.stack([np.bincount(_band_code(np.arange(lo[i], hi[i] + 1), enc), minlength=128) for i in range(T)])
        assert c.max() <= BAND_MAX_COUNT and c.max() * 2.0 ** -8 < 0.5, c.max()
        counts.append(c)
        n_vis.append(hi - lo + 1)
    case.extra.update(counts=counts, n_vis=n_vis, enc=enc)
    return case


def band_mismatches(case: SwaCase, out: torch.Tensor, heads: Optional[Sequence[int]] = None, limit: int = 5) -> List[str]:
    """out [B, T, Hq, 128] -> the first rows whose decoded histogram differs from the expected one ([] = exact)"""
    bad = []
    for b in range(case.B):
        n = torch.from_numpy(case.extra["n_vis"][b]).double()[:, None]
        exp = case.extra["counts"][b]
        for h in (heads_checked(case.Hq) if heads is None else heads):
            o = out[b, :, h].double()
            if not torch.isfinite(o).all():
                bad.append(f"b={b} h={h}: non-finite output")
                continue
            got = torch.round(o * n).to(torch.int64).numpy()
            rows = np.nonzero((got != exp).any(axis=1))[0]
            for i in rows[:limit]:
                cls = np.nonzero(got[i] != exp[i])[0]
                bad.append(f"{case.extra['enc']} b={b} h={h} row={i} (pos {case.seens[b] + i}): classes {cls[:6].tolist()} "
                           f"got {got[i][cls[:6]].tolist()} expected {exp[i][cls[:6]].tolist()}")
            if len(bad) >= limit:
                return bad
    return bad


# ---- probe B ----------------------------------------------------------------------------------------------------------------
NEEDLE_L, NEEDLE_Q = 16.0, 32.0


def _needle_channels(p, d: int):
    """the two channels that carry position p's code: unique within (d/2)^2 consecutive positions (4096 at d = 128)"""
    half = d // 2
    return p % half, half + (p // half) % half


def _needle_keys(p: np.ndarray, Hkv: int, d: int, g_: torch.Generator) -> torch.Tensor:
    k = bf(0.25 * torch.randn(len(p), Hkv, d, generator=g_))
    c0, c1 = _needle_channels(torch.from_numpy(p), d)
    idx = torch.arange(len(p))
    k[idx, :, c0] = NEEDLE_L
    k[idx, :, c1] = NEEDLE_L
    return k


def _inside_candidates(lo: int, hi: int, seen: int, first: int, C: int) -> Tuple[List[int], List[int]]:
    """(edge candidates, seam candidates) of a row's band [lo, hi] (absolute positions): the band's ends and their neighbours;
    the first and last key of every 64-key tile in the four alignments a kernel could tile by (call-local index, absolute
    position, ring slot, offset from the first new key) -- KV splits are whole tiles, so their first / last keys are among
    these; the ring's physical seam (slots C-1 and 0)."""
    p = np.arange(lo, hi + 1)
    edge = np.zeros(len(p), dtype=bool)
    for x in (p - first, p, p % C, p - seen):
        edge |= (x % 64 == 0) | (x % 64 == 63)
    cand = sorted(set(p[edge].tolist()) | {lo, hi, min(lo + 1, hi), max(hi - 1, lo)})
    ringp = p[p < seen]
    seam = ringp[(ringp % C == 0) | (ringp % C == C - 1)].tolist()
    return cand, seam


def inside_sweeps(T: int, Hq: int, W: int, seens: Sequence[int]) -> int:
    """how many needle_probe(..., sweep=s) calls it takes until EVERY query row has aimed at every one of its own inside
    candidates (band ends, seam, first / last key of every 64-key tile in every alignment): its heads take Hq of them per sweep"""
    C, n = W - 1, 0
    for seen in seens:
        n_prev = oswa.n_prev_keys(W, int(seen))
        first = int(seen) - n_prev
        lo, hi = oswa.window_bounds(n_prev, T, W)
        for i in range(T):
            cand, seam = _inside_candidates(int(lo[i]) + first, int(hi[i]) + first, int(seen), first, C)
            n = max(n, len(set(cand) | set(seam)))
    return -(-n // Hq)


def needle_probe(T: int, Hq: int, Hkv: int, W: int, seens: Sequence[int], mode: str = "inside", seed: int = 0,
                 sweep: Optional[int] = None) -> SwaCase:
    """Key at absolute position p: L = 16 on the two channels of its code, 0.25 * randn elsewhere; query (b, i, h): Q = 32 on the
    two channels of its target, 0 elsewhere; scaling 128^-0.5: the target scores 90.5, a key sharing one channel 45.25 + noise
    (|noise| < 4), everything else |noise|; V randn.  All values exact in bf16 and (q, the code channels) in e4m3.
    mode "inside": targets in the band (see _inside_candidates); extra["target"][b, i, h] = absolute position.  Sampled per
    (row, head) by default; `sweep = s` instead walks the row's sorted candidates deterministically -- head h of sweep s takes
    candidate (s * Hq + h) mod their number -- so that inside_sweeps(...) calls of a decode-sized form aim every row at EVERY
    tile / split edge (a T = 1 call has only Hq targets against 128 first / last keys of its 64 splits).
    mode "outside": target lo - 1 or hi + 1 (alternating; whichever exists in the ring or the call -- lo - 1 of a row over a full
    ring whose slot has been overwritten is kept too: other batch rows of a pos_rows call may hold it); the row must equal the
    float64 softmax over its true band."""
    assert W - 1 <= 4096 and mode in ("inside", "outside")
    d = 128
    g_ = torch.Generator().manual_seed(seed)
    rnd = np.random.default_rng(seed)
    seens = [int(s) for s in seens]
    B = len(seens)
    case = SwaCase(T, Hq, Hkv, W, seens, torch.zeros(B, T, Hq, d, dtype=BF), [], [])
    target = np.zeros((B, T, Hq), dtype=np.int64)
    for b in range(B):
        S = case.n_prev(b) + T
        first = case.first(b)
        p = np.arange(first, first + S)
        case.k_loc.append(_needle_keys(p, Hkv, d, g_))
        case.v_loc.append(bf(torch.randn(S, Hkv, d, generator=g_)))
        lo, hi = case.bounds_abs(b)
        for i in range(T):
            if mode == "inside":
                cand, seam = _inside_candidates(int(lo[i]), int(hi[i]), seens[b], first, case.C)
                if sweep is not None:
                    every = sorted(set(cand) | set(seam))
                    for h in range(Hq):
                        target[b, i, h] = every[(sweep * Hq + h) % len(every)]
                    continue
                for h in range(Hq):
                    r = int(rnd.integers(8))
                    if r == 0:
                        t_ = lo[i]
                    elif r == 1:
                        t_ = hi[i]
                    elif r == 2 and seens[b] - 1 >= lo[i]:
                        t_ = seens[b] - 1                              # the last ring key before the new keys
                    elif r == 3 and seam:
                        t_ = seam[int(rnd.integers(len(seam)))]
                    else:
                        t_ = cand[int(rnd.integers(len(cand)))]
                    target[b, i, h] = t_
            else:
                for h in range(Hq):
                    below, above = int(lo[i]) - 1, int(hi[i]) + 1
                    ok_below, ok_above = below >= 0, i + 1 < T
                    pick_below = ok_below and ((i + h) % 2 == 0 or not ok_above)
                    target[b, i, h] = below if pick_below else (above if ok_above else max(below, 0))
    tt = torch.from_numpy(target)
    c0, c1 = _needle_channels(tt, d)
    case.q.scatter_(3, c0[..., None], NEEDLE_Q)
    case.q.scatter_(3, c1[..., None], NEEDLE_Q)
    n_vis_full = []
    for b in range(B):
        lo, hi = case.bounds_abs(b)
        n_vis_full.append(hi - lo + 1 == W)
    case.extra.update(target=target, mode=mode, n_vis_full=n_vis_full)
    return case


def needle_expected(case: SwaCase, round_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """inside mode: [B, T, Hq, d] bf16 = v[target] of the head's kv head (rounded through `round_dtype` for the fp8 kernel)"""
    assert case.extra["mode"] == "inside"
    rep = case.Hq // case.Hkv
    out = torch.empty(case.B, case.T, case.Hq, case.d, dtype=BF)
    for b in range(case.B):
        j = torch.from_numpy(case.extra["target"][b] - case.first(b))           # [T, Hq] local indices
        assert int(j.min()) >= 0 and int(j.max()) < case.k_loc[b].shape[0]
        v = case.v_loc[b].repeat_interleave(rep, dim=1)                         # [S, Hq, d]
        out[b] = v[j, torch.arange(case.Hq)[None, :].expand_as(j)]
    if round_dtype is not None:
        out = out.float().clamp(-448.0, 448.0).to(round_dtype).to(BF)
    return out


def _bits_differ(out: torch.Tensor, expected: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns differ.  Where the expected element is 0 (a v element below e4m3's smallest number), what all other
    keys together leave there (< 1e-16 of a row, times |v| <= 448) is not a difference: |out| < 1e-12 passes, +-0 alike."""
    return (out.to(BF).view(torch.int16) != expected.view(torch.int16)) & ~((expected.float() == 0) & (out.float().abs() < 1e-12))


def needle_mismatches(case: SwaCase, out: torch.Tensor, expected: torch.Tensor, limit: int = 5) -> List[str]:
    neq = _bits_differ(out, expected)
    bad = []
    for b, i, h in neq.any(-1).nonzero().tolist()[:limit]:
        tgt = int(case.extra["target"][b, i, h])
        lo, hi = case.bounds_abs(b)
        bad.append(f"b={b} row={i} (pos {case.seens[b] + i}, band [{lo[i]}, {hi[i]}]) h={h} target key {tgt} "
                   f"(slot {tgt % case.C if tgt < case.seens[b] else 'new'}): got {out[b, i, h, :3].float().tolist()} "
                   f"expected {expected[b, i, h, :3].float().tolist()}")
    return bad


# ---- probe C ----------------------------------------------------------------------------------------------------------------
def peaked_probe(T: int, Hq: int, Hkv: int, W: int, seens: Sequence[int], seed: int = 0, q_scale: float = 8.0) -> SwaCase:
    """randn q scaled by 8, randn k / v (bf16 grid): scores ~ N(0, 64)"""
    g_ = torch.Generator().manual_seed(seed)
    seens = [int(s) for s in seens]
    case = SwaCase(T, Hq, Hkv, W, seens, bf(q_scale * torch.randn(len(seens), T, Hq, 128, generator=g_)), [], [])
    for b in range(case.B):
        S = case.n_prev(b) + T
        case.k_loc.append(bf(torch.randn(S, Hkv, 128, generator=g_)))
        case.v_loc.append(bf(torch.randn(S, Hkv, 128, generator=g_)))
    return case


def swa_row_report(case: SwaCase, out: Optional[torch.Tensor], fp8: bool = False) -> Dict[str, float]:
    """Per-row distances on the checked (batch row, head, slab)s, maxima over all checked rows.
    bf16: `model` = the oracle's own bf16 model (probabilities rounded to bf16 before P V, output rounded to bf16) from the
    float64 result; `kernel` = `out` [B, T, Hq, d] from the float64 result.
    fp8 decode step (as test_swa_fp8_decode_vs_oracle): `model` = the oracle with e4m3 operands from the float64 result on the
    unrounded inputs; `kernel` = `out` from that e4m3-operand oracle."""
    res = {"model": 0.0, "kernel": 0.0, "where": None}
    for b in range(case.B):
        for h in heads_checked(case.Hq):
            for t0, t1 in slabs(case.T):
                ref = swa_f64(case, b, h, t0, t1)
                if fp8:
                    model = swa_oracle(case, b, h, t0, t1, mma_rounding=torch.float8_e4m3fn)
                    res["model"] = max(res["model"], float(row_err(ref, model).max()))
                    ref = model
                else:
                    model = swa_oracle(case, b, h, t0, t1, p_round_dtype=BF).to(BF)
                    res["model"] = max(res["model"], float(row_err(ref, model).max()))
                if out is not None:
                    e = row_err(ref, out[b, t0:t1, h])
                    if not torch.isfinite(e).all():
                        res["kernel"], res["where"] = float("inf"), (b, h, t0)
                    elif float(e.max()) > res["kernel"]:
                        res["kernel"], res["where"] = float(e.max()), (b, h, t0 + int(e.argmax()))
    return res


PEAKED_SEED = 11


def fp8_outside_bound(case: SwaCase) -> Tuple[float, float]:
    """(model distance, kernel bound) of the fp8 decode step on probe B's OUTSIDE inputs themselves: 4/3 (the ratio of
    test_swa_fp8_decode_vs_oracle) of the e4m3-operand oracle's worst row distance from float64 on these inputs (2.7e-2 ..
    5.6e-2: the e4m3 rounding of v; never degenerate, unlike the bf16 model's on rows that one key owns).  Probe C's fp8 bound
    (0.35 .. 0.61 at W >= 96) would let a leak at W = 4096, which only halves the row (error 0.7), pass by a hair."""
    m = swa_row_report(case, None, fp8=True)["model"]
    return m, 4.0 / 3.0 * m


def swa_peaked_bound(T: int, Hq: int, Hkv: int, W: int, seens: Sequence[int], fp8: bool = False) -> Tuple[float, float]:
    """(model distance, kernel bound) of probe C for a shape: bf16 -- row_bound of the bf16 model's worst row; fp8 decode step --
    4/3 (the ratio of test_swa_fp8_decode_vs_oracle) of the e4m3-operand oracle's worst row distance from float64.  Probe B's
    outside rows are held to the same bound (on their own inputs a row that one key owns outright makes the model exact)."""
    m = swa_row_report(peaked_probe(T, Hq, Hkv, W, seens, seed=PEAKED_SEED), None, fp8=fp8)["model"]
    return m, (4.0 / 3.0 * m if fp8 else row_bound(m))


# =============================================================================================================================
# vision window attention (packed segments, non-causal)
# =============================================================================================================================
VISION_SEGMENTS = (0, 1, 63, 64, 65, 129, 0, 900, 1024)        # empty, one patch, around one and two 64-row tiles, long


@dataclass
class VisionCase:
    q: torch.Tensor            # [S, H, d] bf16
    k: torch.Tensor
    v: torch.Tensor
    cu: List[int]
    extra: Dict = field(default_factory=dict)

    @property
    def max_seqlen(self) -> int:
        return max(b - a for a, b in zip(self.cu[:-1], self.cu[1:]))

    def seg_of(self) -> np.ndarray:
        """[S, 2]: the (first, end) of every patch's segment"""
        out = np.zeros((self.q.shape[0], 2), dtype=np.int64)
        for a, b in zip(self.cu[:-1], self.cu[1:]):
            out[a:b] = (a, b)
        return out


def _cu(lengths: Sequence[int]) -> List[int]:
    return [0] + np.cumsum(np.asarray(lengths, dtype=np.int64)).tolist()


def identity_rope(S: int, d: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos = 1, sin = 0: x * 1 + rotate_half(x) * 0 leaves q and k bit-unchanged while the rotating loads run"""
    return torch.ones(S, d), torch.zeros(S, d)


def _vision_code(j: np.ndarray, d: int, enc: str) -> np.ndarray:
    """fine: j % d; coarse: (j // 16) % d -- at most ceil(1024 / d) resp. 16 keys of a segment of up to 1024 share a class"""
    return j % d if enc == "fine" else (j // 16) % d


def vision_band_probe(lengths: Sequence[int], H: int, d: int, enc: str, seed: int = 0) -> VisionCase:
    cu = _cu(lengths)
    S = cu[-1]
    assert max(lengths) <= 1024
    g_ = torch.Generator().manual_seed(seed)
    j = np.arange(S)
    oh = F.one_hot(torch.from_numpy(_vision_code(j, d, enc)), d).to(BF)
    case = VisionCase(torch.zeros(S, H, d, dtype=BF), bf(torch.randn(S, H, d, generator=g_)), oh[:, None].expand(S, H, d).contiguous(), cu)
    seg = case.seg_of()
    counts = np.zeros((S, d), dtype=np.int64)
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            counts[a:b] = np.bincount(_vision_code(np.arange(a, b), d, enc), minlength=d)[None]
    assert counts.max() <= BAND_MAX_COUNT and counts.max() * 2.0 ** -8 < 0.5
    case.extra.update(counts=counts, n_vis=seg[:, 1] - seg[:, 0], enc=enc)
    return case


def vision_band_mismatches(case: VisionCase, out: torch.Tensor, limit: int = 5) -> List[str]:
    """out [S, H, d]; every head is checked"""
    bad = []
    if not torch.isfinite(out.float()).all():
        return ["non-finite output"]
    n = torch.from_numpy(case.extra["n_vis"]).double()[:, None, None]
    got = torch.round(out.double() * n).to(torch.int64).numpy()
    exp = case.extra["counts"][:, None, :]
    seg = case.seg_of()
    for s, h in np.argwhere((got != exp).any(axis=2))[:limit]:
        cls = np.nonzero(got[s, h] != exp[s, 0])[0][:6]
        bad.append(f"{case.extra['enc']} patch {s} (segment [{seg[s, 0]}, {seg[s, 1]})) h={h}: classes {cls.tolist()} got "
                   f"{got[s, h][cls].tolist()} expected {exp[s, 0][cls].tolist()}")
    return bad


def vision_needle_probe(lengths: Sequence[int], H: int, d: int, mode: str = "inside", seed: int = 0) -> VisionCase:
    """The needle construction with the code sized for d: channels j % (d/2) and d/2 + (j // (d/2)) % (d/2), j = index in the
    packed sequence, unique within (d/2)^2 patches (1024 / 1600 / 4096 at d = 64 / 80 / 128).  inside: targets at the segment's
    first and last patch (and random ones between); outside: the last patch of the previous / the first patch of the next
    segment.  The builder asserts that no patch of the row's own segment shares both channels with the target."""
    cu = _cu(lengths)
    S = cu[-1]
    half = d // 2
    g_ = torch.Generator().manual_seed(seed)
    rnd = np.random.default_rng(seed)
    j = np.arange(S)
    k = _needle_keys(j, H, d, g_)
    v = bf(torch.randn(S, H, d, generator=g_))
    case = VisionCase(torch.zeros(S, H, d, dtype=BF), k, v, cu)
    seg = case.seg_of()
    target = np.zeros((S, H), dtype=np.int64)
    for s in range(S):
        a, b = seg[s]
        for h in range(H):
            r = (s + h) % 3
            if mode == "inside":
                target[s, h] = a if r == 0 else (b - 1 if r == 1 else int(rnd.integers(a, b)))
            else:
                below, above = a - 1, b
                pick_below = below >= 0 and ((s + h) % 2 == 0 or above >= S)
                target[s, h] = below if pick_below else (above if above < S else a)     # a single segment has no outside: own first patch
    code = target % half + half * ((target // half) % half)
    for s in range(S):
        a, b = seg[s]
        jj = np.arange(a, b)
        same = (jj % half + half * ((jj // half) % half))[None, :] == code[s][:, None]
        assert (same & (jj[None, :] != target[s][:, None])).sum() == 0, "the code must be unique within a segment and its neighbours"
    tt = torch.from_numpy(target)
    c0, c1 = _needle_channels(tt, d)
    case.q.scatter_(2, c0[..., None], NEEDLE_Q)
    case.q.scatter_(2, c1[..., None], NEEDLE_Q)
    case.extra.update(target=target, mode=mode)
    return case


def vision_needle_expected(case: VisionCase) -> torch.Tensor:
    t = torch.from_numpy(case.extra["target"])
    return case.v[t, torch.arange(case.q.shape[1])[None, :].expand_as(t)]


def vision_needle_mismatches(case: VisionCase, out: torch.Tensor, expected: torch.Tensor, limit: int = 5) -> List[str]:
    neq = _bits_differ(out, expected)
    seg = case.seg_of()
    return [f"patch {s} (segment [{seg[s, 0]}, {seg[s, 1]})) h={h} target {int(case.extra['target'][s, h])}"
            for s, h in neq.any(-1).nonzero().tolist()[:limit]]


def vision_peaked_probe(lengths: Sequence[int], H: int, d: int, seed: int = 0, q_scale: float = 8.0) -> VisionCase:
    cu = _cu(lengths)
    g_ = torch.Generator().manual_seed(seed)
    S = cu[-1]
    return VisionCase(bf(q_scale * torch.randn(S, H, d, generator=g_)), bf(torch.randn(S, H, d, generator=g_)),
                      bf(torch.randn(S, H, d, generator=g_)), cu)


def vision_peaked_bound(lengths: Sequence[int], H: int, d: int) -> Tuple[float, float]:
    m = vision_row_report(vision_peaked_probe(lengths, H, d, seed=PEAKED_SEED), None)["model"]
    return m, row_bound(m)


def vision_f64(case: VisionCase, cu: Optional[Sequence[int]] = None) -> torch.Tensor:
    """segment attention, softmax and both products in float64 -> [S, H, d]"""
    S, H, d = case.q.shape
    out = torch.zeros(S, H, d, dtype=torch.float64)
    cu = case.cu if cu is None else cu
    for a, b in zip(cu[:-1], cu[1:]):
        if b > a:
            q, k, v = (x[a:b].double().transpose(0, 1) for x in (case.q, case.k, case.v))
            out[a:b] = (torch.softmax((q @ k.transpose(1, 2)) * d ** -0.5, dim=-1) @ v).transpose(0, 1)
    return out


def vision_row_report(case: VisionCase, out: Optional[torch.Tensor]) -> Dict[str, float]:
    ref = vision_f64(case)
    model = ovis.segment_attention(case.q, case.k, case.v, case.cu, p_round_dtype=BF).to(BF)
    res = {"model": float(row_err(ref, model).max()), "kernel": 0.0, "where": None}
    if out is not None:
        e = row_err(ref, out)
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        res["kernel"] = float(e.max())
        res["where"] = tuple(int(x) for x in np.unravel_index(int(e.argmax()), e.shape))
    return res


# =============================================================================================================================
# Gated DeltaNet
# =============================================================================================================================
GDN_K, GDN_V = 128, 256
DECAY_A = (0.5, 4.0, 16.0)


def gdn_f64(q, k, v, g, beta, h0=None, scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The token-by-token definition (oracle.gdn.gdn_recurrent; fla:ops/gated_delta_rule/fused_recurrent.py:85-101) in float64,
    l2norm of q / k included: S *= exp(g_t); d = beta_t (v_t - S^T k_t); S += k_t d^T; o_t = S^T (q_t * scale)."""
    B, T, H, K = q.shape
    V = v.shape[-1]
    scale = K ** -0.5 if scale is None else scale
    qd, kd, vd, gd, bd = (x.double() for x in (q, k, v, g, beta))
    qd = qd / torch.sqrt((qd * qd).sum(-1, keepdim=True) + 1e-6)
    kd = kd / torch.sqrt((kd * kd).sum(-1, keepdim=True) + 1e-6)
    S = torch.zeros(B, H, K, V, dtype=torch.float64) if h0 is None else h0.double().clone()
    o = torch.empty(B, T, H, V, dtype=torch.float64)
    for t in range(T):
        S = S * gd[:, t].exp()[..., None, None]
        dlt = bd[:, t][..., None] * (vd[:, t] - torch.einsum("bhkv,bhk->bhv", S, kd[:, t]))
        S = S + kd[:, t][..., None] * dlt[..., None, :]
        o[:, t] = torch.einsum("bhkv,bhk->bhv", S, qd[:, t]) * scale
    return o, S


def gdn_case(kind: str, B: int, T: int, H: int, seed: int = 0, with_h0: bool = True, wipe_at: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Inputs of one GDN operator call on the bf16 grid (g in fp32): q, k [B,T,H,128], v [B,T,H,256], g, beta [B,T,H], h0.
      "decay"   g = -A softplus(x), x ~ randn (the distribution of test_gate_math_vs_oracle), A PINNED per head to 0.5, 4, 16 in
                turn (DECAY_A: the ends and the middle of the model's range; sampling A would leave most cases in the gentle
                middle), one token in 16 with g = 0 exactly; beta drawn from {0, 1, bf16(sigmoid(4 randn))} (saturated as far as bf16 goes)
      "beta"    the same beta with the gentle g = logsigmoid(randn)
      "still"   beta = 0 and g = 0 over the whole call: the state must come back as it went in
      "repeat"  one key for the whole call, beta = 1, g = 0, h0 = 0: S_t = k_hat v_t^T, o_t = scale (q_hat_t . k_hat) v_t
      "large"   v scaled by 64 (v_new passes the e4m3 clamp of 448 on the fp8 path), gentle g, beta = sigmoid(randn)
      "wipe"    gentle g except g = -200 at token `wipe_at`: nothing from before that token survives it"""
    g_ = torch.Generator().manual_seed(seed)
    sn = lambda x: x.to(BF).float()  # noqa: E731
    K, V = GDN_K, GDN_V
    q = sn(torch.randn(B, T, H, K, generator=g_))
    k = sn(torch.randn(B, T, H, K, generator=g_))
    v = sn(torch.randn(B, T, H, V, generator=g_))
    h0 = sn(torch.randn(B, H, K, V, generator=g_)) if with_h0 else None
    gentle = F.logsigmoid(torch.randn(B, T, H, generator=g_))
    sat = sn(torch.sigmoid(4.0 * torch.randn(B, T, H, generator=g_)))
    pick = torch.randint(0, 3, (B, T, H), generator=g_)
    sat = torch.where(pick == 0, torch.zeros(()), torch.where(pick == 1, torch.ones(()), sat))
    g, beta = gentle, sn(torch.sigmoid(torch.randn(B, T, H, generator=g_)))
    if kind == "decay":
        assert H >= len(DECAY_A), "every decay case carries a head of each pinned A"
        A = torch.tensor([DECAY_A[h % len(DECAY_A)] for h in range(H)])
        g = -A * F.softplus(torch.randn(B, T, H, generator=g_))
        g = torch.where(torch.randint(0, 16, (B, T, H), generator=g_) == 0, torch.zeros(()), g)
        beta = sat
        # the range this case is for: per-token g of -10 .. -50 on the A = 16 heads (chunk-local cumulative sums of several
        # hundred: exp(-cumsum) overflows fp32, exp of a difference is tiny but not 0), the gentle middle on the A = 0.5 heads
        g16 = g[..., [h for h in range(H) if DECAY_A[h % len(DECAY_A)] == 16.0]]
        assert float(A.max()) == 16.0 and float(g.min()) < -30.0 and float(g16.median()) < -8.0, (float(g.min()), float(g16.median()))
        assert float(g16.sum(1).min()) < -10.0 * min(T, 64) / 2 and int((g == 0).sum()) > 0
    elif kind == "beta":
        beta = sat
    elif kind == "still":
        g, beta = torch.zeros(B, T, H), torch.zeros(B, T, H)
    elif kind == "repeat":
        k = k[:, :1].expand(B, T, H, K).contiguous()
        g, beta, h0 = torch.zeros(B, T, H), torch.ones(B, T, H), None
    elif kind == "large":
        v = sn(v * 64.0)
    elif kind == "wipe":
        g = gentle.clone()
        g[:, wipe_at] = -200.0
    else:
        raise ValueError(kind)
    return dict(q=q, k=k, v=v, g=g.float().contiguous(), beta=beta.contiguous(), h0=h0)


def gdn_wipe_pair(B: int, T: int, H: int, wipe_at: int, seed: int = 0) -> Tuple[Dict, Dict]:
    """Two calls that share every input from token `wipe_at` on (and the whole g: a different g before the wipe token would
    reach the later tokens of its chunk through the ROUNDING of the chunk-local cumulative sum, not through a factor) and
    differ in h0 and in q, k, v, beta before it.  Every exponent that crosses the wipe token is below -200 + 64 * 0 = -200
    (the other g are <= 0), far below -104, so fp32 exp returns exactly 0: outputs from `wipe_at` on and the final state must be
    bit-identical."""
    a = gdn_case("wipe", B, T, H, seed=seed, wipe_at=wipe_at)
    o = gdn_case("wipe", B, T, H, seed=seed + 7919, wipe_at=wipe_at)
    b = {n: x.clone() for n, x in a.items()}
    b["h0"] = o["h0"]
    for n in ("q", "k", "v", "beta"):
        b[n][:, :wipe_at] = o[n][:, :wipe_at]
    return a, b


def gdn_model(c: Dict, mode: str = "chunk", fp8: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """the oracle's own rounding model of the operator: (o rounded to bf16, state fp32)"""
    if mode == "chunk":
        o, s = ogdn.gdn_chunk(c["q"], c["k"], c["v"], c["g"], c["beta"], initial_state=c["h0"], rounding=BF,
                              mma_rounding=torch.float8_e4m3fn if fp8 else None)
    else:
        o, s = ogdn.gdn_recurrent(c["q"], c["k"], c["v"], c["g"], c["beta"], initial_state=c["h0"], qk_round_dtype=BF)
    return o.to(BF).float(), s


GDN_TINY = 0.02           # a slice whose reference RMS is below this fraction of the call's largest slice RMS is judged absolutely


def _slice_rms(x: torch.Tensor, chunk: int = 64) -> torch.Tensor:
    """o [B,T,H,V] -> RMS per (b, h, 64-token chunk) [B, H, NT] (a ragged last chunk over its own tokens)"""
    B, T, H, V = x.shape
    NT = (T + chunk - 1) // chunk
    out = torch.empty(B, H, NT, dtype=torch.float64)
    for c in range(NT):
        out[:, :, c] = x[:, c * chunk:(c + 1) * chunk].double().square().mean(dim=(1, 3)).sqrt()
    return out


def gdn_slice_verdict(ref_o, ref_s, model_o, model_s, got_o=None, got_s=None) -> Dict:
    """Per (batch, head, 64-token chunk) for o and per (batch, head) for the state:
        kernel vs exact < max(5e-3, 1.1 * model vs exact + 2e-4)      (the rule of test_gdn_random_shapes_vs_oracle)
    relative to the slice's own reference RMS; a slice whose reference RMS is below GDN_TINY of the call's largest is judged by
    its absolute RMS error against the same factors times that largest RMS instead.  No slice is skipped.
    Returns the worst ratio error / bound (`worst` < 1 passes), its place, the number of slices and of absolutely judged ones."""
    res = {"worst": 0.0, "where": None, "slices": 0, "absolute": 0, "model_max": 0.0, "kernel_max": 0.0}
    for name, ref, model, got in (("o", _slice_rms(ref_o), _slice_rms(model_o.double() - ref_o.double()),
                                   None if got_o is None else _slice_rms(got_o.double() - ref_o.double())),
                                  ("state", ref_s.double().square().mean(dim=(2, 3)).sqrt(),
                                   (model_s.double() - ref_s.double()).square().mean(dim=(2, 3)).sqrt(),
                                   None if got_s is None else (got_s.double() - ref_s.double()).square().mean(dim=(2, 3)).sqrt())):
        top = float(ref.max())
        tiny = ref < GDN_TINY * top
        denom = torch.where(tiny, torch.full_like(ref, top), ref) + 1e-300
        bound = torch.clamp(1.1 * model / denom + 2e-4, min=5e-3)
        res["slices"] += ref.numel()
        res["absolute"] += int(tiny.sum())
        res["model_max"] = max(res["model_max"], float((model / denom).max()))
        if got is not None:
            rel = got / denom
            rel = torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))
            ratio = rel / bound
            res["kernel_max"] = max(res["kernel_max"], float(rel.max()))
            if float(ratio.max()) > res["worst"]:
                idx = tuple(int(x) for x in np.unravel_index(int(ratio.argmax()), ratio.shape))
                res["worst"], res["where"] = float(ratio.max()), (name, idx, float(rel[idx]), float(bound[idx]))
    return res


# =============================================================================================================================
# the launch forms of ops.swa_forward (dispatch of ivl_swa_fwd, csrc/swa.hip) and the shapes that reach them
# =============================================================================================================================
@dataclass(frozen=True)
class SwaForm:
    name: str
    T: int
    Hq: int
    Hkv: int
    W: int
    seens: Tuple[int, ...]           # one per batch row; all equal unless `rows`
    kernel: str                      # "packed" | "fp8" | "rows" | "64row" | "prefill" | "ring256": what the dispatch must choose
    nsplit: int                      # KV splits the dispatch must choose (ring256: not split)
    rows: bool = False               # through pos_rows (ivl_swa_decode_rows_fwd)
    rope_ok: bool = True             # the fp8 decode step takes rotated q / k only

    @property
    def B(self) -> int:
        return len(self.seens)


def swa_dispatch(B: int, T: int, Hq: int, Hkv: int, W: int, ring256: bool = False, fp8: bool = False, rows: bool = False) -> Tuple[str, int]:
    """The launch form and KV split count ivl_swa_fwd / ivl_swa_decode_rows_fwd choose for a ring call with T_new == T
    (restated from csrc/swa.hip: SWA_QT = SWA_KT = 64, PF_QT = 128, SWA_MAX_SPLIT = 16, SWA_MAX_SPLIT_PACK = 64):
      ring256   the caller vouches for pos >= C (pos_min), T >= 256 and the shape qualifies (ops.SWA_RING256_CALLS counts it)
      packed    T * Hq/Hkv <= 64: one key tile per workgroup, nsplit = min(max_tiles, 64); > 16 splits merge in the wide combine
      64row     other calls of T <= 64; prefill: T > 64 (128-row workgroups); nsplit = ceil(512 resp. 256 / (B * q-tiles * Hq)),
                capped by 16 and by a quarter of the key tiles; the combine is instantiated for <= 4 / <= 8 / <= 16 splits
      max_tiles = min(W + 128, C + T) // 64 + 2."""
    C, G = W - 1, Hq // Hkv
    if ring256:
        return "ring256", 1
    max_tiles = min(W + 128, C + T) // 64 + 2
    if T * G <= 64 and G <= 16:
        return ("rows" if rows else "fp8" if fp8 else "packed"), min(max_tiles, 64)
    if T > 64:
        base = B * ((T + 127) // 128) * Hq
        ns = min(max((256 + base - 1) // base, 1), 16)
        kern = "prefill"
    else:
        base = B * ((T + 63) // 64) * Hq
        ns = min(max((512 + base - 1) // base, 1), 16)
        kern = "64row"
    return kern, max(min(ns, max_tiles // 4, 16), 1)


def _forms() -> List[SwaForm]:
    C = 4095
    f = []
    for kern in ("packed", "fp8"):
        r = kern != "fp8"
        f += [SwaForm(f"{kern}_T1_W4096_wide", 1, 16, 2, 4096, (5000, 5000), kern, 64, rope_ok=r),          # full ring, wide combine
              SwaForm(f"{kern}_T8_W4096_wide", 8, 16, 2, 4096, (2 * C + 5,), kern, 64, rope_ok=r),
              SwaForm(f"{kern}_T5_W4096_wide_seam", 5, 16, 2, 4096, (C + 2,), kern, 64, rope_ok=r),         # new keys cross the seam
              SwaForm(f"{kern}_T3_W96_partly", 3, 16, 2, 96, (40, 40), kern, 3, rope_ok=r),                 # partly filled, combine 4
              SwaForm(f"{kern}_T5_W300", 5, 16, 2, 300, (1000,), kern, 6, rope_ok=r),                       # combine 8
              SwaForm(f"{kern}_T8_W512", 8, 16, 2, 512, (511,), kern, 10, rope_ok=r),                       # combine 16
              SwaForm(f"{kern}_T1_W2", 1, 16, 2, 2, (5, 5), kern, 2, rope_ok=r)]                            # one-slot ring
    f += [SwaForm("rows_T1_W4096", 1, 16, 2, 4096, (0, C - 1, C, C + 1, 3 * C + 17), "rows", 64, rows=True),
          SwaForm("rows_T4_W4096", 4, 16, 2, 4096, (0, C - 1, C, C + 1, 3 * C + 17), "rows", 64, rows=True),
          SwaForm("rows_T2_W96", 2, 16, 2, 96, (0, 94, 95, 96, 3 * 95 + 17), "rows", 3, rows=True),
          # T <= 64 but T * Hq/Hkv > 64: not packable
          SwaForm("64row_T40_W96_seam", 40, 16, 2, 96, (250,), "64row", 1),
          SwaForm("64row_T64_W4096_s16", 64, 16, 2, 4096, (6000,), "64row", 16),
          SwaForm("64row_T33_W4096_s8", 33, 16, 2, 4096, (C + 7,) * 4, "64row", 8),
          SwaForm("64row_T64_W4096_s4", 64, 16, 2, 4096, (C - 1,) * 8, "64row", 4),
          # T > 64: 128-row workgroups; split = ceil(256 / (B * ceil(T/128) * Hq))
          SwaForm("prefill_T256_s8_fresh", 256, 16, 2, 4096, (0,), "prefill", 8),        # empty ring (the split count goes by the capacity)
          SwaForm("prefill_T256_s8_Cm1", 256, 16, 2, 4096, (C - 1,), "prefill", 8),
          SwaForm("prefill_T256_s8_C", 256, 16, 2, 4096, (C,), "prefill", 8),
          SwaForm("prefill_T256_s8_2C5", 256, 16, 2, 4096, (2 * C + 5,), "prefill", 8),
          SwaForm("prefill_T256_s4", 256, 16, 2, 4096, (2 * C + 5,) * 2, "prefill", 4),
          SwaForm("prefill_T256_s16", 256, 4, 2, 4096, (C - 1,), "prefill", 16),
          SwaForm("prefill_T512_s1", 512, 16, 2, 1024, (1500,) * 4, "prefill", 1),       # rope: pre-pass (T >= 512)
          SwaForm("prefill_T256_s1", 256, 16, 2, 1024, (1500,) * 8, "prefill", 1),       # rope: rotation inside the kernel
          SwaForm("prefill_T1000_ragged", 1000, 16, 2, 4096, (5000,), "prefill", 2),
          SwaForm("prefill_T1000_gtC", 1000, 16, 2, 512, (700,), "prefill", 2),          # T > C
          # the caller's bound pos_min = seen >= C, T a multiple of 256, B * Hq * T / 256 >= 256 workgroups
          SwaForm("ring256_C4095_TeqC1", 4096, 16, 2, 4096, (9000,), "ring256", 1),
          SwaForm("ring256_C1023_TeqC1", 1024, 16, 2, 1024, (2500,) * 4, "ring256", 1),
          SwaForm("ring256_C699_TgtC", 2048, 16, 2, 700, (699,) * 2, "ring256", 1)]
    return f


SWA_FORMS: Dict[str, SwaForm] = {x.name: x for x in _forms()}


# GDN operator cases of probe D: (kind, B, T, H, state dtype, state in place, operands, operator)
GDN_CASES = [
    ("decay", 1, 64, 3, "f32", False, "bf16", "chunk"), ("decay", 1, 65, 3, "bf16", True, "bf16", "chunk"),
    ("decay", 2, 300, 3, "f32", True, "bf16", "chunk"), ("decay", 1, 1000, 3, "bf16", False, "bf16", "chunk"),
    ("decay", 1, 300, 3, "f32", False, "fp8", "chunk"), ("decay", 1, 1000, 3, "bf16", True, "fp8", "chunk"),
    ("decay", 1, 65, 3, "f32", False, "bf16", "recurrent"), ("decay", 1, 300, 3, "bf16", True, "bf16", "recurrent"),
    ("beta", 1, 300, 2, "f32", False, "bf16", "chunk"), ("beta", 1, 300, 2, "f32", False, "fp8", "chunk"),
    ("beta", 1, 64, 2, "f32", False, "bf16", "recurrent"),
    ("repeat", 1, 300, 2, "f32", False, "bf16", "chunk"), ("repeat", 1, 300, 2, "f32", False, "fp8", "chunk"),
    ("repeat", 1, 65, 2, "f32", False, "bf16", "recurrent"),
    ("large", 1, 300, 2, "f32", False, "bf16", "chunk"), ("large", 1, 300, 2, "f32", False, "fp8", "chunk"),
    ("large", 1, 65, 2, "f32", False, "bf16", "recurrent"),
]


def gdn_case_id(c) -> str:
    return "-".join(str(x) for x in c)


def gdn_case_inputs(c) -> Dict[str, torch.Tensor]:
    kind, B, T, H = c[:4]
    return gdn_case(kind, B, T, H, seed=1000 + 17 * T + len(kind))

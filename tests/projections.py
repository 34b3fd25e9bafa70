"""Input builders, float64 references and judges for the PROJECTION kernels (CPU only, pure torch; the pattern of tests/rowwise.py):

  ivl_linear_small_m_fwd / ivl_linear_swiglu_small_m_fwd / ivl_norm_linear_small_m_fwd      linear_small_m_kernel, M = 1 .. 4 rows
  ivl_linear_m256_fwd (plain, GLU), ivl_linear_logprob_m256_fwd (SCORE)                     linear_m256_kernel, M <= 256 rows

THE EXACT-INTEGER PROBE.  x, w (and the bias) hold small INTEGERS, all exact in bf16.  Every product and every partial sum is then
an integer far below 2^24, so fp32 accumulation is exact IN ANY ORDER -- the fmaf chains, wave_sum, the MFMA with its fp32
accumulator -- and the output must be bf16_RNE(exact sum + bias) BIT FOR BIT: no noise term, no tolerance, no excused element.

  "index"  x in [-3, 3], w in {-1, 0, +1} with the density of non-zeros chosen for a standard deviation of the sum of about 48
           (all of them non-zero where K is too small for that).  Condition (asserted here, from the float64 sum alone): at most
           1 % of the elements of a call have |sum| > 256 -- below that bf16 holds every integer, so ONE dropped, doubled or
           misplaced term changes the output.
  "ties"   K >= 64: x in [-A, A] with A chosen per K for a standard deviation of about 300, w = +-1 (a tenth of them 0).
           Conditions: every |sum| < 2^11 and at least 10 % of the elements of a call are exact bf16 TIES (an odd sum in [256, 512),
           a sum = 2 mod 4 in [512, 1024), ...): the rounding rule of f2bf / pack2bf is what decides them.

  plain    expected as above.
  GLU      the gate rows get a density for a standard deviation of about 6 (silu in its curved range); expected =
           rowwise.silu_ref on the exact bf16([g | u]), judged by Report.double (its own window, <= 1 % of a call, none below 100
           elements: the small cases pick their seed so).
  NORM     h = bf16(x + residual) has every entry in {+1, -1}, eps = 1e-6, an integer norm weight in [-4, 4]: sumsq / K == 1,
           rstd = 0.9999995 in fp32, bf16(h rstd) = +-1, so the normalised row is +-w[k] EXACTLY (asserted against
           rowwise.add_rmsnorm_ref, none in its window) and the probe applies unchanged; h_out must equal h bit for bit.
  SCORE    the index variant with every |logit| <= 256 (asserted): the bf16 logits ARE the integers, ties for the row maximum are
           common; top1 must be scoring.ref_logprob's (the lowest index), logprob and lse go through scoring.judge.

`instantiation` restates the dispatch of linear_small_m.hip, SMALL_M lists cases in which all 60 template instantiations occur
(tests/test_projections_cpu.py asserts it), M256 / SCORE list the 256-row shapes.  The fp32 emulations at the end are what
test_projections_cpu.py feeds the judges: the honest one (two summation orders) passes, each wrong one is reported.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import torch

import rowwise as rw
import scoring

BF = torch.bfloat16
NORM_EPS = 1e-6
INDEX_STD, TIES_STD, GATE_STD = 48.0, 300.0, 6.0
INDEX_MAX_SHARE, TIES_MIN_SHARE = 0.01, 0.10


def instantiation(M: int, N: int, K: int, glu: bool, norm: bool) -> Tuple[int, int, bool, bool, int]:
    """(M, RPW, GLU, NORM, NIT) of the linear_small_m_kernel instantiation a call reaches.  This RESTATES lsm_dispatch (rows per
    wave from N: plain 1 / 2 / 4 below 4096 / below 8192 / from 8192, GLU 1 / 2 below / from I = 4096) and launch_lsm (M = 1 .. 4;
    the NORM form stages NIT = 1 vector per thread up to K = 2048, else 2) of csrc/linear_small_m.hip: keep the two in step.
    NIT = 0 without NORM (the parameter is unused there)."""
    assert 1 <= M <= 4
    rpw = (2 if N >= 4096 else 1) if glu else (4 if N >= 8192 else 2 if N >= 4096 else 1)
    return M, rpw, bool(glu), bool(norm), ((1 if K <= 2048 else 2) if norm else 0)


ALL_INSTANTIATIONS = frozenset((M, rpw, glu, norm, nit) for M in (1, 2, 3, 4) for glu, rpws in ((False, (1, 2, 4)), (True, (1, 2)))
                               for rpw in rpws for norm, nits in ((False, (0,)), (True, (1, 2))) for nit in nits)

# =============================================================================================================================
# the case lists
# =============================================================================================================================
K_PLAIN = (8, 136, 512, 520, 2040, 2048, 2056, 4104)       # the weight loop advances by 2048 elements
K_NORM = (512, 520, 2040, 2048, 2056, 4088, 4096)          # NIT changes at 2048
# (glu, N or I): a column tail for every rows-per-wave -- 8195 = 3 mod 16 (RPW 4), 4099 = 3 mod 8 (RPW 2), 4097 (GLU, RPW 2), 7 and 5 (RPW 1)
TAILS = ((False, 7), (False, 4099), (False, 8195), (True, 5), (True, 4097))


def _small_m_list() -> List[Tuple[bool, bool, int, int, Tuple[int, ...], str]]:
    """(glu, norm, N, K, Ms, variant).  Every K with every tail N, at M = 1 and 4 -- all of M = 1 .. 4 at the narrow N, and at the
    wide ones at K = 520 (and K = 4096 with NORM: NIT = 2), which completes the instantiations.  A K above 2048 meets RPW 2 in
    the plain form only (N = 4099), but for NORM at K = 4096, which the GLU RPW 2 NIT 2 instantiations need.  The ties variant:
    plain, every K >= 64 at N = 7, and one wide N per RPW > 1."""
    out = []
    for norm, Ks in ((False, K_PLAIN), (True, K_NORM)):
        for glu, N in TAILS:
            for K in Ks:
                if glu and N > 100 and K > 2048 and not (norm and K == 4096):
                    continue
                every_m = N < 100 or K == 520 or (norm and K == 4096)
                out.append((glu, norm, N, K, (1, 2, 3, 4) if every_m else (1, 4), "index"))
    out += [(False, False, 7, K, (1, 2, 3, 4), "ties") for K in K_PLAIN if K >= 64]
    out += [(False, False, 4099, 520, (1, 4), "ties"), (False, False, 8195, 136, (1, 4), "ties")]
    return out


SMALL_M = _small_m_list()


def _m256_list(glu: bool) -> List[Tuple[int, int, int]]:
    """(M, N or I, K): K = 64, 128, 192, 256, 2048 are 1, 2, 3, 4 and 32 K-tiles against the three-stage ring (prologue only, the
    first wrap, the steady state); N around the 64 (GLU: 48) columns of a workgroup; M around the 32 rows of a wave and the 256 of
    the call.  Every N with K = 192 and K = 2048, every M twice among those, the other K with one (M, N) each."""
    Ns = (4, 44, 48, 52, 100) if glu else (4, 60, 64, 68, 100)
    Ms = (1, 31, 33, 255, 256)
    out = []
    for i, N in enumerate(Ns):
        out += [(Ms[i], N, 192), (Ms[(i + 2) % 5], N, 2048)]
    out += [(33, Ns[3], 64), (255, Ns[1], 128), (31, Ns[4], 256)]
    return out


M256_PLAIN, M256_GLU = _m256_list(False), _m256_list(True)
SCORE = [(M, N, K) for N in (4, 64, 68, 4100) for M in (1, 33, 256) for K in (64, 192)]
GDN_OUT = [(H, N) for H in (2, 3, 5, 16) for N in (7, 2048)]          # H = 2, 3: fewer heads than waves


# =============================================================================================================================
# builders
# =============================================================================================================================
def exact_sum(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [M,K] w [R,K] -> x w^T in float64 (4096 weight rows at a time)"""
    xd = x.double()
    return torch.cat([xd @ w[r:r + 4096].double().T for r in range(0, w.shape[0], 4096)], 1)


def ternary(rows: int, K: int, density: float, g_: torch.Generator) -> torch.Tensor:
    """[rows, K] bf16 in {-1, 0, +1}: +1 and -1 with probability density / 2 each"""
    u = torch.rand(rows, K, generator=g_)
    return ((u < density / 2).to(BF) - (u >= 1.0 - density / 2).to(BF))


def is_tie(v: torch.Tensor) -> torch.Tensor:
    """float64 values that lie exactly half way between two adjacent bf16 values"""
    q = v.abs() / rw.bf_spacing(v)
    return (q - q.floor()) == 0.5


def ties_amplitude(K: int, density: float = 0.9) -> int:
    """A with K * density * A (A + 1) / 3 (the variance of a sum of K terms +-x, x uniform in [-A, A]) about TIES_STD^2"""
    return max(1, min(200, int((-1.0 + math.sqrt(1.0 + 12.0 * TIES_STD ** 2 / (K * density))) / 2.0)))


def conditions(c: Dict, rows: int) -> Optional[str]:
    """the probe's conditions on the first `rows` rows of a case (= one call), with the bias and without; None = they hold"""
    for b in (None, c["bias"]):
        v = c["S"][:rows] + (0.0 if b is None else b.double())
        if c["variant"] == "ties":
            share = float(is_tie(v).double().mean())
            if not (share >= TIES_MIN_SHARE and float(v.abs().max()) < 2048.0):
                return f"ties: share {share:.3f}, max |sum| {float(v.abs().max())}"
        else:
            share = float((v.abs() > 256.0).double().mean())
            if share > INDEX_MAX_SHARE:
                return f"index: {share:.4f} of the elements have |sum| > 256"
        if c.get("score") and float(v.abs().max()) > 256.0:
            return f"score: |logit| up to {float(v.abs().max())}"
        if c["glu"] and not rw.window_ok(rw.silu_ref(rw.round_bf16(v).to(BF))["window"]):
            return "glu: too many elements in the silu window"
    return None


def _seeded(build: Callable[[int], Dict], Ms, small: bool) -> Dict:
    """the first seed whose case meets the conditions for every M of the list (small cases; a large one must meet them at once)"""
    why = None
    for try_ in range(64 if small else 1):
        c = build(try_)
        why = next((w_ for w_ in (conditions(c, M) for M in Ms) if w_), None)
        if why is None:
            return c
    raise AssertionError(f"no seed meets the probe's conditions: {why}")


def int_case(rows: int, N: int, K: int, glu: bool = False, variant: str = "index", Ms=None, score: bool = False) -> Dict:
    """x [rows,K], w [N,K] (GLU: [2N,K], gate rows first), bias [N] / [2N], S = the exact float64 sums [rows, N / 2N]"""
    assert variant == "index" or (K >= 64 and not glu)
    R = 2 * N if glu else N

    def build(try_: int) -> Dict:
        g_ = rw.gen(K * 100003 + N * 17 + rows * 3 + glu + 2 * (variant == "ties") + 4 * score + 7919 * try_)
        if variant == "ties":
            A, dens = ties_amplitude(K), 0.9
        else:
            A, dens = 3, min(1.0, INDEX_STD ** 2 / (4.0 * K))              # var(x) = 4
        x = torch.randint(-A, A + 1, (rows, K), generator=g_).to(BF)
        w = ternary(R, K, dens, g_)
        if glu:
            w[:N] = ternary(N, K, min(1.0, GATE_STD ** 2 / (4.0 * K)), g_)
        bias = torch.randint(-4, 5, (R,), generator=g_).to(BF)
        return dict(x=x, w=w, bias=bias, S=exact_sum(x, w), N=N, K=K, glu=glu, variant=variant, score=score)
    return _seeded(build, Ms or (rows,), rows * R <= 32768)


def norm_case(N: int, K: int, glu: bool, Ms=(1, 2, 3, 4)) -> Dict:
    """4 rows: h in {+1, -1}, x integers in [-3, 3], residual = h - x; norm weight integers in [-4, 4] (variance 20 / 3);
    xn = h * nw is the normalised row the kernel must form, S = xn w^T"""
    R = 2 * N if glu else N

    def build(try_: int) -> Dict:
        g_ = rw.gen(K * 100003 + N * 17 + glu + 8 + 7919 * try_)
        h = (2 * torch.randint(0, 2, (4, K), generator=g_) - 1).to(BF)
        x = torch.randint(-3, 4, (4, K), generator=g_).to(BF)
        res = (h.float() - x.float()).to(BF)
        nw = torch.randint(-4, 5, (K,), generator=g_).to(BF)
        w = ternary(R, K, min(1.0, INDEX_STD ** 2 / (20.0 / 3.0 * K)), g_)
        if glu:
            w[:N] = ternary(N, K, min(1.0, GATE_STD ** 2 / (20.0 / 3.0 * K)), g_)
        bias = torch.randint(-4, 5, (R,), generator=g_).to(BF)
        xn = (h.float() * nw.float()).to(BF)
        return dict(x=x, res=res, h=h, nw=nw, eps=NORM_EPS, xn=xn, w=w, bias=bias, S=exact_sum(xn, w), N=N, K=K, glu=glu, variant="index")
    c = _seeded(build, Ms, 4 * R <= 32768)
    for x, res in ((c["x"], c["res"]), (c["h"], None)):                    # the identity the NORM probe rests on, in float64
        m = rw.add_rmsnorm_ref(x, res, c["nw"], NORM_EPS)
        assert not bool(m["window"].any()) and torch.equal(m["model"], c["xn"].double()) and torch.equal(m["h"], c["h"].double())
    return c


def score_case(M: int, N: int, K: int) -> Dict:
    """the index variant with targets in the first column, the last column, the first column of the last (tail) 64-column block,
    one anywhere, and one row that is not scored (-100)"""
    c = int_case(M, N, K, score=True)
    g_ = rw.gen(M + N + K)
    fixed = torch.tensor([0, N - 1, (N - 1) // 64 * 64, -100])
    t = torch.randint(0, N, (M,), generator=g_)
    pick = torch.arange(M) % 5
    c["target"] = torch.where(pick < 4, fixed[pick.clamp(max=3)], t).to(torch.int64)
    return c


def randn_case(rows: int, N: int, K: int, glu: bool) -> Dict:
    """unit randn x, weights of variance 1 / K (GLU: gate rows twice that), a randn bias"""
    R = 2 * N if glu else N
    g_ = rw.gen(K * 7 + N * 3 + rows + glu)
    x = torch.randn(rows, K, generator=g_).to(BF)
    w = torch.randn(R, K, generator=g_) * K ** -0.5
    if glu:
        w[:N] *= 2.0
    return dict(x=x, w=w.to(BF), bias=torch.randn(R, generator=g_).to(BF), N=N, K=K, glu=glu)


def gdn_out_case(H: int, N: int) -> Dict:
    """one decode step's buffers for 4 rows: proj [4, ld] = q | k | 4 spare | gate | 8 spare, so that the gate starts 8 bytes (not 16)
    into a row and ld = 4 mod 8 (> H * 256, a multiple of 4 and not of 8); o_raw [4, H * 256]; conv states [4, H * 128, 4]"""
    Dq, Dv = H * 128, H * 256
    col_q, col_k, col_g = 0, Dq, 2 * Dq + 4
    ld = col_g + Dv + 8
    assert ld > Dv and ld % 4 == 0 and ld % 8 != 0
    g_ = rw.gen(H * 100 + N)
    rn = lambda *sh: torch.randn(*sh, generator=g_)      # noqa: E731
    return dict(H=H, N=N, ld=ld, col_q=col_q, col_k=col_k, col_g=col_g, proj=rn(4, ld).to(BF), o_raw=(2.0 * rn(4, Dv)).to(BF),
                cq=rn(4, Dq, 4).to(BF), ck=rn(4, Dq, 4).to(BF), nw=rw.weight(256, g_), eps=1e-5,
                w=(rn(N, Dv) * Dv ** -0.5).to(BF), bias=rn(N).to(BF))


def conv_shift_ref(state: torch.Tensor, new: torch.Tensor) -> torch.Tensor:
    """state [M, D, 4], new [M, D]: taps 1 .. 3, then the step's raw projection value"""
    return torch.cat([state[..., 1:], new[..., None]], -1)


# =============================================================================================================================
# judges: `run` is the implementation under test (CPU tensors in, CPU tensors out)
# =============================================================================================================================
def _judge(rep: "Counted", tag, y: torch.Tensor, v: torch.Tensor, glu: bool):
    """y against the exact sums + bias `v` of the call"""
    N = v.shape[-1] // 2 if glu else v.shape[-1]
    if y is None or tuple(y.shape) != (v.shape[0], N):
        rep.fails.append((tag, "missing output / wrong shape"))
    elif glu:
        rep.double(tag, y, rw.silu_ref(rw.round_bf16(v).to(BF)))
    else:
        rep.exact(tag, y, rw.round_bf16(v))
        rep.probed += y.numel()


class Counted(rw.Report):
    """a Report that also counts the elements that went through the bit-for-bit judge"""

    def __init__(self, what: str):
        super().__init__(what)
        self.probed = 0

    def __str__(self):
        return super().__str__() + f"; {self.probed} elements bit for bit"


def check_linear(run, c: Dict, Ms, biases=(False, True)) -> Counted:
    """run(x, w, bias or None, glu) -> y [M, N]: every M of the list (the case's first M rows), with the bias and without"""
    rep = Counted(f"{'glu' if c['glu'] else 'plain'} {c['variant']} N={c['N']} K={c['K']}")
    for M in Ms:
        why = conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in biases:
            y = run(c["x"][:M], c["w"], c["bias"] if wb else None, c["glu"])
            _judge(rep, (M, "bias" if wb else ""), y, c["S"][:M] + (c["bias"].double() if wb else 0.0), c["glu"])
    return rep


def check_norm_linear(run, c: Dict, Ms) -> Counted:
    """run(x, residual or None, norm weight, eps, w, bias or None, glu) -> (y, h_out or None)"""
    rep = Counted(f"norm {'glu' if c['glu'] else 'plain'} N={c['N']} K={c['K']}")
    for M in Ms:
        why = conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in (False, True):
            for wr in (False, True):
                y, h = run((c["x"] if wr else c["h"])[:M], c["res"][:M] if wr else None, c["nw"], c["eps"], c["w"],
                           c["bias"] if wb else None, c["glu"])
                tag = (M, "bias" if wb else "", "residual" if wr else "")
                _judge(rep, tag, y, c["S"][:M] + (c["bias"].double() if wb else 0.0), c["glu"])
                if wr:
                    rep.exact(tag + ("h_out",), h, c["h"][:M].double())
    return rep


def check_score(run, c: Dict) -> Counted:
    """run(x, w, bias or None, target) -> (logprob fp32, top1 int64, lse fp32); rep.worst = the largest scoring.judge ratio"""
    M = c["x"].shape[0]
    rep = Counted(f"score M={M} N={c['N']} K={c['K']}")
    why = conditions(c, M)
    if why:
        rep.fails.append(("conditions", why))
    for wb in (False, True):
        logits = rw.round_bf16(c["S"] + (c["bias"].double() if wb else 0.0))          # exact integers
        lp_ref, top_ref, lse_ref = scoring.ref_logprob(logits, c["target"])
        lp, top1, lse = run(c["x"], c["w"], c["bias"] if wb else None, c["target"])
        if not torch.equal(top1, top_ref):
            r = int((top1 != top_ref).nonzero()[0])
            rep.fails.append((wb, f"top1 differs in {int((top1 != top_ref).sum())} rows; row {r}: got {int(top1[r])}, lowest index of the "
                                  f"maximum {int(top_ref[r])}"))
        rep.probed += M
        for name, got, ref in (("logprob", lp, lp_ref), ("lse", lse, lse_ref)):
            try:
                rep.worst = max(rep.worst, scoring.judge(got, ref, name))
            except AssertionError as e:
                rep.fails.append(((wb, name), str(e)))
    return rep


def randn_tolerance(ref: torch.Tensor) -> torch.Tensor:
    """the project's bound for a bf16 projection output against float64 (test_linear_small_m_vs_fp32)"""
    return ref.abs() * 2.0 ** -8 + 1e-5


def check_randn(run, c: Dict, Ms) -> Counted:
    """plain: |y - float64| <= |ref| 2^-8 + 1e-5 per element.  GLU: the gate of the kernel's OWN plain output on the fused weight,
    rowwise.silu_ref per element (the plain output itself is judged as above)"""
    rep = Counted(f"randn {'glu' if c['glu'] else 'plain'} N={c['N']} K={c['K']}")
    for M in Ms:
        for wb in (False, True):
            b = c["bias"] if wb else None
            gu = run(c["x"][:M], c["w"], b, False)
            ref = exact_sum(c["x"][:M], c["w"]) + (b.double() if wb else 0.0)
            ratio = (gu.double() - ref).abs() / randn_tolerance(ref)
            worst, idx = rw._where(ratio)
            if worst > rep.worst:
                rep.worst, rep.where = worst, ((M, wb), idx, float(gu.double()[idx]), float(ref[idx]))
            if not worst <= 1.0:
                rep.fails.append(((M, wb), f"error / bound {worst} at {idx}"))
            if c["glu"]:
                rep.double((M, wb, "glu"), run(c["x"][:M], c["w"], b, True), rw.silu_ref(gu))
    return rep


# =============================================================================================================================
# fp32 emulations (test_projections_cpu.py): `order` = two different summation orders, `wrong` = a deliberate defect
# =============================================================================================================================
WRONG_LINEAR = ("drop_last_piece", "double_last_piece", "tail_clamped", "swap_rows", "bias_prev", "truncate")
WRONG_GLU = ("up_off_by_one", "glu_bias_gate")
WRONG_NORM = ("norm_reads_x", "norm_row0")


def _fp32_sums(x: torch.Tensor, w: torch.Tensor, order: int) -> torch.Tensor:
    xf, wf = x.float(), w.float()
    if order == 0:
        return xf @ wf.T
    # the kernel's order: lane l of 64 adds the 8-element pieces l, l + 64, ... of a row, then the 64 partial sums meet
    M, K = xf.shape
    pad = (-K) % 512
    xf, wf = torch.nn.functional.pad(xf, (0, pad)), torch.nn.functional.pad(wf, (0, pad))
    part = torch.einsum("mtlk,ntlk->mnl", xf.view(M, -1, 64, 8), wf.view(wf.shape[0], -1, 64, 8))
    return part.flip(-1).sum(-1)


def emu_linear(x, w, bias, glu, wrong: str = "", order: int = 0) -> torch.Tensor:
    s = _fp32_sums(x, w, order)
    if wrong == "drop_last_piece":                       # the last 16-byte piece of every row missing
        s = s - x[:, -8:].float() @ w[:, -8:].float().T
    elif wrong == "double_last_piece":                   # ... counted twice: the clamp without the zeroing
        s = s + x[:, -8:].float() @ w[:, -8:].float().T
    R = w.shape[0]
    N = R // 2 if glu else R
    b = torch.zeros(R) if bias is None else bias.float()
    if wrong == "bias_prev":
        b = b.roll(1)
    if wrong == "glu_bias_gate" and glu:
        b = torch.cat([b[:N], b[:N]])
    if wrong == "up_off_by_one" and glu:
        s = torch.cat([s[:, :N], s[:, N:].roll(-1, 1)], 1)
    v = s + b
    if wrong == "truncate":
        v = (v.view(torch.int32) & -65536).view(torch.float32)
    y = rw.emu_silu_mul(v.to(BF)) if glu else v.to(BF)
    if wrong == "tail_clamped" and N > 1:                # the last column computed from the row the clamp stops at one early
        y = y.clone()
        y[:, N - 1] = y[:, N - 2]
    if wrong == "swap_rows" and y.shape[0] > 1:
        y = y[[1, 0] + list(range(2, y.shape[0]))]
    return y


def emu_norm_linear(x, res, nw, eps, w, bias, glu, wrong: str = "", order: int = 0):
    xn, h = rw.emu_add_rmsnorm(x, None if wrong == "norm_reads_x" else res, nw, eps)
    if wrong == "norm_row0":
        xn = xn[:1].expand_as(xn)
    h_out = None if res is None else (x.float() + res.float()).to(BF)
    return emu_linear(xn, w, bias, glu, "", order), h_out


def emu_score(x, w, bias, target, wrong: str = "", order: int = 0):
    """the kernel's arithmetic: bf16 logits; per 64-column block m_j and an fp32 sum of exp(x - m_j); a float64 combine; fp32 log"""
    xl = emu_linear(x, w, bias, False, "", order).float()
    M, N = xl.shape
    m = xl.max(1).values
    at_max = xl == m[:, None]
    top1 = (N - 1 - at_max.flip(1).to(torch.int64).argmax(1)) if wrong == "top1_highest" else at_max.to(torch.int64).argmax(1)
    xb = torch.nn.functional.pad(xl, (0, (-N) % 64), value=float("-inf")).view(M, -1, 64)
    mj = xb.max(2).values
    zj = torch.exp(xb - mj[:, :, None]).sum(2)
    Z = (zj.double() * torch.exp(mj.double() - m.double()[:, None])).sum(1)
    lz = torch.log(Z.float())
    scored = (target >= 0) & (target < N)
    xt = xl.gather(1, target.clamp(0, N - 1)[:, None])[:, 0]
    lp = torch.where(scored, torch.where(xt == m, torch.zeros_like(xt), xt - m) - lz, torch.zeros_like(xt))
    return lp, top1, m + lz

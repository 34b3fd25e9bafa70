"""Input builders, float64 references and PER-ELEMENT judges for the row-wise kernels every bit-for-bit chain of the GPU suite
ends in (CPU only, pure torch / numpy):

  ivl_add_rmsnorm_fwd                                      h = bf16(x + r);  y = bf16(w * bf16(h * rstd))         double rounding
  ivl_silu_mul_fwd                                         y = bf16(bf16(silu(a)) * b)                            double rounding
  ivl_rmsnorm_swish_gate_fwd / _strided_fwd / _res_fwd     y = bf16(row * rstd * w [* g * sigmoid(g)])            single rounding
  ivl_short_conv_fwd / _bias_fwd, ivl_gdn_prologue_fwd     y = bf16(act(bias + sum_j w_j ext[t + 1 + j]))         single rounding

Every reference evaluates the header's formula in float64 on the bf16 inputs and rounds only where the header says the kernel
rounds.  No tolerance here is a whole-tensor figure; every bound is derived (below), none is fitted to a kernel.

SINGLE rounding (judge_single):   |got - ref| <= half the bf16 spacing at ref + noise + floor        (ref = the UNROUNDED float64)
  the spacing is the wider one when |ref| is within 2^-9 below a power of two (the fp32 value may sit in the next binade);
  noise = delta * scale:
    norms   delta = D_NORM = 2^-18, scale = |ref|: mean square = 32-term fma chain + tree (about 41 * 2^-24), halved by the
            square root, + sqrt, division and the products (4 * 2^-24): about 27 * 2^-24 = 2^-19.2, with a 2 x margin;
    fast sigmoid rcp(1 + __expf(-g)): + d_sigmoid(g) = 2^-21 + |g| 2^-23 (1 ulp each for the hardware exp and reciprocal per the
            ISA manual, + the fp32 rounding of the exp argument, |g| 2^-24 relative on the exponential; all doubled);
    conv    D_CONV = 2^-21 on scale = |bias| + sum_j |w_j x_j| (four products may cancel): 4 roundings of at most 2^-24 * scale
            each = 2^-22, doubled.  With SiLU the pre-activation error passes through |silu'(a)| (+ 2^-10 for its curvature) and
            the product a * sigmoid(a) adds (d_sigmoid(a) + 2^-23) |ref|;
    gates   beta = bf16(1 / (1 + expf(-b))): D_BETA = 2^-21 (expf 1 .. 2 ulp, add, IEEE division: under 4 * 2^-24, doubled);
            g = -expf(A_log) * softplus(a + dt_bias) in fp32 (judge_fp32): (2^-20 + |a + dt| 2^-23) |ref| -- three libm calls of
            1 .. 2 ulp, an add and a product (about 6 * 2^-24, doubled) + the fp32 rounding of a + dt_bias, which moves
            softplus by up to |a + dt| 2^-24 RELATIVE where softplus ~ e^(a + dt) -- and an absolute 2^-126 (e^A + 1): an fp32
            subnormal intermediate may be flushed;
  floor = 2^-120 |x_hat w| for GATED norm outputs only (e^88.7 overflows fp32: below that the fast path returns +-0).

DOUBLE rounding (judge_double): the outer product of two bf16 values is exact in fp32, so the result must be BIT-EQUAL to the
  float64 model, except where the inner value lies within relative `delta` of a bf16 rounding boundary: there it must equal the
  model evaluated with the OTHER neighbour.  delta: D_NORM for add_rmsnorm (rsqrt of the hardware: 1 ulp, inside the margin);
  d_sigmoid(a) + 2^-23 (the product a * sigmoid(a), doubled) for silu_mul.  The share of elements inside the window (`share`)
  must stay under EXCUSED_MAX = 1 % in EVERY case (every single call judged, not a pool of them; Report.double asserts it from the
  float64 model alone, so test_rowwise_cpu.py asserts it for every input set); a case of fewer than 100 elements, where one
  element is already more than 1 %, must have NO element in the window.  The builders of the small cases pick their seed so.
  h_out, the residual-out of the gated norm and the conv states have no window: bit for bit.
No output may hold a non-finite value; zeros compare by value (-0 == +0).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

BF = torch.bfloat16
D_NORM = 2.0 ** -18
D_CONV = 2.0 ** -21
D_BETA = 2.0 ** -21
GATED_FLOOR = 2.0 ** -120
EXCUSED_MAX = 0.01
SWEEP = (0.0, 2.0 ** -7, -2.0 ** -7, 1.0, -1.0, 20.0, -20.0, 60.0, -60.0, 88.0, -88.0, 100.0, -100.0)      # all exact in bf16


def d_sigmoid(g: torch.Tensor) -> torch.Tensor:
    return 2.0 ** -21 + g.abs().double() * 2.0 ** -23


def f32(v: float) -> float:
    """a Python float as the kernel receives it (float argument)"""
    return float(np.float32(v))


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# =============================================================================================================================
# the bf16 grid in float64
# =============================================================================================================================
def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as float64, exactly (e int64, -1022 <= e <= 1023), through the exponent field"""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def bf_spacing(x: torch.Tensor, widen: bool = False) -> torch.Tensor:
    """distance between adjacent bf16 values at |x| (2^-133 in the subnormal range and at 0); widen: the spacing of the next
    binade when |x| is within 2^-9 (relative) below a power of two"""
    m, e = torch.frexp(x.abs().double())
    e = e.to(torch.int64)
    if widen:
        e = e + (m >= 1.0 - 2.0 ** -9).to(torch.int64)
    e = torch.where(m == 0, torch.full_like(e, -1000), e)
    return _pow2(torch.clamp(e - 8, min=-133))


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """float64 -> nearest bf16 (ties to even) in ONE rounding, kept as float64 (torch's own cast goes through fp32)"""
    s = bf_spacing(x)
    return torch.round(x.double() / s) * s


def other_neighbour(inner: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """r = round_bf16(inner): the bf16 value on the other side of `inner`"""
    a, ar = inner.abs(), r.abs()
    s = bf_spacing(ar)
    m, _ = torch.frexp(ar)
    down = torch.where((m == 0.5) & (s > 2.0 ** -133), s / 2, s)
    return torch.copysign(torch.where(a >= ar, ar + s, ar - down), inner)


# =============================================================================================================================
# judges
# =============================================================================================================================
def _where(ratio: torch.Tensor) -> Tuple[float, Tuple[int, ...]]:
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


def judge_single(got: torch.Tensor, ref: torch.Tensor, noise: torch.Tensor, floor=0.0) -> Dict:
    """per element |got - ref| / (half spacing at ref + noise + floor); a non-finite output counts as inf.
    -> worst ratio (<= 1 passes), its index, and what sits there."""
    g = got.double()
    half = 0.5 * bf_spacing(ref, widen=True)
    bound = half + noise + floor
    err = (g - ref).abs()
    ratio = torch.where(torch.isfinite(g), err / bound, torch.full_like(ref, float("inf")))
    worst, idx = _where(ratio)
    # the share of the fp32 allowance (noise + floor) an element needs beyond the half spacing every correct rounding may use:
    # <= 0 everywhere = indistinguishable from exact arithmetic followed by one rounding
    # (elements with no allowance at all -- exact zeros -- have nothing to use and are left out; nan = there is no other element)
    allow = bound - half
    has = (allow > 0) & torch.isfinite(g)
    used = float(((err - half)[has] / allow[has]).max()) if bool(has.any()) else float("nan")
    return dict(worst=worst, where=idx, got=float(g[idx]), ref=float(ref[idx]), bound=float(bound[idx]), used=used)


def judge_fp32(got: torch.Tensor, ref: torch.Tensor, noise: torch.Tensor) -> Dict:
    """an fp32 output: |got - ref| / (half the fp32 spacing at ref + noise)"""
    g = got.double()
    _, e = torch.frexp(ref.abs())
    bound = _pow2(torch.clamp(e.to(torch.int64) - 25, min=-150)) + noise
    ratio = torch.where(torch.isfinite(g), (g - ref).abs() / bound, torch.full_like(ref, float("inf")))
    worst, idx = _where(ratio)
    return dict(worst=worst, where=idx, got=float(g[idx]), ref=float(ref[idx]), bound=float(bound[idx]))


def double_model(inner: torch.Tensor, outer: Callable[[torch.Tensor], torch.Tensor], delta) -> Dict:
    """the float64 model of bf16(outer(bf16(inner))): `model`, the alternative `alt` with the inner value's other neighbour,
    `window` = the elements whose inner value lies within relative delta of the rounding boundary, `share` of them"""
    r = round_bf16(inner)
    o = other_neighbour(inner, r)
    window = ((r + o) / 2 - inner).abs() <= delta * inner.abs()
    return dict(model=round_bf16(outer(r)), alt=round_bf16(outer(o)), window=window, share=float(window.double().mean()))


def judge_double(got: torch.Tensor, m: Dict, limit: int = 5) -> Dict:
    """-> bad: number of elements that are neither the model nor (inside the window) the alternative; the first of them;
    excused: the share of elements that ARE the alternative (at most `share`)"""
    g = got.double()
    alt_ok = m["window"] & (g == m["alt"])
    ok = torch.isfinite(g) & ((g == m["model"]) | alt_ok)
    bad = (~ok).nonzero()
    first = [(tuple(i.tolist()), float(g[tuple(i)]), float(m["model"][tuple(i)]), float(m["alt"][tuple(i)]), bool(m["window"][tuple(i)]))
             for i in bad[:limit]]
    return dict(bad=int(bad.shape[0]), first=first, share=m["share"], excused=float((alt_ok & (g != m["model"])).double().mean()))


def exact_mismatches(got: torch.Tensor, ref: torch.Tensor, limit: int = 5) -> List:
    """bit for bit by VALUE (float64 view; -0 == +0), non-finite = mismatch -> the first differing (index, got, expected)"""
    g, r = got.double(), ref.double()
    bad = (~(torch.isfinite(g) & (g == r))).nonzero()
    return [(tuple(i.tolist()), float(g[tuple(i)]), float(r[tuple(i)])) for i in bad[:limit]]


# =============================================================================================================================
# magnitude classes
# =============================================================================================================================
CLASSES = ("randn", "zero", "tiny", "large", "outlier")


def magnitude_rows(rows: int, N: int, g_: torch.Generator, first: int = 0) -> torch.Tensor:
    """[rows, N] bf16; row i is of class CLASSES[(i + first) % 5]: unit randn / all zero / 2^-40 scale (eps decides rstd) / 2^50 /
    one 2^20 outlier among 2^-10 noise"""
    x = torch.randn(rows, N, generator=g_)
    cls = (torch.arange(rows) + first) % 5
    x[cls == 1] = 0.0
    x[cls == 2] *= 2.0 ** -40
    x[cls == 3] *= 2.0 ** 50
    x[cls == 4] *= 2.0 ** -10
    r = (cls == 4).nonzero().flatten()
    x[r, (r * 7 + 3) % N] = 2.0 ** 20
    return x.to(BF)


def sweep_mix(rows: int, N: int, g_: torch.Generator, scale: float = 2.0) -> torch.Tensor:
    """[rows, N] bf16 gates: even rows scale * randn, odd rows walk SWEEP (0, +-2^-7, +-1, +-20, +-60, +-88, +-100); a single
    row is randn in its first half and walks SWEEP in its second"""
    x = scale * torch.randn(rows, N, generator=g_)
    sw = torch.tensor(SWEEP)[(torch.arange(rows)[:, None] + torch.arange(N)[None, :]) % len(SWEEP)]
    odd = (torch.arange(rows) % 2 == 1)[:, None].expand(rows, N)
    if rows == 1:
        odd = (torch.arange(N) >= N // 2)[None, :]
    return torch.where(odd, sw, x).to(BF)


def weight(N: int, g_: torch.Generator) -> torch.Tensor:
    return (1.0 + 0.5 * torch.randn(N, generator=g_)).to(BF)


def next_bf16(x: torch.Tensor) -> torch.Tensor:
    """the bf16 value one step further from zero (0 stays 0)"""
    bits = x.to(BF).view(torch.int16)
    return torch.where(x == 0, bits, bits + 1).view(BF)


# =============================================================================================================================
# add_rmsnorm
# =============================================================================================================================
ADD_N = (8, 16, 264, 2040, 2048, 2056, 4096, 4104, 6144, 6152, 8184, 8192)      # 256 threads x 4 vectors of 8: `it` changes at 2048 k
ADD_ROWS = (1, 3, 67)
ADD_EPS = 1e-6


def window_ok(window: torch.Tensor) -> bool:
    """the excuse-window rule of one case: no element of fewer than 100, else at most EXCUSED_MAX of them"""
    n, k = window.numel(), int(window.sum())
    return k == 0 if n < 100 else k <= EXCUSED_MAX * n


def add_rmsnorm_case(N: int, rows: int, with_res: bool, try_: Optional[int] = None) -> Dict:
    """x (+ residual) of mixed magnitude classes; with a residual, rows cycle through an independent residual of the row's class,
    x = -residual exactly (h = 0) and x = -residual but for one bf16 step (h = one ulp of x: all cancellation)"""
    if try_ is None:
        # small cases: the first seed whose float64 model meets the excuse-window rule (none below 100 elements, else <= 1 %)
        for try_ in range(64 if rows * N <= 32768 else 1):
            c = add_rmsnorm_case(N, rows, with_res, try_)
            if rows * N > 32768 or window_ok(add_rmsnorm_ref(**c)["window"]):
                break
        return c
    first = ADD_N.index(N) if N in ADD_N else N
    g_ = gen(1000 * N + 10 * rows + with_res + 7919 * try_)
    x = magnitude_rows(rows, N, g_, first)
    res = None
    if with_res:
        res = magnitude_rows(rows, N, g_, first)
        mode = ((torch.arange(rows) + first) // 5) % 3
        res[mode == 1] = -x[mode == 1]
        res[mode == 2] = -next_bf16(x[mode == 2])
        if rows == 1 and first % 3:                   # a single row: let the N sweep reach the cancelling forms too
            res = -x if first % 3 == 1 else -next_bf16(x)
    return dict(x=x, res=res, w=weight(N, g_), eps=ADD_EPS)


def add_rmsnorm_ref(x: torch.Tensor, res: Optional[torch.Tensor], w: torch.Tensor, eps: float) -> Dict:
    """h (exact: the sum of two bf16 values needs at most 24 bits whenever it lands near a bf16 tie, so bf16(fp32 sum) is a single
    rounding) and the double-rounding model of y"""
    h = x.double() if res is None else round_bf16(x.double() + res.double())
    inner = h * torch.rsqrt((h * h).mean(-1, keepdim=True) + f32(eps))
    wd = w.double()
    m = double_model(inner, lambda r: wd * r, D_NORM)
    m["h"] = h
    return m


def onehot_rows(N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The statistics probe: row i = 64 e_c(i), c over one position of every 8-vector (walking the lane: 8 v + v % 8) and every
    position of the first and the last vector.  mean(x^2) = 4096 / N: y_c = w_c * bf16(sqrt(N) (1 - eps N / 8192)) and exact zeros
    elsewhere; an element missing from the sum of squares turns rstd into eps^-1/2: off by hundreds of times."""
    c = sorted({8 * v + v % 8 for v in range(N // 8)} | set(range(8)) | set(range(N - 8, N)))
    c = torch.tensor(c)
    x = torch.zeros(len(c), N)
    x[torch.arange(len(c)), c] = 64.0
    return x.to(BF), c


# =============================================================================================================================
# gated / plain RMSNorm over rows of 256
# =============================================================================================================================
GATED_ROWS = (1, 7, 8, 9, 16389)          # 8 rows per workgroup, 2048 workgroups: 16384 rows are one sweep of the capped grid
GATED_VARIANTS = ("gated", "plain", "res_bf16", "res_fp32", "res_out_fp32")
GATED_EPS = 1e-5
STRIDED = [(H, tokens) for H in (1, 3, 16) for tokens in (1, 5, 1030)]


def first_classes(rows: int) -> Tuple[int, ...]:
    """the class index of row 0: a single row (the decode shape, the smallest partial workgroup) is run once per magnitude
    class -- one row of one class, the all-zero one say, would anchor nothing; longer cases hold every class anyway"""
    return tuple(range(len(CLASSES))) if rows == 1 else (rows % 5,)


def gated_case(rows: int, variant: str, first: int = 0) -> Dict:
    g_ = gen(7 * rows + GATED_VARIANTS.index(variant) + 1009 * first)
    x = magnitude_rows(rows, 256, g_, first)
    gate = None if variant == "plain" else sweep_mix(rows, 256, g_)
    res = None
    if variant in ("res_bf16", "res_fp32"):
        res = magnitude_rows(rows, 256, g_, first)
        mode = ((torch.arange(rows) + first) // 5) % 3
        res[mode == 1] = -x[mode == 1]
        res[mode == 2] = -next_bf16(x[mode == 2])
        if variant == "res_fp32":                      # fp32 values off the bf16 grid
            res = res.float() * (1.0 + 2.0 ** -12 * torch.randn(rows, 256, generator=g_))
    return dict(x=x, gate=gate, res=res, w=weight(256, g_), eps=GATED_EPS, variant=variant)


def strided_case(H: int, tokens: int, first: int = 0) -> Dict:
    """the gate inside a wider buffer: row stride gate_ld = off + H * 256 + pad (multiples of 8, off and pad non-zero)"""
    g_ = gen(100 * H + tokens + 1009 * first)
    off, pad = 8 * (1 + H % 3), 8 * (1 + tokens % 4)
    ld = off + H * 256 + pad
    x = magnitude_rows(tokens * H, 256, g_, first).view(1, tokens, H, 256)
    buf = sweep_mix(tokens, ld, g_)
    return dict(x=x, buf=buf, off=off, ld=ld, H=H, w=weight(256, g_), eps=GATED_EPS,
                gate=buf[:, off:off + H * 256].reshape(tokens * H, 256))


def gated_norm_ref(x: torch.Tensor, gate: Optional[torch.Tensor], w: torch.Tensor, eps: float, res: Optional[torch.Tensor] = None) -> Dict:
    """x [rows, 256] -> ref (float64, unrounded), noise, floor, row (the fp32 row x + residual: its one rounding point)"""
    row = x.double()
    if res is not None:
        row = (row + res.double()).float().double()
    xw = row * torch.rsqrt((row * row).mean(-1, keepdim=True) + f32(eps)) * w.double()
    if gate is None:
        return dict(ref=xw, noise=D_NORM * xw.abs(), floor=0.0, row=row)
    gd = gate.double()
    ref = xw * gd * torch.sigmoid(gd)
    return dict(ref=ref, noise=(D_NORM + d_sigmoid(gd)) * ref.abs(), floor=GATED_FLOOR * xw.abs(), row=row)


# =============================================================================================================================
# silu_mul
# =============================================================================================================================
SILU_SHAPES = ((1, 8), (3, 24), (35, 1376), (130, 32776), (520, 32776))       # the last two: > 524288 vectors; the last: > 32 MB out


def silu_case(rows: int, I: int) -> torch.Tensor:
    """gate|up [rows, 2 I] bf16: a = 2 randn, b = randn; from 35 rows on, the first 104 columns of the odd rows walk SWEEP instead.
    (silu(+-2^-7) = +-2^-8 (1 + 2^-8 - 2^-25.6) sits ON a bf16 tie as far as fp32 can tell, so those two sweep values are inside
    the excuse window by construction: 16 elements per odd row, which the 1 % condition has to absorb -- hence not in the small
    shapes, where one element is more than 1 %.)"""
    g_ = gen(rows * 31 + I)
    a = (2.0 * torch.randn(rows, I, generator=g_)).to(BF)
    if rows >= 35:
        a[1::2, :104] = sweep_mix(rows, 104, g_)[1::2]
    return torch.cat([a, torch.randn(rows, I, generator=g_).to(BF)], -1)


def silu_index_probe(rows: int, I: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """a = 64 (bf16(silu(64)) = 64: 1 - sigmoid(64) = 1.6e-28), b = a digit <= 255 of the element's place, by lane of its
    8-vector: the vector's index in the row (two digits), the row (two digits), the lane -> y = 64 * digit exactly
    -> (gate|up, expected y)"""
    v = (torch.arange(I // 8))[None, :]
    r = torch.arange(rows)[:, None]
    b = torch.empty(rows, I)
    for lane, digit in enumerate((v & 255, v >> 8, r & 255, r >> 8, 255, (v + r) & 255, 1, 7)):
        b[:, lane::8] = digit
    gu = torch.cat([torch.full((rows, I), 64.0), b], -1).to(BF)
    return gu, (64.0 * b).to(BF)


def silu_deep_case() -> torch.Tensor:
    """a = every bf16 value of [-110, -80] (61 values; 1 + e^-a overflows fp32 at -88.7, its reciprocal is an fp32 subnormal from
    -87.3 down; bf16(silu(a)) is a normal number down to a = -91.5, a subnormal down to -97 and 0 from -97.5 on), each against
    b = +-1, +-2^-7, +-100 and randn"""
    a = torch.arange(-110.0, -79.75, 0.5)
    g_ = gen(61)
    b = torch.cat([torch.tensor([1.0, -1.0, 2.0 ** -7, -2.0 ** -7, 100.0, -100.0]), torch.randn(58, generator=g_)])
    return torch.cat([a[:, None].expand(61, 64), b[None, :].expand(61, 64)], -1).to(BF).contiguous()


def silu_ref(gu: torch.Tensor) -> Dict:
    I = gu.shape[-1] // 2
    a, b = gu[..., :I].double(), gu[..., I:].double()
    return double_model(a * torch.sigmoid(a), lambda r: r * b, d_sigmoid(a) + 2.0 ** -23)


# =============================================================================================================================
# short conv (4 taps) and the GDN prologue
# =============================================================================================================================
CONV_T = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33)
CONV_D = (8, 24, 64)
CONV_B = (1, 3)
CONV_WRAP = (2, 520, 32776)           # 2 * 65 * 4097 = 532610 items > 2048 * 256 threads
# state_in given?, state_out: "aliased" (needs state_in) / "separate" / None
CONV_STATE_FORMS = ((True, "aliased"), (True, "separate"), (True, None), (False, "separate"), (False, None))


def conv_case(B: int, T: int, D: int, bias: bool, seed: int = 0) -> Dict:
    """x [B,T,D], w [D,1,4], state [B,D,4], bias [D] bf16.  Channels d % 8 == 1: one tap of 1 on the newest input, which walks
    SWEEP (the pre-activation IS the sweep value); d % 8 == 2: taps (1, -1, 1, -1) on a constant input and state (they cancel);
    d % 8 == 3: x of the magnitude classes by time step (2^50 next to 2^-40 inside one 4-tap window); the rest randn."""
    g_ = gen(seed + 10000 * B + 100 * T + D + bias)
    x = torch.randn(B, T, D, generator=g_)
    w = 0.5 * torch.randn(D, 4, generator=g_)
    st = torch.randn(B, D, 4, generator=g_)
    d = torch.arange(D)
    c1, c2, c3 = d % 8 == 1, d % 8 == 2, d % 8 == 3
    w[c1] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    x[:, :, c1] = torch.tensor(SWEEP)[(torch.arange(T)[:, None] + d[c1][None, :]) % len(SWEEP)]
    w[c2] = torch.tensor([1.0, -1.0, 1.0, -1.0])
    x[:, :, c2] = 3.0
    st[:, c2] = 3.0
    mag = magnitude_rows(T + 4, B * int(c3.sum()), g_, T % 5).float().view(T + 4, B, -1).permute(1, 0, 2)
    x[:, :, c3] = mag[:, 4:]
    st[:, c3] = mag[:, :4].transpose(1, 2)
    b_ = (0.5 * torch.randn(D, generator=g_)).to(BF) if bias else None
    return dict(x=x.to(BF), w=w.to(BF).view(D, 1, 4), state=st.to(BF), bias=b_)


def conv_index_probe(B: int, T: int, D: int, tap: int) -> Dict:
    """one tap of 64 at `tap`, inputs = digits <= 255 of (channel vector, time, batch row) by lane, state = 200 + slot:
    y = 64 * ext[t + 1 + tap] exactly, with SiLU too (sigmoid(64 k) = 1 in fp32, silu(0) = 0) -> x, w, state, y"""
    v, t, b = torch.arange(D // 8)[None, None, :], torch.arange(T)[None, :, None], torch.arange(B)[:, None, None]
    x = torch.empty(B, T, D)
    for lane, digit in enumerate((v & 255, v >> 8, t & 255, t >> 8, b, 255, (v + t) & 255, 1)):
        x[:, :, lane::8] = digit
    st = (200.0 + torch.arange(4).float()).expand(B, D, 4).contiguous()
    w = torch.zeros(D, 4)
    w[:, tap] = 64.0
    ext = torch.cat([st.transpose(1, 2), x], 1)
    return dict(x=x.to(BF), w=w.to(BF).view(D, 1, 4), state=st.to(BF), y=(64.0 * ext[:, 1 + tap:1 + tap + T]).to(BF))


def conv_ref(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], state: Optional[torch.Tensor], silu: bool) -> Dict:
    """y[b,t,d] = act(bias_d + sum_j w[d,j] ext[b, t + 1 + j, d]), ext = [state^T (4 rows: zero history when None), x];
    new state = ext[T : T + 4]  ->  ref (float64, unrounded), noise, state (bit for bit)"""
    B, T, D = x.shape
    wd = w.double().reshape(D, 4)
    st = torch.zeros(B, D, 4, dtype=torch.float64) if state is None else state.double()
    ext = torch.cat([st.transpose(1, 2), x.double()], 1)
    pre = torch.zeros(B, T, D, dtype=torch.float64)
    scale = torch.zeros_like(pre)
    if bias is not None:
        pre += bias.double()
        scale += bias.double().abs()
    for j in range(4):
        term = wd[:, j] * ext[:, 1 + j:1 + j + T]
        pre += term
        scale += term.abs()
    new_state = ext[:, T:T + 4].transpose(1, 2).contiguous()
    if not silu:
        return dict(ref=pre, noise=D_CONV * scale, state=new_state)
    s = torch.sigmoid(pre)
    ref = pre * s
    slope = (s * (1.0 + pre * (1.0 - s))).abs() + 2.0 ** -10
    return dict(ref=ref, noise=slope * D_CONV * scale + (d_sigmoid(pre) + 2.0 ** -23) * ref.abs(), state=new_state)


def gate_ref(a: torch.Tensor, b: torch.Tensor, A_log: torch.Tensor, dt_bias: torch.Tensor) -> Dict:
    """g = -exp(A_log) softplus(a + dt_bias) (torch's softplus: the argument itself above 20), beta = sigmoid(b)"""
    av = a.double() + dt_bias.double()
    sp = torch.where(av > 20.0, av, torch.log1p(torch.exp(av)))
    eA = torch.exp(A_log.double())
    g = -eA * sp
    beta = torch.sigmoid(b.double())
    return dict(g=g, g_noise=(2.0 ** -20 + av.abs() * 2.0 ** -23) * g.abs() + 2.0 ** -126 * (eA + 1.0),
                beta=beta, beta_noise=D_BETA * beta, beta_floor=2.0 ** -126)


# (B, T, H): T <= 1024 runs 4 tokens per thread, above 8; the last two exceed 2048 * 256 conv items (786432 and 660480)
PROLOGUE_SHAPES = ((2, 37, 4), (1, 1029, 2), (3, 1024, 16), (5, 1032, 16))


def prologue_case(B: int, T: int, H: int, index_probe: bool = False) -> Dict:
    """one fused projection [B, T, ld] with q | k | v | a | b column blocks (Dq = Dk = 128 H, Dv = 256 H) and `ld` padded beyond
    the last column; conv inputs as conv_case (or conv_index_probe with the tap on the newest input), a = 4 randn with +20 /
    -120 tokens, b = SWEEP-like +-40 tokens (the gates' edges)"""
    Dq, Dv = 128 * H, 256 * H
    cols = (0, Dq, 2 * Dq, 2 * Dq + Dv, 2 * Dq + Dv + H)
    ld = (cols[4] + H + 7) // 8 * 8 + 16
    g_ = gen(B * 100000 + T * 10 + H)
    proj = torch.randn(B, T, ld, generator=g_).to(BF)
    parts = []
    for i, (c0, D) in enumerate(((0, Dq), (Dq, Dq), (2 * Dq, Dv))):
        c = conv_index_probe(B, T, D, 3) if index_probe else conv_case(B, T, D, False, seed=i)
        proj[..., c0:c0 + D] = c["x"]
        parts.append(c)
    a = 4.0 * torch.randn(B, T, H, generator=g_)
    r = torch.randint(0, 8, (B, T, H), generator=g_)
    a = torch.where(r == 0, torch.full_like(a, 20.0), torch.where(r == 1, torch.full_like(a, -120.0), a))
    bcol = torch.tensor(SWEEP)[torch.randint(0, len(SWEEP), (B, T, H), generator=g_)]
    bcol = torch.where(r == 2, torch.full_like(bcol, 40.0), torch.where(r == 3, torch.full_like(bcol, -40.0), bcol))
    proj[..., cols[3]:cols[3] + H] = a.to(BF)
    proj[..., cols[4]:cols[4] + H] = bcol.to(BF)
    A_log = torch.log(torch.tensor([16.0, 0.5, 4.0, 1.0] * H)[:H])
    dt_bias = 0.5 * torch.randn(H, generator=g_)
    return dict(proj=proj, cols=cols, ld=ld, H=H, D=(Dq, Dq, Dv), w=[c["w"] for c in parts], state=[c["state"] for c in parts],
                y=[c.get("y") for c in parts], A_log=A_log, dt_bias=dt_bias)


def prologue_slices(c: Dict) -> List[torch.Tensor]:
    return [c["proj"][..., c0:c0 + D] for c0, D in zip(c["cols"][:3], c["D"])]


# =============================================================================================================================
# fp32 emulations with the kernels' rounding points (test_rowwise_cpu.py: the honest one passes every judge, the wrong ones do not)
# =============================================================================================================================
def _r(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).float()


def emu_add_rmsnorm(x, res, w, eps, wrong: str = ""):
    h = x.float() if res is None else _r(x.float() + res.float())
    N = h.shape[-1]
    sq = h * h
    ss = (sq[..., :-8] if wrong == "drop_last_vector" else sq).sum(-1, keepdim=True)
    rstd = torch.rsqrt(ss / N + np.float32(eps * (10.0 if wrong == "eps" else 1.0)))
    if wrong == "scale":
        rstd = rstd * 1.003
    inner = h * rstd
    if wrong != "no_inner_round":
        inner = _r(inner)
    return (w.float() * inner).to(BF), h.to(BF)


def emu_gated_norm(x, gate, w, eps, res=None, wrong: str = "", gate_wrong_ld: Optional[torch.Tensor] = None):
    row = x.float() if res is None else x.float() + res.float()
    rstd = 1.0 / torch.sqrt((row * row).sum(-1, keepdim=True) * np.float32(1.0 / 256.0) + np.float32(eps * (10.0 if wrong == "eps" else 1.0)))
    if wrong == "scale":
        rstd = rstd * 1.003
    y = row * rstd
    if wrong == "extra_round":
        y = _r(y)
    y = y * w.float()
    if gate is not None:
        g = (gate_wrong_ld if wrong == "gate_ld" else gate).float()
        y = y * g * torch.sigmoid(row if wrong == "sigmoid_of_x" else g)
    return y.to(BF), row


def emu_silu_mul(gu, wrong: str = ""):
    I = gu.shape[-1] // 2
    a, b = gu[..., :I].float(), gu[..., I:].float()
    if wrong == "halves_swapped":
        a, b = b, a
    deep = a < -80.0          # as siluf_n_ (ivl_common.h): a e^a = (a 2^(a log2 e + 64)) 2^-64 where 1 / (1 + e^-a) leaves the fp32 normals
    inner = torch.where(deep, a * torch.exp2(torch.clamp(a, min=-200.0) * 1.4426950408889634 + 64.0) * 2.0 ** -64, a * torch.sigmoid(a))
    if wrong != "no_inner_round":
        inner = _r(inner)
    return (inner * b).to(BF)


def emu_conv(x, w, bias, state, silu: bool, wrong: str = ""):
    """-> (y bf16, new state bf16)"""
    B, T, D = x.shape
    wf = w.float().reshape(D, 4)
    if wrong == "taps_reversed":
        wf = wf.flip(-1)
    st = torch.zeros(B, D, 4) if state is None else state.float()
    ext = torch.cat([st.transpose(1, 2), x.float()], 1)
    src = ext
    if wrong == "state_slot":                       # history read from slots 0..2 instead of 1..3
        src = torch.cat([st.transpose(1, 2)[:, :1], st.transpose(1, 2)[:, :3], x.float()], 1)
    acc = torch.zeros(B, T, D)
    if bias is not None and wrong != "bias_after_silu":
        acc = acc + bias.float()
    for j in range(4):
        acc = acc + wf[:, j] * src[:, 1 + j:1 + j + T]
    if silu:
        acc = acc * torch.sigmoid(acc)
    if bias is not None and wrong == "bias_after_silu":
        acc = acc + bias.float()
    new = ext[:, T:T + 4].transpose(1, 2).clone()
    if wrong == "state_not_carried" and T < 4:
        new[..., :4 - T] = 0.0
    return acc.to(BF), new.to(BF)


def emu_gate(a, b, A_log, dt_bias):
    av = a.float() + dt_bias.float()
    sp = torch.where(av > 20.0, av, torch.log1p(torch.exp(av)))
    return -torch.exp(A_log.float()) * sp, (1.0 / (1.0 + torch.exp(-b.float()))).to(BF)


# =============================================================================================================================
# the checks: `run` is the implementation under test (the HIP kernel behind ops / the modules on the GPU, an emulation on the
# CPU), fed CPU tensors and returning CPU tensors.  Each check returns a Report; Report.ok() is the verdict.
# =============================================================================================================================
class Report:
    def __init__(self, what: str):
        self.what, self.fails, self.worst, self.where = what, [], 0.0, None
        self.elems = self.window = self.excused = 0.0
        self.used = float("-inf")
        self.shares = []                 # excuse-window share of every double-rounding case judged

    def single(self, tag, got, ref, noise, floor=0.0):
        j = judge_single(got, ref, noise, floor)
        if j["used"] == j["used"]:
            self.used = max(self.used, j["used"])
        if j["worst"] > self.worst:
            self.worst, self.where = j["worst"], (tag, j["where"], j["got"], j["ref"], j["bound"])
        if not j["worst"] <= 1.0:
            self.fails.append((tag, j))

    def fp32(self, tag, got, ref, noise):
        j = judge_fp32(got, ref, noise)
        if j["worst"] > self.worst:
            self.worst, self.where = j["worst"], (tag, j["where"], j["got"], j["ref"], j["bound"])
        if not j["worst"] <= 1.0:
            self.fails.append((tag, j))

    def double(self, tag, got, m):
        j = judge_double(got, m)
        n = got.numel()
        self.elems += n
        self.window += j["share"] * n
        self.excused += j["excused"] * n
        self.shares.append(j["share"])
        if not window_ok(m["window"]):
            self.fails.append((tag, f"{int(m['window'].sum())} of {n} elements of this case lie in the excuse window: more than the rule "
                                    f"allows (none below 100 elements, else {EXCUSED_MAX:.0%})"))
        if j["bad"]:
            self.fails.append((tag, f"{j['bad']} of {n} elements are neither the model nor an excused neighbour; "
                                    f"(index, got, model, alt, in window): {j['first']}"))

    def exact(self, tag, got, ref):
        if got is None or tuple(got.shape) != tuple(ref.shape):
            self.fails.append((tag, "missing output / wrong shape"))
            return
        bad = exact_mismatches(got, ref)
        if bad:
            self.fails.append((tag, f"not bit-equal; (index, got, expected): {bad}"))

    @property
    def share(self) -> float:
        return self.window / self.elems if self.elems else 0.0

    def ok(self) -> bool:
        return not self.fails

    def __str__(self):
        s = f"{self.what}: worst error / bound {self.worst:.5f} at {self.where}"
        if self.used > float("-inf"):
            s += "; fp32 allowance used beyond half a spacing: " + (f"at most {self.used:.3f} of it" if self.used > 0 else "none")
        if self.elems:
            s += (f"; in the excuse window {100 * min(self.shares):.3f} .. {100 * max(self.shares):.3f} % per case ({len(self.shares)} cases, "
                  f"{int(self.elems)} elements), excused {100 * self.excused / self.elems:.3f} % of all")
        return s + (f"; FAILS: {self.fails[:3]}" if self.fails else "")


def check_add_rmsnorm(run, N: int) -> Report:
    """run(x, res, w, eps) -> (y, h)"""
    rep = Report(f"add_rmsnorm N={N}")
    for rows in ADD_ROWS:
        for with_res in (False, True):
            c = add_rmsnorm_case(N, rows, with_res)
            m = add_rmsnorm_ref(**c)
            y, h = run(**c)
            rep.double((rows, with_res, "y"), y, m)
            rep.exact((rows, with_res, "h"), h, m["h"])
    return rep


def check_add_rmsnorm_onehot(run, N: int) -> Report:
    rep = Report(f"add_rmsnorm one-hot N={N}")
    x, c = onehot_rows(N)
    w = weight(N, gen(N))
    m = add_rmsnorm_ref(x, None, w, ADD_EPS)
    y, _ = run(x=x, res=None, w=w, eps=ADD_EPS)
    rep.double("y", y, m)
    peak = round_bf16(torch.tensor(float(N), dtype=torch.float64).sqrt() * (1.0 - 0.5 * ADD_EPS * N / 4096.0))
    expected = torch.zeros(len(c), N, dtype=torch.float64)
    expected[torch.arange(len(c)), c] = round_bf16(w.double()[c] * peak)
    assert not bool(m["window"].any()) and torch.equal(m["model"], expected), "the closed form of the probe"
    rep.exact("closed form", y, expected)
    return rep


def check_gated(run, rows: int, variant: str) -> Report:
    """run(x, gate, w, eps, res, variant) -> (y, residual_out or None)"""
    rep = Report(f"gated norm rows={rows} {variant}")
    for first in first_classes(rows):
        c = gated_case(rows, variant, first)
        assert rows > 1 or first == 1 or bool((c["x"] != 0).any()), "a case must not be vacuous"
        r = gated_norm_ref(c["x"], c["gate"], c["w"], c["eps"], c["res"])
        y, res_out = run(**c)
        rep.single(("row 0: " + CLASSES[first], "y"), y, r["ref"], r["noise"], r["floor"])
        if variant == "res_bf16":
            rep.exact(("row 0: " + CLASSES[first], "residual_out"), res_out, round_bf16(r["row"]))
        elif variant in ("res_fp32", "res_out_fp32"):
            rep.exact(("row 0: " + CLASSES[first], "residual_out"), res_out, r["row"])
    return rep


def check_gated_onehot(run, variant: str) -> Report:
    """gate = 1 (silu(1) within the sigmoid's delta), so the closed form is w_c * 16 * silu(1) at c and exact zeros elsewhere"""
    rep = Report(f"gated norm one-hot {variant}")
    x, c = onehot_rows(256)
    w = weight(256, gen(256))
    gate = None if variant == "plain" else torch.ones(len(c), 256, dtype=BF)
    r = gated_norm_ref(x, gate, w, GATED_EPS)
    y, _ = run(x=x, gate=gate, w=w, eps=GATED_EPS, res=None, variant=variant)
    rep.single("y", y, r["ref"], r["noise"], r["floor"])
    off = torch.ones(len(c), 256, dtype=torch.bool)
    off[torch.arange(len(c)), c] = False
    rep.exact("zeros off the hot element", y.double() * off, torch.zeros(len(c), 256, dtype=torch.float64))
    return rep


def check_strided(run, H: int, tokens: int) -> Report:
    """run(case) -> y [tokens * H, 256]"""
    rep = Report(f"strided gated norm H={H} tokens={tokens}")
    for first in first_classes(tokens * H):
        c = strided_case(H, tokens, first)
        r = gated_norm_ref(c["x"].view(-1, 256), c["gate"], c["w"], c["eps"])
        rep.single(("row 0: " + CLASSES[first], "y"), run(c).reshape(-1, 256), r["ref"], r["noise"], r["floor"])
    return rep


def check_silu(run, rows: int, I: int) -> Report:
    """run(gate_up) -> y"""
    rep = Report(f"silu_mul {rows} x {I}")
    gu = silu_case(rows, I)
    rep.double("y", run(gu), silu_ref(gu))
    gu, y = silu_index_probe(rows, I)
    assert not bool(silu_ref(gu)["window"].any())
    rep.exact("index probe", run(gu), y)
    return rep


def check_silu_deep(run) -> Report:
    rep = Report("silu_mul, a in [-110, -80]")
    gu = silu_deep_case()
    rep.double("y", run(gu), silu_ref(gu))
    return rep


def _conv_forms(T: int):
    for B in CONV_B:
        for D in CONV_D:
            for bias in (False, True):
                for silu in (False, True):
                    for has_in, out in CONV_STATE_FORMS:
                        yield B, D, bias, silu, has_in, out


def check_conv(run, T: int) -> Report:
    """run(x, w, bias, state_in or None, state_out form, silu) -> (y, state_out or None); the state_in handed over is a copy"""
    rep = Report(f"short_conv T={T}")
    for B, D, bias, silu, has_in, out in _conv_forms(T):
        c = conv_case(B, T, D, bias)
        st = c["state"] if has_in else None
        r = conv_ref(c["x"], c["w"], c["bias"], st, silu)
        y, so = run(c["x"], c["w"], c["bias"], None if st is None else st.clone(), out, silu)
        tag = (B, D, "bias" if bias else "", "silu" if silu else "", "state_in" if has_in else "", out)
        rep.single(tag + ("y",), y, r["ref"], r["noise"])
        if out is not None:
            rep.exact(tag + ("state",), so, r["state"])
    for tap in range(4):                                               # index probe, SiLU off and on
        c = conv_index_probe(2, T, 24, tap)
        for silu in (False, True):
            y, so = run(c["x"], c["w"], None, c["state"].clone(), "aliased", silu)
            rep.exact(("index probe", tap, silu), y, c["y"])
    return rep


def _slab(x: torch.Tensor, state: Optional[torch.Tensor], t0: int, t1: int):
    """tokens [t0, t1) of a call with the history they see as their state"""
    if t0 == 0:
        return x[:, :t1], state
    assert t0 >= 4
    return x[:, t0:t1], x[:, t0 - 4:t0].transpose(1, 2).contiguous()


def _slabs(T: int):
    return [(0, T)] if T <= 64 else [(0, 16), (T - 48, T)]


def check_conv_wrap(run) -> Report:
    """B = 2, T = 520, D = 32776 (more items than the capped grid has threads): the index probe on the whole tensor bit for bit,
    the float64 judge on the first 16 and the last 48 tokens of every batch row (the wrapped items are the last of row 1)"""
    B, T, D = CONV_WRAP
    rep = Report(f"short_conv wrap {CONV_WRAP}")
    c = conv_index_probe(B, T, D, 2)
    y, so = run(c["x"], c["w"], None, c["state"].clone(), "aliased", True)
    rep.exact("index probe", y, c["y"])
    rep.exact("index probe state", so, c["x"][:, T - 4:].transpose(1, 2).double())
    c = conv_case(B, T, D, False)
    y, so = run(c["x"], c["w"], None, c["state"].clone(), "separate", True)
    for t0, t1 in _slabs(T):
        xs, st = _slab(c["x"], c["state"], t0, t1)
        r = conv_ref(xs, c["w"], None, st, True)
        rep.single(("y", t0), y[:, t0:t1], r["ref"], r["noise"])
    rep.exact("state", so, c["x"][:, T - 4:].transpose(1, 2).double())
    return rep


def check_prologue(run, B: int, T: int, H: int) -> Report:
    """run(case, aliased) -> (q, k, v, g, beta, [3 states out]); states separate and aliased in place; the index probe over the
    whole call; float64 on ALL tokens, but for the two grid-wrap shapes (tens of millions of elements): there on the first 16
    and the last 48 tokens of every batch row (the wrapped items are the last of the last row)"""
    rep = Report(f"gdn_prologue B={B} T={T} H={H}")
    slabs = _slabs(T) if B * T * 512 * H > (1 << 23) else [(0, T)]
    c = prologue_case(B, T, H, index_probe=True)
    out = run(c, True)
    for i in range(3):
        rep.exact(("index probe", "qkv"[i]), out[i], c["y"][i])
    c = prologue_case(B, T, H)
    gr = gate_ref(c["proj"][..., c["cols"][3]:c["cols"][3] + H], c["proj"][..., c["cols"][4]:c["cols"][4] + H], c["A_log"], c["dt_bias"])
    for aliased in (False, True):
        out = run(c, aliased)
        for i, x in enumerate(prologue_slices(c)):
            for t0, t1 in slabs:
                xs, st = _slab(x, c["state"][i], t0, t1)
                r = conv_ref(xs, c["w"][i], None, st, True)
                rep.single(("qkv"[i], t0, aliased), out[i][:, t0:t1], r["ref"], r["noise"])
            new = torch.cat([c["state"][i].transpose(1, 2), x], 1)[:, T:T + 4].transpose(1, 2)
            rep.exact(("state", "qkv"[i], aliased), out[5][i], new.double())
        rep.fp32(("g", aliased), out[3], gr["g"], gr["g_noise"])
        rep.single(("beta", aliased), out[4], gr["beta"], gr["beta_noise"], gr["beta_floor"])
    return rep

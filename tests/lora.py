"""Input builders, the float64 reference and the judges for ivl_lora_add_small_m_fwd (CPU only, pure torch; the pattern of
tests/projections.py), the per-row LoRA delta on the output of a decode projection:

    t[m,j] = bf16( sum_k A_a[j,k] x[m,k] )     d[m,n] = bf16( sum_j B_a[n,j] t[m, seg(n) R + j] )
    e[m,n] = bf16( fp32(s_a) d[m,n] )          y[m,n] = bf16( y0[m,n] + e[m,n] )          a = idx[m]

`chain` evaluates it in float64 with ONE round-to-nearest-even at t and at d (rowwise.round_bf16); e and the final add are single
fp32 operations by definition (order-free), evaluated as such.  Rows with idx outside [0, n_adapters) and columns in no segment are
NOT TOUCHED: the judges compare them with y0 / the t sentinel BIT for bit (raw bits: y0 holds -0.0, which a rewrite y0 + 0 flips).

THE EXACT-INTEGER PROBE.  Everything is a small integer, every sum an integer far below 2^24: fp32 accumulation is exact in any
order and t_ws and y must equal the chain bit for bit -- no tolerance, no excused element.
  "index"  x in [-3, 3]; A in {-1, 0, +1} with the density for std(t) about 6; B integers whose amplitude and density give
           std(s_a d) about 48 for the adapter's scaling s_a in {0.5, 1, 2, 3} (std(d) = 48 at s = 1; the y of a call must stay
           below 256 as well); y0 in [-8, 8] with -0.0 among its zeros.  Condition (asserted from the reference alone): at most
           1 % of a call's touched t, d and y exceed 256 in magnitude -- below that bf16 holds every integer (and every half below
           128), so ONE misplaced term, segment or adapter changes the output.
  "ties"   x in [-A, A], A = projections.ties_amplitude(R); every row of A is one +-1 (t = +-x[k], exact); B = +-1 (a tenth 0);
           s in {1, 3, 1}; y0 in {-4, ..., 4}.  Conditions: every |sum_j B t| < 2^11, and at least 10 % of a call's d sums, and of
           its y0 + e, are exact bf16 ties: the rounding rule decides them (and s = 3 tells bf16(s bf16(d)) from bf16(s d)).
  NORM     projections.norm_case's identity: h = bf16(x + residual) in {+1, -1}, an integer norm weight in [-4, 4], eps = 1e-6:
           the normalised row is +-w[k] exactly and the index probe applies unchanged.

THE RANDN JUDGE.  t_ws against float64 within projections.randn_tolerance (the project's bound for a bf16 K-long dot product);
y against the chain evaluated FROM THE KERNEL'S OWN t (as check_randn judges GLU on the kernel's own plain output).  A window is
accepted only at the d rounding: where the float64 sum_j B t lies within R 2^-24 sum_j |B t| (R fp32 roundings of the fmaf chain) of
a bf16 rounding boundary, y may be the chain of either neighbour.  At most 1 % of a call's elements may be DECIDED by the window.

The fp32 emulations at the end are what tests/test_lora_cpu.py feeds the judges: the honest one (two summation orders) passes with
identical bits, each wrong one is reported.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

import projections as pj
import rowwise as rw

BF = torch.bfloat16
T_LD = 512                        # row pitch of t_ws
T_SENTINEL = 24576.0              # what the runner fills t_ws with before a call
N_ADAPTERS = 3
INDEX_SCALINGS = (0.5, 3.0, 2.0)  # adapter 0, 1, 2 (s = 1 is the ties variant's)
TIES_SCALINGS = (1.0, 3.0, 1.0)
T_STD, D_STD = 6.0, 48.0
MAX_SHARE, TIES_MIN_SHARE, WINDOW_MAX = 0.01, 0.10, 0.01


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def segment_of(c: Dict) -> torch.Tensor:
    """int64 [N]: the segment that owns each output column, -1 = none"""
    seg = torch.full((c["N"],), -1, dtype=torch.int64)
    for i in range(len(c["seg_cols"]) - 1):
        seg[c["seg_cols"][i]:c["seg_cols"][i + 1]] = i
    return seg


def valid(c: Dict, a: int) -> bool:
    return 0 <= a < c["n_adapters"]


# =============================================================================================================================
# the reference
# =============================================================================================================================
def t_exact(c: Dict, xn: torch.Tensor, idx: Sequence[int]) -> torch.Tensor:
    """float64 [M, n_seg R]: the unrounded A_a xn[m] (nan in rows without an adapter)"""
    out = torch.full((xn.shape[0], c["A"].shape[1]), float("nan"), dtype=torch.float64)
    for m, a in enumerate(idx):
        if valid(c, a):
            out[m] = c["A"][a].double() @ xn[m].double()
    return out


def expand_ref(c: Dict, t: torch.Tensor, y0: torch.Tensor, idx: Sequence[int]) -> Dict:
    """from t (float64 [M, n_seg R], bf16 values) on: D = the exact sums, d, e, y, the second neighbour of d with its chain, the
    window (D within R 2^-24 sum |B t| of the boundary between them) and `touched` [M, N]"""
    M, N, R = t.shape[0], c["N"], c["R"]
    seg = segment_of(c)
    D = torch.zeros(M, N, dtype=torch.float64)
    absD = torch.zeros(M, N, dtype=torch.float64)
    s = torch.ones(M, dtype=torch.float32)
    touched = torch.zeros(M, N, dtype=torch.bool)
    for m, a in enumerate(idx):
        if not valid(c, a):
            continue
        s[m] = c["s"][a]
        for i in range(len(c["seg_cols"]) - 1):
            c0, c1 = c["seg_cols"][i], c["seg_cols"][i + 1]
            if c1 > c0:
                Bd, tt = c["B"][a, c0:c1].double(), t[m, i * R:(i + 1) * R]
                D[m, c0:c1] = Bd @ tt
                absD[m, c0:c1] = Bd.abs() @ tt.abs()
                touched[m, c0:c1] = True

    def tail(d):          # e and the add: single fp32 operations on bf16 values, each rounded to bf16
        e = (s[:, None] * d.float()).to(BF)
        return e, (y0.float() + e.float()).to(BF)
    d = rw.round_bf16(D)
    other = rw.other_neighbour(D, d)
    e, y = tail(d)
    _, y_alt = tail(other)
    window = ((d + other) / 2 - D).abs() <= R * 2.0 ** -24 * absD
    return dict(D=D, d=d, e=e, y=torch.where(touched, y, y0), y_alt=torch.where(touched, y_alt, y0), window=window & touched,
                touched=touched, seg=seg, y0=y0)


def chain(c: Dict, xn: torch.Tensor, y0: torch.Tensor, idx: Sequence[int]) -> Dict:
    """the whole chain in float64 from the (normalised) input: t = bf16(A xn), then expand_ref"""
    tx = t_exact(c, xn, idx)
    t = rw.round_bf16(torch.nan_to_num(tx))
    r = expand_ref(c, t, y0, idx)
    r.update(t=t, t_exact=tx, rows=[valid(c, a) for a in idx])
    return r


def conditions(c: Dict, r: Dict) -> Optional[str]:
    """the probe's conditions on one call, from the reference alone; None = they hold (a call that touches nothing: vacuous)"""
    rows = torch.tensor(r["rows"])
    if not bool(r["touched"].any()):
        return None
    t, D = r["t"][rows], r["D"][r["touched"]]
    ysum = (r["y0"].double() + r["e"].double())[r["touched"]]
    if c["variant"] == "ties":
        sd, sy = float(pj.is_tie(D).double().mean()), float(pj.is_tie(ysum).double().mean())
        if not (sd >= TIES_MIN_SHARE and sy >= TIES_MIN_SHARE and float(D.abs().max()) < 2048.0 and float(t.abs().max()) <= 256.0):
            return f"ties: share of d {sd:.3f}, of y0 + e {sy:.3f}, max |sum| {float(D.abs().max())}"
        return None
    for name, v in (("t", t), ("d", D), ("y", ysum)):
        share = float((v.abs() > 256.0).double().mean())
        if share > MAX_SHARE:
            return f"index: {share:.4f} of the call's {name} exceed 256"
    return None


# =============================================================================================================================
# builders
# =============================================================================================================================
def index_patterns(M: int) -> List[Tuple[str, List[int]]]:
    """all -1; mixed; the same adapter on two rows; all different; out of range (n_adapters, a negative one, 2^30)"""
    pats = [("none", [-1, -1, -1, -1]), ("mixed", [1, -1, 0, 2]), ("same", [2, 2, -1, 0]), ("different", [0, 1, 2, -1]),
            ("range", [N_ADAPTERS, 1, -7, 1 << 30])]
    if M == 1:
        pats = [("none", [-1]), ("mixed", [1]), ("same", [2]), ("different", [0]), ("range", [N_ADAPTERS])]
    return [(n, p[:M]) for n, p in pats]


def _int_amplitude(target_var: float) -> Tuple[int, float]:
    """(Ab, density) of integers uniform in [-Ab, Ab] kept with probability `density`: variance density Ab (Ab + 1) / 3 = target"""
    Ab = 1
    while Ab < 7 and Ab * (Ab + 1) / 3.0 < target_var:
        Ab += 1
    return Ab, min(1.0, target_var / (Ab * (Ab + 1) / 3.0))


def _sparse_ints(shape, Ab: int, density: float, g_: torch.Generator) -> torch.Tensor:
    v = torch.randint(-Ab, Ab + 1, shape, generator=g_)
    return (v * (torch.rand(shape, generator=g_) < density)).to(BF)


def _y0(M: int, N: int, A_: int, g_: torch.Generator) -> torch.Tensor:
    y0 = torch.randint(-A_, A_ + 1, (M, N), generator=g_).to(BF)
    neg0 = (y0 == 0) & (torch.rand(M, N, generator=g_) < 0.5)
    y0 = torch.where(neg0, torch.tensor(-0.0, dtype=BF), y0)
    for m in range(M):                                           # (at least one in every row, whatever the draw)
        y0[m, (5 * m + 1) % N] = -0.0
    return y0


def case(K: int, N: int, seg_cols: Sequence[int], R: int, rank: Optional[int] = None, variant: str = "index", norm: bool = False,
         Ms=(1, 2, 3, 4)) -> Dict:
    """4 rows; A [3, n_seg R, K], B [3, N, R] zero-padded from `rank` (default R) to R, s [3] fp32, y0 [4, N]; NORM: x, res, nw, eps
    and xn = the normalised rows the kernel must form.  The first seed whose calls (every M of Ms, every index pattern) meet the
    probe's conditions."""
    rank = R if rank is None else rank
    n_seg = len(seg_cols) - 1
    assert 1 <= rank <= R and 1 <= n_seg <= 8 and K % 8 == 0 and variant in ("index", "ties", "randn")
    assert not (norm and variant != "index")

    def build(try_: int) -> Dict:
        g_ = rw.gen(K * 100003 + N * 17 + R * 5 + rank + 3 * n_seg + 2 * (variant == "ties") + 8 * norm + 7919 * try_)
        c = dict(K=K, N=N, R=R, rank=rank, seg_cols=tuple(seg_cols), n_adapters=N_ADAPTERS, variant=variant, norm=norm, eps=pj.NORM_EPS)
        A = torch.zeros(N_ADAPTERS, n_seg * R, K, dtype=BF)
        B = torch.zeros(N_ADAPTERS, N, R, dtype=BF)
        rows = [i * R + j for i in range(n_seg) for j in range(rank)]          # the rows of A that hold data
        if variant == "randn":
            c["s"] = torch.tensor([0.5, 2.75, 1.3125], dtype=torch.float32)
            c["x"] = torch.randn(4, K, generator=g_).to(BF)
            A[:, rows] = (torch.randn(N_ADAPTERS, len(rows), K, generator=g_) * K ** -0.5).to(BF)
            B[:, :, :rank] = (torch.randn(N_ADAPTERS, N, rank, generator=g_) * rank ** -0.5).to(BF)
            c["y0"] = torch.randn(4, N, generator=g_).to(BF)
        elif variant == "ties":
            c["s"] = torch.tensor(TIES_SCALINGS, dtype=torch.float32)
            amp = pj.ties_amplitude(rank)
            c["x"] = torch.randint(-amp, amp + 1, (4, K), generator=g_).to(BF)
            hot = torch.randint(0, K, (N_ADAPTERS, len(rows)), generator=g_)
            sign = (2 * torch.randint(0, 2, (N_ADAPTERS, len(rows)), generator=g_) - 1).to(BF)
            for a in range(N_ADAPTERS):
                A[a, rows, hot[a]] = sign[a]
            B[:, :, :rank] = pj.ternary(N_ADAPTERS * N, rank, 0.9, g_).view(N_ADAPTERS, N, rank)
            c["y0"] = _y0(4, N, 4, g_)
        else:
            c["s"] = torch.tensor(INDEX_SCALINGS, dtype=torch.float32)
            if norm:
                h = (2 * torch.randint(0, 2, (4, K), generator=g_) - 1).to(BF)
                c["x"] = torch.randint(-3, 4, (4, K), generator=g_).to(BF)
                c["res"] = (h.float() - c["x"].float()).to(BF)
                c["nw"] = torch.randint(-4, 5, (K,), generator=g_).to(BF)
                c["h"], c["xn"] = h, (h.float() * c["nw"].float()).to(BF)
                xvar = 20.0 / 3.0
            else:
                c["x"] = torch.randint(-3, 4, (4, K), generator=g_).to(BF)
                xvar = 4.0
            A[:, rows] = pj.ternary(N_ADAPTERS * len(rows), K, min(1.0, T_STD ** 2 / (xvar * K)), g_).view(N_ADAPTERS, len(rows), K)
            tvar = xvar * K * min(1.0, T_STD ** 2 / (xvar * K))
            for a in range(N_ADAPTERS):
                Ab, dens = _int_amplitude((D_STD / float(c["s"][a])) ** 2 / (rank * tvar))
                B[a, :, :rank] = _sparse_ints((N, rank), Ab, dens, g_)
            c["y0"] = _y0(4, N, 8, g_)
        if "xn" not in c:
            c["xn"] = c["x"]
        seg = torch.full((N,), -1, dtype=torch.int64)
        for i in range(n_seg):
            seg[seg_cols[i]:seg_cols[i + 1]] = i
        B[:, seg < 0] = 0                                        # (columns in no segment have no B row)
        c["A"], c["B"] = A, B
        return c

    why = None
    for try_ in range(64):
        c = build(try_)
        if variant == "randn":
            return c
        why = None
        for M in Ms:
            for _, idx in index_patterns(M):
                why = why or conditions(c, chain(c, c["xn"][:M], c["y0"][:M], idx))
        if why is None:
            if norm:                                             # the identity the NORM probe rests on, in float64
                for x, res in ((c["x"], c["res"]), (c["h"], None)):
                    m_ = rw.add_rmsnorm_ref(x, res, c["nw"], pj.NORM_EPS)
                    assert not bool(m_["window"].any()) and torch.equal(m_["model"], c["xn"].double())
            return c
    raise AssertionError(f"no seed meets the probe's conditions: {why}")


# =============================================================================================================================
# judges.  run(c, x, res, y0, idx) -> (y [M, N] bf16, t_ws [M, T_LD] bf16): the implementation under test on the case's tables;
# x is the raw input and res the residual of a NORM case (res may be None there: x = h), else x = the projection's input.  The
# runner fills t_ws with T_SENTINEL first.
# =============================================================================================================================
class Counted(rw.Report):
    def __init__(self, what: str):
        super().__init__(what)
        self.probed = self.decided = self.judged = 0

    def __str__(self):
        return super().__str__() + f"; {self.probed} elements bit for bit, {self.decided} of {self.judged} decided by the d window"


def _untouched(rep: Counted, tag, r: Dict, y0: torch.Tensor, y: torch.Tensor, t: torch.Tensor, nrank: int):
    """rows without an adapter and columns in no segment keep y0's BITS; t_ws keeps the sentinel outside [0, n_seg R) of the rows
    with an adapter"""
    same = bits(y) == bits(y0)
    bad = (~same & ~r["touched"]).nonzero()
    if bad.numel():
        i = tuple(bad[0].tolist())
        rep.fails.append((tag, f"{bad.shape[0]} untouched elements of y were rewritten, first at {i}: bits {int(bits(y)[i]) & 0xffff:#06x} "
                               f"for {int(bits(y0)[i]) & 0xffff:#06x}"))
    keep = torch.ones_like(t, dtype=torch.bool)
    for m, ok in enumerate(r["rows"]):
        if ok:
            keep[m, :nrank] = False
    if bool(((t.float() != T_SENTINEL) & keep).any()):
        rep.fails.append((tag, "t_ws was written outside the rows / rank rows of the call"))


def _call(run, c: Dict, M: int, idx, with_res: bool = True):
    if c["norm"]:
        x, res = (c["x"][:M], c["res"][:M]) if with_res else (c["h"][:M], None)
    else:
        x, res = c["x"][:M], None
    y, t = run(c, x, res, c["y0"][:M].clone(), list(idx))
    return y, t


def check_probe(run, c: Dict, Ms=(1, 2, 3, 4)) -> Counted:
    """the exact-integer probe (index, ties, NORM): every M, every index pattern; bit for bit"""
    rep = Counted(f"{c['variant']}{' norm' if c['norm'] else ''} K={c['K']} N={c['N']} R={c['R']} r={c['rank']} segs={c['seg_cols']}")
    nrank = c["A"].shape[1]
    for M in Ms:
        for name, idx in index_patterns(M):
            for with_res in ((True, False) if c["norm"] else (True,)):
                tag = (M, name) + (("residual",) if c["norm"] and with_res else ())
                r = chain(c, c["xn"][:M], c["y0"][:M], idx)
                why = conditions(c, r)
                if why:
                    rep.fails.append((tag, "the probe's conditions do not hold: " + why))
                y, t = _call(run, c, M, idx, with_res)
                if y is None or tuple(y.shape) != (M, c["N"]) or tuple(t.shape) != (M, T_LD):
                    rep.fails.append((tag, "missing output / wrong shape"))
                    continue
                rows = torch.tensor(r["rows"])
                rep.exact(tag + ("t",), t[rows][:, :nrank], r["t"][rows])
                rep.exact(tag + ("y",), y, r["y"].double())
                _untouched(rep, tag, r, c["y0"][:M], y, t, nrank)
                rep.probed += int(r["touched"].sum()) + int(rows.sum()) * nrank
    return rep


def check_randn(run, c: Dict, Ms=(1, 2, 3, 4)) -> Counted:
    rep = Counted(f"randn K={c['K']} N={c['N']} R={c['R']} r={c['rank']} segs={c['seg_cols']}")
    nrank = c["A"].shape[1]
    for M in Ms:
        for name, idx in index_patterns(M):
            tag = (M, name)
            y, t = _call(run, c, M, idx)
            rows = torch.tensor([valid(c, a) for a in idx])
            tx = t_exact(c, c["xn"][:M], idx)
            if bool(rows.any()):
                ref = tx[rows]
                ratio = (t[rows][:, :nrank].double() - ref).abs() / pj.randn_tolerance(ref)
                worst, where = rw._where(ratio)
                if worst > rep.worst:
                    rep.worst, rep.where = worst, (tag, where)
                if not worst <= 1.0:
                    rep.fails.append((tag, f"t: error / bound {worst} at {where}"))
            tk = torch.where(rows[:, None], t[:, :nrank].double(), torch.zeros(M, nrank, dtype=torch.float64))
            r = expand_ref(c, tk, c["y0"][:M], idx)
            r["rows"] = rows.tolist()
            yd = y.double()
            first = yd == r["y"].double()
            second = r["window"] & (yd == r["y_alt"].double())
            bad = (~(torch.isfinite(yd) & (first | second))).nonzero()
            if bad.numel():
                i = tuple(bad[0].tolist())
                rep.fails.append((tag, f"{bad.shape[0]} elements of y are neither the chain of the kernel's own t nor (inside the window) "
                                       f"of d's other neighbour; first at {i}: got {float(yd[i])}, chain {float(r['y'][i])}, other "
                                       f"{float(r['y_alt'][i])}, in window {bool(r['window'][i])}"))
            decided = int((second & ~first).sum())
            n = int(r["touched"].sum())
            rep.decided, rep.judged = rep.decided + decided, rep.judged + n
            if n and decided > WINDOW_MAX * n:
                rep.fails.append((tag, f"{decided} of {n} elements are decided by the d window: more than {WINDOW_MAX:.0%}"))
            _untouched(rep, tag, r, c["y0"][:M], y, t, nrank)
    return rep


# =============================================================================================================================
# fp32 emulations (tests/test_lora_cpu.py): `order` = two summation orders, `wrong` = a deliberate defect
# =============================================================================================================================
WRONG = ("t_not_rounded", "e_not_rounded", "scale_before_round", "wrong_segment", "adapter_prev_row", "adapterless_rewritten",
         "rank_padding_read", "drop_last_piece", "tail_clamped")


def _sums32(w: torch.Tensor, x: torch.Tensor, order: int) -> torch.Tensor:
    """w [J, K] . x [K] in fp32: order 0 = 64 interleaved partial sums (lane l: chunks l + 64 i) then a tree; order 1 = straight"""
    wf, xf = w.float(), x.float()
    if order == 1 or w.shape[1] % 8:
        acc = torch.zeros(w.shape[0], dtype=torch.float32)
        for k in range(w.shape[1]):
            acc = acc + wf[:, k] * xf[k]
        return acc
    K = w.shape[1]
    pad = (-K) % 512
    p = torch.nn.functional.pad(wf * xf[None], (0, pad)).view(w.shape[0], -1, 64, 8)          # [J, trip, lane, element]
    lane = torch.zeros(w.shape[0], 64, dtype=torch.float32)
    for i in range(p.shape[1]):
        for e_ in range(8):
            lane = lane + p[:, i, :, e_]
    while lane.shape[1] > 1:
        lane = lane[:, :lane.shape[1] // 2] + lane[:, lane.shape[1] // 2:]
    return lane[:, 0]


def emu_norm(x: torch.Tensor, res: Optional[torch.Tensor], nw: torch.Tensor, eps: float) -> torch.Tensor:
    return rw.emu_add_rmsnorm(x, res, nw, eps)[0]


def emu(c: Dict, x: torch.Tensor, res, y0: torch.Tensor, idx: Sequence[int], wrong: str = "", order: int = 0):
    """the kernels' arithmetic in fp32 on the CPU -> (y, t_ws)"""
    M, N, K, R = x.shape[0], c["N"], c["K"], c["R"]
    xn = emu_norm(x, res, c["nw"], c["eps"]) if c["norm"] else x
    n_seg = len(c["seg_cols"]) - 1
    nrank = n_seg * R
    seg = segment_of(c)
    t_ws = torch.full((M, T_LD), T_SENTINEL, dtype=BF)
    y = y0.clone()
    A, B = c["A"], c["B"]
    if wrong == "rank_padding_read" and c["rank"] < R:           # the padding holds a copy of the data
        A, B = A.clone(), B.clone()
        r_ = c["rank"]
        for i in range(n_seg):
            A[:, i * R + r_:i * R + min(R, 2 * r_)] = A[:, i * R:i * R + min(R, 2 * r_) - r_]
        B[:, :, r_:min(R, 2 * r_)] = B[:, :, :min(R, 2 * r_) - r_]
    for m in range(M):
        a = idx[m - 1] if wrong == "adapter_prev_row" and m > 0 else idx[m]
        if not valid(c, a):
            if wrong == "adapterless_rewritten":
                y[m] = (y0[m].float() + 0.0).to(BF)
            continue
        kk = K - 8 if wrong == "drop_last_piece" and K > 8 else K
        t32 = _sums32(A[a][:, :kk], xn[m][:kk], order)
        t = t32.to(BF)
        t_ws[m, :nrank] = t
        tf = t32 if wrong == "t_not_rounded" else t.float()
        s = c["s"][a]
        cols = (seg >= 0).nonzero()[:, 0]                        # every column of a segment at once; j stays a sequential fp32 sum
        si = (seg[cols] + 1) % n_seg if wrong == "wrong_segment" else seg[cols]
        nb = torch.where(cols >= N - N % 8, torch.full_like(cols, max(0, N - N % 8 - 1)), cols) if wrong == "tail_clamped" else cols
        bsel, tsel = B[a, nb].float(), tf.view(n_seg, R)[si]
        d32 = torch.zeros(cols.shape[0], dtype=torch.float32)
        for j in (range(R) if order == 0 else reversed(range(R))):
            d32 = d32 + bsel[:, j] * tsel[:, j]
        if wrong == "scale_before_round":
            e = (s * d32).to(BF)
        else:
            e = (s * d32.to(BF).float()).to(BF)
        if wrong == "e_not_rounded":
            y[m, cols] = (y0[m, cols].float() + s * d32.to(BF).float()).to(BF)
        else:
            y[m, cols] = (y0[m, cols].float() + e.float()).to(BF)
    return y, t_ws

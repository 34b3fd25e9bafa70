"""The 16-row builders and judges for ivl_lora_add_m16_fwd and the LoRA epilogue of ivl_linear_m16_lora*_fwd (CPU only, pure torch).
Everything that defines the computation is tests/lora.py's and row-count-agnostic there: `chain`, `expand_ref`, `conditions`, `_untouched`
and the fp32 emulations.  This module adds what that file fixes at 4 rows and 3 adapters:

  * `case`: 16 rows of x and y0 and 17 adapters (16 different ones on the rows of one call plus one more, so that "every row another
    adapter" and "an index past the table" are both real), by the "index" and "ties" recipes of lora.case (and its randn recipe);
    scalings cycle (0.5, 3, 2, 1) for "index" and (1, 3, 1) for "ties".  The first seed of at most 64 whose every call (M in MS, every
    pattern below) meets lora.conditions, from the reference alone.  The caps are lora.py's and are conditions, not measurements: at
    most 1 % of a call's touched t, d, y above 256; at least 10 % ties; at most 1 % of the elements decided by the d window.
  * `index_patterns(M)`: all -1; only the last row; one adapter on every row; 16 different (a permutation); mixed with -1 on every
    third row; out of range (n_adapters, -7, 2^30) between valid ones.
  * `check_probe` / `check_randn`: lora.check_probe / check_randn over these patterns and row counts.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

import lora
import projections as pj
import rowwise as rw

BF = torch.bfloat16
ROWS = 16
MS = (5, 8, 13, 16)
N_ADAPTERS = 17
INDEX_SCALINGS = (0.5, 3.0, 2.0, 1.0)
TIES_SCALINGS = (1.0, 3.0, 1.0)
RANDN_SCALINGS = (0.5, 2.75, 1.3125)

# (K, N, seg_cols, R, rank, variant): the shapes of the probe -- one chunk; borders off any multiple of 4 with untouched columns in
# front, an empty segment and rank 3 inside R = 8; six segments; K past one trip of the 64 lanes (512) with R = 64; N past 32 x 256
SEG6 = (0, 100, 200, 300, 400, 500, 600)
SHAPES = [(8, 1, (0, 1), 8, None, "index"),
          (72, 97, (3, 50, 50, 97), 8, 3, "index"),
          (520, 600, SEG6, 16, None, "index"),
          (2080, 100, (0, 100), 64, None, "index"),
          (96, 8209, (0, 4000, 8209), 16, None, "index"),
          (96, 200, (0, 100, 200), 16, None, "ties"),
          (2080, 17, (0, 17), 8, None, "ties"),
          (4128, 600, (0, 300, 600), 64, None, "ties")]


def shape_id(s) -> str:
    K, N, seg, R, rank, variant = s
    return f"{variant}-K{K}-N{N}-seg{len(seg) - 1}-R{R}" + (f"-r{rank}" if rank else "")


def index_patterns(M: int) -> List[Tuple[str, List[int]]]:
    perm = [(7 * m + 2) % N_ADAPTERS for m in range(ROWS)]                    # 16 different adapters (7 and 17 are coprime)
    mixed = [-1 if m % 3 == 2 else (5 * m + 1) % N_ADAPTERS for m in range(ROWS)]
    bad = (N_ADAPTERS, -7, 1 << 30)
    rng = [bad[(m // 2) % 3] if m % 2 == 0 else (3 * m) % N_ADAPTERS for m in range(ROWS)]
    pats = [("none", [-1] * M), ("last", [-1] * (M - 1) + [3]), ("same", [5] * M), ("different", perm[:M]), ("mixed", mixed[:M]),
            ("range", rng[:M])]
    assert len(set(perm)) == ROWS
    return pats


def case(K: int, N: int, seg_cols: Sequence[int], R: int, rank: Optional[int] = None, variant: str = "index", Ms=MS) -> Dict:
    """16 rows; A [17, n_seg R, K], B [17, N, R] zero-padded from `rank` (default R) to R, s [17] fp32, y0 [16, N]"""
    rank = R if rank is None else rank
    n_seg = len(seg_cols) - 1
    assert 1 <= rank <= R and 1 <= n_seg <= 8 and K % 8 == 0 and variant in ("index", "ties", "randn")
    nA = N_ADAPTERS

    def build(try_: int) -> Dict:
        g_ = rw.gen(K * 100003 + N * 17 + R * 5 + rank + 3 * n_seg + 2 * (variant == "ties") + 16 + 7919 * try_)
        c = dict(K=K, N=N, R=R, rank=rank, seg_cols=tuple(seg_cols), n_adapters=nA, variant=variant, norm=False, eps=pj.NORM_EPS)
        A = torch.zeros(nA, n_seg * R, K, dtype=BF)
        B = torch.zeros(nA, N, R, dtype=BF)
        rows = [i * R + j for i in range(n_seg) for j in range(rank)]         # the rows of A that hold data
        cyc = lambda v: torch.tensor([v[a % len(v)] for a in range(nA)], dtype=torch.float32)
        if variant == "randn":
            c["s"] = cyc(RANDN_SCALINGS)
            c["x"] = torch.randn(ROWS, K, generator=g_).to(BF)
            A[:, rows] = (torch.randn(nA, len(rows), K, generator=g_) * K ** -0.5).to(BF)
            B[:, :, :rank] = (torch.randn(nA, N, rank, generator=g_) * rank ** -0.5).to(BF)
            c["y0"] = torch.randn(ROWS, N, generator=g_).to(BF)
        elif variant == "ties":
            c["s"] = cyc(TIES_SCALINGS)
            amp = pj.ties_amplitude(rank)
            c["x"] = torch.randint(-amp, amp + 1, (ROWS, K), generator=g_).to(BF)
            hot = torch.randint(0, K, (nA, len(rows)), generator=g_)
            sign = (2 * torch.randint(0, 2, (nA, len(rows)), generator=g_) - 1).to(BF)
            for a in range(nA):
                A[a, rows, hot[a]] = sign[a]
            B[:, :, :rank] = pj.ternary(nA * N, rank, 0.9, g_).view(nA, N, rank)
            c["y0"] = lora._y0(ROWS, N, 4, g_)
        else:
            c["s"] = cyc(INDEX_SCALINGS)
            c["x"] = torch.randint(-3, 4, (ROWS, K), generator=g_).to(BF)
            xvar = 4.0
            dens = min(1.0, lora.T_STD ** 2 / (xvar * K))
            A[:, rows] = pj.ternary(nA * len(rows), K, dens, g_).view(nA, len(rows), K)
            tvar = xvar * K * dens
            for a in range(nA):
                Ab, dn = lora._int_amplitude((lora.D_STD / float(c["s"][a])) ** 2 / (rank * tvar))
                B[a, :, :rank] = lora._sparse_ints((N, rank), Ab, dn, g_)
            c["y0"] = lora._y0(ROWS, N, 8, g_)
        c["xn"] = c["x"]
        B[:, lora.segment_of(c) < 0] = 0                                      # (columns in no segment have no B row)
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
                why = why or lora.conditions(c, lora.chain(c, c["xn"][:M], c["y0"][:M], idx))
            if why:
                break
        if why is None:
            c["tries"] = try_ + 1
            return c
    raise AssertionError(f"no seed within 64 meets the probe's conditions: {why}")


_CASES: Dict = {}


def shared_case(shape) -> Dict:
    """one build per shape and process (the reference is computed once and left unchanged)"""
    if shape not in _CASES:
        K, N, seg, R, rank, variant = shape
        _CASES[shape] = case(K, N, seg, R, rank, variant)
    return _CASES[shape]


# run(c, x, res, y0, idx) -> (y [M, N], t_ws [M, T_LD]) as in tests/lora.py (res is always None here); t_ws pre-filled with T_SENTINEL
def check_probe(run, c: Dict, Ms=MS, patterns=None) -> lora.Counted:
    """the exact-integer probe over every M and index pattern: y and t_ws equal the chain bit for bit"""
    rep = lora.Counted(f"{c['variant']} 16 rows K={c['K']} N={c['N']} R={c['R']} r={c['rank']} segs={c['seg_cols']}")
    nrank = c["A"].shape[1]
    for M in Ms:
        for name, idx in index_patterns(M):
            if patterns is not None and name not in patterns:
                continue
            tag = (M, name)
            r = lora.chain(c, c["xn"][:M], c["y0"][:M], idx)
            why = lora.conditions(c, r)
            if why:
                rep.fails.append((tag, "the probe's conditions do not hold: " + why))
            y, t = run(c, c["x"][:M], None, c["y0"][:M].clone(), list(idx))
            if y is None or tuple(y.shape) != (M, c["N"]) or tuple(t.shape) != (M, lora.T_LD):
                rep.fails.append((tag, "missing output / wrong shape"))
                continue
            rows = torch.tensor(r["rows"])
            rep.exact(tag + ("t",), t[rows][:, :nrank], r["t"][rows])
            rep.exact(tag + ("y",), y, r["y"].double())
            lora._untouched(rep, tag, r, c["y0"][:M], y, t, nrank)
            rep.probed += int(r["touched"].sum()) + int(rows.sum()) * nrank
    return rep


def check_randn(run, c: Dict, Ms=MS) -> lora.Counted:
    """lora.check_randn's judgement (t within the project's bound of float64; y = the chain of the kernel's own t, the d window)"""
    rep = lora.Counted(f"randn 16 rows K={c['K']} N={c['N']} R={c['R']} r={c['rank']} segs={c['seg_cols']}")
    nrank = c["A"].shape[1]
    for M in Ms:
        for name, idx in index_patterns(M):
            tag = (M, name)
            y, t = run(c, c["x"][:M], None, c["y0"][:M].clone(), list(idx))
            rows = torch.tensor([lora.valid(c, a) for a in idx])
            tx = lora.t_exact(c, c["xn"][:M], idx)
            if bool(rows.any()):
                ref = tx[rows]
                ratio = (t[rows][:, :nrank].double() - ref).abs() / pj.randn_tolerance(ref)
                worst, where = rw._where(ratio)
                if worst > rep.worst:
                    rep.worst, rep.where = worst, (tag, where)
                if not worst <= 1.0:
                    rep.fails.append((tag, f"t: error / bound {worst} at {where}"))
            tk = torch.where(rows[:, None], t[:, :nrank].double(), torch.zeros(M, nrank, dtype=torch.float64))
            r = lora.expand_ref(c, tk, c["y0"][:M], idx)
            r["rows"] = rows.tolist()
            yd = y.double()
            first = yd == r["y"].double()
            second = r["window"] & (yd == r["y_alt"].double())
            bad = (~(torch.isfinite(yd) & (first | second))).nonzero()
            if bad.numel():
                i = tuple(bad[0].tolist())
                rep.fails.append((tag, f"{bad.shape[0]} elements of y are neither the chain of the kernel's own t nor (inside the window) "
                                       f"of d's other neighbour; first at {i}: got {float(yd[i])}, chain {float(r['y'][i])}"))
            decided = int((second & ~first).sum())
            n = int(r["touched"].sum())
            rep.decided, rep.judged = rep.decided + decided, rep.judged + n
            if n and decided > lora.WINDOW_MAX * n:
                rep.fails.append((tag, f"{decided} of {n} elements are decided by the d window: more than {lora.WINDOW_MAX:.0%}"))
            lora._untouched(rep, tag, r, c["y0"][:M], y, t, nrank)
    return rep

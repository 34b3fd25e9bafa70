"""Input builders, references and judges for the rotary embedding, the one formula with the most copies on the hot path (CPU only,
pure torch / numpy plus the oracle):

  ivl_rope_tables_fwd                       cos / sin of fp32(fp32(pos) * inv_freq[j]), scaled, bf16          against float64
  ivl_mrope_fwd / ivl_mrope_strided_fwd     bf16(bf16(x c) + bf16(rotate_half(x) s)), tables by section       against the eager chain
  rope_pair / rope_apply (csrc/swa_shared.h, every fused site of ops.swa_forward / swa_forward_rows / swa_cache_append)
                                            the same arithmetic while q / k_new are loaded                    against the eager chain
  vision_rope_piece / the vision pre-pass   bf16(fp32(x c) + fp32(rotate_half(x) s)), no contraction          against the fp32 chain

TABLES.  Reference per element: f = fp32(fp32(pos) * inv_freq[j]) (int64 -> fp32 to nearest even, ONE fp32 rounding of the product:
the reference's position_ids.float() * inv_freq), ref = cos_float64(f) * scaling, scaling the fp32 value the kernel receives.  The
output must be BIT-EQUAL to bf16_RNE(ref), except where ref lies within relative D_TRIG of a bf16 rounding boundary: there either
neighbour passes (rowwise.judge_double).  D_TRIG is derived, not fitted: the device cosf / sinf are taken as 2 ulp of fp32 = 2^-23
relative (the figure rowwise.py assumes for every libm call; no ROCm math documentation ships with the toolchain to cite another),
doubled: 2^-22; + 2^-23 when scaling != 1 (the extra fp32 product, 2^-24, doubled).  Both channel halves carry the same bits, zeros
compare by value, nothing may be non-finite, and the share of elements inside the window -- computed from the float64 reference alone
-- must stay under rowwise.EXCUSED_MAX = 1 % in every call.

ROTATIONS.  Expected = oracle.swa.apply_mrope on CPU bf16 tensors (each product and the sum is one bf16 rounding) resp.
oracle.vision.apply_rotary_pos_emb_vision (fp32 product, product, sum as three tensor operations: nothing is contracted on the CPU),
compared with torch.equal: no tolerance.  The ADVERSARIAL tables are randn -- the two channel halves differ, the three axes are
unrelated, every (b, t) row is different -- so a site that reads the wrong half, axis, section or row of the [3, B, T, d] plane cannot
hide behind cos = cat(freqs, freqs).  For the vision rotation a third kind, CANCELLING tables (sin chosen so that x cos + rotate_half(x)
sin of q head 0 cancels to 2^-15 of its terms), turns the rounding of ONE product -- all a contracted multiply-add changes -- into a
relative 2^-10 of the sum, which the bf16 rounding of the result cannot hide: with randn tables a contraction moves a bf16 result only
about once in 2^16 elements.  The keys of head 0 are scaled by 2^14 there, so that the scores -- all the attention output shows of
q -- are of order 1 and move with it.  "cancel_k" is the mirror image: sin cancels k head 0 and q head 0 is scaled, for the copies of
the rotation that only keys pass through (the key loads, the key pre-pass, the form without a workspace).
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import adversarial as adv
import rowwise as rw
from oracle import swa as oswa
from oracle import vision as ovis

BF = torch.bfloat16
D_TRIG = 2.0 ** -22                 # derived (above): 2 ulp of fp32 for cosf / sinf, doubled
D_TRIG_SCALED = 2.0 ** -23          # added when scaling != 1


def d_trig(scaling: float) -> float:
    return D_TRIG + (D_TRIG_SCALED if rw.f32(scaling) != 1.0 else 0.0)


# =============================================================================================================================
# 1. the tables
# =============================================================================================================================
NAMED_POSITIONS = (0, 1, 2, 3, 7, 63, 64, 4095, 4096, 131071, 131072, 2 ** 20,
                   2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3,            # the last two round down and up to even
                   10 ** 8 + 7, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 12345, 10 ** 15 + 1)
N_RANDOM = 300                      # random positions below 2^26
SCALINGS = (1.0, 0.75, 1.1)         # 1.1 reaches the kernel as f32(1.1)
TABLE_CASES = ((64, 1e6), (8, 1e4))                     # (half_dim, theta): the model, the tiny config
WRAP_T = 1400                       # positions [3, 1, 1400]: 4200 rows * 64 > 1024 blocks * 256 threads


def position_list(n_random: int = N_RANDOM, seed: int = 0) -> List[int]:
    r = torch.randint(0, 2 ** 26, (n_random,), generator=rw.gen(seed)).tolist()
    return list(NAMED_POSITIONS) + r


def table_positions(T: Optional[int] = None) -> torch.Tensor:
    """int64 [3, 1, n]: the position list on axis 0, rotated by one on axis 1, reversed on axis 2 (all three axes distinct);
    T: the list repeated (with other random positions each time) up to T columns"""
    L = position_list()
    seed = 1
    while T is not None and len(L) < T:
        L += position_list(seed=seed)
        seed += 1
    L = torch.tensor(L[:T] if T is not None else L, dtype=torch.int64)
    return torch.stack([L, L.roll(1), L.flip(0)])[:, None, :].contiguous()


def inv_freq(half_dim: int, theta: float) -> torch.Tensor:
    """the 'default' rope init, as InfiniteVLRotaryEmbedding builds it (fp32 on the CPU)"""
    d = 2 * half_dim
    return 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))


def pos_to_f32(pos: torch.Tensor, wrong: str = "") -> np.ndarray:
    """int64 -> fp32, to nearest even (numpy's cast); wrong = "truncate": towards zero"""
    p = pos.numpy()
    f = p.astype(np.float32)
    if wrong == "truncate":
        over = f.astype(np.float64) > p.astype(np.float64)          # (exact below 2^53: every position here is)
        f = np.where(over, np.nextafter(f, np.float32(0.0)), f)
    return f


def table_angles(pos: torch.Tensor, inv: torch.Tensor, wrong: str = "") -> np.ndarray:
    """f = fp32(fp32(pos) * inv_freq[j]) as float64 [..., half_dim]; wrong = "float64": the product without the two fp32 roundings"""
    if wrong == "float64":
        return pos.numpy().astype(np.float64)[..., None] * inv.numpy().astype(np.float64)
    return (pos_to_f32(pos, wrong)[..., None] * inv.numpy()).astype(np.float64)      # fp32 * fp32 -> fp32: one rounding


def tables_ref(pos: torch.Tensor, inv: torch.Tensor, scaling: float) -> Dict:
    """the float64 reference and its double-rounding models -> cos, sin: rowwise.double_model dicts (+ "ref")"""
    f = table_angles(pos, inv)
    s = rw.f32(scaling)
    out = {}
    for name, fn in (("cos", np.cos), ("sin", np.sin)):             # numpy's float64 cos / sin reduce the argument exactly
        ref = torch.from_numpy(fn(f) * s)
        out[name] = rw.double_model(ref, lambda r: r, d_trig(scaling))
        out[name]["ref"] = ref
    return out


def implied_ulps(got: torch.Tensor, m: Dict) -> float:
    """What a bf16 table can tell of the fp32 value behind it: an element that took the OTHER neighbour was at least as far from the
    float64 reference as the rounding boundary is -> the largest such distance, in fp32 ulps of the reference (0: none did)."""
    g = got.double()
    took = (g != m["model"]) & (g == m["alt"])
    if not bool(took.any()):
        return 0.0
    ref = m["ref"][took]
    _, e = torch.frexp(ref.abs())
    return float((((m["model"][took] + m["alt"][took]) / 2 - ref).abs() / torch.pow(2.0, e.double() - 24)).max())


def check_tables(run: Callable, half_dim: int, theta: float, scaling: float, pos: Optional[torch.Tensor] = None) -> rw.Report:
    """run(pos int64 [3, B, T], inv_freq fp32 [half_dim], scaling) -> (cos, sin) bf16 [3, B, T, 2 half_dim], CPU tensors"""
    pos = table_positions() if pos is None else pos
    inv = inv_freq(half_dim, theta)
    rep = rw.Report(f"rope tables half_dim={half_dim} theta={theta:g} scaling={scaling:g} rows={pos.numel()}")
    ref = tables_ref(pos, inv, scaling)
    got = dict(zip(("cos", "sin"), run(pos, inv, scaling)))
    rep.ulps = 0.0
    for name in ("cos", "sin"):
        t = got[name]
        if tuple(t.shape) != tuple(pos.shape) + (2 * half_dim,) or t.dtype != BF:
            rep.fails.append((name, f"shape / dtype {tuple(t.shape)} {t.dtype}"))
            continue
        rep.double((name, "index = (axis, b, t, j); positions", "table_positions()"), t[..., :half_dim], ref[name])
        rep.exact((name, "second half == first half"), t[..., half_dim:], t[..., :half_dim].double())
        rep.ulps = max(rep.ulps, implied_ulps(t[..., :half_dim], ref[name]))
    return rep


def emu_tables(pos: torch.Tensor, inv: torch.Tensor, scaling: float, wrong: str = "") -> Tuple[torch.Tensor, torch.Tensor]:
    """the honest fp32 chain: numpy fp32 cos / sin of the fp32 product, one fp32 product with the scaling, bf16.  wrong: "float64"
    (angles without the fp32 roundings), "truncate" (int64 -> fp32 towards zero), "fast" (a fast cosine: the argument reduced in
    fp32, x - 2 pi round(x / 2 pi), as the hardware path does)"""
    f = table_angles(pos, inv, wrong if wrong in ("float64", "truncate") else "")
    if wrong != "float64":
        f = f.astype(np.float32)
    if wrong == "fast":
        two_pi = np.float32(2.0 * np.pi)
        f = f - np.round(f * np.float32(1.0 / (2.0 * np.pi))) * two_pi
    s = np.float32(scaling)
    tab = [torch.from_numpy((fn(f) * s).astype(np.float32)).to(BF) for fn in (np.cos, np.sin)]
    return tuple(torch.cat([t, t], -1) for t in tab)


# =============================================================================================================================
# 2. M-RoPE: tables, cases, the eager arithmetic, wrong emulations, the read map
# =============================================================================================================================
# (B, T, Hq, Hkv, d, sections); the fourth: sections that are no multiples of 8 (ivl_mrope_fwd only); the fifth: one channel group;
# the last: B * T * (Hq + Hkv) * d / 16 = 589824 items > grid_cap's 2048 blocks * 256 threads
MROPE_SHAPES = ((1, 1, 16, 2, 128, (16, 24, 24)), (3, 5, 16, 2, 128, (16, 24, 24)), (2, 7, 4, 4, 128, (8, 24, 32)),
                (2, 7, 2, 1, 128, (24, 20, 20)), (2, 9, 2, 1, 16, (2, 3, 3)), (1, 4096, 16, 2, 128, (16, 24, 24)))
STRIDED_SHAPES = ((3, 5, 16, 2, 128, (16, 24, 24)), (2, 7, 4, 4, 128, (8, 24, 32)), (3, 1, 16, 2, 128, (16, 24, 24)),     # T = 1: the
                  (1, 1, 4, 4, 128, (8, 24, 32)), (1, 4096, 16, 2, 128, (16, 24, 24)))                     # other branch of row_stride
SITE_SECTIONS = ((16, 24, 24), (8, 24, 32))            # the fused sites take multiples of 8
TABLE_KINDS = ("randn", "real")


def shape_id(s) -> str:
    return "B{}_T{}_Hq{}_Hkv{}_d{}_s{}".format(*s[:5], "-".join(str(v) for v in s[5]))


def mrope_positions(B: int, T: int) -> torch.Tensor:
    """int64 [3, B, T]: three unrelated axes, every batch row somewhere else"""
    t, b = torch.arange(T)[None, :], torch.arange(B)[:, None]
    return torch.stack([1000 * b + 17 + t, 517 * b + 3 + t // 3, 29 * b + 11 + t % 7]).contiguous()


def mrope_tables(kind: str, B: int, T: int, d: int, seed: int = 0, run_tables: Optional[Callable] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin bf16 [3, B, T, d].  "randn": adversarial; "real": of mrope_positions, from `run_tables` (the table kernel on the GPU),
    by default the honest emulation"""
    if kind == "randn":
        g_ = rw.gen(7001 + seed)
        return torch.randn(3, B, T, d, generator=g_).to(BF), torch.randn(3, B, T, d, generator=g_).to(BF)
    run_tables = run_tables or emu_tables
    return run_tables(mrope_positions(B, T), inv_freq(d // 2, 1e6), 1.0)


def mrope_case(shape, kind: str = "randn", run_tables: Optional[Callable] = None) -> Dict:
    """q [B, T, Hq, d], k [B, T, Hkv, d] bf16 randn (time-major, as the kernels take them) and the tables"""
    B, T, Hq, Hkv, d, sec = shape
    g_ = rw.gen(100 * B + T + Hq)
    q, k = torch.randn(B, T, Hq, d, generator=g_).to(BF), torch.randn(B, T, Hkv, d, generator=g_).to(BF)
    cos, sin = mrope_tables(kind, B, T, d, seed=T, run_tables=run_tables)
    return dict(q=q, k=k, cos=cos, sin=sin, sections=tuple(sec))


def mrope_expected(q, k, cos, sin, sections) -> Tuple[torch.Tensor, torch.Tensor]:
    """oracle.swa.apply_mrope (head-major there) on the time-major tensors"""
    qr, kr = oswa.apply_mrope(q.transpose(1, 2), k.transpose(1, 2), cos, sin, list(sections))
    return qr.transpose(1, 2).contiguous(), kr.transpose(1, 2).contiguous()


MROPE_WRONG = ("half", "boundary", "axes", "batch", "fused")


def _select(tab: torch.Tensor, sections, wrong: str) -> torch.Tensor:
    """[3, B, T, d] -> [B, T, 1, d]: the table entry every channel reads"""
    d = tab.shape[-1]
    half = d // 2
    s0, s1 = sections[0], sections[1]
    if wrong == "boundary":                            # the first boundary moved by 8
        s0, s1 = s0 + 8, s1 - 8
    c = torch.arange(half)
    ax = (c >= s0).long() + (c >= s0 + s1).long()
    if wrong == "axes":                                # axes 1 and 2 swapped
        ax = torch.tensor([0, 2, 1])[ax]
    ch = torch.cat([c, c]) if wrong == "half" else torch.arange(d)      # the second half reads the first half's piece
    if wrong == "batch":                               # the wrong batch row of the plane
        tab = tab.roll(1, 1)
    return tab[torch.cat([ax, ax]), :, :, ch].permute(1, 2, 0)[:, :, None, :]


def emu_mrope(q, k, cos, sin, sections, wrong: str = "") -> Tuple[torch.Tensor, torch.Tensor]:
    """the kernels' arithmetic on time-major CPU bf16 tensors: bf16(bf16(x c) + bf16(rotate_half(x) s)); wrong = "fused": the two
    products and the sum in one rounding; the other wrong forms: _select"""
    c, s = _select(cos, sections, wrong), _select(sin, sections, wrong)

    def rot(x):
        r = oswa.rotate_half(x)
        if wrong == "fused":
            return (x.double() * c.double() + r.double() * s.double()).to(BF)
        return (x * c) + (r * s)
    return rot(q), rot(k)


def rotation_mismatches(got: torch.Tensor, expected: torch.Tensor, names=("b", "t", "head", "channel"), limit: int = 3) -> str:
    """"" when bit-equal by value, else the number of differing elements and the first of them by name"""
    if got is None or tuple(got.shape) != tuple(expected.shape):
        return "missing output / wrong shape"
    bad = rw.exact_mismatches(got, expected, limit=limit)
    if not bad:
        return ""
    n = int((~(torch.isfinite(got.double()) & (got.double() == expected.double()))).sum())
    return f"{n} of {got.numel()} elements differ; first: " + "; ".join(
        "(" + ", ".join(f"{nm}={i}" for nm, i in zip(names, idx)) + f") got {g} expected {e}" for idx, g, e in bad)


READ_MAP_PASSES = ("channel", "axis", "token", "batch")


def _read_map_tables(what: str, B: int, T: int, d: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """integer codes exact in bf16 (<= 256): cos = 1 + code, sin = 129 + code (code < 128)"""
    a, b, t, c = torch.meshgrid(torch.arange(3), torch.arange(B), torch.arange(T), torch.arange(d), indexing="ij")
    code = {"channel": c, "axis": a, "token": t % 127, "batch": b % 127}[what].float()
    return (1.0 + code).to(BF), (129.0 + code).to(BF)


def read_map_report(run: Callable, B: int, T: int, Hq: int, Hkv: int, d: int, sections) -> str:
    """Diagnosis: with (x1, x2) = (1, 0) the output is (cos[c], sin[c + d/2]), with (0, 1) it is (-sin[c], cos[c + d/2]) -- the table
    entry the kernel READ, which integer-coded tables name: one pass each for the channel, the axis, the token (mod 127) and the
    batch row.  run(q, k, cos, sin, sections) -> (q, k).  -> "" or, for the first mismatch of every pass that has one,
    (b, t, head, channel), the entry expected and the entry read."""
    half = d // 2
    out = []
    for what in READ_MAP_PASSES:
        cos, sin = _read_map_tables(what, B, T, d)
        for first in (1.0, 0.0):
            x = torch.cat([torch.full((half,), first), torch.full((half,), 1.0 - first)]).to(BF)
            q, k = x.expand(B, T, Hq, d).contiguous(), x.expand(B, T, Hkv, d).contiguous()
            exp = mrope_expected(q, k, cos, sin, sections)
            got = run(q.clone(), k.clone(), cos, sin, sections)
            for name, g, e in (("q", got[0], exp[0]), ("k", got[1], exp[1])):
                bad = rw.exact_mismatches(g, e, limit=1)
                if bad:
                    (b, t, h, c), gv, ev = bad[0]
                    tab = lambda v: f"{'sin' if abs(v) >= 129 else 'cos'} entry with {what} code {int(abs(v)) - (129 if abs(v) >= 129 else 1)}"      # noqa: E731
                    out.append(f"read map, {what} pass, {name}[b={b}, t={t}, head={h}, channel={c}] with (x1, x2) = ({first:g}, "
                               f"{1 - first:g}): expected the {tab(ev)}, read the {tab(gv)} (values {ev} / {gv})")
                    break
            else:
                continue
            break
    return "\n".join(out)


def strided_case(shape, kind: str = "randn", run_tables: Optional[Callable] = None) -> Dict:
    """mrope_case inside one [B * T, ld] qkv buffer: junk | q block | junk | k block | junk (offsets multiples of 8 elements)"""
    c = mrope_case(shape, kind, run_tables)
    B, T, Hq, Hkv, d, _ = shape
    q_off, k_off = 8, 8 + Hq * d + 24
    ld = k_off + Hkv * d + 40
    buf = torch.randn(B * T, ld, generator=rw.gen(ld + T)).to(BF)
    buf[:, q_off:q_off + Hq * d] = c["q"].reshape(B * T, Hq * d)
    buf[:, k_off:k_off + Hkv * d] = c["k"].reshape(B * T, Hkv * d)
    c.update(buf=buf, q_off=q_off, k_off=k_off, ld=ld)
    return c


def strided_views(c: Dict, buf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B, T, Hq, d] / k [B, T, Hkv, d] views into `buf` (any device)"""
    B, T, Hq, d = c["q"].shape
    Hkv = c["k"].shape[2]
    rows = buf.view(B, T, c["ld"])
    return (rows[..., c["q_off"]:c["q_off"] + Hq * d].unflatten(-1, (Hq, d)), rows[..., c["k_off"]:c["k_off"] + Hkv * d].unflatten(-1, (Hkv, d)))


def strided_report(c: Dict, after: torch.Tensor) -> str:
    """the q and k blocks of the buffer must hold the contiguous result, every other column what it held before"""
    eq, ek = mrope_expected(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    gq, gk = strided_views(c, after)
    msg = [f"{n}: {m}" for n, m in (("q", rotation_mismatches(gq, eq)), ("k", rotation_mismatches(gk, ek))) if m]
    keep = torch.ones(c["ld"], dtype=torch.bool)
    B, T, Hq, d = c["q"].shape
    keep[c["q_off"]:c["q_off"] + Hq * d] = False
    keep[c["k_off"]:c["k_off"] + c["k"].shape[2] * d] = False
    m = rotation_mismatches(after[:, keep], c["buf"][:, keep], names=("row", "column outside the blocks (compacted)"))
    if m:
        msg.append("columns outside q | k were written: " + m)
    return "\n".join(msg)


# =============================================================================================================================
# 3. the fused sites of the sliding-window attention
# =============================================================================================================================
@dataclass(frozen=True)
class Site:
    name: str
    entry: str                       # "fwd" ops.swa_forward(pos_dev=, append=True) | "append" ops.swa_cache_append | "decode_rows"
    #                                  swa_forward(pos_rows=) | "hold" (+ frozen=) | "rows" ops.swa_forward_rows | "rows_n" (+ n_rows=)
    T: int
    Hq: int
    Hkv: int
    W: int
    seens: Tuple[int, ...]           # ring position per batch row (all equal for the scalar-position entries)
    kernel: str                      # what the dispatch must choose (adversarial.swa_dispatch); "" for the stand-alone append
    nsplit: int
    prepass: bool = False            # the rotation runs in the rope pre-pass of the long calls
    wraps: Optional[bool] = None     # the appended tokens cross the ring's seam (None: the rows differ)
    mask: Tuple[int, ...] = ()       # hold: frozen per row; rows_n: n_rows per row

    @property
    def B(self) -> int:
        return len(self.seens)


def _sites() -> List[Site]:
    s = []
    for wraps in (False, True):
        w = "wrap" if wraps else "nowrap"
        p = (lambda a, b, n: (b if wraps else a,) * n)
        s += [Site(f"packed_{w}", "fwd", 3, 16, 2, 96, p(40, 283, 2), "packed", 3, wraps=wraps),              # split-KV + combine, append folded in
              Site(f"64row_{w}", "fwd", 40, 16, 2, 96, p(30, 250, 2), "64row", 1, wraps=wraps),
              Site(f"128row_{w}", "fwd", 130, 16, 2, 200, p(20, 500, 2), "prefill", 1, wraps=wraps),           # rotation inside the 128-row kernel
              Site(f"prepass_single_{w}", "fwd", 512, 16, 2, 1024, p(100, 1700, 4), "prefill", 1, True, wraps=wraps),
              Site(f"prepass_split_{w}", "fwd", 512, 16, 2, 1024, p(100, 1700, 1), "prefill", 4, True, wraps=wraps),
              Site(f"append_{w}", "append", 5, 16, 2, 96, p(40, 188, 3), "", 0, wraps=wraps)]
    # a full ring (pos_min = seen >= C): linearize pre-pass + the in-kernel query rotation; T > C: the append always crosses the seam
    s += [Site("ring256_slot0", "fwd", 1024, 16, 2, 1024, (1023,) * 4, "ring256", 1, wraps=True),
          Site("ring256_wrapped", "fwd", 1024, 16, 2, 1024, (2500,) * 4, "ring256", 1, wraps=True)]
    mixed = (10, 94, 250)                                # B = 3 rows: inside the ring, across the seam, wrapped
    s += [Site("decode_rows", "decode_rows", 2, 16, 2, 96, mixed, "rows", 3),
          Site("hold", "hold", 2, 16, 2, 96, mixed, "rows", 3, mask=(0, 1, 0)),
          Site("rows_packed", "rows", 2, 16, 2, 96, mixed, "rows", 3),
          Site("rows_64row", "rows", 40, 16, 2, 96, mixed, "64row", 1),
          Site("rows_128row", "rows", 130, 16, 2, 200, (20, 150, 450), "prefill", 1),
          Site("rows_prepass", "rows", 512, 16, 2, 1024, (100, 600, 1500), "prefill", 2, True),
          Site("rows_n_64row", "rows_n", 40, 16, 2, 96, mixed, "64row", 1, mask=(40, 17, 0)),
          Site("rows_n_128row", "rows_n", 130, 16, 2, 200, (20, 150, 450), "prefill", 1, mask=(130, 65, 1))]
    return s


SITES: Dict[str, Site] = {x.name: x for x in _sites()}
# every launch form a rotation is inlined into: (entry, kernel, pre-pass)
SITE_FORMS = {("fwd", "packed", False), ("fwd", "64row", False), ("fwd", "prefill", False), ("fwd", "prefill", True), ("fwd", "ring256", False),
              ("append", "", False), ("decode_rows", "rows", False), ("hold", "rows", False), ("rows", "rows", False), ("rows", "64row", False),
              ("rows", "prefill", False), ("rows", "prefill", True), ("rows_n", "64row", False), ("rows_n", "prefill", False)}


@lru_cache(maxsize=4)
def site_inputs(name: str, sections: Tuple[int, int, int]) -> Dict:
    """q, k, v (un-rotated), the rings, adversarial tables and q, k rotated on the CPU by the eager chain.
    READ-ONLY: the dict and its tensors are cached and shared by every caller of the site (the reference is computed once); a test
    hands them to the device or clones them, and never writes them in place."""
    s = SITES[name]
    B, T, C, d = s.B, s.T, s.W - 1, 128
    g_ = rw.gen(s.T * 1000 + s.W + B + sections[0])
    rn = lambda *sh: torch.randn(*sh, generator=g_).to(BF)      # noqa: E731
    c = dict(q=rn(B, T, s.Hq, d), k=rn(B, T, s.Hkv, d), v=rn(B, T, s.Hkv, d), kc=rn(B, s.Hkv, C, d), vc=rn(B, s.Hkv, C, d),
             cos=rn(3, B, T, d), sin=rn(3, B, T, d), sections=sections)
    c["q_rot"], c["k_rot"] = mrope_expected(c["q"], c["k"], c["cos"], c["sin"], sections)
    return c


def site_report(s: Site, with_rope: Dict, rotated: Dict) -> str:
    """with_rope / rotated: dict(o=, kc=, vc=) (CPU) of the call with rope= on un-rotated inputs and of the call with rope=None on
    inputs rotated on the CPU -> "" or what differs.  hold: o of the frozen rows is unspecified; rows_n: o[b, :n_b] only."""
    msg = []
    if s.entry != "append":
        o1, o2 = with_rope["o"], rotated["o"]
        for b in range(s.B):
            n = s.T
            if s.entry == "hold" and s.mask[b]:
                n = 0
            if s.entry == "rows_n":
                n = min(s.mask[b], s.T)
            m = rotation_mismatches(o1[b, :n], o2[b, :n], names=("t", "head", "channel"))
            if m:
                msg.append(f"o[b={b}]: {m}")
    for ring in ("kc", "vc"):
        m = rotation_mismatches(with_rope[ring], rotated[ring], names=("b", "kv head", "slot", "channel"))
        if m:
            msg.append(f"{ring} ring: {m}")
    return "\n".join(msg)


# =============================================================================================================================
# 4. the vision rotation
# =============================================================================================================================
VISION_D = (64, 80, 128)
VISION_H = (2, 4)
VISION_FORMS = ("inload", "prepass", "prepass_null_ws", "rows128")
VISION_TABLES = ("randn", "real", "cancel", "cancel_k")
VISION_MAX_SEQLEN = {"inload": 64, "prepass": 130, "prepass_null_ws": 130, "rows128": 130}


def vision_segments(form: str, H: int) -> List[int]:
    """inload: every segment <= 64 (one query tile: the keys are rotated in the tile loads); prepass: several query tiles per segment
    (key pre-pass into the workspace; with a NULL workspace the rotation is redone per query tile); rows128: n_seg * 2 * H = 512, the
    launcher's threshold for the 128-row workgroups, with segments on both sides of the tile borders"""
    if form == "inload":
        return [64, 1, 0, 37]
    if form in ("prepass", "prepass_null_ws"):
        return [65, 130, 64]
    n_seg = 256 // H
    return ([65, 130, 64, 1, 0, 37, 129, 128] + [1, 2, 3] * n_seg)[:n_seg]


def vision_case(d: int, H: int, form: str, tables: str) -> Dict:
    """qkv [S, 3, H, d] bf16 randn (q, k, v are its strided slices), cu_seqlens, fp32 tables [S, d]:
    randn (distinct halves, no unit norm) | real (oracle.vision.vision_rotary_tables) | cancel, cancel_k (module docstring)"""
    lens = vision_segments(form, H)
    S = sum(lens)
    g_ = rw.gen(1000 * d + 10 * H + VISION_FORMS.index(form))
    qkv = torch.randn(S, 3, H, d, generator=g_).to(BF)
    if tables == "real":
        cos, sin = ovis.vision_rotary_tables(torch.randint(0, 32, (S, 2), generator=g_), d)
    else:
        cos, sin = torch.randn(S, d, generator=g_), torch.randn(S, d, generator=g_)
        if tables in ("cancel", "cancel_k"):
            # cancel: q head 0 is the cancelled operand (guards the rotation in the query loads), k head 0 the scaled one;
            # cancel_k: k head 0 is cancelled (the key loads, the key pre-pass, the NULL-workspace form), q head 0 scaled.
            # the cancelled one: |x| in [0.5, 1.5) (every partner can be cancelled against); the other: times 2^14, so that the
            # scores of head 0 -- all the attention output shows of q and k -- are of order 1 although one side is 2^-15 of its terms
            small, big = (0, 1) if tables == "cancel" else (1, 0)
            qkv[:, small, 0] = ((0.5 + torch.rand(S, d, generator=g_)) * (2.0 * torch.randint(0, 2, (S, d), generator=g_) - 1.0)).to(BF)
            qkv[:, big, 0] = (qkv[:, big, 0].float() * 2.0 ** 14).to(BF)
            a = qkv[:, small, 0].float()
            r = ovis.rotate_half(a)
            s = -(a * cos) / r * (1.0 + 2.0 ** -15 * torch.randn(S, d, generator=g_))
            sin = torch.where(torch.isfinite(s) & (r.abs() >= 0.25), s, sin)          # (a small partner would need a huge sin: left randn)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return dict(qkv=qkv, cos=cos.contiguous(), sin=sin.contiguous(), cu=cu, max_seqlen=VISION_MAX_SEQLEN[form], lens=lens, d=d, H=H, form=form)


def vision_rotated(c: Dict, emu: Optional[Callable] = None) -> torch.Tensor:
    """the qkv buffer with q and k rotated on the CPU (oracle.vision.apply_rotary_pos_emb_vision, or `emu`)"""
    fn = emu or ovis.apply_rotary_pos_emb_vision
    out = c["qkv"].clone()
    out[:, 0], out[:, 1] = fn(c["qkv"][:, 0], c["qkv"][:, 1], c["cos"], c["sin"])
    return out


VISION_WRONG = ("fma", "fma_other", "half")


def emu_vision(q, k, cos, sin, wrong: str = ""):
    """the kernel's arithmetic: fp32 x * cos, fp32 rotate_half(x) * sin, fp32 sum, bf16.  wrong: "fma" (x * cos exact inside a fused
    multiply-add), "fma_other" (the other product is the fused one), "half" (the upper half reads the lower half's table piece)"""
    d = q.shape[-1]
    if wrong == "half":
        cos, sin = (torch.cat([t[:, :d // 2], t[:, :d // 2]], -1) for t in (cos, sin))
    c, s = cos.unsqueeze(-2).float(), sin.unsqueeze(-2).float()

    def rot(x):
        x = x.float()
        r = ovis.rotate_half(x)
        if wrong == "fma":                             # (a bf16 times an fp32 value is exact in float64)
            return (x.double() * c.double() + (r * s).double()).float().to(BF)
        if wrong == "fma_other":
            return ((x * c).double() + r.double() * s.double()).float().to(BF)
        return ((x * c) + (r * s)).to(BF)
    return rot(q), rot(k)


def vision_report(got: torch.Tensor, expected: torch.Tensor) -> str:
    return rotation_mismatches(got, expected, names=("token", "head", "channel"))


# =============================================================================================================================
# the launch plan of a site, from the library itself (no device: a call with a NULL workspace is refused with the plan in the message)
# =============================================================================================================================
def stated_plan(s: Site) -> Tuple[str, int, bool]:
    """(kernel, KV splits, rope pre-pass) by tests/adversarial.swa_dispatch, the restatement test_swa_plan_cpu.py holds against the library"""
    if s.kernel == "ring256":
        return "ring256", 1, False
    kern, nsplit = adv.swa_dispatch(s.B, s.T, s.Hq, s.Hkv, s.W, rows=s.entry in ("decode_rows", "hold", "rows") and s.T * (s.Hq // s.Hkv) <= 64)
    return kern, nsplit, kern == "prefill" and (nsplit > 1 or s.T >= 512)

"""Helpers for the weight-only MXFP4 projections (CPU only, pure torch; the pattern of tests/w8.py):

  ivl_linear_small_m_w4_fwd / ivl_linear_swiglu_small_m_w4_fwd / ivl_norm_linear_small_m_w4_fwd / ivl_gdn_out_linear_small_m_w4_fwd

  * an INDEPENDENT restatement of ops.quantize_rows_mxfp4: the block exponent by a search in float64 (the smallest e with
    amax <= 6 2^e -- no frexp rule), the codes by the nearest entry of the decoded e2m1 table, ties to the even code;
  * an INDEPENDENT restatement of the shuffled layout of include/ivl_hip.h, byte offset by byte offset (shuffle_ref);
  * the exact-integer probe of tests/projections.py on 4-bit weights.  "index" and "ties": the probe's weights {-1, 0, +1} are
    the exact e2m1 codes 0xA, 0x0, 0x2; "index" gives every block of 32 its own exponent in -2 .. 2 (and keeps a quarter of the
    non-zeros, so that the scaled sums keep the probe's spread), "ties" gives every ROW one exponent, different between rows
    (a power of two keeps a tie a tie; it runs without the bias, as in w8).  "codes": all 16 codes drawn uniformly, x integers in
    -3 .. 3, block exponents in -2 .. 2: every term is a multiple of 2^-3 and every sum lies below 2^21, so fp32 accumulation
    is exact IN ANY ORDER here too -- it is there to meet every code, the -0 code and both nibbles, not the probe's spread.
    In all of them the output must be bf16_RNE(float64 sum + bias) BIT FOR BIT.  The probe's own conditions (index: at most 1 %
    of the sums above 256; ties: at least 10 % ties) are evaluated on the SCALED float64 sums; the draw of exponents is the
    first of a seeded sequence for which they hold;
  * an fp32 emulation of the stated order (w8.emu_chain on the per-block scaled weights), honest or with one deliberate defect.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

import projections as pj
import rowwise as rw
import w8

BF = torch.bfloat16
E_RANGE = (-2, 2)                                          # the probe's block exponents
BLOCK, TILE = 32, 2048
KEEP = 0.25                                                # index: mean(4^e), e uniform in -2 .. 2, is 4.26
WRONG = ("nibbles_swapped", "scale_of_neighbour", "scales_unshuffled", "mantissa_ignored", "ties_to_odd")
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)

# (glu, norm, N or I, K, Ms, variant): a lane boundary (K = 32: 4 chunks; 544: 68), a tile boundary (2016 / 2048 / 2080), two NORM
# vectors per thread (4096), every rows-per-wave branch with a column tail (4099, 8197; GLU 4099) at K = 512
PROBE: List[Tuple[bool, bool, int, int, Tuple[int, ...], str]] = (
    [(False, False, 5, K, (1, 2, 3, 4), "index") for K in (32, 512, 544, 2016, 2048, 2080)]
    + [(False, False, 4099, 512, (1, 4), "index"), (False, False, 8197, 512, (1, 4), "index")]
    + [(False, False, 5, K, (1, 2, 3, 4), "ties") for K in (544, 2080)] + [(False, False, 4099, 512, (1, 4), "ties")]
    + [(False, False, 5, K, (1, 2, 3, 4), "codes") for K in (32, 544, 2080)] + [(False, False, 4099, 512, (1, 4), "codes")]
    + [(True, False, 7, K, (1, 2, 3, 4), "index") for K in (32, 544, 2080)] + [(True, False, 4099, 512, (1, 4), "index")]
    + [(False, True, 5, K, (1, 2, 3, 4), "index") for K in (512, 544, 2080, 4096)]
    + [(True, True, 7, K, (1, 2, 3, 4), "index") for K in (544, 4096)])


# =============================================================================================================================
# e2m1 / e8m0 by the formula, the quantiser restated
# =============================================================================================================================
def decode_e2m1(nib: torch.Tensor) -> torch.Tensor:
    """4-bit codes -> float64: bit 3 the sign, bits 2..1 the exponent (bias 1), bit 0 the mantissa; exponent 0 = subnormal (m / 2)"""
    c = nib.to(torch.int64)
    s, ex, m = (c >> 3) & 1, (c >> 1) & 3, c & 1
    v = torch.where(ex == 0, m.double() * 0.5, (2 + m).double() * rw._pow2(ex - 2))
    return torch.where(s == 1, -v, v)


def unpack(codes: torch.Tensor) -> torch.Tensor:
    """bytes [N,K/2] -> 4-bit codes [N,K] (int64): element 2j in the low nibble of byte j"""
    c = codes.to(torch.int64)
    return torch.stack([c & 15, c >> 4], -1).view(codes.shape[0], -1)


def pack(nib: torch.Tensor) -> torch.Tensor:
    n = nib.to(torch.int64).view(nib.shape[0], -1, 2)
    return (n[..., 0] | (n[..., 1] << 4)).to(torch.uint8)


def encode_e2m1(v: torch.Tensor) -> torch.Tensor:
    """float64, |v| <= 6 -> 4-bit codes: the nearest table entry, ties to the even code; the sign bit is signbit(v)"""
    a = v.abs().double()
    assert bool((a <= 6.0).all())
    hi = torch.bucketize(a, E2M1).clamp(max=7)             # first table entry >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - E2M1[lo], E2M1[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    return torch.where(pick_hi, hi, lo) + 8 * torch.signbit(v).to(torch.int64)


def block_exponents_ref(w: torch.Tensor) -> torch.Tensor:
    """int64 [N,K/32]: the smallest integer e with amax(block) <= 6 2^e, by a search in float64; 0 for a zero block"""
    amax = w.double().view(w.shape[0], -1, BLOCK).abs().amax(2)
    e = torch.zeros_like(amax, dtype=torch.int64)
    nz = amax > 0
    for _ in range(400):
        up = nz & (amax > 6.0 * rw._pow2(e))
        down = nz & ~up & (amax <= 6.0 * rw._pow2(e - 1))
        if not bool((up | down).any()):
            return e
        e = e + up.to(torch.int64) - down.to(torch.int64)
    raise AssertionError("no exponent found")


def quantize_ref(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(codes uint8 [N,K/2], e8m0 uint8 [N,K/32], exp int32 [N,K/32])"""
    e = block_exponents_ref(w)
    v = w.double().view(w.shape[0], -1, BLOCK) / rw._pow2(e)[..., None]
    return pack(encode_e2m1(v).view(w.shape[0], -1)), (e + 127).to(torch.uint8), e.to(torch.int32)


def dequantize_ref(nib: torch.Tensor, e8m0: torch.Tensor) -> torch.Tensor:
    """float64 W' [N,K] from 4-bit codes [N,K] and scale bytes [N,K/32]"""
    e = e8m0.to(torch.int64) - 127
    return (decode_e2m1(nib).view(nib.shape[0], -1, BLOCK) * rw._pow2(e)[..., None]).view(nib.shape[0], -1)


# =============================================================================================================================
# the shuffled layout, offset by offset
# =============================================================================================================================
def code_offset(c: int, b: int = 0) -> int:
    """byte b of chunk c (8 elements, 4 bytes) of a row: chunk 256 t + l + 64 u sits at 1024 t + 16 l + 4 u"""
    t, r = divmod(c, 256)
    u, l = divmod(r, 64)
    return 1024 * t + 16 * l + 4 * u + b


def scale_offset(i: int) -> int:
    """the scale of block i = 64 t + (l >> 2) + 16 u sits at 64 t + 4 (l >> 2) + u"""
    t, r = divmod(i, 64)
    u, g = divmod(r, 16)
    return 64 * t + 4 * g + u


def shuffle_ref(codes: torch.Tensor, e8m0: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """plain row-major (codes [N,K/2], e8m0 [N,K/32]) -> (wq [N,Kp/2], sq [N,Kp/32]); padding: code 0x0, scale byte 127"""
    N, Kh = codes.shape
    K = 2 * Kh
    Kp = -(-K // TILE) * TILE
    wq = torch.zeros(N, Kp // 2, dtype=torch.uint8)
    sq = torch.full((N, Kp // BLOCK), 127, dtype=torch.uint8)
    wq[:, torch.tensor([code_offset(j // 4, j % 4) for j in range(Kh)])] = codes
    sq[:, torch.tensor([scale_offset(i) for i in range(K // BLOCK)])] = e8m0
    return wq, sq


# =============================================================================================================================
# the integer probe on 4-bit weights
# =============================================================================================================================
def ternary_nibbles(w: torch.Tensor) -> torch.Tensor:
    assert bool(((w == 0) | (w.abs() == 1)).all())
    return torch.where(w == 0, 0, torch.where(w > 0, 0x2, 0xA)).to(torch.int64)


def _conditions(c: Dict, M: int) -> Optional[str]:
    """the probe's conditions on the SCALED float64 sums of one call; None = they hold"""
    if c["variant"] == "ties":
        share = float(pj.is_tie(c["S"][:M]).double().mean())
        return None if share >= pj.TIES_MIN_SHARE else f"ties: share {share:.3f}"
    if c["variant"] == "codes":
        top = float(c["S"].abs().max()) + 4.0
        return None if top < 2.0 ** 21 else f"codes: |sum + bias| up to {top}: fp32 need not be exact"
    return pj.conditions(c, M)                             # index: <= 1 % above 256, with the bias and without; GLU: the silu window


def probe_case(glu: bool, norm: bool, N: int, K: int, Ms, variant: str) -> Dict:
    """x (NORM: x, res, h, nw, xn), 4-bit codes `nib` [R,K], scale bytes `e8m0` [R,K/32], bias, S = the exact float64 sums of the
    call's input rows with W' = decode(nib) 2^e"""
    assert K % BLOCK == 0 and not (norm and variant != "index") and not (glu and variant != "index")
    base = pj.norm_case(N, K, glu, Ms) if norm else pj.int_case(4, N, K, glu, "ties" if variant == "ties" else "index", Ms)
    R = base["w"].shape[0]
    xin = base["xn"] if norm else base["x"]
    small = max(Ms) * R <= 32768
    why = None
    for try_ in range(64 if small else 8):
        g_ = rw.gen(K * 37 + N * 11 + glu + 2 * norm + 4 * len(variant) + 15485863 * try_)
        if variant == "ties":
            e = torch.randint(E_RANGE[0], E_RANGE[1] + 1, (R, 1), generator=g_)
            if R > 1 and len(e.unique()) == 1:
                e[0, 0] += 1 if int(e[0, 0]) < E_RANGE[1] else -1
            e = e.expand(R, K // BLOCK).contiguous()
            nib = ternary_nibbles(base["w"])
        else:
            e = torch.randint(E_RANGE[0], E_RANGE[1] + 1, (R, K // BLOCK), generator=g_)
            if variant == "codes":
                nib = torch.randint(0, 16, (R, K), generator=g_)
            else:
                nib = ternary_nibbles(base["w"] * (torch.rand(R, K, generator=g_) < KEEP).to(BF))
        e8m0 = (e + 127).to(torch.uint8)
        c = dict(base, nib=nib, e8m0=e8m0, S=pj.exact_sum(xin, dequantize_ref(nib, e8m0)), variant=variant)
        why = next((w_ for w_ in (_conditions(c, M) for M in Ms) if w_), None)
        if why is None:
            if variant == "ties":
                assert R == 1 or len(e[:, 0].unique()) > 1
            if variant == "codes":
                assert set(nib.unique().tolist()) == set(range(16))
            return c
    raise AssertionError(f"no draw meets the probe's conditions: {why}")


def check_linear(run, c: Dict, Ms) -> pj.Counted:
    """run(x, nib [R,K], e8m0 [R,K/32], bias or None, glu) -> y [M, N]: every M, with the bias and without (ties: without)"""
    rep = pj.Counted(f"w4 {'glu' if c['glu'] else 'plain'} {c['variant']} N={c['N']} K={c['K']}")
    for M in Ms:
        why = _conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in (False,) if c["variant"] == "ties" else (False, True):
            y = run(c["x"][:M], c["nib"], c["e8m0"], c["bias"] if wb else None, c["glu"])
            pj._judge(rep, (M, "bias" if wb else ""), y, c["S"][:M] + (c["bias"].double() if wb else 0.0), c["glu"])
    return rep


def check_norm_linear(run, c: Dict, Ms) -> pj.Counted:
    """run(x, residual or None, norm weight, eps, nib, e8m0, bias or None, glu) -> (y, h_out or None)"""
    rep = pj.Counted(f"w4 norm {'glu' if c['glu'] else 'plain'} N={c['N']} K={c['K']}")
    for M in Ms:
        why = _conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in (False, True):
            for wr in (False, True):
                y, h = run((c["x"] if wr else c["h"])[:M], c["res"][:M] if wr else None, c["nw"], c["eps"], c["nib"], c["e8m0"],
                           c["bias"] if wb else None, c["glu"])
                tag = (M, "bias" if wb else "", "residual" if wr else "")
                pj._judge(rep, tag, y, c["S"][:M] + (c["bias"].double() if wb else 0.0), c["glu"])
                if wr:
                    rep.exact(tag + ("h_out",), h, c["h"][:M].double())
    return rep


# =============================================================================================================================
# fp32 emulation of the stated order
# =============================================================================================================================
def _bf16_ties_to_odd(v: torch.Tensor) -> torch.Tensor:
    bits = v.float().contiguous().view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    odd = (((bits >> 16) | 1) << 16).view(torch.float32)
    return torch.where(tie, odd, v.float().to(BF).float()).to(BF)


def emu_w4_linear(x, nib, e8m0, bias, glu, wrong: str = "") -> torch.Tensor:
    R, K = nib.shape
    if wrong == "nibbles_swapped":
        nib = nib.view(R, K // 2, 2).flip(-1).reshape(R, K)
    if wrong == "mantissa_ignored":
        nib = nib & ~1
    if wrong == "scale_of_neighbour":
        e8m0 = e8m0.roll(1, 1)
    if wrong == "scales_unshuffled":                       # the kernel's offsets into a scale row that was left in plain order
        nb = K // BLOCK
        plain = torch.nn.functional.pad(e8m0, (0, -(-K // TILE) * (TILE // BLOCK) - nb), value=127)
        e8m0 = plain[:, torch.tensor([scale_offset(i) for i in range(nb)])]
    acc = w8.emu_chain(x, dequantize_ref(nib, e8m0).float())
    v = acc + (torch.zeros(R) if bias is None else bias.float())
    out = _bf16_ties_to_odd(v) if wrong == "ties_to_odd" else v.to(BF)
    return rw.emu_silu_mul(out) if glu else out


def emu_w4_norm_linear(x, res, nw, eps, nib, e8m0, bias, glu, wrong: str = ""):
    xn, _ = rw.emu_add_rmsnorm(x, res, nw, eps)
    h_out = None if res is None else (x.float() + res.float()).to(BF)
    return emu_w4_linear(xn, nib, e8m0, bias, glu, wrong), h_out

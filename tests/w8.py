"""Helpers for the weight-only e4m3 projections (CPU only, pure torch; the pattern of tests/projections.py):

  ivl_linear_small_m_w8_fwd / ivl_linear_swiglu_small_m_w8_fwd / ivl_norm_linear_small_m_w8_fwd / ivl_gdn_out_linear_small_m_w8_fwd

  * an INDEPENDENT restatement of ops.quantize_rows_e4m3: the exponent by a search in float64 (the smallest e with
    amax <= 448 2^e -- no frexp rule), the codes by the nearest entry of the decoded e4m3fn table, ties to the even code;
  * the float64 expectation of an entry point, bf16(scale * exact_sum + bias) in ONE rounding;
  * the exact-integer probe of tests/projections.py with per-row scales 2^e: the probe's weights {-1, 0, +1} are exact e4m3
    values (codes 0xB8, 0x00, 0x38), x and the bias are small integers, so scale * sum + bias is exact in fp32 in ANY order and
    the output must be bf16_RNE(2^e sum + bias) BIT FOR BIT.  The probe's own conditions (at most 1 % of the sums above 256, at
    least 10 % ties) are evaluated on the float64 sums of the case, as projections.conditions does; a power of two keeps a tie a
    tie, so the ties variant runs without the bias;
  * an fp32 emulation of the stated order (lane l adds the 8 products of chunk l + 64 i with fmaf, i ascending; pieces past the
    row end add fmaf(w, 0, acc); wave_sum's xor butterfly), honest or with one deliberate defect.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

import projections as pj
import rowwise as rw

BF = torch.bfloat16
E_RANGE = (-3, 3)                                          # the probe's per-row exponents
WRONG = ("scale_after_rounding", "bias_scaled", "scale_of_neighbour", "fnuz_decode")


# =============================================================================================================================
# OCP e4m3fn (and, for the judge self-test, e4m3fnuz) by the formula
# =============================================================================================================================
def decode_e4m3fn(codes: torch.Tensor) -> torch.Tensor:
    """uint8 -> float64: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 = subnormal (m 2^-9); 0x7F / 0xFF = NaN"""
    c = codes.to(torch.int64)
    s, ex, m = c >> 7, (c >> 3) & 15, c & 7
    v = torch.where(ex == 0, m.double() * 2.0 ** -9, (8 + m).double() * rw._pow2(ex - 10))
    v = torch.where((c & 0x7F) == 0x7F, torch.full_like(v, float("nan")), v)
    return torch.where(s == 1, -v, v)


def decode_e4m3fnuz(codes: torch.Tensor) -> torch.Tensor:
    """the MI300 encoding (bias 8, 0x80 = NaN, no negative zero): what a gfx942 conversion would make of the same bytes"""
    c = codes.to(torch.int64)
    s, ex, m = c >> 7, (c >> 3) & 15, c & 7
    v = torch.where(ex == 0, m.double() * 2.0 ** -10, (8 + m).double() * rw._pow2(ex - 11))
    v = torch.where(s == 1, -v, v)
    return torch.where(c == 0x80, torch.full_like(v, float("nan")), v)


_GRID = decode_e4m3fn(torch.arange(127, dtype=torch.uint8))          # the 127 finite magnitudes, ascending with the code


def encode_e4m3fn(v: torch.Tensor) -> torch.Tensor:
    """float64, |v| <= 448 -> uint8: the nearest e4m3fn value, ties to the even code (= the even mantissa)"""
    a = v.abs().double()
    assert bool((a <= 448.0).all())
    hi = torch.bucketize(a, _GRID).clamp(max=126)          # first grid value >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - _GRID[lo], _GRID[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    code = torch.where(pick_hi, hi, lo)
    return (code + 128 * torch.signbit(v).to(torch.int64)).to(torch.uint8)          # (a negative value keeps its sign at zero)


def quantize_ref(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(codes uint8 [N,K], exp int32 [N], scale fp32 [N]): per row the smallest integer e with max|w| <= 448 2^e, found by a
    search in float64 (every product with a power of two is exact); e = 0 for a zero row"""
    wd = w.double()
    amax = wd.abs().amax(1)
    e = torch.zeros_like(amax, dtype=torch.int64)
    nz = amax > 0
    for _ in range(400):
        up = nz & (amax > 448.0 * rw._pow2(e))
        down = nz & ~up & (amax <= 448.0 * rw._pow2(e - 1))
        if not bool((up | down).any()):
            break
        e = e + up.to(torch.int64) - down.to(torch.int64)
    else:
        raise AssertionError("no exponent found")
    codes = encode_e4m3fn(wd / rw._pow2(e)[:, None])
    return codes, e.to(torch.int32), rw._pow2(e).float()


def dequantize_ref(codes: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """float64 W' = decode(code) 2^e"""
    return decode_e4m3fn(codes) * rw._pow2(exp.to(torch.int64))[:, None]


def expected(x: torch.Tensor, codes: torch.Tensor, exp: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """float64: bf16(2^e * exact sum + bias) in one rounding (exact_sum is exact where the probe's inputs go in)"""
    v = pj.exact_sum(x, decode_e4m3fn(codes)) * rw._pow2(exp.to(torch.int64))[None, :]
    return rw.round_bf16(v + (0.0 if bias is None else bias.double()))


# =============================================================================================================================
# the integer probe with per-row scales
# =============================================================================================================================
def ternary_codes(w: torch.Tensor) -> torch.Tensor:
    """the probe's weights {-1, 0, +1} as e4m3fn codes"""
    assert bool(((w == 0) | (w.abs() == 1)).all())
    return torch.where(w == 0, 0, torch.where(w > 0, 0x38, 0xB8)).to(torch.uint8)


def probe_exponents(c: Dict, Ms) -> torch.Tensor:
    """int64 [R], drawn from E_RANGE; GLU: the first draw whose scaled [gate | up] keeps rowwise.silu_ref's window rule for every
    M and with the bias and without (the seed search of projections._seeded)"""
    R = c["w"].shape[0]
    small = max(Ms) * R <= 32768
    for try_ in range(64 if small else 8):
        e = torch.randint(E_RANGE[0], E_RANGE[1] + 1, (R,), generator=rw.gen(c["K"] * 31 + c["N"] * 7 + 104729 * try_))
        if not c["glu"]:
            return e
        ok = True
        for M in Ms:
            for b in (None, c["bias"]):
                v = c["S"][:M] * rw._pow2(e)[None, :] + (0.0 if b is None else b.double())
                ok = ok and rw.window_ok(rw.silu_ref(rw.round_bf16(v).to(BF))["window"])
        if ok:
            return e
    raise AssertionError("no draw of exponents keeps the silu window rule")


def check_linear(run, c: Dict, Ms, e: torch.Tensor) -> pj.Counted:
    """run(x, codes, scale fp32, bias or None, glu) -> y [M, N]: every M, with the bias and without (ties: without)"""
    rep = pj.Counted(f"w8 {'glu' if c['glu'] else 'plain'} {c['variant']} N={c['N']} K={c['K']}")
    codes, scale = ternary_codes(c["w"]), rw._pow2(e).float()
    assert torch.equal(decode_e4m3fn(codes), c["w"].double())
    for M in Ms:
        why = pj.conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in (False,) if c["variant"] == "ties" else (False, True):
            v = c["S"][:M] * rw._pow2(e)[None, :] + (c["bias"].double() if wb else 0.0)
            if c["variant"] == "ties" and not float(pj.is_tie(v).double().mean()) >= pj.TIES_MIN_SHARE:
                rep.fails.append((M, "the scaled sums lost their ties"))
            y = run(c["x"][:M], codes, scale, c["bias"] if wb else None, c["glu"])
            pj._judge(rep, (M, "bias" if wb else ""), y, v, c["glu"])
    return rep


def check_norm_linear(run, c: Dict, Ms, e: torch.Tensor) -> pj.Counted:
    """run(x, residual or None, norm weight, eps, codes, scale, bias or None, glu) -> (y, h_out or None)"""
    rep = pj.Counted(f"w8 norm {'glu' if c['glu'] else 'plain'} N={c['N']} K={c['K']}")
    codes, scale = ternary_codes(c["w"]), rw._pow2(e).float()
    for M in Ms:
        why = pj.conditions(c, M)
        if why:
            rep.fails.append((M, "the probe's conditions do not hold: " + why))
        for wb in (False, True):
            for wr in (False, True):
                y, h = run((c["x"] if wr else c["h"])[:M], c["res"][:M] if wr else None, c["nw"], c["eps"], codes, scale,
                           c["bias"] if wb else None, c["glu"])
                tag = (M, "bias" if wb else "", "residual" if wr else "")
                pj._judge(rep, tag, y, c["S"][:M] * rw._pow2(e)[None, :] + (c["bias"].double() if wb else 0.0), c["glu"])
                if wr:
                    rep.exact(tag + ("h_out",), h, c["h"][:M].double())
    return rep


# =============================================================================================================================
# fp32 emulation of the stated order
# =============================================================================================================================
def _fmaf(a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """fp32 fmaf: the product of an e4m3 value and a bf16 value has 12 significant bits, so product + acc in float64 is exact
    unless the two lie more than 2^28 apart (then the float64 sum rounds once before the fp32 rounding: not met by these inputs)"""
    return (a.double() * b.double() + acc.double()).float()


def emu_chain(x: torch.Tensor, wf: torch.Tensor) -> torch.Tensor:
    """x [M,K] bf16, wf [R,K] fp32 (decoded codes) -> acc fp32 [M,R] in the kernels' order"""
    M, K = x.shape
    R = wf.shape[0]
    assert K % 8 == 0
    nchunk = K // 8
    trips = (nchunk + 63) // 64
    pad = trips * 512 - K
    xf = torch.nn.functional.pad(x.float(), (0, pad)).view(M, 1, trips, 64, 8)
    # a piece past the row end: the LAST piece's weights (the clamp) against zeros
    wp = torch.cat([wf, wf[:, -8:].repeat(1, pad // 8)], 1).view(1, R, trips, 64, 8)
    acc = torch.zeros(M, R, 64)
    for i in range(trips):
        for k in range(8):
            acc = _fmaf(wp[:, :, i, :, k], xf[:, :, i, :, k], acc)
    for o in (32, 16, 8, 4, 2, 1):                          # wave_sum: v += shfl_xor(v, o)
        acc = acc + acc[..., torch.arange(64) ^ o]
    return acc[..., 0]


def emu_w8_linear(x, codes, scale, bias, glu, wrong: str = "") -> torch.Tensor:
    wf = (decode_e4m3fnuz(codes) if wrong == "fnuz_decode" else decode_e4m3fn(codes)).float()
    acc = emu_chain(x, wf)
    R = codes.shape[0]
    b = torch.zeros(R) if bias is None else bias.float()
    sc = scale.float().roll(1) if wrong == "scale_of_neighbour" else scale.float()
    if wrong == "scale_after_rounding":
        v = (acc + b).to(BF).float() * sc
    elif wrong == "bias_scaled":
        v = sc * (acc + b)
    else:
        v = sc * acc + b
    return rw.emu_silu_mul(v.to(BF)) if glu else v.to(BF)


def emu_w8_norm_linear(x, res, nw, eps, codes, scale, bias, glu, wrong: str = ""):
    xn, _ = rw.emu_add_rmsnorm(x, res, nw, eps)
    h_out = None if res is None else (x.float() + res.float()).to(BF)
    return emu_w8_linear(xn, codes, scale, bias, glu, wrong), h_out

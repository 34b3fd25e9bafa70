"""Host reference, case builders and the judge of the guidance launch (ivl_logit_guide_fwd, GUIDE-0 .. GUIDE-5 in
include/ivl_hip.h; ops.guide_logits) and of ops.rows_follow.  CPU only, numpy only.

THE REFERENCE is float64 on the bf16 inputs: the two rows' exact log-softmaxes lc, lu (a NaN read as -inf), ref = lu + s (lc - lu)
with s and the cut taken as the fp32 values the kernel receives, and the rules for infinities of GUIDE-3.

THE JUDGE.  For a finite ref(v) the kernel's bf16 must lie in [bf16_rne(ref - E), bf16_rne(ref + E)],
    E = (2 |s| + 1) 2^-15 + 2^-22 |ref|,
i.e. it is the correctly rounded bf16, or its neighbour where ref lies within E of a rounding boundary.  Infinities must match
exactly, and no element is excused.

WHERE E COMES FROM.  The kernel's stated arithmetic (GUIDE-1, GUIDE-2) in fp32, for finite logits within 64 of their row's maximum
(what the builders emit) and V < 2^23:
  * dc = c(v) - mc: one rounding of a value of at most 64, at most 2^-24 * 64 = 3.8e-6 (often exact).
  * L: the Q40 weights carry the error tests/sampling.py derives for them, at most about 32 * 2^-23 relative each, so does
    their sum Z; the floor of each weight and the weights below 2^-40 that count as 0 add at most V 2^-40 < 2^-17 relative at
    the model's vocabulary; (float)Z adds 2^-24.  Together below 3.9e-6 on L = log Z.  logf is within 2 ulp of a value below 16
    (ln V < 16): 1.9e-6.  L is off by at most 5.8e-6.
  * lc = dc - Lc: |lc| < 64 + 16 < 128, one rounding: 7.6e-6.  So lc (and lu) is off by at most 3.8 + 5.8 + 7.6 = 17.2e-6.
  * lc - lu: both lie in (-80, 0], the difference is below 128 in size: one rounding, 7.6e-6.
  * y = fmaf(s, lc - lu, lu): one rounding, 2^-24 |y|; the errors above arrive as |s| (2 * 17.2 + 7.6)e-6 + 17.2e-6.
  Total: |s| 4.2e-5 + 1.7e-5 + 2^-24 |y|, against E = |s| 6.1e-5 + 3.05e-5 + 2^-22 |ref|: a margin of 1.4 on the scale's term,
  1.8 on the constant and 4 on the last rounding.  The bound was fixed before the kernel ran; if the kernel cannot meet the
  stated sequence, the kernel is wrong, not E.

THE CUT is a comparison of fp32(c(v) - mc) with cut, so an element whose exact difference lies within a rounding of the cut could
fall either way.  Only one side can: cut is an fp32 value and rounding is monotone, so dc >= cut stays; dc < cut flips only if it
rounds up to cut, within 2^-24 |cut|.  The builders emit only rows in which no element has 0 < cut - (c - mc) < 2^-16 |cut|
(margin_ok), and the CPU test asserts that for every case."""
import numpy as np

NINF_BITS = np.int16(-128)                  # 0xFF80: bf16 -inf
SPAN = 64.0                                 # the builders keep finite logits within this of their row's maximum
MAX_SCALE = 8.0


def bf16_value(bits):
    """int16 / uint16 bf16 bit patterns -> float32"""
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_bits(x):
    """float32 values that ARE bf16 values -> int16 bit patterns"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    assert (u & 0xFFFF == 0).all(), "not bf16 values"
    return (u >> 16).astype(np.uint16).view(np.int16)


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64; straight from float64, no rounding in between.  Finite
    inputs well inside bf16's range (the judge's: log-probabilities times a scale of at most 8)."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                                   # |x| = m 2^e, m in [0.5, 1)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)                           # 8 significant bits; bf16's subnormal spacing below 2^-126
    return np.rint(x / q) * q


def to_bf16(x):
    """float64 -> bf16 bits (int16), round to nearest even; +-inf stay"""
    x = np.asarray(x, dtype=np.float64)
    out = np.where(np.isfinite(x), bf16_rne(np.where(np.isfinite(x), x, 0.0)), x)
    return bf16_bits(out.astype(np.float32))


def guided(partner, scale, done, r):
    """GUIDE-0: is row r a guided leader"""
    S, p = len(partner), int(partner[r])
    if not 0 <= p < S or p == r:
        return False
    pp = int(partner[p])
    if 0 <= pp < S and pp != p:
        return False
    return bool(np.isfinite(np.float32(scale[r]))) and (done is None or int(done[r]) == 0)


def followers(partner):
    """{partner row: its lowest valid leader} (GUIDE-0 without the done and scale clauses)"""
    S, out = len(partner), {}
    for r in range(S):
        if guided(partner, np.zeros(S, np.float32), None, r):
            out.setdefault(int(partner[r]), r)
    return out


def log_softmax64(x):
    """float64 log-softmax of one row of bf16 values, a NaN read as -inf; an all -inf row stays all -inf"""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(np.isnan(x), -np.inf, x)
    m = x.max()
    if m == -np.inf:
        return x, m
    d = x - m
    return d - np.log(np.exp(d).sum()), m


def ref_row(c_bits, u_bits, s, cut):
    """GUIDE-1..3 in float64 on the bf16 rows c, u (bit patterns, [V]); s and cut: the fp32 values of the launch"""
    s, cut = float(np.float32(s)), float(np.float32(cut))
    c = np.where(np.isnan(bf16_value(c_bits)), -np.inf, bf16_value(c_bits).astype(np.float64))
    lc, mc = log_softmax64(c)
    lu, _ = log_softmax64(bf16_value(u_bits))
    with np.errstate(invalid="ignore"):
        y = np.where(np.isneginf(lu), lc, lu + s * (lc - lu))
        y = np.where(np.isneginf(lc), -np.inf, y)
        if mc > -np.inf:
            y = np.where(((c - mc) < cut) & (c != mc), -np.inf, y)       # the leader's maximum always survives
    return y


def margin_ok(c_bits, cut):
    """the builders' condition: no element of the leader's row within 2^-16 |cut| below the cut"""
    cut = float(np.float32(cut))
    if not np.isfinite(cut):
        return True
    c = bf16_value(c_bits).astype(np.float64)
    c = np.where(np.isnan(c), -np.inf, c)
    m = c.max()
    if m == -np.inf:
        return True
    with np.errstate(invalid="ignore"):
        gap = cut - (c - m)
    return not bool(((gap > 0) & (gap < 2.0 ** -16 * abs(cut))).any())


def reference(bits, V, partner, scale, cut, done=None):
    """{leader row: float64 [V]} of a call over the bit patterns bits [S, ld]"""
    return {r: ref_row(bits[r, :V], bits[int(partner[r]), :V], scale[r], cut[r])
            for r in range(len(partner)) if guided(partner, scale, done, r)}


def tolerance(ref, s):
    return (2.0 * abs(float(np.float32(s))) + 1.0) * 2.0 ** -15 + 2.0 ** -22 * np.abs(ref)


def judge(out_bits, ref, s):
    """(indices outside the bound, the number of finite elements that are not the correctly rounded bf16) of one row"""
    out = bf16_value(out_bits).astype(np.float64)
    fin = np.isfinite(ref)
    bad = np.zeros(ref.shape, dtype=bool)
    bad[~fin] = ~((out[~fin] == ref[~fin]))                              # infinities match exactly (a NaN equals nothing)
    E = tolerance(ref[fin], s)
    lo, hi = bf16_rne(ref[fin] - E), bf16_rne(ref[fin] + E)
    with np.errstate(invalid="ignore"):
        bad[fin] = ~((out[fin] >= lo) & (out[fin] <= hi))
    near = int((out[fin] != bf16_rne(ref[fin])).sum())
    return np.nonzero(bad)[0], near


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
def random_bits(rows, ld, seed):
    """random 16-bit patterns: NaN payloads, -0, +-inf, subnormals"""
    return np.random.default_rng(seed).integers(-2 ** 15, 2 ** 15, size=(rows, ld)).astype(np.int16)


def logit_row(V, rng, spread=3.0, ninf=0.0, shift=0.0):
    """a row of bf16 logits: normal(shift, spread) rounded to bf16, every finite one within SPAN of the maximum; a fraction
    `ninf` of the elements -inf"""
    x = rng.normal(shift, spread, size=V)
    b = bf16_value(to_bf16(x)).astype(np.float64)
    b = np.maximum(b, bf16_rne(b.max() - SPAN + 1.0))
    if ninf > 0.0:
        b = np.where(rng.random(V) < ninf, -np.inf, b)
    return to_bf16(b)


def pair_rows(V, seed, s, beta=0.0, spread=3.0, u_ninf=0.0, c_ninf=0.0):
    """(c bits, u bits, fp32 s, fp32 cut) of one guided pair; u is c plus noise (a negative prompt's logits resemble the
    prompt's).  With a cut the leader's row is redrawn until margin_ok holds."""
    assert abs(s) <= MAX_SCALE and 0.0 <= beta < 1.0
    cut = np.float32(np.log(beta)) if beta > 0.0 else np.float32(-np.inf)
    for k in range(64):
        rng = np.random.default_rng([seed, k])
        c = logit_row(V, rng, spread, c_ninf)
        if margin_ok(c, cut):
            break
    else:
        raise AssertionError("no row with the margin")
    cv = bf16_value(c).astype(np.float64)
    base = np.where(np.isfinite(cv), cv, 0.0) + rng.normal(0.0, 1.0, size=V)
    u = bf16_value(to_bf16(base)).astype(np.float64)
    u = np.maximum(u, bf16_rne(u.max() - SPAN + 1.0))
    if u_ninf > 0.0:
        u = np.where(rng.random(V) < u_ninf, -np.inf, u)
    return c, to_bf16(u), np.float32(s), cut


# the pairs (leader, partner) of the operator tests' calls of S = 6 rows; the rows between them are off
LAYOUTS = (((0, 1), (2, 5)), ((3, 0), (2, 5)))
# (s, beta, u_ninf, c_ninf) of the two pairs of a call, by variant
VARIANTS = {
    "plain": ((1.5, 0.0, 0.0, 0.0), (3.0, 0.1, 0.0, 0.0)),
    "edges": ((0.0, 0.0, 0.3, 0.0), (1.0, 0.0, 0.0, 0.2)),
    "harsh": ((8.0, 0.999, 0.0, 0.0), (-2.0, 0.5, 0.5, 0.1)),
}


def call(V, ld, layout, variant, seed):
    """One call of S = 6 rows over bits [7, ld] (a guard row behind): the two pairs of `layout` with the parameters of
    `variant`; the other rows are OFF in the ways GUIDE-0 lists -- random bit patterns (NaN payloads) with partner -1 / S / the
    row itself, and one row with a valid partner but done != 0.  Everything outside the pairs' first V columns is random bits."""
    S = 6
    bits = random_bits(S + 1, ld, seed)
    partner = np.full(S, -1, dtype=np.int32)
    scale = np.full(S, 2.5, dtype=np.float32)
    cut = np.full(S, np.log(0.3), dtype=np.float32)
    done = np.zeros(S, dtype=np.int32)
    for i, ((r, p), (s, beta, u_ninf, c_ninf)) in enumerate(zip(layout, VARIANTS[variant])):
        c, u, s32, cut32 = pair_rows(V, seed * 16 + i, s, beta, u_ninf=u_ninf, c_ninf=c_ninf)
        bits[r, :V], bits[p, :V] = c, u
        partner[r], scale[r], cut[r] = p, s32, cut32
    used = {x for pr in layout for x in pr}
    first, last = [r for r in range(S) if r not in used]                 # the two rows that are off
    partner[first] = S if seed % 2 else first                            # out of range above / the row itself (else: -1 stays)
    if seed % 3 == 0:
        partner[first] = -1
    partner[last], done[last] = layout[0][1], 1 + seed % 4               # a valid partner: `done` alone switches the row off
    return dict(V=V, ld=ld, bits=bits, partner=partner, scale=scale, cut=cut, done=done, leaders=[r for r, _ in layout])


def all_cases():
    """the cases the CPU test checks the builders on (small V; the GPU test builds its own at its sizes with the same call())"""
    return [call(V, V + 3 + (V % 2 == 1), layout, variant, 100 * i + j)
            for i, V in enumerate((1, 7, 8, 9, 1023, 1025)) for j, (layout, variant) in
            enumerate((l, v) for l in LAYOUTS for v in VARIANTS)]

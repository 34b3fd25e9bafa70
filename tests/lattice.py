"""Exact-lattice probes of the Gated DeltaNet operators (CPU only, pure torch; no GPU import).

With use_qk_l2norm_in_kernel=False, a power-of-two scale, keys that are SIGNED ONE-HOT rows, small-integer q / v / h0, beta in
{0, 1} and g in {0, -200} (exp(0) = 1 and exp(-200) = 0 exactly in fp32) the gated delta rule is a key/value memory: write a
row, overwrite it, forget everything, read rows back.  Every intermediate of the chunk form -- L, (I + L)^-1, w, u, v_new, Aqk,
the state, the output -- is then a small integer that bf16 (and, at or below 16, e4m3) represents exactly, so no rounding point
of a kernel can show and a kernel must equal the token-by-token definition BIT FOR BIT, element by element.

  lattice_case        inputs on the lattice ("memory", "half", "onehot_q", "still")
  lattice_expected    the token-by-token rule in float64, l2norm off
  lattice_features    what a case actually exercises (rewrites in a chunk / across a seam, wipes, reads ...)
  lattice_required    what a case of its kind and length has to exercise
  lattice_mismatches  the first differing elements, named by token, chunk, row in chunk, head and column

tests/test_lattice_cpu.py shows that the oracle's rounding models are exact on every case the GPU file uses and that no case is
degenerate; tests/test_gpu_lattice.py drives the HIP kernels.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

GDN_K, GDN_V, CHUNK = 128, 256, 64
WIPE = -200.0
KINDS = ("memory", "half", "onehot_q", "still")
# largest |operand| and |intermediate| a kind may reach (asserted by lattice_expected on the state and the output, argued for the
# rest in DESIGN.md): integers up to 256 are exact in bf16, up to 16 in e4m3 (three mantissa bits)
BOUND_E4M3, BOUND_BF16 = 16.0, 256.0
HALF_DEPTH = 3            # "half": at most this many beta = 0.5 writes of one key between two beta = 1 writes of it


def slot_columns(n_slots: int) -> torch.Tensor:
    """Key slot i -> column of K: the slots go round the four 32-wide contraction blocks, 5 columns apart inside a block
    (distinct for n_slots <= 128)."""
    assert 2 <= n_slots <= GDN_K
    i = torch.arange(n_slots)
    col = 32 * (i % 4) + (5 * (i // 4)) % 32
    assert len(set(col.tolist())) == n_slots
    return col


def _one_hot_rows(col: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """[...] columns, [...] coefficients -> [..., K] rows coef * e_col"""
    out = torch.zeros(*col.shape, GDN_K)
    out.scatter_(-1, col[..., None], coef[..., None])
    return out


def lattice_case(kind: str, B: int, T: int, H: int, seed: int = 0, n_slots: int = 24, v_max: int = 4, wipe_every: int = 97,
                 with_h0: bool = True) -> Dict:
    """Inputs of one GDN operator call on the exact lattice: q, k [B,T,H,128], v [B,T,H,256], g, beta [B,T,H], h0 [B,H,128,256]
    (fp32 tensors holding lattice values), deterministic in `seed`.  Extra keys: kind, slot / qa / qb [B,T,H] (the key slot a
    token writes and the slots its query reads), bound (the case's magnitude limit, BOUND_E4M3 or BOUND_BF16).

      "memory"    k = +-e_slot over `n_slots` slots (slot_columns); a token's slot repeats the one 1, 17, 40 or 64 tokens back
                  one time in two, so the same key recurs inside a 16 x 16 diagonal block of (I + L)^-1, outside it in the same
                  chunk, and across chunk seams; q = e_a - 2 e_b (a: this token's key, a key of the last 100 tokens, or any);
                  v, h0 integers in [-v_max, v_max]; beta in {0, 1, 1}; g = -200 one token in `wipe_every` (0: never), else 0.
                  Largest magnitudes: state v_max, beta (v - S^T k) and u 2 v_max, o 3 v_max (scale <= 1): 12 at v_max = 4.
      "half"      as "memory" with beta in {0, 0.5, 1} and v, h0 on multiples of 8 up to 8 v_max: bf16 only (a row that is
                  half-written m times carries m binary digits below 8).
      "onehot_q"  as "memory" with q = e_a: a unit row, on which the l2norm is the identity after rounding
                  (1 / sqrt(1 + 1e-6) rounds to 1 in bf16 and in fp16).
      "still"     beta = 0, g = 0: the state comes back as it went in; q = e_a - 2 e_b with a walking through all 128 rows
                  (a = (t + 41 (b H + h)) % 128, b = a + 64), so o_t = scale (h0[a] - 2 h0[b]) reads every state row.

    Placed by construction, per stream s = b H + h (so that no case depends on luck for them):
      even s   beta = 1 at token 0 and q reads that token's own key; T >= 2: token 1 rewrites token 0's key; T >= 3: one wipe
               strictly inside a chunk; T >= 64: one wipe at the LAST token of chunk s % (T // 64)
      odd s    at every seam t = 64 c: no wipe, beta = 1 at t - 1 and t, token t rewrites token t - 1's key and its query reads
               it (a) and the key of token t - 2 (b)."""
    assert kind in KINDS, kind
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)  # noqa: E731
    cols = slot_columns(n_slots)
    step = 8 if kind == "half" else 1
    v = (ri(-v_max, v_max + 1, B, T, H, GDN_V) * step).float()
    h0 = (ri(-v_max, v_max + 1, B, H, GDN_K, GDN_V) * step).float() if with_h0 else None
    slot = ri(0, n_slots, B, T, H)
    sign = (2 * ri(0, 2, B, T, H) - 1).float()
    lag_pick = ri(0, 8, B, T, H)
    for t in range(T):
        for code, lag in enumerate((1, 17, 40, 64)):
            if t >= lag:
                slot[:, t] = torch.where(lag_pick[:, t] == code, slot[:, t - lag], slot[:, t])
    beta = ri(0, 3, B, T, H).clamp(max=2).float()
    beta = torch.where(beta == 0, torch.zeros(()), torch.ones(())) if kind != "half" else beta * 0.5
    g = torch.zeros(B, T, H)
    if wipe_every:
        g = torch.where(ri(0, wipe_every, B, T, H) == 0, torch.full((), WIPE), g)
    q_pick, q_back = ri(0, 4, B, T, H), ri(1, 101, B, T, H)
    qa = ri(0, n_slots, B, T, H)
    tt = torch.arange(T)[None, :, None]
    back = torch.gather(slot, 1, (tt - q_back).clamp(min=0))
    qa = torch.where(q_pick == 0, slot, torch.where(q_pick == 1, back, qa))
    qb_off = ri(1, n_slots, B, T, H)

    if kind == "still":
        beta, g = torch.zeros(B, T, H), torch.zeros(B, T, H)
    else:
        for b in range(B):
            for h in range(H):
                s = b * H + h
                if s % 2 == 0:
                    beta[b, 0, h] = 1.0
                    qa[b, 0, h] = slot[b, 0, h]
                    if T >= 2:
                        slot[b, 1, h], beta[b, 1, h] = slot[b, 0, h], 1.0
                    if T >= 3:
                        t_in = 1 + (7 * s) % (T - 2)
                        t_in -= 2 if t_in % CHUNK == 0 else (1 if t_in % CHUNK == CHUNK - 1 else 0)
                        g[b, t_in, h] = WIPE
                    if T >= CHUNK:
                        g[b, CHUNK * (s % (T // CHUNK)) + CHUNK - 1, h] = WIPE
                else:
                    for t in range(CHUNK, T, CHUNK):
                        g[b, t, h] = 0.0
                        beta[b, t - 1, h] = beta[b, t, h] = 1.0
                        slot[b, t, h] = slot[b, t - 1, h]
                        qa[b, t, h] = slot[b, t, h]
                        if slot[b, t - 2, h] != slot[b, t, h]:
                            qb_off[b, t, h] = (slot[b, t - 2, h] - slot[b, t, h]) % n_slots
    if kind == "half":
        # a row half-written m times in a row carries m binary digits below 8: the fourth half-write of a key becomes a full one
        # (wipes do not reset the count: (I + L)^-1 itself does not see the gates)
        sl, bt = slot.tolist(), beta.tolist()
        for b in range(B):
            for h in range(H):
                depth: Dict[int, int] = {}
                for t in range(T):
                    if bt[b][t][h] == 0.5:
                        depth[sl[b][t][h]] = depth.get(sl[b][t][h], 0) + 1
                        if depth[sl[b][t][h]] > HALF_DEPTH:
                            beta[b, t, h] = 1.0
                    if bt[b][t][h] == 1.0 or depth.get(sl[b][t][h], 0) > HALF_DEPTH:
                        depth[sl[b][t][h]] = 0
    qb = (qa + qb_off) % n_slots
    assert bool((qa != qb).all())
    k = _one_hot_rows(cols[slot], sign)
    if kind == "still":
        s_of = (torch.arange(B)[:, None, None] * H + torch.arange(H)[None, None, :])
        ca = (tt + 41 * s_of) % GDN_K
        q = _one_hot_rows(ca, torch.ones(B, T, H)) + _one_hot_rows((ca + 64) % GDN_K, torch.full((B, T, H), -2.0))
    elif kind == "onehot_q":
        q = _one_hot_rows(cols[qa], torch.ones(B, T, H))
    else:
        q = _one_hot_rows(cols[qa], torch.ones(B, T, H)) + _one_hot_rows(cols[qb], torch.full((B, T, H), -2.0))
    bound = BOUND_BF16 if kind == "half" else BOUND_E4M3
    assert 3 * v_max * step <= bound, "o = S[a] - 2 S[b] must stay within the case's magnitude limit"
    return dict(kind=kind, q=q, k=k, v=v, g=g.contiguous(), beta=beta.contiguous(), h0=h0, slot=slot, qa=qa, qb=qb, bound=bound)


def gdn_rule_f64(q, k, v, g, beta, h0=None, scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The token-by-token definition in float64, q and k taken AS THEY ARE (l2norm off;
    fla:ops/gated_delta_rule/fused_recurrent.py:85-101): S *= exp(g_t); d = beta_t (v_t - S^T k_t); S += k_t d^T;
    o_t = S^T (q_t * scale).  -> (o [B,T,H,V], S [B,H,K,V]) float64."""
    B, T, H, K = q.shape
    V = v.shape[-1]
    qd, kd, vd, gd, bd = (x.double() for x in (q, k, v, g, beta))
    S = torch.zeros(B, H, K, V, dtype=torch.float64) if h0 is None else h0.double().clone()
    o = torch.empty(B, T, H, V, dtype=torch.float64)
    for t in range(T):
        S = S * gd[:, t].exp()[..., None, None]
        dlt = bd[:, t][..., None] * (vd[:, t] - torch.einsum("bhkv,bhk->bhv", S, kd[:, t]))
        S = S + kd[:, t][..., None] * dlt[..., None, :]
        o[:, t] = torch.einsum("bhkv,bhk->bhv", S, qd[:, t]) * scale
    return o, S


def lattice_expected(case: Dict, scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(o [B,T,H,V], final state [B,H,K,V]) float64 of the case by the token-by-token rule.  exp(-200) is 1.4e-87 in float64,
    not 0 as in fp32: the wipe tokens carry -inf here, so that what fp32 forgets exactly is forgotten exactly.  Asserts the case's
    magnitude bound on both results."""
    g = torch.where(case["g"] == WIPE, torch.full((), float("-inf")), case["g"].double())
    o, S = gdn_rule_f64(case["q"], case["k"], case["v"], g, case["beta"], case["h0"], scale)
    assert float(o.abs().max()) <= case["bound"] * max(scale, 1.0) and float(S.abs().max()) <= case["bound"], \
        (float(o.abs().max()), float(S.abs().max()))
    return o, S


def default_scale_expected(o_int: torch.Tensor) -> torch.Tensor:
    """scale=None: the operators multiply by float32(128 ** -0.5), which no lattice output survives exactly; the chunk kernel's
    epilogue rounds once -- bf16(float32(o_int) * float32(128 ** -0.5)) for the integer output `o_int` of scale = 1."""
    return (o_int.float() * torch.tensor(GDN_K ** -0.5, dtype=torch.float32)).to(torch.bfloat16)


# ---- what a case exercises --------------------------------------------------------------------------------------------------
FEATURES = ("rewrite_in_block16", "rewrite_across_block16", "rewrite_across_seam", "wipe_inside_chunk", "wipe_at_chunk_end",
            "read_same_chunk", "read_earlier_chunk", "o_nonzero_every_chunk", "state_differs_from_h0")


def lattice_features(case: Dict, expected: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Dict[str, bool]:
    """Which of FEATURES the case shows in at least one stream.  A write counts when beta != 0, a rewrite / read when the key's
    earlier write has not been wiped since: rewrite_in_block16 -- the earlier write lies in the same 16-token block of the same
    chunk (an off-diagonal entry of (I + L)^-1 inside a 16 x 16 diagonal block), rewrite_across_block16 -- in another block of
    the same chunk, rewrite_across_seam -- in an earlier chunk; wipe_inside_chunk -- a wipe token that is neither the first nor
    the last token of its chunk (nor of the call); read_* -- a query slot whose key was last written in the same chunk (this
    token included) / in an earlier one."""
    f = {n: False for n in FEATURES}
    B, T, H = case["g"].shape
    slot, qa, qb = (case[n].tolist() for n in ("slot", "qa", "qb"))
    g, beta = case["g"].tolist(), case["beta"].tolist()
    if case["kind"] != "still":
        for b in range(B):
            for h in range(H):
                last: Dict[int, int] = {}
                for t in range(T):
                    c, r = divmod(t, CHUNK)
                    if g[b][t][h] == WIPE:
                        last.clear()
                        end = min(CHUNK, T - c * CHUNK) - 1
                        f["wipe_inside_chunk"] |= 0 < r < end
                        f["wipe_at_chunk_end"] |= r == CHUNK - 1
                    reads = (qa[b][t][h],) if case["kind"] == "onehot_q" else (qa[b][t][h], qb[b][t][h])
                    sl = slot[b][t][h]
                    for s_ in reads:
                        if s_ in last:
                            same = last[s_] // CHUNK == c
                            f["read_same_chunk"] |= same
                            f["read_earlier_chunk"] |= not same
                        if s_ == sl and beta[b][t][h] != 0:
                            f["read_same_chunk"] = True
                    if beta[b][t][h] != 0:
                        if sl in last:
                            t1 = last[sl]
                            if t1 // CHUNK != c:
                                f["rewrite_across_seam"] = True
                            elif t1 // 16 == t // 16:
                                f["rewrite_in_block16"] = True
                            else:
                                f["rewrite_across_block16"] = True
                        last[sl] = t
    o, S = lattice_expected(case) if expected is None else expected
    f["o_nonzero_every_chunk"] = all(bool((o[:, c0:c0 + CHUNK] != 0).any()) for c0 in range(0, T, CHUNK))
    f["state_differs_from_h0"] = case["h0"] is None or not torch.equal(S, case["h0"].double())
    return f


def lattice_required(kind: str, T: int) -> Tuple[str, ...]:
    """The features a case of this kind and length must show (the CPU test asserts them for every case the GPU file uses).
    What needs a second token, a second 16-token block, a whole chunk or a second chunk is asked for from the length on at which
    lattice_case places it by construction (second block: from T = 33 on, where the repeat lags make it certain enough that a
    failing seed is changed, not tolerated).  "still" writes nothing: its state must NOT differ and its output must read."""
    if kind == "still":
        return ("o_nonzero_every_chunk",)
    req = ["read_same_chunk", "o_nonzero_every_chunk", "state_differs_from_h0"]
    if T >= 2:
        req.append("rewrite_in_block16")
    if T >= 3:
        req.append("wipe_inside_chunk")
    if T >= 33:
        req.append("rewrite_across_block16")
    if T >= CHUNK:
        req.append("wipe_at_chunk_end")
    if T > CHUNK:
        req += ["rewrite_across_seam", "read_earlier_chunk"]
    return tuple(req)


# ---- reporting ---------------------------------------------------------------------------------------------------------------
def lattice_mismatches(expected_o, expected_s, got_o, got_s, limit: int = 5) -> List[str]:
    """The first `limit` elements of o [B,T,H,V] and of the state [B,H,K,V] that differ from the expectation ([] = equal
    everywhere; a non-finite element differs), each named by its place: (batch, token, chunk, row in chunk, head, column) for o
    and (batch, head, k row, v column) for the state, with the expected and the returned value.  Either pair may be None."""
    bad: List[str] = []
    if got_o is not None:
        assert tuple(got_o.shape) == tuple(expected_o.shape), (tuple(got_o.shape), tuple(expected_o.shape))
        e, o_ = expected_o.double(), got_o.double()
        neq = ~(e == o_)
        n = int(neq.sum())
        for b, t, h, c in neq.nonzero()[:limit].tolist():
            bad.append(f"o[batch {b}, token {t} (chunk {t // CHUNK}, row {t % CHUNK}), head {h}, column {c}]: "
                       f"expected {float(e[b, t, h, c])!r} got {float(o_[b, t, h, c])!r}")
        if n:
            tok = neq.any(-1).any(-1).any(0).nonzero().flatten()
            bad.append(f"o: {n} of {neq.numel()} elements differ, tokens {int(tok[0])}..{int(tok[-1])}")
    if got_s is not None:
        assert tuple(got_s.shape) == tuple(expected_s.shape), (tuple(got_s.shape), tuple(expected_s.shape))
        e, s_ = expected_s.double(), got_s.double()
        neq = ~(e == s_)
        n = int(neq.sum())
        for b, h, r, c in neq.nonzero()[:limit].tolist():
            bad.append(f"state[batch {b}, head {h}, k row {r}, v column {c}]: expected {float(e[b, h, r, c])!r} "
                       f"got {float(s_[b, h, r, c])!r}")
        if n:
            bad.append(f"state: {n} of {neq.numel()} elements differ")
    return bad


# ---- the cases the GPU file runs (shared with the CPU file, which checks the preconditions of every one) ---------------------
SCALES = (1.0, 0.5, 0.125)
CHUNK_T = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 200)          # B = 2, H = 3: B*H <= 32, 32-column scan workgroups
CHUNK_T_FP8 = CHUNK_T                                            # the e4m3 serial pass: the same lengths
WIDE = (3, 70, 16)                                               # B, T, H: B*H = 48 > 32, 64-column scan workgroups
LONG_T = 64 * CHUNK + 65                                         # 4161: crosses the 64-chunk workspace segment at token 4096
RECURRENT_T = (1, 7, 33, 64, 70)
SPLIT = (130, 37)                                                # T, first call's length: 37 | 93
VARLEN_LENGTHS = (70, 1, 0, 64, 65)


def case_seed(kind: str, B: int, T: int, H: int) -> int:
    return 7000 + 131 * T + 17 * B + H + 1000 * KINDS.index(kind)


def make(kind: str, B: int, T: int, H: int, **kw) -> Dict:
    return lattice_case(kind, B, T, H, seed=case_seed(kind, B, T, H), **kw)


def gpu_case_list() -> List[Tuple[str, int, int, int]]:
    """(kind, B, T, H) of every case tests/test_gpu_lattice.py builds"""
    out = []
    for T in CHUNK_T:
        out += [("memory", 2, T, 3), ("still", 2, T, 3), ("half", 2, T, 3), ("onehot_q", 2, T, 3)]
    for T in RECURRENT_T:
        out += [("memory", 2, T, 3), ("onehot_q", 2, T, 3), ("still", 2, T, 3), ("half", 2, T, 3)]
    B, T, H = WIDE
    out += [("memory", B, T, H), ("still", B, T, H), ("half", B, T, H)]
    out += [("memory", 1, LONG_T, 1), ("memory", 2, SPLIT[0], 2), ("memory", 1, sum(VARLEN_LENGTHS), 2)]
    return sorted(set(out))


def varlen_sequences(flat: Dict, lengths: Sequence[int]) -> List[Optional[Dict]]:
    """The flattened case [1, sum(lengths), H, .] cut into one case per sequence (None for an empty one), each with its own
    initial state flat["h0_seq"][i]."""
    out, a = [], 0
    for i, n in enumerate(lengths):
        if n == 0:
            out.append(None)
            continue
        c = {x: flat[x][:, a:a + n] for x in ("q", "k", "v", "g", "beta", "slot", "qa", "qb")}
        c.update(kind=flat["kind"], bound=flat["bound"], h0=flat["h0_seq"][i:i + 1])
        out.append(c)
        a += n
    return out


def varlen_case(H: int = 2) -> Dict:
    """one flattened "memory" case over VARLEN_LENGTHS with an initial state per sequence (h0_seq [5, H, K, V])"""
    T = sum(VARLEN_LENGTHS)
    flat = make("memory", 1, T, H)
    gen = torch.Generator().manual_seed(case_seed("memory", len(VARLEN_LENGTHS), T, H))
    flat["h0_seq"] = torch.randint(-4, 5, (len(VARLEN_LENGTHS), H, GDN_K, GDN_V), generator=gen).float()
    flat["h0"] = None
    return flat

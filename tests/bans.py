"""The host reference of ivl_token_ban_fwd (BAN-0 .. BAN-5 in include/ivl_hip.h) and the builders of its test cases: plain
Python over lists, written from the header's text and from nothing of the kernel.

A case is a dict: V; hist (int64 [hist_ld]) with n_new; ctx (int64 [ctx_ld] or None) with n_ctx; g (the n-gram size); min_new
with stop (int64 [n_stop]); table (None, or a list of token-id lists: the row's bad-words table); done."""
import numpy as np

NINF_BITS = np.int16(-128)                # 0xFF80: bf16 -inf
SEQ_LD = 16


def ring_window(ring, n, ld=None):
    """the min(n, ld) newest entries of a ring that `n` entries were pushed into, oldest first: entry number i sits at i % ld"""
    ld = len(ring) if ld is None else ld
    n = max(int(n), 0)
    h = min(n, ld)
    return [int(ring[(n - h + k) % ld]) for k in range(h)]


def push(ring, n, ids):
    """`ids` appended to a ring (in place) that holds n entries so far; the new n"""
    for t in ids:
        ring[n % len(ring)] = t
        n += 1
    return n


def sequence(c):
    """the row's sequence: context, then generated tokens"""
    ctx = [] if c.get("ctx") is None else ring_window(c["ctx"], c["n_ctx"])
    return ctx + ring_window(c["hist"], c["n_new"])


def _eq(a, b, V):
    """an id outside [0, V) equals nothing, not even itself"""
    return 0 <= a < V and a == b


def banned(c):
    """bool [V]: the tokens of the case's row that BAN-1 .. BAN-3 ban (nothing for a finished row)"""
    V = c["V"]
    out = np.zeros(V, dtype=bool)
    if c.get("done", 0) != 0:
        return out
    seq = sequence(c)
    L, g = len(seq), int(c.get("g", 0))
    if g >= 1 and L >= g:                                              # BAN-1
        tail = seq[L - (g - 1):] if g > 1 else []
        for i in range(0, L - g + 1):
            if all(_eq(seq[i + k], tail[k], V) for k in range(g - 1)) and 0 <= seq[i + g - 1] < V:
                out[seq[i + g - 1]] = True
    for words in (c.get("table") or []):                               # BAN-2
        words = list(words)
        m = len(words)
        if m < 1 or words[-1] < 0:
            continue
        if m - 1 <= L and all(_eq(words[m - 1 - k], seq[L - k], V) for k in range(1, m)) and words[-1] < V:
            out[words[-1]] = True
    if c.get("min_new") is not None and c["n_new"] < c["min_new"]:     # BAN-3
        for t in c["stop"]:
            if 0 <= t < V:
                out[int(t)] = True
    return out


def touches(c):
    """BAN-0: False for a row of which no byte may be written and nothing beyond done / the switches read"""
    if c.get("done", 0) != 0:
        return False
    return c.get("g", 0) >= 1 or c.get("table") is not None or (c.get("min_new") is not None and c["n_new"] < c["min_new"])


def apply(bits, cases):
    """the expected buffer: bits int16 [rows, ld] (the bf16 logits as they are, guard rows and padding columns included) with
    BAN-4's edit of row s for cases[s]; a copy"""
    out = bits.copy()
    for s, c in enumerate(cases):
        out[s, :c["V"]][banned(c)] = NINF_BITS
    return out


def table_rows(words, n_seq, seq_ld=SEQ_LD):
    """a list of token-id lists as int64 [n_seq, seq_ld], right-aligned, -1 elsewhere (what BanTables.load writes)"""
    rows = np.full((n_seq, seq_ld), -1, dtype=np.int64)
    for r, w in enumerate(words):
        rows[r, seq_ld - len(w):] = w
    return rows


def case(V, hist_ld, tokens=(), *, ctx_ld=None, context=(), g=0, min_new=None, stop=(-1,), table=None, done=0, junk=-7):
    """a case whose history ring was pushed `tokens` and whose context ring `context` (rings start as `junk`)"""
    hist = np.full(hist_ld, junk, dtype=np.int64)
    n_new = push(hist, 0, tokens)
    c = dict(V=V, hist=hist, n_new=n_new, ctx=None, n_ctx=0, g=g, min_new=min_new, stop=np.asarray(stop, dtype=np.int64),
             table=table, done=done)
    if ctx_ld is not None:
        c["ctx"] = np.full(ctx_ld, junk, dtype=np.int64)
        c["n_ctx"] = push(c["ctx"], 0, context)
    return c


def random_logit_bits(rows, ld, seed):
    """int16 [rows, ld]: random bf16 bit patterns -- NaNs with payloads, -0, +-inf and subnormals among them"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(-2 ** 15, 2 ** 15, size=(rows, ld)).astype(np.int16)
    special = np.array([0x8000, 0x7F80, 0xFF80, 0x7FC1, 0xFFFF, 0x0001, 0x0000], dtype=np.uint16).view(np.int16)
    where = rng.random((rows, ld)) < 0.1
    bits[where] = special[rng.integers(0, len(special), size=int(where.sum()))]
    return bits


def ngram_sweep(V=97, hist_ld=8, ctx_ld=4, alphabet=5, seed=0):
    """the n-gram sweep: n_new x n_ctx x g, tokens from `alphabet` values (matches are frequent), both rings wrapped among them"""
    rng = np.random.default_rng(seed)
    cs = []
    for n_new in (0, 1, 2, 7, 8, 9, 13, 16, 19):
        for n_ctx in (0, 1, 4, 6):
            for g in (1, 2, 3, 4, 13):
                cs.append(case(V, hist_ld, rng.integers(0, alphabet, size=n_new).tolist(), ctx_ld=ctx_ld,
                               context=rng.integers(0, alphabet, size=n_ctx).tolist(), g=g))
    return cs


def random_tiny_case(rng):
    """one case of the comparison with HF: no ring overflowed, every id inside [0, V)"""
    V = int(rng.integers(2, 9))
    ctx_ld, hist_ld = int(rng.integers(1, 6)), int(rng.integers(1, 7))
    n_ctx, n_new = int(rng.integers(0, ctx_ld + 1)), int(rng.integers(0, hist_ld + 1))
    small = int(rng.integers(2, V + 1))                                # a small alphabet: matches are frequent
    tok = lambda n: rng.integers(0, small, size=n).tolist()
    table = [tok(int(rng.integers(1, 5))) for _ in range(int(rng.integers(0, 4)))] or None
    min_new = int(rng.integers(0, 5)) if rng.random() < 0.5 else None
    return case(V, hist_ld, tok(n_new), ctx_ld=ctx_ld, context=tok(n_ctx), g=int(rng.integers(0, 5)), min_new=min_new,
                stop=rng.integers(0, V, size=int(rng.integers(1, 3))).tolist(), table=table)

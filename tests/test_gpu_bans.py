"""GPU (-m gpu): the token bans in front of the sampling launch (ops.ban_tokens -> ivl_token_ban_fwd, BAN-0 .. BAN-5) and their
use in the graphed multi-stream step, judged by tests/bans.py.

Every operator test packs its cases as the rows of ONE call over random bf16 bit patterns (NaN payloads, -0, +-inf) and
compares the whole buffer -- the elements in front of the first row, the columns V..ld and one guard row behind the last
included -- as int16 with the host's edit.  V = 97 at ld = 104 with row starts off 16 bytes; one mixed call at V = 4099."""
import numpy as np
import pytest
import torch

import adjust
import bans
import test_gpu_adjust as tga

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64 = torch.int32, torch.int64
SHIFT = 3                                   # elements in front of row 0: every row of ld = 104 starts 6 bytes into a 16-byte tile
POISON = 1 << 40                            # an id far out of range


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


class _Call:
    """the device tensors of one call over `cases` (rows of the call, in order).  tables: None, or (words, index per case): a
    holder of seq / n_tables / n_seq / seq_ld and what ban_idx holds.  A finished row gets poison in everything it may not
    read; the rings of a row that is off hold whatever its case says (the builders put ids far out of range there)."""

    def __init__(self, cases, ld, seed, tables=None, done=True, n_stop=4, bits=None):
        self.cases, S, V = cases, len(cases), cases[0]["V"]
        self.S, self.V, self.ld = S, V, ld
        self.bits = bans.random_logit_bits(S + 1, ld, seed) if bits is None else bits
        self.front = np.random.default_rng(seed + 1).integers(-2 ** 15, 2 ** 15, size=SHIFT).astype(np.int16)
        flat = np.concatenate([self.front, self.bits.reshape(-1)])
        self.buf = torch.from_numpy(flat).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.lg = self.buf[SHIFT:].view(S + 1, ld)[:S, :V].view(torch.bfloat16)
        assert self.lg.data_ptr() % 16 == 2 * SHIFT
        fin = [c.get("done", 0) != 0 for c in cases]
        col = lambda key, dt, poison, off=0: torch.tensor(
            [poison if f else (off if c.get(key) is None else c[key]) for c, f in zip(cases, fin)], dtype=dt, device=DEV)
        rows = lambda key: torch.from_numpy(np.stack([np.full_like(c[key], POISON) if f else c[key] for c, f in zip(cases, fin)])).to(DEV)
        self.kw = dict(n_new=col("n_new", I64, 1 << 62), history=rows("hist"), ngram=col("g", I32, 7))
        if done:
            self.kw["done"] = torch.tensor([c.get("done", 0) for c in cases], dtype=I32, device=DEV)
        if cases[0].get("ctx") is not None:
            self.kw.update(ctx=rows("ctx"), n_ctx=col("n_ctx", I64, 1 << 61))
        if any(c.get("min_new") is not None for c in cases):
            stop = np.full((S, n_stop), -1, dtype=np.int64)
            for s, c in enumerate(cases):
                stop[s, :len(c["stop"])] = c["stop"]
                if fin[s]:
                    stop[s] = 5
            self.kw.update(min_new=col("min_new", I64, 1 << 62), stop_ids=torch.from_numpy(stop).to(DEV))
        if tables is not None:
            self.kw.update(words=tables[0], ban_idx=torch.tensor(tables[1], dtype=I32, device=DEV))
        self.ro = {k: t.clone() for k, t in self.kw.items() if isinstance(t, torch.Tensor)}

    def run(self):
        from infinitevl_amd import ops
        assert ops.ban_tokens(self.lg, **self.kw) is self.lg
        return self

    def got(self):
        torch.cuda.synchronize()
        for k, was in self.ro.items():
            assert torch.equal(self.kw[k], was), f"{k} is only read"
        flat = self.buf.cpu().numpy()
        assert (flat[:SHIFT] == self.front).all(), "the elements in front of row 0"
        return flat[SHIFT:].reshape(self.S + 1, self.ld)

    def check(self, where=""):
        got, want = self.got(), bans.apply(self.bits, self.cases)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (where, bad[:6].tolist(), [self.cases[r] if r < self.S else "guard row" for r in sorted(set(bad[:6, 0].tolist()))])
        assert (got[self.S] == self.bits[self.S]).all() and (got[:, self.V:] == self.bits[:, self.V:]).all()
        return got


def _table(words_per_table, n_seq=8, seq_ld=bans.SEQ_LD):
    import types
    seq = np.stack([bans.table_rows(w, n_seq, seq_ld) for w in words_per_table])
    return types.SimpleNamespace(seq=torch.from_numpy(seq).to(DEV), n_tables=len(words_per_table), n_seq=n_seq, seq_ld=seq_ld)


def _with_tables(cases, extra=0):
    """one table per case that has one (the others point outside [0, n_tables), below or above), behind `extra` unused tables"""
    words, idx = [[[1]]] * max(extra, 1), {}
    for s, c in enumerate(cases):
        if c.get("table") is not None and not c.get("done"):
            idx[s] = len(words)
            words.append(c["table"])
    return _table(words), [idx.get(s, -1 if s % 2 else len(words) + s % 3) for s in range(len(cases))]


# ---------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------
def test_ngram_sweep():
    from infinitevl_amd import ops
    cs = bans.ngram_sweep(97, hist_ld=8, ctx_ld=4)
    assert len(cs) == 9 * 4 * 5
    n0 = ops.BAN_CALLS["ban"]
    _Call(cs, 104, 1).run().check("sweep")
    assert ops.BAN_CALLS["ban"] == n0 + 1
    n_banned = [int(bans.banned(c).sum()) for c in cs]
    assert sum(n > 0 for n in n_banned) > 50 and sum(n == 0 for n in n_banned) > 20
    # among them: both rings wrapped, and a match whose n-gram lies across the context boundary / across the ring's wrap
    across = wrapped = 0
    for c in cs:
        if c["g"] in (2, 3, 4) and c["n_ctx"] > 0 and c["n_new"] > 0 and bans.banned(c).any():
            alone = {**c, "ctx": None, "n_ctx": 0}
            across += bool((bans.banned(c) & ~bans.banned(alone)).any())
        wrapped += c["n_new"] > 8 and c["n_ctx"] > 4 and bans.banned(c).any() and c["g"] > 1
    assert across >= 5 and wrapped >= 3, (across, wrapped)


def _mixed(V):
    """one call of everything: n-grams over both rings, tables, the minimum length, rows that are off and finished rows"""
    rng = np.random.default_rng(V)
    tok = lambda n, hi=6: rng.integers(0, hi, size=n).tolist()
    far = lambda n: [POISON + 3] * n
    cs = [
        bans.case(V, 8, tok(13), ctx_ld=4, context=tok(6), g=2, table=[[1], [2, 3], [V - 1]], min_new=20, stop=[0, V - 1, -1, V]),
        bans.case(V, 8, far(11), ctx_ld=4, context=far(9), g=0, junk=POISON),                                         # off
        bans.case(V, 8, tok(5), ctx_ld=4, context=tok(2), g=3, table=[tok(3, 3), tok(2, 3), tok(4, 3), tok(5, 3)]),
        bans.case(V, 8, tok(8), ctx_ld=4, context=tok(4), g=2, table=[[0], [1]], min_new=99, stop=[3], done=1),       # finished
        bans.case(V, 8, tok(3), ctx_ld=4, context=tok(1), g=0, min_new=3, stop=[V - 1, 0]),                             # at the minimum: off
        bans.case(V, 8, tok(19, V), ctx_ld=4, context=tok(4, V), g=1),
        bans.case(V, 8, far(4), ctx_ld=4, context=far(4), g=0, min_new=0, stop=[1], done=4, junk=POISON),              # held
        bans.case(V, 8, tok(2), ctx_ld=4, context=[], g=0, min_new=3, stop=[V - 1, 5, -1, 1 << 33]),
    ]
    tail = bans.sequence(cs[2])[-2:]
    cs[2]["table"].append(tail + [V - 2])                              # one sequence of row 2 is sure to match
    return cs


@pytest.mark.parametrize("V,ld", [(97, 104), (4099, 4107)])
def test_mixed_call_off_and_finished_rows_idempotence(V, ld):
    cs = _mixed(V)
    tabs = _with_tables(cs, extra=1)
    call = _Call(cs, ld, 2, tables=tabs).run()
    got = call.check(f"mixed V{V}")
    for s in (1, 3, 4, 6):                                             # off and finished rows: byte-identical
        assert not bans.touches(cs[s]) and (got[s] == call.bits[s]).all(), s
    assert all(bans.banned(cs[s]).any() for s in (0, 2, 5, 7))
    assert (got[7, [5, V - 1]] == -128).all() and (got[0, [0, V - 1]] == -128).all()
    again = call.run().got()                                           # BAN-4: two calls equal one
    assert (again == got).all()
    # without `done` the finished rows are live ones (the call's tensors hold poison for them: rebuild them as live)
    live = [{**c, "done": 0} for c in cs]
    _Call(live, ld, 2, tables=_with_tables(live, extra=1), done=False).run().check(f"mixed V{V}, done NULL")


def test_neighbours_in_one_word_and_a_row_banned_entirely():
    V, H = 97, 128
    every = list(range(V))
    cs = [bans.case(V, H, [10, 11], g=1), bans.case(V, H, [11, 12], g=1), bans.case(V, H, [0, V - 1], g=1),
          bans.case(V, H, [0, 1, V - 2, V - 1], g=1), bans.case(V, H, every, g=1), bans.case(V, H, every + every[:40], g=1),
          bans.case(V, H, [V, 1 << 31, (1 << 32) + 5, -1, 96], g=1)]
    call = _Call(cs, 104, 3).run()
    got = call.check("neighbours")
    assert (got[4, :V] == -128).all() and (got[5, :V] == -128).all() and (got[4, V:] == call.bits[4, V:]).all()
    assert (got[0, 10:12] == -128).all() and (got[1, 11:13] == -128).all() and got[0, 12] == call.bits[0, 12]
    assert (got[6, :96] == call.bits[6, :96]).all() and got[6, 96] == -128


def test_sequences():
    from infinitevl_amd import ops
    V = 97
    seq16 = list(range(20, 36))
    ctx, hist = [20, 21, 22, 23, 24, 25, 26, 27], [28, 29, 30, 31, 32, 33, 34]
    words = [[40], [34, 41], [33, 34, 42], [32, 33, 34, 43], [31, 32, 33, 34, 44], seq16,         # lengths 1 .. 5 and seq_ld: all match
             [34, 45], [34, 41],                                                                    # two with one prefix, one twice
             [33, 33, 46], [35, 34, 47], [34, V], [34, 1 << 40], [V + 3], [96]]                      # no match; a last token >= V
    assert bans.banned(bans.case(V, 8, hist, ctx_ld=8, context=ctx, table=words)).nonzero()[0].tolist() == [35, 40, 41, 42, 43, 44, 45, 96]
    short = [[5, 6, 7, 50], [6, 7, 51], [4, 5, 6, 7, 52]]                                             # L = 3: m - 1 = 3 fits, 4 does not
    cs = [bans.case(V, 8, hist, ctx_ld=8, context=ctx, table=words),
          bans.case(V, 8, [5, 6, 7], ctx_ld=8, context=[], table=short),
          bans.case(V, 8, [34, V + 1, 34], ctx_ld=8, context=[V + 1], table=[[V + 1, 34, 60], [34, 61], [V + 1, 62]]),    # an id >= V in a ring
          bans.case(V, 8, hist[:3] + hist, ctx_ld=8, context=ctx * 2, table=words),                 # both rings wrapped
          bans.case(V, 8, hist, ctx_ld=8, context=ctx, table=None),
          bans.case(V, 8, hist, ctx_ld=8, context=ctx, table=None)]
    assert bans.banned(cs[1]).nonzero()[0].tolist() == [50, 51] and bans.banned(cs[2]).nonzero()[0].tolist() == [61]
    tabs = ops.BanTables(DEV, 3, n_seq=16, max_len=16)
    h0, h1, h2 = tabs.load(words), tabs.load(short), tabs.load(cs[2]["table"])
    ptr = tabs.seq.data_ptr()
    idx = [h0.index, h1.index, h2.index, h0.index, -1, tabs.n_tables]         # two rows on one table; below and above the range
    _Call(cs, 104, 4, tables=(tabs, idx)).run().check("sequences")
    # unload, load and reload between calls at fixed pointers: the same rows obey what the tables hold now
    tabs.unload(h0)
    off = [{**c, "table": None} if i in (0, 3) else c for i, c in enumerate(cs)]
    _Call(off, 104, 5, tables=(tabs, idx)).run().check("unloaded")
    h3 = tabs.load([[34, 70], [71]])
    assert h3.index == h0.index and h3 != h0 and tabs.seq.data_ptr() == ptr
    new = [{**c, "table": [[34, 70], [71]]} if i in (0, 3) else c for i, c in enumerate(cs)]
    got = _Call(new, 104, 6, tables=(tabs, idx)).run().check("reloaded")
    assert (got[0, [70, 71]] == -128).all() and (got[3, [70, 71]] == -128).all()


def test_min_new():
    V = 97
    stop = [7, -1, V, 96]
    cs = [bans.case(V, 4, [1] * n, min_new=m, stop=stop) for n, m in ((0, 1), (2, 3), (3, 3), (4, 3), (0, 0), (9, 10), (10, 10))]
    cs.append(bans.case(V, 4, [1, 2], min_new=5, stop=[-1, -1, 1 << 35, -(1 << 35)]))
    call = _Call(cs, 104, 7).run()
    got = call.check("min_new")
    assert [bans.touches(c) for c in cs] == [True, True, False, False, False, True, False, True]
    assert (got[0, [7, 96]] == -128).all() and int((got[0, :V] != call.bits[0, :V]).sum()) <= 2
    assert (got[7] == call.bits[7]).all()
    # min_new alone, without a history: nothing but n_new is needed
    from infinitevl_amd import ops
    c2 = _Call(cs, 104, 8)
    ops.ban_tokens(c2.lg, n_new=c2.kw["n_new"], min_new=c2.kw["min_new"], stop_ids=c2.kw["stop_ids"])
    assert (c2.got() == bans.apply(c2.bits, cs)).all()


def test_a_row_alone_equals_the_same_row_among_others():
    V = 97
    cs = _mixed(V)
    me = cs[0]
    bits_row = bans.random_logit_bits(1, 104, 9)
    outs = []
    for S, at in ((1, 0), (4, 2), (63, 62)):
        others = [cs[(i % 7) + 1] for i in range(S)]
        rows = others[:at] + [me] + others[at + 1:]
        bits = bans.random_logit_bits(S + 1, 104, 10 + S)
        bits[at] = bits_row[0]
        got = _Call(rows, 104, 20, tables=_with_tables(rows, extra=S % 2), bits=bits).run().check(f"row {at} of {S}")
        outs.append(got[at].copy())
    assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all() and (outs[0] != bits_row[0]).any()


# ---------------------------------------------------------------------------------------------
# composition with the sampling launch (BAN-5)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ctl", "lp", "adj"])
@pytest.mark.parametrize("V", [97, 4099])
def test_ban_then_sample_equals_sample_on_the_host_edited_row(V, form):
    from infinitevl_amd import ops
    cs = adjust.operator_cases(V)[:6]
    S = len(cs)
    rng = np.random.default_rng(V)
    hist = [rng.integers(0, 4, size=tga.HIST).tolist() for _ in range(S - 1)] + [list(range(3))]
    n_new0 = 4                                                         # the ring of HIST = 3 holds entries 1, 2, 3: it has wrapped
    top = [int(np.argmax(np.nan_to_num(c["x"].float().numpy(), nan=-np.inf))) for c in cs]
    tables = [[[top[s]], [hist[s][0], (top[s] + 1) % V]] if s % 2 == 0 else None for s in range(S)]
    bcs = []
    for s in range(S):
        ring = np.asarray(hist[s], dtype=np.int64)
        bcs.append(dict(V=V, hist=ring, n_new=n_new0, ctx=None, n_ctx=0, g=(1, 2, 0)[s % 3], min_new=(6 if s < 3 else 2),
                        stop=np.asarray([V - 1, 3 % V, -1], dtype=np.int64), table=tables[s], done=0))
    bcs[-1]["g"] = 1 if V == 97 else 2
    edited = []
    for c, b in zip(cs, bcs):
        x = adjust.bits(c["x"]).view(np.int16).copy()
        x[bans.banned(b)] = bans.NINF_BITS
        edited.append(torch.from_numpy(x).view(torch.bfloat16))
    assert sum(bool(bans.banned(b)[top[s]]) for s, b in enumerate(bcs)) >= 3, "the most likely token of some rows is banned"
    kind, adj = ("ctl" if form == "adj" else form), (tga._adj_of(cs) if form == "adj" else None)
    common = dict(shift=3, seen=[c["seen"] for c in cs], n_new0=n_new0)
    a = tga._Call([c["x"] for c in cs], cs, kind, adj, **common)
    b = tga._Call(edited, cs, kind, adj, **common)
    ring = torch.tensor(hist, dtype=I64, device=DEV)
    for call in (a, b):
        call.T["history"].t.copy_(ring)
    words, idx = _with_tables(bcs)
    ops.ban_tokens(a.lg, n_new=a.T["n_new"].t, history=a.T["history"].t, done=a.T["done"].t, min_new=torch.tensor(
        [c["min_new"] for c in bcs], dtype=I64, device=DEV), stop_ids=a.T["stop_ids"].t, ngram=torch.tensor(
        [c["g"] for c in bcs], dtype=I32, device=DEV), ban_idx=torch.tensor(idx, dtype=I32, device=DEV), words=words)
    assert torch.equal(a.lg.view(torch.int16), b.lg.view(torch.int16)), "the edit is the host's"
    assert torch.equal(a.keep.view(torch.int16), b.keep.view(torch.int16)), "and nothing around the rows moved"
    got, ref = a.run().host(), b.run().host()
    tga._same(got, ref, range(S), f"V{V} {form}")
    if adj is not None:
        assert got["count"].tobytes() == ref["count"].tobytes()
    for s, bc in enumerate(bcs):
        assert not bans.banned(bc)[int(got["token"][s, 0])] or bans.banned(bc).all(), (s, got["token"][s, 0])


# ---------------------------------------------------------------------------------------------
# the graphed multi-stream step
# ---------------------------------------------------------------------------------------------
PROMPTS = ((50, 5), (40, 6), (33, 7), (40, 8))
N_STEPS = 12


def _decoder(bans_on, **kw):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = tga._small()
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
    extra = dict(bans=True, ban_context=16, ban_tables=2, ban_seqs=8, ban_len=4) if bans_on else {}
    smp = Sampler(4, DEV, vocab_size=hc.vocab_size, history=32, **{**extra, **kw})
    return GraphedMultiStreamDecode(stack, cache, sampler=smp), hc


def _prompt_ids(hc, n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, hc.vocab_size, size=n)).to(DEV)


def _run(dec, hc, sampling, graph, words=None):
    h = dec.sampler.load_bad_words(words) if words else None
    for slot, (T, seed) in enumerate(PROMPTS):
        dec.admit(slot, tga._prompt(hc, T, seed), sampling=sampling[slot], prompt_ids=_prompt_ids(hc, 6, seed) if slot == 0 else None,
                  bad_words=h if slot == 1 else None)
    toks = [dec.token[:, 0].tolist()]
    for _ in range(N_STEPS):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
    return [[t[s] for t in toks] for s in range(4)]


def test_the_step_obeys_the_bans_replayed_as_eager():
    from infinitevl_amd import ops
    n0 = ops.BAN_CALLS["ban"]
    free = {0: dict(), 1: dict(), 2: dict(), 3: dict(temperature=1.0, seed=11, top_k=50)}
    plain, hc = _decoder(False)
    base = _run(plain, hc, free, True)
    assert ops.BAN_CALLS["ban"] == n0, "a sampler built without bans launches what it always did"
    words = [[base[1][i], base[1][i + 1]] for i in (0, 2, 5)]
    ctl = {0: dict(no_repeat_ngram_size=2), 1: dict(), 2: dict(min_new_tokens=3, stop_token_ids=[base[2][0]]), 3: free[3]}
    dec_g, _ = _decoder(True)
    got = _run(dec_g, hc, ctl, True, words)
    assert ops.BAN_CALLS["ban"] > n0
    dec_e, _ = _decoder(True)
    eager = _run(dec_e, hc, ctl, False, words)
    assert got == eager, "replayed steps equal the eager steps"
    sg, se = dec_g.sampler.state(), dec_e.sampler.state()
    for k, v in sg.items():
        assert v.cpu().numpy().tobytes() == se[k].cpu().numpy().tobytes(), k
    # slot 0: no bigram twice, the prompt's tokens included
    seq = _prompt_ids(hc, 6, PROMPTS[0][1]).tolist() + got[0]
    grams = list(zip(seq, seq[1:]))
    assert len(set(grams)) == len(grams), grams
    assert dec_g.sampler.n_ctx.tolist() == [6, 0, 0, 0] and dec_g.sampler.ctx[0, :6].tolist() == seq[:6]
    # slot 1: never a banned sequence, and it left the unconstrained path
    assert not set(zip(got[1], got[1][1:])) & {tuple(w) for w in words} and got[1] != base[1] and got[1][0] == base[1][0]
    # slot 2: its stop id is banned for three tokens: it differs from the unconstrained run and does not end before three
    stop = base[2][0]
    assert stop not in got[2][:3] and got[2] != base[2]
    done, n_new = dec_g.sampler.poll()
    if stop in got[2]:
        assert int(done[2]) == 1 and int(n_new[2]) == got[2].index(stop) + 1 >= 4
    else:
        assert int(done[2]) == 0 and int(n_new[2]) == N_STEPS + 1
    # slot 3 is off: token for token the run of the sampler without bans
    assert got[3] == base[3] and len(set(got[3])) > 3


def test_bans_change_between_replays_without_a_recapture_and_fork_copies_them():
    def start():
        dec, hc = _decoder(True)
        for slot, seed in ((0, 10), (1, 10), (2, 12), (3, 12)):
            dec.admit(slot, tga._prompt(hc, 40, seed), sampling=dict(), prompt_ids=_prompt_ids(hc, 20, seed))
        for _ in range(3):
            dec.step()
        return dec, hc

    dec, hc = start()
    base, base2 = [], []
    for _ in range(4):
        dec.step()
        base.append(dec.token[0, 0].item())
        base2.append(dec.token[2, 0].item())
    assert dec.token[1, 0].item() == base[-1] and dec.token[3, 0].item() == base2[-1], "two pairs of identical slots"
    dec, hc = start()
    graph, smp = dec.graph, dec.sampler
    assert graph is not None and smp.n_ctx.tolist() == [20] * 4 and smp.ctx.shape[1] == 16
    # a table loaded and set between two replays bans slot 0's next token; slot 1 follows the old future
    h = smp.load_bad_words([[base[0]]])
    smp.set_bad_words(0, h)
    dec.step()
    assert dec.graph is graph and dec.token[0, 0].item() != base[0] and dec.token[1, 0].item() == base[0]
    # min_new_tokens and a stop id written between replays: slot 2's next token is banned, slot 3 emits it
    smp.stop_ids[2, 0] = base2[1]
    smp.min_new[2] = 1000
    dec.step()
    assert dec.graph is graph and dec.token[2, 0].item() != base2[1] and dec.token[3, 0].item() == base2[1]
    assert int(smp.done[2]) == 0
    # no_repeat_ngram_size = 1 from now on: slot 1 emits nothing it has emitted or was given as its prompt's tail
    smp.ngram[1] = 1
    before = set(smp.tokens(1).tolist()) | set(bans.ring_window(smp.ctx[1].tolist(), 20))
    fresh = []
    for _ in range(6):
        dec.step()
        fresh.append(dec.token[1, 0].item())
    assert dec.graph is graph and len(set(fresh)) == len(fresh) and not set(fresh) & before, (fresh, before)
    # fork copies the parameters, the table index and the context ring
    dec.fork(0, [3])
    for k in ("ngram", "min_new", "ban_idx", "n_ctx", "ctx"):
        t = getattr(smp, k)
        assert torch.equal(t[3], t[0]), k
    assert smp.ban_idx.tolist() == [h.index, -1, -1, h.index]
    dec.fork(1, [2])
    assert smp.ngram.tolist() == [0, 1, 1, 0] and smp.min_new.tolist() == [0, 0, 0, 0]
    dec.step()
    assert dec.graph is graph and dec.token[2, 0].item() == dec.token[1, 0].item()


def test_second_turn_on_a_finished_slot_still_sees_the_first_answer():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = tga._small()
    cache = MultiStreamCache(config=hc, n_slots=2, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(2, DEV, vocab_size=hc.vocab_size, history=32, bans=True, ban_context=16)
    dec = GraphedMultiStreamDecode(stack, cache, sampler=smp, holds=True)
    ids = _prompt_ids(hc, 5, 77)
    dec.admit(0, tga._prompt(hc, 40, 21), prompt_ids=ids, sampling=dict(no_repeat_ngram_size=1, max_new_tokens=3))
    dec.admit(1, tga._prompt(hc, 40, 21), sampling=dict())
    first = dec.run_until_done(8, poll_every=4)[0].tolist()
    assert len(first) == 3 and int(smp.done[0]) == 2 and len(set(first) | set(ids.tolist())) == 8
    dec.extend(0, tga._prompt(hc, 10, 22), max_new_tokens=4)
    assert smp.n_ctx.tolist() == [8, 0] and smp.ctx[0, :8].tolist() == ids.tolist() + first and int(smp.n_new[0]) == 1
    for _ in range(3):
        dec.step()
    second = smp.tokens(0).tolist()
    assert len(second) == 4 and len(set(second)) == 4 and not set(second) & (set(first) | set(ids.tolist())), (first, second)


def test_admit_n_draws_every_slot_from_its_own_logits():
    dec, hc = _decoder(True)
    free, _ = _decoder(True)
    f = free.admit(0, tga._prompt(hc, 40, 31), sampling=dict()).item()
    got = dec.admit_n([0, 1, 2], tga._prompt(hc, 40, 31), sampling=[dict(), dict(min_new_tokens=2, stop_token_ids=[f]), dict()])
    assert got[0, 0].item() == f and got[2, 0].item() == f and got[1, 0].item() != f, "slot 1's ban is in slot 1's logits alone"
    assert dec.sampler.min_new.tolist() == [0, 2, 0, 0] and dec.sampler.n_new.tolist() == [1, 1, 1, 0]


def test_graphed_decode_batch_rows_get_the_bans_through_the_same_call():
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = tga._small()
    runs = {}
    for on in (False, True):
        cache = stack.allocate_inference_cache(2)
        x = torch.cat([tga._prompt(hc, 48, 41), tga._prompt(hc, 48, 41)])
        with torch.no_grad():
            pid = torch.arange(48, device=DEV)[None, None, :].expand(3, 2, 48)
            _, lg = stack(inputs_embeds=x, position_ids=pid, past_key_values=cache, logits_to_keep=1)
        smp = Sampler(2, DEV, vocab_size=hc.vocab_size, history=32, **(dict(bans=True, ban_context=8) if on else {}))
        if on:
            smp.set(0, no_repeat_ngram_size=1)
        dec = GraphedDecode(stack, cache, 2, sampler=smp)
        smp.sample(lg[:, -1], dec.token)
        toks = [dec.token[:, 0].tolist()]
        for _ in range(10):
            dec.step()
            toks.append(dec.token[:, 0].tolist())
        runs[on] = [[t[r] for t in toks] for r in range(2)]
    assert runs[False][0] == runs[False][1], "two rows of one prompt"
    assert len(set(runs[True][0])) == 11 and runs[True][1] == runs[False][1] and len(set(runs[False][0])) < 11

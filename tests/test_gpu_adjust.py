"""GPU (-m gpu): logit bias, frequency / presence penalties and min-p inside the sampling launch (ops.sample_tokens min_p= /
freq_penalty= / pres_penalty= / count= / bias_idx= / bias= -> ivl_sample_rows_adj_fwd) and their use in the graphed decode
steps, judged by tests/adjust.py.

  1 composition (ADJ-2), exact: the adjusted call == ivl_sample_rows_fwd on the host-computed x'' with r = 1, every output and
    every state tensor, for the controlled, the scoring and the constrained form; count grows by one exactly at the token.
    V in {1, 97, 4099}, calls of 1 .. 4 rows in a +inf surround at odd ld and shifted bases (tile offsets 0, 3 and 7 among them),
    a finished and an all-off row beside the adjusted ones, every padding word poisoned, guard words around every tensor;
  2 min-p through the float64 judge: TAUS x {0.05, 0.3, 1.0} x (k, p) pairs, 256 draws each, n_kept exact;
  3 identity (ADJ-0): an all-off group and all-off rows against the old entry, once at V = 151936;
  4 special values; 5 bounds; 6 the feedback chain, eager and in a replayed graph; 7 row independence;
  8 GraphedMultiStreamDecode with Sampler(penalties=True, bias_tables=2) on the tiny stack of the fork tests."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import adjust
import generation
import grammar
import parity
import sampling
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
FILL = 7
GUARD = 8
N_TOP = 5
HIST = 3
SENT = {torch.float32: 1234.5, torch.float64: 1234.5, torch.int32: 0x5A5A5A5, torch.int64: 0x5A5A5A5A5A5}
OUTPUTS = ("token", "counter", "n_kept", "prob", "seen", "n_new", "done", "history", "logprob", "top_ids", "top_logprobs",
           "cum_logprob", "lp_history", "top_hist_ids", "top_hist_lp", "fsm_state")
F32, I32, I64, F64 = torch.float32, torch.int32, torch.int64, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _odd_ld(V):
    return (V + 3) | 1


def _place(rows, ld, shift):
    """rows (bf16 [V] each) in a buffer of +inf (an element read from outside a row would take all the mass): row s at element
    shift + s * ld of a 256-byte aligned allocation"""
    S, V = len(rows), rows[0].shape[0]
    buf = torch.full((shift + S * ld + 8,), INF, dtype=torch.bfloat16, device=DEV)
    lg = buf[shift:shift + S * ld].view(S, ld)[:, :V]
    lg.copy_(torch.stack(list(rows)).to(DEV))
    assert buf.data_ptr() % 256 == 0
    return buf, lg


class _T:
    """a tensor between GUARD sentinel words on either side"""

    def __init__(self, shape, dt, data=None, fill=0):
        n = int(np.prod(shape))
        self.dt = dt
        self.buf = torch.full((n + 2 * GUARD,), SENT[dt], dtype=dt, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if data is None:
            self.t.fill_(fill)
        else:
            self.t.copy_(torch.as_tensor(np.asarray(data), dtype=dt).reshape(shape))

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENT[self.dt]).all() and (b[-GUARD:] == SENT[self.dt]).all())

    def host(self):
        return self.t.cpu().numpy().copy()


def _words(bits_list, W, beyond):
    return np.stack([generation.pack(b, W, beyond=beyond).view(np.int32) for b in bits_list])


class _Call:
    """ONE launch over rows: every tensor fresh and between guards; run() launches, host() returns host copies and checks the
    guards.  cs: [{"tau", "k", "p", "seed", "r"}]; form: "ctl", "lp" or "fsm"; adj: None (ivl_sample_rows_fwd) or
    {"min_p", "f", "pp": [S] or None, "count": [int32 [V]] or None, "bias_idx": [S] or None, "tables": [(mask, val)] or None}.
    poison: every padding word (bits and words beyond V of seen, the bias masks and values and the counts) is set / +inf /
    2^30, and the bias values outside their bitmap are NaN."""

    def __init__(self, xs, cs, form, adj=None, *, ld=None, shift=0, seen=None, done=None, fsm=None, states=None, n_new0=0,
                 counter0=0, poison=True, extra_pad=0):
        from infinitevl_amd import ops
        S, V = len(xs), xs[0].shape[0]
        W = generation.words_for(V) + 1
        self.S, self.V, self.adj = S, V, adj
        self.keep, self.lg = _place(xs, ld or _odd_ld(V), shift)
        self.off = [((self.lg[s].data_ptr() & 15) >> 1) for s in range(S)]
        seen = [np.zeros(V, dtype=bool)] * S if seen is None else seen
        T = self.T = {}
        T["temperature"], T["top_k"] = _T((S,), F32, [c["tau"] for c in cs]), _T((S,), I32, [c["k"] for c in cs])
        T["top_p"], T["seed"] = _T((S,), F32, [c["p"] for c in cs]), _T((S,), I64, [c["seed"] for c in cs])
        T["counter"] = _T((S,), I64, fill=counter0)
        T["token"], T["n_kept"], T["prob"] = _T((S, 1), I64, fill=-1), _T((S,), I32, fill=-1), _T((S,), F32, fill=-1.0)
        T["rep_penalty"] = _T((S,), F32, [c["r"] for c in cs])
        T["seen"] = _T((S, W), I32, _words(seen, W, poison))
        T["stop_ids"] = _T((S, 3), I64, [[V - 1, 3 % V, -1]] * S)
        T["budget"] = _T((S,), I64, [n_new0 + 1 if s % 2 else -1 for s in range(S)])
        T["fill"], T["n_new"] = _T((S,), I64, fill=FILL), _T((S,), I64, fill=n_new0)
        T["done"] = _T((S,), I32, [0] * S if done is None else done)
        T["history"] = _T((S, HIST), I64, fill=-5)
        if form in ("lp", "fsm"):
            T["logprob"], T["cum_logprob"] = _T((S,), F32, fill=9.0), _T((S,), F64, fill=-1.5)
            T["top_ids"], T["top_logprobs"] = _T((S, N_TOP), I64, fill=-7), _T((S, N_TOP), F32, fill=9.0)
            T["lp_history"] = _T((S, HIST), F32, fill=9.0)
            T["top_hist_ids"], T["top_hist_lp"] = _T((S, HIST, N_TOP), I64, fill=-7), _T((S, HIST, N_TOP), F32, fill=9.0)
        self.kw = {k_: T[k_].t for k_ in T if k_ not in ("temperature", "top_k", "top_p", "seed", "counter", "token", "n_kept", "prob")}
        if form == "fsm":
            T["fsm_state"] = _T((S,), I32, states)
            self.kw.update(fsm_state=T["fsm_state"].t, fsm=fsm)
        if adj is not None:
            for name, key in (("min_p", "min_p"), ("freq_penalty", "f"), ("pres_penalty", "pp")):
                if adj.get(key) is not None:
                    T[name] = _T((S,), F32, adj[key])
                    self.kw[name] = T[name].t
            if adj.get("count") is not None:
                C = V + 5 + extra_pad
                full = np.full((S, C), 2 ** 30 if poison else 0, dtype=np.int32)
                full[:, :V] = np.stack(adj["count"])
                T["count"] = _T((S, C), I32, full)
                self.kw["count"] = T["count"].t
            if adj.get("bias_idx") is not None:
                tabs = adj["tables"]
                n, L = len(tabs), V + 3
                val = np.full((n, L), INF if poison else 0.0, dtype=np.float32)
                for i, (m, v) in enumerate(tabs):
                    val[i, :V] = np.where(m, v, np.nan if poison else 0.0)
                T["bias_idx"] = _T((S,), I32, adj["bias_idx"])
                T["bias_mask"] = _T((n, W), I32, _words([m for m, _ in tabs], W, poison))
                T["bias_val"] = _T((n, L), F32, val)
                self.kw.update(bias_idx=T["bias_idx"].t, bias=types.SimpleNamespace(
                    mask=T["bias_mask"].t, val=T["bias_val"].t, n_bias=n, mask_ld=W, ld=L))
        self._ops = ops

    def run(self):
        T = self.T
        self._ops.sample_tokens(self.lg, T["temperature"].t, T["top_k"].t, T["top_p"].t, T["seed"].t, T["counter"].t,
                                out=T["token"].t, n_kept=T["n_kept"].t, prob=T["prob"].t, **self.kw)
        return self

    def host(self):
        torch.cuda.synchronize()
        for k_, t in self.T.items():
            assert t.intact(), f"guard words of {k_} changed"
        return {k_: t.host() for k_, t in self.T.items()}


def _adj_of(cs, extra_tables=()):
    """the adjustment group of the cases of tests/adjust.py: one bias table per biased case behind the extra ones (a table
    nobody points at when there is none); a case without a bias points outside [0, n_bias), below or above"""
    tabs, at = list(extra_tables), {}
    for s, c in enumerate(cs):
        if c["bias_mask"] is not None:
            at[s] = len(tabs)
            tabs.append((c["bias_mask"], c["bias_val"]))
    if not tabs:
        tabs = [(np.ones(cs[0]["x"].shape[0], dtype=bool), np.full(cs[0]["x"].shape[0], 5.0, dtype=np.float32))]
    idx = [at[s] if s in at else (-1 if s % 2 else len(tabs) + 50) for s in range(len(cs))]
    return {"min_p": [c["min_p"] for c in cs], "f": [c["f"] for c in cs], "pp": [c["pp"] for c in cs],
            "count": [c["count"] for c in cs], "bias_idx": idx, "tables": tabs}


def _same(got, ref, rows, where, names=OUTPUTS):
    for k_ in names:
        if k_ in ref:
            for s in rows:
                assert got[k_][s].tobytes() == ref[k_][s].tobytes(), (where, k_, s, got[k_][s], ref[k_][s])


def _count_moved_by_the_token(before, got, cs, dones, where):
    """ADJ-4: count grows by one exactly at the token of a live row; a finished row's and the padding stay"""
    V = cs[0]["x"].shape[0]
    for s in range(len(cs)):
        want = before[s].copy()
        if not dones[s]:
            want[int(got["token"][s, 0])] += 1
        assert (got["count"][s] == want).all(), (where, s, np.nonzero(got["count"][s] != want)[0][:4])


# ---------------------------------------------------------------------------------------------
# 1. composition
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op_cases(V):
    cs = adjust.operator_cases(V)
    off = adjust.case(f"V{V}-all-off", sampling.random_row(V, 61), generation.random_seen(V, 62), None, tau=0.7, k=0, p=1.0, seed=3)
    off["count"] = adjust.random_count(V, off["seen"], 63)
    fin = adjust.case(f"V{V}-finished", sampling.random_row(V, 64), generation.random_seen(V, 65), None, r=1.3, f=0.5, pp=0.5,
                      bias=adjust.random_bias(V, 66), tau=0.7, seed=4)
    fin["count"] = adjust.random_count(V, fin["seen"], 67)
    fin["done"] = 1
    cs = cs[:1] + [off] + cs[1:3] + [fin] + cs[3:]
    return cs, [adjust.adjusted_row(c) for c in cs]


@functools.lru_cache(maxsize=None)
def _fsm_for(V):
    """two states: every third token -> state 1; half of the tokens -> the row becomes free"""
    from infinitevl_amd import ops
    from infinitevl_amd.grammar import TokenFsm
    a, b = grammar.every(V, 3, 1), np.random.default_rng(V).random(V) < 0.5
    b[0] = True
    fsm = TokenFsm.from_edges(V, 2, [(0, np.nonzero(a)[0].tolist(), 1), (1, np.nonzero(b)[0].tolist(), TokenFsm.FREE)])
    tab = ops.FsmTables(DEV, V, 3, 1, 2 * fsm.n_classes, mask_ld=generation.words_for(V) + 1)
    h = tab.load(fsm)
    return tab, h


@pytest.mark.parametrize("form", ["ctl", "lp", "fsm"])
@pytest.mark.parametrize("V", [1, 97, 4099])
def test_composition_is_the_old_entry_on_the_adjusted_row(V, form):
    cs, x2 = _op_cases(V)
    tab, h = _fsm_for(V) if form == "fsm" else (None, None)
    a = call = 0
    offs, old_entry = set(), 0
    while a < len(cs):
        S = min((1, 4, 3, 2)[call % 4], len(cs) - a)
        part, part2 = cs[a:a + S], x2[a:a + S]
        ld, shift = _odd_ld(V) + 2 * (call % 3), (0, 3, 7, 8, 5)[call % 5]
        dones = [c.get("done", 0) for c in part]
        states = [(h.base, h.base + 1, -1)[(a + s) % 3] for s in range(S)] if form == "fsm" else None
        common = dict(ld=ld, shift=shift, seen=[c["seen"] for c in part], done=dones, fsm=tab, states=states, n_new0=4)
        got_c = _Call([c["x"] for c in part], part, form, _adj_of(part), **common)
        before = got_c.T["count"].host()
        got = got_c.run().host()
        offs.update(got_c.off)
        # the reference: r = 1 on x''; min-p is not part of x'', so a row with min_p > 0 keeps it (and it alone)
        mps = [c["min_p"] for c in part]
        ref_adj = {"min_p": mps} if any(mps) else None
        old_entry += ref_adj is None
        ref = _Call(part2, [{**c, "r": 1.0} for c in part], form, ref_adj, **common).run().host()
        where = f"V{V} {form} rows {a}..{a + S - 1}"
        _same(got, ref, range(S), where)
        _count_moved_by_the_token(before, got, part, dones, where)
        for s, c in enumerate(part):
            if dones[s]:
                assert got["token"][s, 0] == FILL and got["n_kept"][s] == 0, where
            elif form != "fsm":
                adjust.judge(c, 0, got["token"][s, 0], got["n_kept"][s], got["prob"][s], where=f"{where}: {c['name']}")
        a, call = a + S, call + 1
    assert old_entry >= 2
    assert V == 1 or {0, 3, 7} <= offs, offs


# ---------------------------------------------------------------------------------------------
# 2. min-p
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [97, 4099])
def test_min_p_draws_through_the_judge(V):
    from infinitevl_amd import ops
    n_before = ops.SAMPLE_ADJ_CALLS["adj"]
    for i, c in enumerate(adjust.minp_cases(V)):
        S, per = 4, 64                                                 # 4 rows of the same logits, 64 draws each: counters 0 .. 255
        _, lg = _place([c["x"]] * S, _odd_ld(V), (0, 3, 7)[i % 3])
        dev = lambda v, dt: torch.tensor([v] * S, dtype=dt, device=DEV)
        counter = torch.arange(S, dtype=I64, device=DEV) * per
        tok = torch.full((per, S), -1, dtype=I64, device=DEV)
        kept, prob = torch.full((per, S), -1, dtype=I32, device=DEV), torch.full((per, S), -1.0, device=DEV)
        args = (dev(c["tau"], F32), dev(c["k"], I32), dev(c["p"], F32), dev(c["seed"], I64), counter)
        mp = dev(c["min_p"], F32)
        for j in range(per):
            ops.sample_tokens(lg, *args, out=tok[j], n_kept=kept[j], prob=prob[j], min_p=mp)
        torch.cuda.synchronize()
        assert counter.tolist() == [per * (s + 1) for s in range(S)]
        ref = adjust.reference(c["x"], c["tau"], c["k"], c["p"], c["min_p"])
        assert adjust.has_margins(ref), c["name"]
        ctr = (np.arange(per)[:, None] + per * np.arange(S)[None, :]).reshape(-1)
        sampling.judge(ref, c, ctr, tok.cpu().numpy().reshape(-1), kept.cpu().numpy().reshape(-1), prob.cpu().numpy().reshape(-1),
                       where=c["name"])
        if c["min_p"] == 1.0:                                          # the top class alone
            v = sampling.logits64(c["x"])
            assert ref.n_kept == int((v == v.max()).sum()) and (kept.cpu().numpy() == ref.n_kept).all(), c["name"]
    assert ops.SAMPLE_ADJ_CALLS["adj"] - n_before == 36 * 64


# ---------------------------------------------------------------------------------------------
# 3. identity
# ---------------------------------------------------------------------------------------------
def _off_rows(V, S, seed0):
    cs = []
    for s in range(S):
        seen = generation.random_seen(V, seed0 + s)
        tau, k, p = ((0.0, 0, 1.0), (0.7, 50, 0.9), (1.5, 0, 1.0), (0.7, 0, 0.5))[s % 4]
        c = adjust.case(f"V{V}-off{s}", sampling.random_row(V, seed0 + 10 + s), seen, adjust.random_count(V, seen, seed0 + 20 + s),
                        r=(1.3, 1.0)[s % 2], tau=tau, k=k, p=p, seed=seed0 + s)
        cs.append(c)
    return cs


@pytest.mark.parametrize("form", ["ctl", "lp", "fsm"])
def test_all_off_rows_are_the_call_without_the_group(form):
    V, S = 4099, 4
    cs = _off_rows(V, S, 500)
    tab, h = _fsm_for(V) if form == "fsm" else (None, None)
    states = [h.base, -1, h.base + 1, h.base] if form == "fsm" else None
    common = dict(shift=3, seen=[c["seen"] for c in cs], fsm=tab, states=states)
    xs = [c["x"] for c in cs]
    ref = _Call(xs, cs, form, None, **common).run().host()
    adj = _adj_of(cs, extra_tables=[adjust.random_bias(V, 1)])         # zeros, an honest count, a table nobody points at
    assert not any(adj["min_p"]) and not any(adj["f"]) and not any(adj["pp"]) and all(not 0 <= i < len(adj["tables"]) for i in adj["bias_idx"])
    call = _Call(xs, cs, form, adj, **common)
    before = call.T["count"].host()
    got = call.run().host()
    _same(got, ref, range(S), f"all-off {form}")
    _count_moved_by_the_token(before, got, cs, [0] * S, f"all-off {form}")      # its counts are still kept
    for names in (("min_p",), ("bias_idx",), ("count",), ("f", "pp", "count")):  # any one member of the group alone
        part = {k_: v for k_, v in adj.items() if k_ in names or (k_ == "tables" and "bias_idx" in names)}
        _same(_Call(xs, cs, form, part, **common).run().host(), ref, range(S), f"all-off {form} {names}")


def test_a_null_or_empty_group_is_the_old_entry_and_the_model_vocabulary():
    from infinitevl_amd import _lib, ops
    V = 151936
    cs = _off_rows(V, 2, 700)
    xs = [c["x"] for c in cs]
    common = dict(shift=5, seen=[c["seen"] for c in cs])
    ref = _Call(xs, cs, "ctl", None, **common).run().host()
    got = _Call(xs, cs, "ctl", _adj_of(cs, extra_tables=[adjust.random_bias(V, 2)]), **common).run().host()
    _same(got, ref, range(2), "V151936 all-off")
    # the C entry with adj == NULL and with a group of nothing but NULL / 0
    lib = _lib.load()
    for group in (None, _lib.SampleAdjArgs()):
        c = _Call(xs, cs, "ctl", None, **common)
        T = c.T
        tensors = {k_: T[k_].t for k_ in ("temperature", "top_k", "top_p", "seed", "counter", "n_kept", "prob", "rep_penalty", "seen",
                                         "stop_ids", "budget", "fill", "n_new", "done", "history")}
        a = ops._sample_args(c.lg, dict(tensors, token=T["token"].t), token_stride=1, n_stop=3, hist_ld=HIST)
        rc = lib.ivl_sample_rows_adj_fwd(ctypes.byref(a), None if group is None else ctypes.byref(group),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.ivl_last_error()
        _same(c.host(), ref, range(2), f"V151936 group {group}")


def test_adjusted_rows_of_the_model_vocabulary():
    V = 151936
    seen = generation.random_seen(V, 800, frac=0.1)
    c = adjust.with_margins(lambda s: adjust.case(f"V{V}-s{s}", sampling.random_row(V, s), seen, adjust.random_count(V, seen, 801),
                                                  1.3, 0.5, 0.25, adjust.random_bias(V, 802, ban=3), 0.7, 50, 0.9, 0.05, seed=17), 803)
    g = {**c, "name": "V151936-greedy", "tau": 0.0}
    cs, x2 = [c, g], [adjust.adjusted_row(c)] * 2
    common = dict(shift=3, seen=[seen, seen], n_new0=2)
    call = _Call([c["x"]] * 2, cs, "lp", _adj_of(cs), **common)
    before = call.T["count"].host()
    got = call.run().host()
    ref = _Call(x2, [{**k_, "r": 1.0} for k_ in cs], "lp", {"min_p": [0.05, 0.05]}, **common).run().host()
    _same(got, ref, range(2), "V151936")
    _count_moved_by_the_token(before, got, cs, [0, 0], "V151936")
    for s in range(2):
        adjust.judge(cs[s], 0, got["token"][s, 0], got["n_kept"][s], got["prob"][s])


# ---------------------------------------------------------------------------------------------
# 4. special values
# ---------------------------------------------------------------------------------------------
def test_a_banned_token_is_never_drawn_and_a_forced_one_always():
    from infinitevl_amd import ops
    V, S, n = 97, 4, 1024                                              # 4096 draws of each kind: rows 0, 1 ban, rows 2, 3 force
    x = sampling.random_row(V, 90).float()
    x[40] = 30.0                                                       # without the ban token 40 takes every draw
    x = x.to(torch.bfloat16)
    _, lg = _place([x] * S, _odd_ld(V), 3)
    ban, force = (np.arange(V) == 40, np.full(V, -INF, dtype=np.float32)), (np.arange(V) == 77, np.full(V, INF, dtype=np.float32))
    W = generation.words_for(V)
    bias = types.SimpleNamespace(mask=torch.from_numpy(_words([ban[0], force[0]], W, False)).to(DEV),
                                 val=torch.from_numpy(np.stack([ban[1], force[1]])).to(DEV), n_bias=2, mask_ld=W, ld=V)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    args = (dev([0.7, 1.5] * 2, F32), dev([0, 50, 0, 0], I32), dev([1.0, 0.9, 1.0, 0.5], F32), dev([1, 2, 3, 4], I64),
            torch.zeros(S, dtype=I64, device=DEV))
    idx = dev([0, 0, 1, 1], I32)
    tok = torch.full((n, S), -1, dtype=I64, device=DEV)
    plain = ops.sample_tokens(lg, *[a.clone() for a in args])
    for j in range(n):
        ops.sample_tokens(lg, *args, out=tok[j], bias_idx=idx, bias=bias)
    tok = tok.cpu().numpy()
    assert plain.tolist() == [40] * S
    assert (tok[:, :2] != 40).all() and ((tok[:, :2] >= 0) & (tok[:, :2] < V)).all() and len(np.unique(tok[:, :2])) > 10
    assert (tok[:, 2:] == 77).all()


def test_special_rows_compose_like_any_other():
    V = 97
    sp = adjust.special_row(V)
    x2 = adjust.adjusted_row(sp)
    keys = sampling.logits64(x2)
    assert np.isneginf(keys[[0, 1, 2, 4, 5, 6, 11]]).all() and np.isposinf(keys[[3, 12]]).all(), "NaN / banned = -inf; +inf stays and is forced"
    everything = (np.ones(V, dtype=bool), np.full(V, -INF, dtype=np.float32))
    banned = adjust.case("all-banned", sampling.random_row(V, 91), bias=everything, tau=0.7, k=5, p=0.9, seed=5)
    banned_greedy = {**banned, "name": "all-banned-greedy", "tau": 0.0}
    neg = adjust.case("negative-penalties", sampling.random_row(V, 92), np.ones(V, dtype=bool), np.arange(V, dtype=np.int32) % 4,
                      f=-0.5, pp=-1.0, tau=0.0)
    cs = [sp, banned, banned_greedy, neg]
    for form in ("ctl", "lp"):
        common = dict(shift=7, seen=[c["seen"] for c in cs])
        got = _Call([c["x"] for c in cs], cs, form, _adj_of(cs), **common).run().host()
        ref = _Call([adjust.adjusted_row(c) for c in cs], [{**c, "r": 1.0} for c in cs], form, None, **common).run().host()
        _same(got, ref, range(4), f"special {form}")
        assert got["token"][0, 0] in (3, 12)                           # the two +inf share the mass
        assert 0 <= got["token"][1, 0] < V and got["n_kept"][1] == V   # the all -inf rules: every token weight 1, no top-k cut
        assert got["token"][2, 0] == 0 and got["done"].tolist()[2] == 0
        want = adjust.adjusted_row(neg).float().numpy()
        assert got["token"][3, 0] == int(np.argmax(want)) and (want >= neg["x"].float().numpy()).all()
        if form == "lp":
            assert abs(float(got["logprob"][1]) + np.log(V)) < 1e-5, "the scored distribution is the adjusted one"


# ---------------------------------------------------------------------------------------------
# 5. bounds
# ---------------------------------------------------------------------------------------------
def test_poison_outside_what_a_row_may_read_has_no_effect():
    V = 97
    cs, _ = _op_cases(V)
    cs = [c for c in cs if not c.get("done") and c["bias_mask"] is not None and (c["f"] or c["pp"])][:3]
    assert len(cs) == 3
    xs, common = [c["x"] for c in cs], dict(shift=3, seen=[c["seen"] for c in cs])
    clean = _Call(xs, cs, "lp", _adj_of(cs), poison=False, **common).run().host()
    # padding poisoned (words and bits beyond V, bias values outside the bitmap), a wider count pitch, garbage tables around
    junk = (np.ones(V, dtype=bool), np.full(V, INF, dtype=np.float32))
    adj = _adj_of(cs, extra_tables=[junk])
    adj["tables"].append(junk)
    rng = np.random.default_rng(7)
    for s, c in enumerate(cs):                                         # count words under clear seen bits: anything at all
        garbage = rng.integers(-2 ** 31, 2 ** 31 - 1, size=V).astype(np.int32)
        adj["count"][s] = np.where(c["seen"], c["count"], garbage).astype(np.int32)
    call = _Call(xs, cs, "lp", adj, poison=True, extra_pad=11, **common)
    before = call.T["count"].host()
    ro = {k_: call.T[k_].buf.clone() for k_ in ("bias_mask", "bias_val", "bias_idx", "min_p", "freq_penalty", "pres_penalty")}
    got = call.run().host()
    _same(got, clean, range(3), "poison", names=[n for n in OUTPUTS if n != "seen"])
    for s, c in enumerate(cs):
        bits_, bits_c = generation.unpack(got["seen"][s].view(np.uint32)), generation.unpack(clean["seen"][s].view(np.uint32))
        assert (bits_[:V] == bits_c[:V]).all() and bits_[V:].all() and not bits_c[V:].any()
    _count_moved_by_the_token(before, got, cs, [0] * 3, "poison")
    for k_, was in ro.items():
        assert call.T[k_].buf.cpu().numpy().tobytes() == was.cpu().numpy().tobytes(), f"{k_} is only read"
    # a neighbouring row's parameters, counts and table do not reach this row: row 1 alone, its neighbours replaced
    others = [cs[2], cs[1], cs[0]]
    adj2 = _adj_of(others)
    swapped = _Call([c["x"] for c in others], others, "lp", adj2, poison=False, shift=3, seen=[c["seen"] for c in others]).run().host()
    _same(swapped, clean, [1], "row 1 between other neighbours")


# ---------------------------------------------------------------------------------------------
# 6. the feedback chain
# ---------------------------------------------------------------------------------------------
def _chain_call(x, f, pp):
    c = adjust.case("chain", x, f=f, pp=pp)
    return _Call([x], [c], "ctl", {"f": [f], "pp": [pp], "count": [c["count"]]}, shift=3)


@pytest.mark.parametrize("V,f,pp", [(97, 0.5, 0.0), (4099, 0.25, 0.5), (97, -0.5, 0.0)])
def test_greedy_chain_under_a_frequency_penalty_is_the_hosts(V, f, pp):
    n = 64
    x = sampling.random_row(V, 3)
    want = adjust.frequency_chain(x, f, pp, n)
    assert f < 0 or len(set(want)) > 4
    call = _chain_call(x, f, pp)
    call.T["budget"].t.fill_(-1)
    call.T["stop_ids"].t.fill_(-1)
    toks = torch.full((n, 1), -1, dtype=I64, device=DEV)
    for i in range(n):
        call.run()
        toks[i].copy_(call.T["token"].t[0])
    got = call.host()
    assert toks[:, 0].tolist() == want
    assert got["count"][0, :V].tolist() == np.bincount(want, minlength=V).tolist() and got["n_new"][0] == n
    # the same launch captured in a graph and replayed from the same start: the same bits
    again = _chain_call(x, f, pp)
    again.T["budget"].t.fill_(-1)
    again.T["stop_ids"].t.fill_(-1)
    start = {k_: t.buf.clone() for k_, t in again.T.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again.run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        again.run()
    for k_, was in start.items():
        again.T[k_].buf.copy_(was)
    toks2 = torch.full((n, 1), -1, dtype=I64, device=DEV)
    for i in range(n):
        graph.replay()
        toks2[i].copy_(again.T["token"].t[0])
    rep = again.host()
    assert toks2[:, 0].tolist() == want
    for k_ in got:
        assert rep[k_].tobytes() == got[k_].tobytes(), k_


# ---------------------------------------------------------------------------------------------
# 7. row independence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ctl", "lp", "fsm"])
def test_a_row_alone_equals_the_same_row_as_row_2_of_4(form):
    V = 4099
    cs, _ = _op_cases(V)
    live = [c for c in cs if not c.get("done")]
    tab, h = _fsm_for(V) if form == "fsm" else (None, None)
    for pick in (2, 5, 9):
        me = live[pick]
        four = [live[0], live[7], me, live[11]]
        st4 = [h.base, -1, h.base, h.base + 1] if form == "fsm" else None
        alone = _Call([me["x"]], [me], form, _adj_of([me]), shift=0, seen=[me["seen"]], fsm=tab, states=st4[2:3] if st4 else None)
        among = _Call([c["x"] for c in four], four, form, _adj_of(four), shift=5, seen=[c["seen"] for c in four], fsm=tab, states=st4)
        a, b = alone.run().host(), among.run().host()
        for k_ in OUTPUTS + ("count",):
            if k_ in a:
                assert b[k_][2].tobytes() == a[k_][0].tobytes(), (form, pick, k_)
        # and twice the same call: the same bits
        c = _Call([c["x"] for c in four], four, form, _adj_of(four), shift=5, seen=[c["seen"] for c in four], fsm=tab, states=st4).run().host()
        for k_ in b:
            assert c[k_].tobytes() == b[k_].tobytes(), (form, pick, k_)


# ---------------------------------------------------------------------------------------------
# 8. the graphed decode steps
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(window=96, seed=3):
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(window)
    params = parity.bf16_params(omodel.random_params(oc, seed=seed, vocab=hc.vocab_size))
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, params)
    return stack.to(DEV, torch.bfloat16).eval().fuse_(), hc


def _prompt(hc, T, seed):
    g_ = torch.Generator().manual_seed(seed)
    return (torch.randn(1, T, hc.hidden_size, generator=g_) * 0.5).to(torch.bfloat16).to(DEV)


def _bytes(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()


def _multistream(**kw):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(4, DEV, vocab_size=hc.vocab_size, history=32, logprobs=2, **{"penalties": True, "bias_tables": 2, **kw})
    return GraphedMultiStreamDecode(stack, cache, sampler=smp), hc


BIAS = {5: -INF, 17: 4.0, 300: -2.5, 511: 1.0}
MS_SAMPLING = {0: dict(frequency_penalty=0.8, presence_penalty=0.3), 1: dict(temperature=1.0, seed=5, min_p=0.2, top_k=50),
               2: dict(temperature=1.5, seed=6, frequency_penalty=-0.2), 3: dict()}
N_STEPS = 8


def _ms_run(graph):
    dec, hc = _multistream()
    h = dec.sampler.load_logit_bias(BIAS)
    for slot, (T, seed) in enumerate(((130, 5), (70, 6), (33, 7), (40, 8))):
        dec.admit(slot, _prompt(hc, T, seed), sampling=MS_SAMPLING[slot], logit_bias=h if slot in (1, 2) else None)
    toks = [dec.token[:, 0].tolist()]
    for _ in range(N_STEPS):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
    return dec, toks, h


def test_multistream_captured_step_equals_the_eager_step():
    from infinitevl_amd import ops
    n0 = ops.SAMPLE_ADJ_CALLS["adj"]
    (dec_g, toks_g, h), (dec_e, toks_e, _) = _ms_run(True), _ms_run(False)
    assert ops.SAMPLE_ADJ_CALLS["adj"] > n0
    assert toks_g == toks_e
    sg, se = dec_g.sampler.state(), dec_e.sampler.state()
    for k_, v in sg.items():
        assert v.cpu().numpy().tobytes() == se[k_].cpu().numpy().tobytes(), k_
    assert dec_g.sampler.bias_idx.tolist() == [-1, h.index, h.index, -1]
    count = sg["count"].cpu().numpy()
    for slot in range(4):                                              # counts are of the generated tokens: the first one included
        seq = [t[slot] for t in toks_g]
        assert count[slot].tolist() == np.bincount(seq, minlength=count.shape[1]).tolist(), slot
        assert dec_g.sampler.tokens(slot).tolist() == seq
    assert all(t[1] != 5 and t[2] != 5 for t in toks_g), "token 5 is banned in slots 1 and 2"
    plain, hc = _multistream(penalties=False, bias_tables=0)          # slot 3 has nothing on: a sampler without the keywords
    for slot, (T, seed) in enumerate(((130, 5), (70, 6), (33, 7), (40, 8))):
        plain.admit(slot, _prompt(hc, T, seed), sampling={k_: v for k_, v in MS_SAMPLING[slot].items() if k_ in ("temperature", "seed", "top_k")})
    seq = [plain.token[3, 0].item()]
    for _ in range(N_STEPS):
        plain.step()
        seq.append(plain.token[3, 0].item())
    assert seq == [t[3] for t in toks_g]


def test_parameters_and_tables_change_between_replays_without_a_recapture():
    def start():
        dec, hc = _multistream()
        dec.admit(0, _prompt(hc, 60, 10), sampling=dict(max_new_tokens=None))
        dec.admit(1, _prompt(hc, 60, 10), sampling=dict())
        for _ in range(3):
            dec.step()
        return dec, hc

    dec, hc = start()
    graph = dec.graph
    assert graph is not None
    base = []
    for _ in range(6):
        dec.step()
        base.append(dec.token[0, 0].item())
    assert dec.token[1, 0].item() == base[-1], "two slots with the same prompt and parameters"
    # the same start again; the token that came next is banned in a table loaded between two replays, for slot 0 only
    dec, hc = start()
    graph = dec.graph
    h = dec.sampler.load_logit_bias({base[0]: -INF})
    dec.sampler.set_logit_bias(0, h)
    dec.step()
    assert dec.graph is graph
    assert dec.token[0, 0].item() != base[0] and dec.token[1, 0].item() == base[0]
    assert dec.token[0, 0].item() == dec.sampler.top_ids[0, 0].item(), "the scored distribution is the adjusted one"
    # swapping the table: another one bans what slot 1 would emit next; slot 1 follows slot 0's old future until then
    h2 = dec.sampler.load_logit_bias({base[1]: -INF, (base[1] + 1) % hc.vocab_size: 3.0})
    dec.sampler.set_logit_bias(1, h2)
    dec.step()
    assert dec.graph is graph and dec.token[1, 0].item() != base[1]
    # a penalty changed between replays: from now on slot 1 never repeats a token it has generated
    dec.sampler.unload_logit_bias(h2)                                  # (a freed table biases nothing)
    dec.sampler.freq_penalty[1] = 100.0
    seen_before = set(dec.sampler.tokens(1).tolist())
    fresh = []
    for _ in range(8):
        dec.step()
        fresh.append(dec.token[1, 0].item())
    assert dec.graph is graph
    assert len(set(fresh)) == len(fresh) and not (set(fresh) & seen_before), (fresh, seen_before)


def test_fork_copies_counts_and_the_bias_table_and_capture_leaves_no_trace():
    dec, hc = _multistream()
    h = dec.sampler.load_logit_bias(BIAS)
    dec.admit(0, _prompt(hc, 60, 11), sampling=dict(frequency_penalty=0.6, presence_penalty=0.2), logit_bias=h)
    for _ in range(4):
        dec.step(graph=False)
    owned = dec._slot_tensors() + [dec.sampler.biases.mask, dec.sampler.biases.val]
    was = [t.clone() for t in owned]
    dec.capture()
    for i, (t, w) in enumerate(zip(owned, was)):
        assert _bytes(t) == _bytes(w), f"capture() changed owned tensor {i}"
    dec.fork(0, [1, 2], sampling=[dict(), dict(temperature=1.0, seed=9)])
    smp = dec.sampler
    assert smp.bias_idx.tolist()[:3] == [h.index] * 3 and smp.count[0].any()
    assert torch.equal(smp.count[1], smp.count[0]) and torch.equal(smp.count[2], smp.count[0])
    assert smp.freq_penalty.tolist()[:3] == [float(np.float32(0.6))] * 3
    for _ in range(5):
        dec.step()
        assert dec.token[0, 0].item() == dec.token[1, 0].item()       # the greedy copy follows its parent
        assert dec.token[2, 0].item() != 5
    # admit_n: the table travels with the forked row
    dec2, _ = _multistream()
    h2 = dec2.sampler.load_logit_bias(BIAS)
    dec2.admit_n([0, 1, 2], _prompt(hc, 60, 11), sampling=[dict(temperature=1.0, seed=s, min_p=0.1) for s in (1, 2, 3)], logit_bias=h2)
    assert dec2.sampler.bias_idx.tolist() == [h2.index] * 3 + [-1] and dec2.sampler.min_p.tolist()[:3] == [float(np.float32(0.1))] * 3
    assert dec2.sampler.count.sum(1).tolist() == [1, 1, 1, 0]

"""GPU (-m gpu): constrained decoding inside the sampling launch (ops.sample_tokens fsm_state= / fsm= -> ivl_sample_rows_fwd)
and its use in the graphed decode steps, judged by tests/grammar.py.

  * operator: V in {1, 97, 4099} and one row of 151936; calls of 1 .. 4 rows in a +inf surround at odd ld, shifted bases and
    mask_ld = words + 1 with every bit beyond V set; rows in different states of two grammars beside a free and a finished row.
    Every output bit-equal to the scoring launch on the gathered row x[A] (F3 of the header) AND judged by the float64 references;
  * masks (all allowed = the scoring entry on the same rows, one token, bits 31 / 32 / V-1, allowed logits -inf / NaN under
    disallowed +inf / NaN / maximum, every 7th token), parameters (greedy, sampled, top_k around |A|, top_p, n_top up to 20 > |A|,
    a penalty on allowed seen tokens) -- the cases of grammar.operator_cases;
  * the form without any score keyword (a sampler with grammars and no logprobs) commits the same bits;
  * dead ends (an empty set, a state >= n_states, tables whose transition is missing), determinism, chains over a 5-choice trie;
  * GraphedMultiStreamDecode / GraphedDecode with Sampler(grammar_states=...): eager == replayed graph, a grammar loaded after
    the capture, a free slot beside constrained ones, fork, run_until_done."""
import functools

import numpy as np
import pytest
import torch

import generation
import grammar
import parity
import sampling
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
N_TOPS = (0, 1, 5, 20)
FILL = 7


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
    return buf, lg


def _arena(fsms, V, extra_states=0):
    """the grammars in one arena with mask_ld = words + 1 and EVERY bit at or above V set, in every state's row"""
    from infinitevl_amd import ops
    words = (V + 31) // 32
    tab = ops.FsmTables(DEV, V, sum(f.n_states for f in fsms) + extra_states, len(fsms),
                        sum(f.n_states * f.n_classes for f in fsms), mask_ld=words + 1)
    handles = [tab.load(f) for f in fsms]
    beyond = generation.to_i32(generation.pack(np.zeros(V, dtype=bool), words + 1, beyond=True)).to(DEV)
    tab.mask |= beyond[None, :]
    return tab, handles


def _dev(v, dt):
    return torch.tensor(v, dtype=dt, device=DEV)


def _call(lg, cases, n_top, hist_ld, n_new0, stops, budgets, seen_rows, fsm_state=None, fsm=None, scores=True):
    """ONE launch over the rows of `lg` with every output and state tensor fresh; returns host copies.  scores=False: no score
    keyword at all (n_top must be 0)"""
    from infinitevl_amd import ops
    S = len(cases)
    tab = (_dev([c["tau"] for c in cases], torch.float32), _dev([c["k"] for c in cases], torch.int32),
           _dev([c["p"] for c in cases], torch.float32), _dev([c["seed"] for c in cases], torch.int64),
           torch.zeros(S, dtype=torch.int64, device=DEV))
    t = {"seen": torch.stack(seen_rows).to(DEV), "n_new": _dev([n_new0] * S, torch.int64),
         "done": _dev([c["done"] for c in cases], torch.int32), "stop_ids": _dev(stops, torch.int64),
         "budget": _dev(budgets, torch.int64), "logprob": torch.full((S,), 9.0, device=DEV),
         "cum_logprob": torch.full((S,), -1.5, dtype=torch.float64, device=DEV)}
    kw = dict(t, rep_penalty=_dev([c["r"] for c in cases], torch.float32), fill=_dev([FILL] * S, torch.int64))
    if n_top:
        t["top_ids"] = kw["top_ids"] = torch.full((S, n_top), -7, dtype=torch.int64, device=DEV)
        t["top_logprobs"] = kw["top_logprobs"] = torch.full((S, n_top), 9.0, device=DEV)
    if not scores:
        assert n_top == 0
        for k_ in ("logprob", "cum_logprob"):
            del t[k_], kw[k_]
    if hist_ld:
        t["history"] = kw["history"] = torch.full((S, hist_ld), -5, dtype=torch.int64, device=DEV)
    if hist_ld and scores:
        t["lp_history"] = kw["lp_history"] = torch.full((S, hist_ld), 9.0, device=DEV)
        if n_top:
            t["top_hist_ids"] = kw["top_hist_ids"] = torch.full((S, hist_ld, n_top), -7, dtype=torch.int64, device=DEV)
            t["top_hist_lp"] = kw["top_hist_lp"] = torch.full((S, hist_ld, n_top), 9.0, device=DEV)
    if fsm is not None:
        t["fsm_state"] = kw["fsm_state"] = fsm_state.clone()
        kw["fsm"] = fsm
    t["token"] = torch.full((S, 1), -1, dtype=torch.int64, device=DEV)
    t["n_kept"], t["prob"] = torch.full((S,), -1, dtype=torch.int32, device=DEV), torch.full((S,), -1.0, device=DEV)
    t["counter"] = tab[4]
    ops.sample_tokens(lg, *tab, out=t["token"], n_kept=t["n_kept"], prob=t["prob"], **kw)
    torch.cuda.synchronize()
    return {k_: v.cpu().numpy().copy() for k_, v in t.items()}


STOPS = lambda V: [V - 1, 3 % V, -1]                                  # (a draw that hits one ends its row: done = 1)


def _constrained(cases, states, tab, n_top, ld, shift, hist_ld=0, n_new0=0, scores=True):
    V = cases[0]["x"].shape[0]
    W = generation.words_for(V) + 1
    _, lg = _place([c["x"] for c in cases], ld, shift)
    seen = [generation.to_i32(generation.pack(c["seen"], W, beyond=True)) for c in cases]
    budgets = [n_new0 + 1 if i % 2 else -1 for i in range(len(cases))]
    return _call(lg, cases, n_top, hist_ld, n_new0, [STOPS(V)] * len(cases), budgets, seen,
                 fsm_state=_dev(states, torch.int32), fsm=tab, scores=scores)


def _gathered(c, i, n_top, hist_ld=0, n_new0=0):
    """row i of a call as the scoring launch sees its allowed sub-vocabulary: x[A], the seen bits of A, the stop ids inside A"""
    V = c["x"].shape[0]
    xg, sg, A = grammar.gather(c["x"], c["seen"], c["allow"])
    Vg = A.shape[0]
    lg = xg.to(DEV)[None, :].contiguous()
    stops = [int(np.searchsorted(A, t)) if 0 <= t and (A == t).any() else -1 for t in STOPS(V)]
    seen = [generation.to_i32(generation.pack(sg, generation.words_for(Vg), beyond=True))]
    return _call(lg, [c], n_top, hist_ld, n_new0, [stops], [n_new0 + 1 if i % 2 else -1], seen), A


def _same_as_gathered(c, s, got, ref, A, n_top, hist_ld, where):
    """F3: every output of row s of `got` is, bit for bit, the scoring launch's on the gathered row (ids mapped through A)"""
    V = c["x"].shape[0]
    live = not c["done"]
    assert got["token"][s, 0] == (A[ref["token"][0, 0]] if live else FILL), where
    for k_ in ("counter", "n_kept", "prob", "logprob", "n_new", "done", "cum_logprob") + (("lp_history",) if hist_ld else ()):
        assert got[k_][s].tobytes() == ref[k_][0].tobytes(), (where, k_, got[k_][s], ref[k_][0])
    if n_top:
        assert got["top_ids"][s].tolist() == grammar.to_vocab(ref["top_ids"][0], A).tolist(), where
        assert got["top_logprobs"][s].tobytes() == ref["top_logprobs"][0].tobytes(), where
        assert (got["top_ids"][s][min(n_top, A.shape[0]):] == -1).all(), where
    if hist_ld:
        h = ref["history"][0]
        assert got["history"][s].tolist() == np.where(h >= 0, A[np.clip(h, 0, A.shape[0] - 1)], h).tolist(), where
        if n_top:
            assert got["top_hist_ids"][s].tolist() == np.where(ref["top_hist_ids"][0] >= 0, A[np.clip(ref["top_hist_ids"][0], 0,
                                                               A.shape[0] - 1)], ref["top_hist_ids"][0]).tolist(), where
            assert got["top_hist_lp"][s].tobytes() == ref["top_hist_lp"][0].tobytes(), where
    # the bitmap: the bits of A are the gathered call's; nothing else moved (other tokens, the tail beyond V)
    bits, bits_g = generation.unpack(got["seen"][s].view(np.uint32)), generation.unpack(ref["seen"][0].view(np.uint32))
    assert (bits[:V][A] == bits_g[:A.shape[0]]).all(), where
    rest = np.ones(V, dtype=bool)
    rest[A] = False
    assert (bits[:V][rest] == c["seen"][rest]).all() and bits[V:].all(), where


def _check_call(cases, states, fsms, handles, owner, tab, n_top, ld, shift, hist_ld=0, n_new0=0):
    got = _constrained(cases, states, tab, n_top, ld, shift, hist_ld, n_new0)
    for s, c in enumerate(cases):
        where = f"{c['name']} n_top={n_top} row {s} of {len(cases)}"
        ref, A = _gathered(c, s, n_top, hist_ld, n_new0)
        _same_as_gathered(c, s, got, ref, A, n_top, hist_ld, where)
        if c["done"]:
            assert got["fsm_state"][s] == states[s], where            # a finished row: not even its state is looked at
            continue
        tok = int(got["token"][s, 0])
        grammar.judge(c, 0, tok, got["n_kept"][s], got["prob"][s], got["logprob"][s], got["top_ids"][s] if n_top else None,
                      got["top_logprobs"][s] if n_top else None, where=where)
        if owner[s] is None:
            assert got["fsm_state"][s] == -1, where
        else:
            g, q = owner[s]
            nxt = fsms[g].step(q, tok)
            assert got["fsm_state"][s] == (nxt + handles[g].base if nxt >= 0 else nxt), where
    return got


@functools.lru_cache(maxsize=None)
def _setup(V):
    cases = grammar.operator_cases(V)
    free = grammar.case(f"V{V}-free-row", sampling.random_row(V, 21, scale=2.0), None, tau=0.7, k=50, p=1.0, seed=13)
    fin = grammar.case(f"V{V}-finished-row", sampling.random_row(V, 22), grammar.every(V, 3), tau=0.7, seed=14, done=1)
    cases = cases[:2] + [free] + cases[2:3] + [fin] + cases[3:]      # rows 1 .. 4 are one call of four
    fa, fb, where = grammar.grammars_for(cases, V)
    tab, handles = _arena([fa, fb], V)
    states = [-1 if w is None else handles[w[0]].base + w[1] for w in where]
    return cases, states, (fa, fb), handles, where, tab


# ---------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 97, 4099])
def test_operator_every_row_kind_and_n_top(V):
    cases, states, fsms, handles, where, tab = _setup(V)
    a = call = 0
    sizes, kinds = set(), set()
    while a < len(cases):
        S = min((1, 4, 3, 2)[call % 4], len(cases) - a)
        sl = slice(a, a + S)
        ld, shift = _odd_ld(V) + 2 * (call % 3), (0, 1, 5, 8, 3)[call % 5]
        for n_top in N_TOPS:
            hist_ld, n_new0 = ((3, 4) if n_top in (0, 5) else (0, 0))    # with the rings: the ring index is 4 % 3
            _check_call(cases[sl], states[sl], fsms, handles, where[sl], tab, n_top, ld, shift, hist_ld, n_new0)
        sizes.add(S)
        if S == 4:
            kinds.add((any(w is None for w in where[sl]), any(c["done"] for c in cases[sl]), len({w[0] for w in where[sl] if w})))
        a, call = a + S, call + 1
    assert {1, 4} <= sizes
    assert V == 1 or (True, True, 2) in kinds                          # one call: both grammars, a free and a finished row


def test_single_row_of_the_model_vocabulary():
    from infinitevl_amd.grammar import TokenFsm
    V = 151936
    e7 = grammar.every(V, 7, 3)
    half = np.random.default_rng(5).random(V) < 0.5
    q = generation.random_seen(V, 5, frac=0.1)
    rows = [(grammar.sampled("V151936-every7-pen", V, e7, 0.7, 50, 0.9, 300, r=1.3, seen=q), 20),
            (grammar.case("V151936-half-greedy", sampling.random_row(V, 23), half), 5)]
    fsm = TokenFsm.from_edges(V, 2, [(0, np.nonzero(e7)[0].tolist(), 1), (1, np.nonzero(half)[0].tolist(), TokenFsm.FREE)])
    tab, (h,) = _arena([fsm], V)
    for i, (c, n_top) in enumerate(rows):
        _check_call([c], [h.base + i], (fsm,), (h,), [(0, i)], tab, n_top, _odd_ld(V), 3)


def test_all_allowed_is_the_scoring_entry_on_the_same_rows():
    V = 4099
    cases, states, fsms, handles, where, tab = _setup(V)
    full = [i for i, c in enumerate(cases) if c["allow"] is not None and c["allow"].all() and not c["done"]]
    pen = [i for i, c in enumerate(cases) if "half-pen" in c["name"]]
    grp = [dict(cases[i], allow=np.ones(V, dtype=bool)) for i in full + pen]
    st = [states[full[0]]] * len(grp)                                  # every row in one state that allows everything
    ld, shift = _odd_ld(V), 5
    got = _constrained(grp, st, tab, 5, ld, shift, hist_ld=3, n_new0=4)
    W = generation.words_for(V) + 1
    _, lg = _place([c["x"] for c in grp], ld, shift)
    ref = _call(lg, grp, 5, 3, 4, [STOPS(V)] * len(grp), [5 if i % 2 else -1 for i in range(len(grp))],
                [generation.to_i32(generation.pack(c["seen"], W, beyond=True)) for c in grp])
    for k_, v in ref.items():
        assert got[k_].tobytes() == v.tobytes(), k_


@pytest.mark.parametrize("V", [97, 4099])
def test_without_a_score_keyword_the_draw_and_the_state_are_the_same(V):
    """a sampler with grammars and no logprobs: the form skips L1-L3 and commits what it commits with them"""
    cases, states, fsms, handles, where, tab = _setup(V)
    empty = handles[0].base + fsms[0].n_states - 1
    for a in range(0, len(cases), 4):
        grp, st = cases[a:a + 4], list(states[a:a + 4])
        if a == 4:
            st[1] = empty                                             # a dead end among them
        with_scores = _constrained(grp, st, tab, 0, _odd_ld(V), 3, hist_ld=3, n_new0=4)
        without = _constrained(grp, st, tab, 0, _odd_ld(V), 3, hist_ld=3, n_new0=4, scores=False)
        assert set(with_scores) - set(without) == {"logprob", "cum_logprob", "lp_history"}
        for k_, v in without.items():
            assert with_scores[k_].tobytes() == v.tobytes(), (a, k_)
        if a == 4:
            assert without["done"][1] == 3 and without["token"][1, 0] == FILL


# ---------------------------------------------------------------------------------------------
# 2. dead ends
# ---------------------------------------------------------------------------------------------
def test_dead_ends_leave_the_row_and_its_neighbours_alone():
    V = 97
    cases, states, fsms, handles, where, tab = _setup(V)
    live = [i for i, c in enumerate(cases) if "half-pen-1.3" in c["name"] or "every7-topp" in c["name"]]
    empty = handles[0].base + fsms[0].n_states - 1                     # allows nothing below V (its bits beyond V are set)
    dead = [dict(cases[live[0]], name="dead-empty"), dict(cases[live[1]], name="dead-no-such-state")]
    grp = [cases[live[0]], dead[0], dead[1], cases[live[1]]]
    for no_such in (tab.n_states, 2 ** 31 - 1):
        st = [states[live[0]], empty, no_such, states[live[1]]]
        for n_top in (0, 5):
            got = _constrained(grp, st, tab, n_top, _odd_ld(V), 1, hist_ld=3, n_new0=4)
            for s in (1, 2):
                assert got["done"][s] == 3 and got["token"][s, 0] == FILL and got["n_kept"][s] == 0 and got["prob"][s] == 0.0
                assert got["counter"][s] == 0 and got["n_new"][s] == 4 and got["fsm_state"][s] == st[s]
                assert got["logprob"][s] == 0.0 and got["cum_logprob"][s] == -1.5
                assert (got["history"][s] == -5).all() and (got["lp_history"][s] == 9.0).all()
                want = generation.pack(grp[s]["seen"], generation.words_for(V) + 1, beyond=True)
                assert (got["seen"][s].view(np.uint32) == want).all()
                if n_top:
                    assert (got["top_ids"][s] == -1).all() and (got["top_logprobs"][s] == -INF).all()
                    assert (got["top_hist_ids"][s] == -7).all()
            for s, i in ((0, live[0]), (3, live[1])):                 # the neighbours: what they give alone
                alone = _constrained([cases[i]], [states[i]], tab, n_top, _odd_ld(V), 1, hist_ld=3, n_new0=4)
                for k_ in alone:
                    if k_ not in ("budget", "done", "n_new"):         # (the budget of a row follows its place in the call)
                        assert got[k_][s].tobytes() == alone[k_][0].tobytes(), (k_, s)


def test_a_missing_transition_ends_the_row_behind_its_draw():
    from infinitevl_amd.grammar import TokenFsm
    V = 97
    fsm = TokenFsm.from_edges(V, 2, [(0, list(range(0, V, 2)), 1), (1, list(range(V)), 0)])
    tab, (h,) = _arena([fsm], V)
    tab.trans[:fsm.n_classes] = -2                                     # state 0's bitmap still allows the even tokens
    c = grammar.case("no-transition", sampling.random_row(V, 41), fsm.allowed(0), tau=0.7, seed=3)
    got = _constrained([c, c], [h.base, h.base + 1], tab, 5, _odd_ld(V), 0)
    ref, A = _gathered(c, 0, 5)
    assert got["token"][0, 0] == A[ref["token"][0, 0]] and got["token"][0, 0] % 2 == 0
    assert got["done"][0] == 3 and got["fsm_state"][0] == h.base and got["counter"][0] == 1 and got["n_new"][0] == 1
    assert got["logprob"][0].tobytes() == ref["logprob"][0].tobytes()
    assert got["done"][1] in (1, 2) and got["fsm_state"][1] == h.base      # the neighbour went on to state 0 (its budget is 1)


# ---------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------
def test_same_call_twice_and_a_row_alone_or_among_four():
    V = 4099
    cases, states, fsms, handles, where, tab = _setup(V)
    pick = [i for i, c in enumerate(cases) if any(t in c["name"] for t in ("all-sampled", "half-pen-1.3", "every7-topp",
                                                                            "ninf-inside-sampled"))]
    assert len(pick) == 4
    grp, st = [cases[i] for i in pick], [states[i] for i in pick]
    a = _constrained(grp, st, tab, 20, _odd_ld(V), 5, hist_ld=3, n_new0=4)
    b = _constrained(grp, st, tab, 20, _odd_ld(V), 5, hist_ld=3, n_new0=4)
    for k_ in a:
        assert a[k_].tobytes() == b[k_].tobytes(), k_
    for s in (0, 2):                                                  # (even places: the same budget alone and in the call)
        alone = _constrained([grp[s]], [st[s]], tab, 20, _odd_ld(V) + 4, 2, hist_ld=3, n_new0=4)
        for k_ in a:
            assert a[k_][s].tobytes() == alone[k_][0].tobytes(), (k_, s)


# ---------------------------------------------------------------------------------------------
# 4. chains
# ---------------------------------------------------------------------------------------------
CHOICES = ([11, 60], [11, 61, 5], [40], [41, 41, 41, 2], [96, 0])
STOP = 90


def _chain(then, steps=12):
    """`steps` launches on fixed logits: four sampled rows with their own seeds and a greedy one, all from the start state"""
    from infinitevl_amd import ops
    from infinitevl_amd.grammar import TokenFsm
    V, S = 97, 5
    fsm = TokenFsm.from_choices(V, CHOICES, stop_token_ids=[STOP] if then == TokenFsm.END else (), then=then)
    tab, (h,) = _arena([fsm], V, extra_states=2)
    _, lg = _place([sampling.random_row(V, 70 + s, scale=2.0) for s in range(S)], _odd_ld(V), 3)
    par = (_dev([1.0, 1.5, 0.7, 2.0, 0.0], torch.float32), torch.zeros(S, dtype=torch.int32, device=DEV),
           torch.ones(S, device=DEV), _dev([5, 6, 7, 8, 9], torch.int64), torch.zeros(S, dtype=torch.int64, device=DEV))
    st = {"fsm_state": _dev([h.base + fsm.start] * S, torch.int32), "done": torch.zeros(S, dtype=torch.int32, device=DEV),
          "n_new": torch.zeros(S, dtype=torch.int64, device=DEV), "stop_ids": _dev([[STOP if then == TokenFsm.END else -1]] * S, torch.int64),
          "fill": _dev([FILL] * S, torch.int64), "logprob": torch.zeros(S, device=DEV)}
    tok = torch.zeros(S, 1, dtype=torch.int64, device=DEV)
    log = []
    for _ in range(steps):
        before = par[4].cpu().tolist()
        ops.sample_tokens(lg, *par, out=tok, **st, fsm=tab)
        log.append({"token": tok[:, 0].cpu().tolist(), "state": st["fsm_state"].cpu().tolist(), "done": st["done"].cpu().tolist(),
                    "counter": before, "logprob": st["logprob"].cpu().tolist()})
    return fsm, h, lg, par, log


def test_chain_emits_one_of_the_choices_then_the_stop_id():
    from infinitevl_amd.grammar import TokenFsm
    fsm, h, _, _, log = _chain(TokenFsm.END)
    seqs = set()
    for s in range(5):
        q, out = fsm.start, []
        for i, step in enumerate(log):
            if out and out[-1] == STOP:                               # ended: the fill token, the state where it stopped
                assert step["token"][s] == FILL and step["done"][s] == 1 and step["state"][s] == h.base + q, (s, i)
                continue
            t = step["token"][s]
            assert fsm.allowed(q)[t], (s, i, t)
            q = fsm.step(q, t)
            out.append(t)
            assert step["state"][s] == h.base + q and step["done"][s] == (1 if t == STOP else 0), (s, i)
        assert out[-1] == STOP and out[:-1] in [list(c) for c in CHOICES], (s, out)
        seqs.add(tuple(out))
    assert len(seqs) >= 2                                             # the seeds did not all take one branch


def test_chain_that_frees_the_row_then_matches_the_unconstrained_sampler():
    from infinitevl_amd import ops
    from infinitevl_amd.grammar import TokenFsm
    fsm, h, lg, par, log = _chain(TokenFsm.FREE)
    S = 5
    for s in range(S):
        q = fsm.start
        for i, step in enumerate(log):
            t = step["token"][s]
            assert q == TokenFsm.FREE or fsm.allowed(q)[t], (s, i, t)
            q = fsm.step(q, t)
            assert step["state"][s] == (h.base + q if q >= 0 else -1) and step["done"][s] == 0, (s, i)
        assert q == TokenFsm.FREE
    # from the step behind the last choice on, every row is free: the plain scoring launch from the same counters
    first_free = max(len(c) for c in CHOICES)
    for i in range(first_free, len(log)):
        ctr = _dev(log[i]["counter"], torch.int64)
        tok = torch.zeros(S, 1, dtype=torch.int64, device=DEV)
        lp = torch.zeros(S, device=DEV)
        ops.sample_tokens(lg, par[0], par[1], par[2], par[3], ctr, out=tok, logprob=lp)
        assert tok[:, 0].cpu().tolist() == log[i]["token"], i
        assert lp.cpu().numpy().tobytes() == np.asarray(log[i]["logprob"], dtype=np.float32).tobytes(), i
    assert len({tuple(st["token"]) for st in log[first_free:]}) > 1


# ---------------------------------------------------------------------------------------------
# 5. the graphed decode steps
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


G_STOP = 500
G_A = ([17, 300, 3], [17, 300, 511], [17, 5], [256], [31, 32, 33, 31])
G_B = ([100, 101], [100, 102, 103], [7])
SAMPLING = {0: dict(temperature=1.5, seed=11, stop_token_ids=[G_STOP]), 1: dict(stop_token_ids=[G_STOP]),
            2: dict(temperature=0.7, top_k=50, top_p=0.9, seed=12)}
N_STEPS = 7


def _fsms(V):
    from infinitevl_amd.grammar import TokenFsm
    return (TokenFsm.from_choices(V, G_A, stop_token_ids=[G_STOP]), TokenFsm.from_choices(V, G_B, stop_token_ids=[G_STOP]))


def _multistream(with_grammars=True):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(4, DEV, vocab_size=hc.vocab_size, history=16, logprobs=2, grammar_states=32 if with_grammars else 0)
    return GraphedMultiStreamDecode(stack, cache, sampler=smp), hc


def _walk(fsm, tokens, stop=G_STOP):
    """the host's chain over a slot's tokens: every token allowed where it was emitted; returns the states behind each token"""
    q, states = fsm.start, []
    for t in tokens:
        assert fsm.allowed(q)[t], (tokens, t, q)
        q = fsm.step(q, t)
        states.append(q)
        if t == stop:
            break
    return states


def _ms_run(graph, with_grammars=True):
    """slots 0 and 1 under two grammars (sampled / greedy), slot 2 free; the tokens of every step and the decoder"""
    dec, hc = _multistream(with_grammars)
    fa, fb = _fsms(hc.vocab_size)
    hs = (dec.sampler.load_grammar(fa), dec.sampler.load_grammar(fb)) if with_grammars else (None, None)
    for slot, (T, seed) in enumerate(((130, 5), (70, 6), (33, 7))):
        dec.admit(slot, _prompt(hc, T, seed), sampling=SAMPLING[slot], grammar=hs[slot] if slot < 2 else None)
    toks, states = [dec.token[:, 0].tolist()], []
    if with_grammars:
        states.append([dec.sampler.grammar_state(s) for s in range(3)])
    for _ in range(N_STEPS):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
        if with_grammars:
            states.append([dec.sampler.grammar_state(s) for s in range(3)])
    return dec, toks, states, (fa, fb)


def test_multistream_eager_equals_graph_beside_a_free_slot():
    (dec_g, toks_g, st_g, fsms), (dec_e, toks_e, st_e, _) = _ms_run(True), _ms_run(False)
    assert toks_g == toks_e and st_g == st_e
    for k_, v in dec_g.sampler.state().items():
        assert v.cpu().numpy().tobytes() == dec_e.sampler.state()[k_].cpu().numpy().tobytes(), k_
    done = dec_g.sampler.poll()[0].tolist()
    for slot, fsm in enumerate(fsms):                                 # the first token is constrained too
        seq = [t[slot] for t in toks_g]
        walked = _walk(fsm, seq)
        n = len(walked)
        assert seq[n - 1] == G_STOP and seq[:n - 1] in [list(c) for c in (G_A, G_B)[slot]], (slot, seq)
        assert all(t == 0 for t in seq[n:]) and done[slot] == 1       # then the fill token
        assert [s[slot] for s in st_g[:n]] == walked and dec_g.sampler.tokens(slot).tolist() == seq[:n]
    assert all(s[2] is None for s in st_g) and done[2] == 0
    _, toks_plain, _, _ = _ms_run(True, with_grammars=False)          # the free slot: a sampler without grammars
    assert [t[2] for t in toks_plain] == [t[2] for t in toks_g]
    assert [t[0] for t in toks_plain] != [t[0] for t in toks_g]       # (and the grammars did change the other slots)


def test_a_grammar_loaded_after_the_capture_is_obeyed_without_a_recapture():
    dec, hc = _multistream()
    fa, fb = _fsms(hc.vocab_size)
    for slot, (T, seed) in enumerate(((40, 8), (50, 9))):
        dec.admit(slot, _prompt(hc, T, seed), sampling=dict(temperature=1.0, seed=20 + slot, stop_token_ids=[G_STOP]))
    dec.step()
    dec.step()
    graph = dec.graph
    assert graph is not None
    hb = dec.sampler.load_grammar(fb)                                 # loaded and set between two replays
    dec.sampler.set_grammar(1, hb)
    seq = []
    for _ in range(5):
        dec.step()
        seq.append(dec.token[1, 0].item())
    assert dec.graph is graph
    n = len(_walk(fb, seq))
    assert seq[n - 1] == G_STOP and seq[:n - 1] in [list(c) for c in G_B], seq
    assert dec.sampler.grammar_state(0) is None and dec.sampler.poll()[0].tolist()[:2] == [0, 1]
    dec.sampler.unload_grammar(hb)                                    # its states allow nothing now
    dec.sampler.set(0, temperature=1.0, seed=3)
    dec.sampler.fsm_state[0] = hb.base
    dec.step()
    assert dec.graph is graph and dec.sampler.poll()[0].tolist()[0] == 3


def test_fork_continues_from_the_parents_state_and_run_until_done():
    dec, hc = _multistream()
    fa, _ = _fsms(hc.vocab_size)
    ha = dec.sampler.load_grammar(fa)
    dec.admit(0, _prompt(hc, 60, 10), sampling=dict(temperature=2.0, seed=1, stop_token_ids=[G_STOP]), grammar=ha)
    first = dec.token[0, 0].item()
    parent = dec.sampler.grammar_state(0)
    assert parent == fa.step(fa.start, first)
    dec.fork(0, [1, 2, 3], sampling=[dict(seed=2), dict(seed=3), dict(seed=4)])
    assert [dec.sampler.grammar_state(s) for s in range(4)] == [parent] * 4
    out = dec.run_until_done(12, poll_every=3)
    assert dec.sampler.poll()[0].tolist() == [1, 1, 1, 1]
    for slot in range(4):
        seq = out[slot].tolist()
        assert seq[0] == first and seq[-1] == G_STOP and seq[:-1] in [list(c) for c in G_A], (slot, seq)
        assert len(_walk(fa, seq)) == len(seq)
    # admit_n: the grammar travels with the forked row, every slot draws its own first token under it
    dec2, _ = _multistream()
    hb = dec2.sampler.load_grammar(_fsms(hc.vocab_size)[1])
    dec2.admit_n([0, 1, 2], _prompt(hc, 60, 10), sampling=[dict(temperature=2.0, seed=s, stop_token_ids=[G_STOP]) for s in (1, 2, 3)],
                 grammar=hb)
    out = dec2.run_until_done(12, poll_every=3)
    for slot in range(3):
        seq = out[slot].tolist()
        assert seq[-1] == G_STOP and seq[:-1] in [list(c) for c in G_B], (slot, seq)


def test_graphed_decode_batch_one_under_a_grammar():
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = _small()
    fa, _ = _fsms(hc.vocab_size)
    runs = []
    for graphed in (True, False):
        cache = stack.allocate_inference_cache(1)
        with torch.no_grad():
            pid = torch.arange(64, device=DEV)[None, None, :].expand(3, 1, 64)
            _, lg = stack(inputs_embeds=_prompt(hc, 64, 31), position_ids=pid, past_key_values=cache, logits_to_keep=1)
        smp = Sampler(1, DEV, vocab_size=hc.vocab_size, history=16, logprobs=2, grammar_states=16)
        smp.set(0, temperature=1.5, seed=42, stop_token_ids=[G_STOP])
        smp.set_grammar(0, smp.load_grammar(fa))
        dec = GraphedDecode(stack, cache, 1, sampler=smp)
        smp.sample(lg[:, -1], dec.token)
        toks = [dec.token[0, 0].item()]
        for _ in range(6):
            if graphed:
                dec.step()
            else:
                with torch.no_grad():
                    dec.logits = dec._run()
                cache.advance(1)
            toks.append(dec.token[0, 0].item())
        runs.append((toks, {k_: v.cpu() for k_, v in smp.state().items()}))
        n = len(_walk(fa, toks))
        assert toks[n - 1] == G_STOP and toks[:n - 1] in [list(c) for c in G_A] and smp.tokens(0).tolist() == toks[:n]
    assert runs[0][0] == runs[1][0]
    for k_ in runs[0][1]:
        assert runs[0][1][k_].numpy().tobytes() == runs[1][1][k_].numpy().tobytes(), k_

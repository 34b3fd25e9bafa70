"""CPU (-m "not gpu"): the host side of constrained decoding -- grammar.TokenFsm's three builders against tables written by hand,
its token classes, tails and refusals; the constraint group of ivl_sample_args and ivl_sample_rows_fwd's
error codes for it on pointers that are never dereferenced; the ABI version; ops.FsmTables, ops.sample_tokens' and Sampler's new
arguments; what the graphed classes refuse before any device work; and the builders of tests/grammar.py."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import fork as fk
import generation
import grammar
import sampling
from conftest import ROOT
from infinitevl_amd.grammar import TokenFsm

FREE, NONE = TokenFsm.FREE, TokenFsm.NONE


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def _bits(mask_row, V):
    return generation.unpack(mask_row)[:V]


def _consistent(f):
    """bit set <=> transition != NONE, for every state; cls and trans in range; the words' tail is clear"""
    assert f.mask.dtype == np.uint32 and f.mask.shape == (f.n_states, (f.vocab_size + 31) // 32)
    assert f.cls.dtype == np.int32 and f.cls.shape == (f.vocab_size,) and f.cls.min() == 0 and f.cls.max() == f.n_classes - 1
    assert f.trans.dtype == np.int32 and f.trans.shape == (f.n_states, f.n_classes)
    assert ((f.trans >= NONE) & (f.trans < f.n_states)).all()
    for q in range(f.n_states):
        full = generation.unpack(f.mask[q])
        assert (full[:f.vocab_size] == (f.trans[q][f.cls] != NONE)).all() and not full[f.vocab_size:].any(), q
        assert (f.allowed(q) == full[:f.vocab_size]).all()


# ---------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------
def test_from_edges_against_a_table_by_hand():
    f = TokenFsm.from_edges(6, 3, [(0, [1, 4], 1), (0, [2], FREE), (1, [1, 4], 2), (1, [5], 0), (2, 3, 2)], start=0)
    # classes by the lowest token id: {0} never allowed, {1, 4}, {2}, {3}, {5}
    assert f.cls.tolist() == [0, 1, 2, 3, 1, 4] and f.n_classes == 5 and f.start == 0
    assert f.trans.tolist() == [[NONE, 1, FREE, NONE, NONE], [NONE, 2, NONE, NONE, 0], [NONE, NONE, NONE, 2, NONE]]
    assert f.mask.tolist() == [[0b010110], [0b110010], [0b001000]]
    _consistent(f)
    assert f.step(0, 4) == 1 and f.step(0, 2) == FREE and f.step(FREE, 0) == FREE and f.step(1, 5) == 0 and f.step(2, 3) == 2
    assert f.allowed(FREE).all() and f.allowed(1).tolist() == [False, True, False, False, True, True]
    with pytest.raises(ValueError, match="does not allow"):
        f.step(0, 3)
    with pytest.raises(ValueError, match="token"):
        f.step(0, 6)
    with pytest.raises(ValueError, match="two targets"):
        TokenFsm.from_edges(6, 2, [(0, [1], 1), (0, [1], 0), (1, [0], 0)])
    for bad in ([(2, [1], 0)], [(0, [6], 0)], [(0, [1], 2)], [(0, [1], -2)], [(0, [True], 0)]):
        with pytest.raises(ValueError):
            TokenFsm.from_edges(6, 2, bad)
    with pytest.raises(ValueError, match="start"):
        TokenFsm.from_edges(6, 2, [(0, [1], 0)], start=2)


def test_from_choices_two_choice_trie_by_hand():
    # "yes" = [3, 7], "no" = [5]; stop id 9
    f = TokenFsm.from_choices(10, [[3, 7], [5]], stop_token_ids=[9])
    assert f.n_states == 3 and f.start == 0                           # the root, the node behind 3, the end state
    assert f.cls.tolist() == [0, 0, 0, 1, 0, 2, 0, 3, 0, 4]
    assert f.trans.tolist() == [[NONE, 1, 2, NONE, NONE], [NONE, NONE, NONE, 2, NONE], [NONE, NONE, NONE, NONE, 2]]
    assert f.mask.tolist() == [[(1 << 3) | (1 << 5)], [1 << 7], [1 << 9]]
    _consistent(f)
    q = f.start
    for t in (3, 7, 9, 9):
        q = f.step(q, t)
    assert q == 2


def test_token_classes_merge_over_a_wide_vocabulary():
    V = 4099
    choices = [[17, 4000, 3], [17, 4000, 4098], [17, 5], [2048], [31, 32, 33, 31]]
    used = {t for c in choices for t in c}
    f = TokenFsm.from_choices(V, choices, stop_token_ids=[2])
    assert f.n_classes <= len(used) + 2 and f.trans.size < 200
    _consistent(f)
    g = TokenFsm.from_choices(V, choices, then=FREE)
    assert g.n_classes <= len(used) + 2
    _consistent(g)


def test_prefix_choices_and_the_two_tails():
    # [4] is a prefix of [4, 6]
    end = TokenFsm.from_choices(8, [[4], [4, 6], [1, 2]], stop_token_ids=[7], then=TokenFsm.END)
    _consistent(end)
    q = end.step(end.start, 4)
    assert np.nonzero(end.allowed(q))[0].tolist() == [6, 7]           # go on, or stop here
    e = end.step(q, 7)
    assert np.nonzero(end.allowed(e))[0].tolist() == [7] and end.step(e, 7) == e and end.step(end.step(q, 6), 7) == e
    assert np.nonzero(end.allowed(end.start))[0].tolist() == [1, 4]
    free = TokenFsm.from_choices(8, [[4], [4, 6], [1, 2]], then=FREE)
    _consistent(free)
    assert free.step(free.start, 4) == FREE                           # the shortest complete choice frees the row
    assert free.step(free.step(free.start, 1), 2) == FREE and free.n_states == 2
    with pytest.raises(ValueError, match="stop_token_ids"):
        TokenFsm.from_choices(8, [[4]], then=TokenFsm.END)
    for bad in (dict(choices=[]), dict(choices=[[]]), dict(choices=[[8]]), dict(choices=[[1]], stop_token_ids=[-1]),
                dict(choices=[[1]], stop_token_ids=[2], then=0)):
        with pytest.raises(ValueError):
            TokenFsm.from_choices(8, **{"stop_token_ids": [7], **bad})


def test_a_reachable_state_without_tokens_is_named():
    with pytest.raises(ValueError, match="state 2 is reachable"):
        TokenFsm.from_edges(5, 3, [(0, [1], 1), (1, [2], 2)])
    TokenFsm.from_edges(5, 3, [(0, [1], 1), (1, [2], 0)])             # state 2 allows nothing and is never reached: legal


def _integer_dfa():
    """-?[0-9]+ : 0 start, 1 after the sign, 2 inside the digits (accepting)"""
    bt = np.full((3, 256), -1, dtype=np.int32)
    bt[0, ord("-")] = 1
    for d in b"0123456789":
        bt[0, d] = bt[1, d] = bt[2, d] = 2
    return bt


def test_from_byte_dfa_on_a_toy_vocabulary():
    vocab = [b"", b"-", b"0", b"1", b"12", b"-3", b"a", b"1a", b"--", b"9", b"<eos>", b"00"]
    f = TokenFsm.from_byte_dfa(vocab, _integer_dfa(), 0, [2], stop_token_ids=[10])
    assert f.n_states == 4 and f.vocab_size == 12 and f.start == 0
    allowed = [np.nonzero(f.allowed(q))[0].tolist() for q in range(4)]
    digits = [2, 3, 4, 9, 11]
    assert allowed == [[1] + digits[:3] + [5] + digits[3:], digits, digits[:4] + [10, 11], [10]]
    assert f.step(0, 1) == 1 and f.step(0, 5) == 2 and f.step(1, 4) == 2 and f.step(2, 11) == 2 and f.step(2, 10) == 3
    assert f.step(3, 10) == 3
    # "-", the digits, "-3", the stop id and the never-allowed rest: five classes
    assert f.cls.tolist() == [0, 1, 2, 2, 2, 3, 0, 0, 0, 2, 4, 2]
    _consistent(f)
    # token by token against a walk of the bytes
    bt = _integer_dfa()
    for q in range(3):
        for t, b in enumerate(vocab):
            if t == 10:
                continue
            cur = q
            for ch in b:
                cur = bt[cur, ch] if cur >= 0 else -1
            want = NONE if (cur < 0 or not b) else cur
            assert f.trans[q, f.cls[t]] == want, (q, t)
    g = TokenFsm.from_byte_dfa(vocab, _integer_dfa(), 0, [2])          # no stop id: no further state
    assert g.n_states == 3 and not g.allowed(2)[10]
    with pytest.raises(ValueError, match="256"):
        TokenFsm.from_byte_dfa(vocab, np.zeros((3, 255), dtype=np.int32), 0, [2])
    with pytest.raises(ValueError, match="bytes"):
        TokenFsm.from_byte_dfa(["a"], _integer_dfa(), 0, [2])
    with pytest.raises(ValueError, match="accepting"):
        TokenFsm.from_byte_dfa(vocab, _integer_dfa(), 0, [3])


def test_from_byte_dfa_is_vectorised_over_a_real_sized_vocabulary():
    V = 151936
    rng = np.random.default_rng(0)
    alphabet = np.frombuffer(b"0123456789-ab ", dtype=np.uint8)
    vocab = [bytes(rng.choice(alphabet, size=rng.integers(0, 7))) for _ in range(V)]
    f = TokenFsm.from_byte_dfa(vocab, _integer_dfa(), 0, [2], stop_token_ids=[V - 1])
    assert f.n_classes <= 8                                           # (target from 0, 1, 2) in {2, -2} + "-" first + the stop id
    for t in rng.integers(0, V - 1, size=200).tolist():
        s = vocab[t].decode()
        assert f.allowed(2)[t] == (len(s) > 0 and s.isdigit()), s
        assert f.allowed(0)[t] == (len(s) > 0 and (s.isdigit() or s == "-" or (s[0] == "-" and s[1:].isdigit()))), s


def test_the_gpu_tests_cases_are_well_formed():
    for V in (1, 97, 4099):
        cases = grammar.operator_cases(V)
        assert len({c["name"] for c in cases}) == len(cases)
        for c in cases:
            xg, sg, A = grammar.gather(c["x"], c["seen"], c["allow"])
            assert A.shape[0] >= 1
            ref = sampling.reference(generation.penalise(xg, sg, c["r"]), c["tau"], c["k"], c["p"])
            assert ref.greedy or ref.margin >= sampling.MARGIN, c["name"]
            tok = int(A[sampling.draw(ref, c["seed"], 0)])
            grammar.judge(c, 0, tok, ref.n_kept)                      # the judge accepts the reference's own token
            if (~c["allow"]).any():
                with pytest.raises(AssertionError, match="outside the allowed set"):
                    grammar.judge(c, 0, int(np.nonzero(~c["allow"])[0][0]))
        a, b, where = grammar.grammars_for(cases, V)
        for (g, q), c in zip(where, cases):
            f = (a, b)[g]
            assert (f.allowed(q) == c["allow"]).all()
            t = int(np.nonzero(c["allow"])[0][0])
            assert f.step(q, t) == (0 if t % 2 == 0 else FREE)
        assert not a.allowed(a.n_states - 1).any() and not b.allowed(b.n_states - 1).any()
    ks = {c["k"] for c in grammar.operator_cases(97) if "every7-k" in c["name"]}
    nA = int(grammar.every(97, 7, 3).sum())
    assert ks == {nA - 1, nA, nA + 1, 96}


# ---------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_validates(lib):
    from infinitevl_amd import _lib
    assert _lib.PROTOTYPES["ivl_sample_rows_fwd"] == (ctypes.c_int, [ctypes.POINTER(_lib.SampleArgs), ctypes.c_void_p])
    assert [(n, t) for n, t in _lib.SampleArgs._fields_ if n in sampling.ARG_FIELDS[32:39]] == list(zip(
        ("fsm_state", "fsm_mask", "mask_ld", "n_states", "fsm_desc", "fsm_cls", "fsm_trans"),
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3))
    assert lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12

    one, INV = sampling.ONE, _lib.IVL_ERR_INVALID_ARG
    fsm = {"done": one, "fsm_state": one, "fsm_mask": one, "mask_ld": 2, "n_states": 3, "fsm_desc": one, "fsm_cls": one,
           "fsm_trans": one}

    def refused(word, **kw):
        return sampling.c_refused(lib, INV, word, **{**fsm, **kw})

    for name in ("fsm_mask", "fsm_desc", "fsm_cls", "fsm_trans", "done"):
        assert refused(name.encode(), **{name: None}), name
    assert refused(b"mask_ld", mask_ld=1) and refused(b"mask_ld", mask_ld=0) and refused(b"mask_ld", mask_ld=-1)
    assert refused(b"n_states", n_states=0) and refused(b"n_states", n_states=-4)
    # whatever the scores and the controls refuse
    assert refused(b"n_top", n_top=21, top_ids=one, top_logprobs=one)
    assert refused(b"top_ids", n_top=5)
    assert refused(b"n_new", lp_history=one, hist_ld=4)
    assert refused(b"rep_penalty needs seen", rep_penalty=one)
    assert refused(b"n_stop=", n_stop=17, stop_ids=one) and refused(b"budget", budget=one)
    assert refused(b"history", history=one, hist_ld=4)
    for name in ("logits", "temperature", "top_k", "top_p", "seed", "counter", "token"):          # with the constraint on
        assert refused(b"NULL", **{name: None}), name
    assert sampling.c_refused(lib, _lib.IVL_ERR_UNSUPPORTED, b"2^23", **{**fsm, "V": 1 << 23, "ld": 1 << 24, "mask_ld": 1 << 18})
    # the group off: its own checks do not apply (scalars alone select nothing), the others do
    assert refused(b"n_top", fsm_state=None, done=None, n_top=21, top_ids=one, top_logprobs=one)
    assert refused(b"n_top", fsm_state=None, fsm_mask=None, mask_ld=0, n_states=0, n_top=21, top_ids=one, top_logprobs=one)


# ---------------------------------------------------------------------------------------------
# ops and Sampler
# ---------------------------------------------------------------------------------------------
def _yes_no(V=97):
    return TokenFsm.from_choices(V, [[3, 7], [5]], stop_token_ids=[9])


def test_arena_load_unload_and_full():
    from infinitevl_amd import ops
    V = 97
    f = _yes_no(V)                                                    # 3 states, 5 classes
    tab = ops.FsmTables("cpu", V, states=8, grammars=3, trans=40)
    assert (tab.n_states, tab.mask_ld) == (8, 4) and tab.mask.dtype == torch.int32 and tuple(tab.mask.shape) == (8, 4)
    assert tuple(tab.desc.shape) == (8, 2) and tab.desc.dtype == torch.int64 and tab.cls.numel() == 3 * V and tab.trans.numel() == 40
    ptrs = [t.data_ptr() for t in (tab.mask, tab.desc, tab.cls, tab.trans)]
    a, b = tab.load(f), tab.load(f)
    assert (a.base, a.start, a.n_states) == (0, 0, 3) and (b.base, b.start, b.n_states) == (3, 0, 3)
    # the second copy: targets rebased to global states, FREE and NONE kept; its own class table and transition range
    for h in (a, b):
        for q in range(3):
            toff, coff = tab.desc[h.base + q].tolist()
            row = tab.trans[toff:toff + f.n_classes].numpy()
            assert (row == np.where(f.trans[q] >= 0, f.trans[q] + h.base, f.trans[q])).all()
            assert (tab.cls[coff:coff + V].numpy() == f.cls).all()
            assert (tab.mask[h.base + q].numpy().view(np.uint32)[:f.mask.shape[1]] == f.mask[q]).all()
    assert tab.desc[3, 1].item() != tab.desc[0, 1].item()
    with pytest.raises(ValueError, match="full"):                     # 2 states left
        tab.load(f)
    tab.unload(a)
    assert not tab.mask[:3].any() and tab.mask[3:6].any()             # its states allow nothing now
    with pytest.raises(ValueError, match="not loaded"):
        tab.unload(a)
    c = tab.load(f)
    assert c.base == 0 and tab.local(4) == (b, 1) and tab.local(7) is None
    small = TokenFsm.from_edges(V, 2, [(0, [1], 1), (1, [2], FREE)])
    d = tab.load(small)
    assert d.base == 6 and d.n_states == 2
    with pytest.raises(ValueError, match="full"):                     # no grammar slot left
        tab.load(small)
    tab.unload(d)
    tab2 = ops.FsmTables("cpu", V, states=8, grammars=3, trans=20)
    tab2.load(f)
    with pytest.raises(ValueError, match="full"):                     # 15 of 20 transition entries taken
        tab2.load(f)
    assert [t.data_ptr() for t in (tab.mask, tab.desc, tab.cls, tab.trans)] == ptrs
    with pytest.raises(ValueError, match="vocab"):
        tab.load(_yes_no(98))
    for bad in (dict(states=0), dict(grammars=0), dict(trans=0), dict(vocab_size=0), dict(mask_ld=3), dict(states=True)):
        with pytest.raises(ValueError):
            ops.FsmTables("cpu", **{"vocab_size": V, "states": 8, "grammars": 3, "trans": 40, **bad})
    assert ops.FsmTables("cpu", V, 8, 3, 40, mask_ld=5).mask.shape[1] == 5


def test_ops_check_the_constraint_arguments():
    from infinitevl_amd import ops
    S, V = 2, 40
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    tab = (torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S), torch.zeros(S, dtype=torch.int64),
           torch.zeros(S, dtype=torch.int64))
    done, st = torch.zeros(S, dtype=torch.int32), torch.zeros(S, dtype=torch.int32)
    fsm = ops.FsmTables("cpu", V, 4, 1, 16)
    with pytest.raises(ValueError, match="come together"):
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st)
    with pytest.raises(ValueError, match="come together"):
        ops.sample_tokens(lg, *tab, done=done, fsm=fsm)
    with pytest.raises(ValueError, match="needs done"):
        ops.sample_tokens(lg, *tab, fsm_state=st, fsm=fsm)
    with pytest.raises(ValueError, match="fsm_state"):
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st.long(), fsm=fsm)
    with pytest.raises(ValueError, match="words per state"):
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st, fsm=ops.FsmTables("cpu", 32, 4, 1, 16))
    holder = types.SimpleNamespace(mask=fsm.mask, desc=fsm.desc, cls=fsm.cls.long(), trans=fsm.trans, mask_ld=2, n_states=4)
    with pytest.raises(ValueError, match="fsm.cls"):
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st, fsm=holder)
    holder = types.SimpleNamespace(mask=fsm.mask, desc=fsm.desc, cls=fsm.cls, trans=fsm.trans, mask_ld=2, n_states=5)
    with pytest.raises(ValueError, match="n_states"):
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st, fsm=holder)
    with pytest.raises(RuntimeError, match="MI355X"):                 # everything checks out: only the device is missing
        ops.sample_tokens(lg, *tab, done=done, fsm_state=st, fsm=fsm)


def test_sampler_grammar_tensors_and_state():
    from infinitevl_amd.harness import Sampler
    assert len(Sampler(4, "cpu").row_tensors()) == 11
    smp = Sampler(4, "cpu", vocab_size=97, history=4, logprobs=2, grammar_states=8)
    assert len(smp.row_tensors()) == 21 and smp.controlled
    assert smp.fsm_state.dtype == torch.int32 and smp.fsm_state.tolist() == [-1] * 4 and "fsm_state" in smp.state()
    assert smp.grammars.n_states == 8 and len(smp.grammars._slots) == 4 and smp.grammars.trans.numel() == 8 * 256
    plain = Sampler(4, "cpu", vocab_size=97, history=4, logprobs=2)
    assert plain.fsm_state is None and plain.grammars is None and len(plain.row_tensors()) == 20
    assert "fsm_state" not in plain.state()
    for who in (plain.load_grammar, plain.unload_grammar, lambda h: plain.set_grammar(0, h), lambda h: plain.grammar_state(0)):
        with pytest.raises(ValueError, match="grammar_states"):
            who(None)
    a, b = smp.load_grammar(_yes_no()), smp.load_grammar(_yes_no())
    smp.set_grammar(1, a)
    smp.set_grammar(2, b, state=1)
    assert smp.fsm_state.tolist() == [-1, 0, 4, -1]
    assert [smp.grammar_state(r) for r in range(4)] == [None, 0, 1, None]
    st = smp.state()
    smp.set(2, temperature=0.7)                                       # set() clears the row to unconstrained
    assert smp.fsm_state.tolist() == [-1, 0, -1, -1] and smp.grammar_state(2) is None
    smp.load_state(st)
    assert smp.fsm_state.tolist() == [-1, 0, 4, -1]
    smp.set_grammar(1, None)
    assert smp.grammar_state(1) is None
    for bad in (dict(state=3), dict(state=-1), dict(state=True)):
        with pytest.raises(ValueError, match="state"):
            smp.set_grammar(0, a, **bad)
    with pytest.raises(ValueError, match="a state needs a grammar"):
        smp.set_grammar(0, None, state=0)
    smp.unload_grammar(a)
    with pytest.raises(ValueError, match="not loaded"):
        smp.set_grammar(0, a)
    with pytest.raises(ValueError, match="full"):                     # 8 states: two more copies do not fit beside b
        smp.load_grammar(_yes_no())
        smp.load_grammar(_yes_no())
    for bad in (dict(grammar_states=8), dict(vocab_size=97, grammar_states=-1), dict(vocab_size=97, grammar_slots=2),
                dict(vocab_size=97, grammar_trans=2), dict(vocab_size=97, grammar_states=True)):
        with pytest.raises(ValueError, match="grammar"):
            Sampler(4, "cpu", **bad)
    assert Sampler(2, "cpu", vocab_size=97, grammar_states=8, grammar_slots=3, grammar_trans=50).grammars.trans.numel() == 50


def test_graphed_classes_refuse_on_the_host():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode, GraphedMultiStreamDecode, Sampler
    stack, hc = fk.small_stack("cpu")
    cache = MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16)
    K = 4
    with pytest.raises(ValueError, match="constrained beam search"):
        GraphedBeamDecode(stack, cache, 2, hc.vocab_size, 16, sampler=Sampler(4, "cpu", vocab_size=hc.vocab_size, max_stop=0,
                                                                            history=16, logprobs=K, score_rings=False,
                                                                            grammar_states=8))
    with pytest.raises(ValueError, match="the sampler must be"):
        GraphedBeamDecode(stack, cache, 2, hc.vocab_size, 16, sampler=Sampler(4, "cpu", vocab_size=hc.vocab_size, history=16))
    own = Sampler(4, "cpu", vocab_size=hc.vocab_size, max_stop=0, history=16, logprobs=K, score_rings=False)
    assert GraphedBeamDecode(stack, cache, 2, hc.vocab_size, 16, sampler=own).sampler is own
    x = fk.prompt(hc, 5, 1, "cpu")[0]
    smp = Sampler(4, "cpu", vocab_size=hc.vocab_size, grammar_states=8)
    h = smp.load_grammar(_yes_no(hc.vocab_size))
    dec = GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16),
                                   sampler=Sampler(4, "cpu", vocab_size=hc.vocab_size))
    for call in (lambda: dec.admit(0, x, grammar=h), lambda: dec.admit_n([0, 1], x, grammar=h),
                 lambda: dec.load([0], None, grammar=h)):
        with pytest.raises(ValueError, match="grammar_states"):
            call()
    dec = GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16), sampler=smp)
    smp.unload_grammar(h)
    with pytest.raises(ValueError, match="not loaded"):
        dec.admit(0, x, grammar=h)

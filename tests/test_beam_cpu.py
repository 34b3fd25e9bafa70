"""CPU (-m "not gpu"): the host side of beam search -- the plain-Python reference of tests/beam.py against brute force and on
unit cases of every rule; the four new entry points in the header, the binding and the library, with their argument errors
(returned before any launch, on pointers that are never dereferenced); what ops.RowGatherPlan, ops.beam_width and
GraphedBeamDecode.admit refuse before any device work; and the share of synthetic cases the GPU test may call contested."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

import beam
import fork as fk
import sampling
from conftest import ROOT

NEW = ("ivl_rows_gather_fwd", "ivl_beam_select_fwd", "ivl_beam_commit_fwd")      # (the score-only form: ivl_sample_rows_fwd)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_equals_brute_force_when_the_beam_holds_every_prefix(seed):
    """V = 6, length 4, length_penalty 0, no stop id, B = V^3: no prefix is ever dropped, so the B hypotheses filed at the
    budget are the B best of all V^4 sequences, with the same float64 sums (both add left to right)."""
    V, n = 6, 4
    table = beam.markov_table(V, seed)
    g = beam.markov_beam(table, V, n, V ** 3)
    brute = beam.markov_brute(table, V, n)
    got = g.result(V ** 3)
    assert g.done == 2 and len(got) == V ** 3
    assert [(t, s) for t, _, s in got] == brute[:V ** 3]
    assert got[0][1] == got[0][2] == brute[0][1]
    narrow = beam.markov_beam(table, V, n, 2).result(1)[0]          # a narrow beam never beats the optimum
    assert narrow[2] <= brute[0][1]


def _group(B=2, **kw):
    g = beam.BeamGroup(B, **kw)
    g.cum = [0.0] * B
    g.n_new = [2] * B
    g.history = [[10 + b, 20 + b] for b in range(B)]
    return g


def test_stop_id_beyond_rank_B_is_skipped_and_inside_becomes_a_hypothesis():
    g = _group(2, stop_ids=[7], length_penalty=1.0)
    # ranked: (b0,5,-0.1) (b1,6,-0.2) | (b0,7,-0.3): the stop id at walk position 2 >= B is skipped
    assert g.select([[5, 7, 1, 2], [6, 3, 4, 8]], [[-0.1, -0.3, -2.0, -3.0], [-0.2, -1.0, -4.0, -5.0]])
    assert g.hyps == [] and g.parent == [0, 1] and g.next_token == [5, 6] and g.next_score == [-0.1, -0.2]
    g = _group(2, stop_ids=[7], length_penalty=1.0)
    assert g.select([[7, 5, 1, 2], [6, 3, 4, 8]], [[-0.1, -0.3, -2.0, -3.0], [-0.2, -1.0, -4.0, -5.0]])
    assert g.hyps == [{"tokens": [10, 20, 7], "score": -0.1 / 3.0, "sum": -0.1}]
    assert g.parent == [1, 0] and g.next_token == [6, 5] and g.done == 0


def test_worst_hypothesis_is_evicted_and_ties_keep_the_earlier():
    g = beam.BeamGroup(2, length_penalty=0.0)
    g.insert([1], -3.0, 1)
    g.insert([2], -1.0, 1)
    g.insert([3], -2.0, 1)                     # evicts -3
    assert [h["tokens"] for h in g.hyps] == [[2], [3]]
    g.insert([4], -2.0, 1)                     # not better than the worst: refused
    assert [h["tokens"] for h in g.hyps] == [[2], [3]]
    g.insert([5], -1.0, 1)
    assert [h["tokens"] for h in g.hyps] == [[2], [5]]
    assert [r[0] for r in g.result(2)] == [[2], [5]]      # equal scores: the earlier insertion first


@pytest.mark.parametrize("early", [True, False])
def test_done_rule_with_and_without_early_stopping(early):
    g = _group(2, stop_ids=[7, 8], length_penalty=1.0, early_stopping=early)
    ids = [[7, 8, 1, 2, 3, 4], [5, 6, 9, 11, 12, 13]]
    lps = [[-0.1, -0.2, -0.3, -3.0, -4.0, -5.0], [-1.0, -1.1, -1.2, -1.3, -1.4, -1.5]]
    assert g.select(ids, lps)
    assert len(g.hyps) == 2                    # two hypotheses of length 3: scores -0.1/3 and -0.2/3
    # best candidate -0.1 at length 3 -> -0.0333 ; worst hypothesis -0.0667 < it: not done by the heuristic
    assert g.done == (1 if early else 0)
    if early:
        assert g.parent == [0, 1]
    else:
        assert g.parent == [0, 1] and g.next_token == [1, 5]
    # and the heuristic fires when the worst hypothesis is at least as good as anything still attainable
    h = _group(2, length_penalty=1.0)
    h.hyps = [{"tokens": [1], "score": -0.01, "sum": -0.01}, {"tokens": [2], "score": -0.02, "sum": -0.02}]
    assert h.select([[1, 2, 3, 4], [5, 6, 8, 9]], [[-0.3, -0.4, -1.0, -2.0]] * 2) and h.done == 1 and h.parent == [0, 1]


@pytest.mark.parametrize("lp, want", [(0.0, -2.0), (1.0, -2.0 / 3.0), (2.0, -2.0 / 9.0)])
def test_budget_files_every_beam_and_length_penalty_scores_it(lp, want):
    g = _group(2, length_penalty=lp, budget=3)
    g.cum = [-1.0, -1.5]
    g.step([[1, 2, 3, 4], [5, 6, 7, 8]], [[-1.0, -2.0, -3.0, -4.0], [-1.0, -2.0, -3.0, -4.0]])
    assert g.done == 2 and g.n_new == [3, 3] and g.parent == [0, 1]
    assert [h["tokens"] for h in g.hyps] == [[10, 20, 1], [11, 21, 5]]
    assert g.hyps[0]["sum"] == -2.0 and g.hyps[0]["score"] == want and g.hyps[1]["score"] == beam.hyp_score(-2.5, 3, lp)
    assert beam.hyp_score(-2.0, 3, 0.5) == -2.0 / math.pow(3.0, 0.5)
    g.step([[1]], [[0.0]])                     # a finished group stays as it is
    assert g.n_new == [3, 3] and len(g.hyps) == 2


def test_score_ties_go_to_the_lower_beam_then_the_lower_rank():
    g = _group(3, length_penalty=1.0)
    g.cum = [-0.5, -0.25, -0.25]
    ids = [[1, 2, 3, 4, 5, 6], [11, 12, 13, 14, 15, 16], [21, 22, 23, 24, 25, 26]]
    lps = [[-0.25, -0.5, -9.0, -9.0, -9.0, -9.0], [-0.5, -0.5, -9.0, -9.0, -9.0, -9.0], [-0.5, -9.0, -9.0, -9.0, -9.0, -9.0]]
    g.select(ids, lps)                         # five candidates at -0.75: (0,0) (1,0) (1,1) (2,0) and, lower, (0,1) at -1.0
    assert g.next_score == [-0.75] * 3 and g.parent == [0, 1, 1] and g.next_token == [1, 11, 12]


def test_a_beam_without_a_finite_sum_offers_nothing():
    g = beam.BeamGroup(3)                      # an admission: sums [0, -inf, -inf]
    g.step([[4, 5, 6, 7, 8, 9]] * 3, [[-0.1, -0.2, -0.3, -0.4, -0.5, -0.6]] * 3)
    assert g.parent == [0, 0, 0] and g.token == [4, 5, 6] and g.cum == [-0.1, -0.2, -0.3] and g.history == [[4], [5], [6]]


def test_the_synthetic_cases_stay_under_the_contested_cap_and_cover_the_rules():
    """The GPU test may set a case aside when two hypothesis scores that went through pow() are within 2^-40 of each other:
    at most 2 % of the cases, counted here on the reference alone."""
    total = contested = 0
    seen = dict(done1=0, done2=0, hyp=0, ninf=0, skipped=0, pow=0, tie=0)
    for B, n_stop, cases in beam.all_cases():
        assert beam.HIST >= 2 and max(2, 1 + n_stop) * B <= 20
        for c in cases:
            g = beam.reference_group(c)
            n0, was_done = len(g.hyps), g.done
            g.step(c["ids"], c["lps"])
            total += 1
            contested += g.contested
            seen["done1"] += g.done == 1 and not was_done
            seen["done2"] += g.done == 2
            seen["hyp"] += len(g.hyps) != n0
            seen["ninf"] += any(math.isinf(v) for v in c["cum"])
            seen["skipped"] += bool(was_done)
            seen["pow"] += c["lp"] not in (0.0, 1.0)
            seen["tie"] += len(set(g.next_score)) < len(g.next_score)
    assert total >= 200 and contested <= 0.02 * total, (total, contested)
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------------------------------------
# header, binding, library
# ---------------------------------------------------------------------------------------------
def test_header_yields_the_prototypes_and_the_abi_version(lib):
    from infinitevl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    structs = {}
    consts, _, protos = _lib.parse_header(hdr, structs)
    assert consts["IVL_ABI_VERSION"] == 12 and lib.ivl_abi_version() == 12
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert protos["ivl_rows_gather_fwd"] == (i, [vp, i, i64, i, i, vp, vp])
    assert protos["ivl_sample_rows_fwd"] == (i, [ctypes.POINTER(structs["ivl_sample_args"]), vp])
    assert structs["ivl_sample_args"]._fields_[-1] == ("score_only", i)
    assert protos["ivl_beam_select_fwd"] == (i, [i, i, i, i64, vp, vp, vp, vp, vp, i64, vp, i, vp, vp] + [vp] * 9 + [vp])
    assert protos["ivl_beam_commit_fwd"] == (i, [i, i, i64, vp, vp, vp, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp] + [vp] * 7 + [vp])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert f"IVL_API int {name}(" in hdr and name in _lib.EXPORTED_SYMBOLS and name in exported, name


def _expect(lib, rc, code, fn, word, what):
    assert rc == code, (what, rc)
    err = lib.ivl_last_error()
    assert fn in err and word in err, (what, err)


def test_gather_entry_point_refuses_bad_arguments(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    one = ctypes.c_void_p(0x1000)
    good = dict(table=one, n_entries=3, max_row_bytes=4096, row0=0, n_rows=4, parent=one)
    for kw, code, word in (({"table": None}, INV, b"NULL"), ({"parent": None}, INV, b"NULL"), ({"n_entries": 0}, INV, b"n_entries"),
                           ({"max_row_bytes": 0}, INV, b"max_row_bytes"), ({"row0": -1}, INV, b"row0"),
                           ({"n_rows": 0}, INV, b"n_rows"), ({"n_rows": 9}, INV, b"n_rows"),
                           ({"row0": 60, "n_rows": 4}, UNS, b"63")):
        a = dict(good, **kw)
        rc = lib.ivl_rows_gather_fwd(a["table"], a["n_entries"], a["max_row_bytes"], a["row0"], a["n_rows"], a["parent"], None)
        _expect(lib, rc, code, b"ivl_rows_gather_fwd", word, kw)


def test_score_entry_point_refuses_bad_arguments(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    one = sampling.ONE
    sampled = dict.fromkeys(("temperature", "top_k", "top_p", "seed", "counter", "token"))             # NULL in this form
    good = dict(sampled, token_stride=0, score_only=1, ld=1000, S=2, V=1000, rep_penalty=one, seen=one, seen_ld=32, done=one,
                n_top=8, top_ids=one, top_logprobs=one)
    for kw, code, word in (({"logits": None}, INV, b"NULL"), ({"top_ids": None}, INV, b"NULL"),
                           ({"top_logprobs": None}, INV, b"NULL"),
                           ({"S": 0}, INV, b"S=0"), ({"V": 0}, INV, b"V=0"), ({"ld": 999}, INV, b"ld=999"),
                           ({"seen": None}, INV, b"rep_penalty needs seen"), ({"seen_ld": 31}, INV, b"seen_ld"),
                           ({"n_top": 0}, INV, b"n_top"), ({"n_top": 21}, INV, b"n_top"),
                           ({"V": 1 << 23, "ld": 1 << 23, "seen_ld": 1 << 18}, UNS, b"2^23")):
        assert sampling.c_refused(lib, code, word, **dict(good, **kw)), kw
    # a field outside the form's list that is set is refused, not ignored: pointers and scalars alike
    own = ("logits", "ld", "S", "V", "rep_penalty", "seen", "seen_ld", "done", "n_top", "top_ids", "top_logprobs", "score_only")
    foreign = [n for n in sampling.ARG_FIELDS if n not in own]
    assert len(foreign) == 28
    for name in foreign:
        assert sampling.c_refused(lib, INV, b"score_only", **dict(good, **{name: one})), name
    assert sampling.c_refused(lib, INV, b"NULL", **dict(good, score_only=0))                # the sampling forms' required pointers


def test_beam_entry_points_refuse_bad_arguments(lib):
    from infinitevl_amd import _lib
    INV = _lib.IVL_ERR_INVALID_ARG
    one = ctypes.c_void_p(0x1000)
    tables = [one] * 6                         # beam_done, n_hyp, hyp_score, hyp_sum, hyp_len, hyp_tokens

    def select(G=2, B=2, K=4, mask=3, ptrs=None, hist_ld=16, stop=one, n_stop=1, tab=None, out=None):
        p = ptrs or [one] * 5
        return lib.ivl_beam_select_fwd(G, B, K, mask, p[0], p[1], p[2], p[3], p[4], hist_ld, stop, n_stop, one, one,
                                       *(tab or tables), *(out or [one] * 3), None)

    def commit(G=2, B=2, mask=3, ptrs=None, stride=1, seen=one, seen_ld=32, V=1000, hist_ld=16, tab=None, par=one):
        p = ptrs or [one] * 8                  # next_token, next_score, token, history, n_new, cum, budget, length_penalty
        return lib.ivl_beam_commit_fwd(G, B, mask, p[0], p[1], p[2], stride, seen, seen_ld, V, p[3], hist_ld, p[4], p[5], p[6], p[7],
                                       *(tab or tables), par, None)

    fn = b"ivl_beam_select_fwd"
    for kw, word in ((dict(G=0), b"G=0"), (dict(G=64), b"G=64"), (dict(B=0), b"B=0"), (dict(B=9), b"B=9"), (dict(K=0), b"K=0"),
                     (dict(K=21), b"K=21"), (dict(hist_ld=0), b"hist_ld"), (dict(n_stop=17), b"n_stop"),
                     (dict(stop=None), b"stop_ids"), (dict(ptrs=[one, None, one, one, one]), b"NULL"),
                     (dict(tab=[one, one, None, one, one, one]), b"NULL"), (dict(out=[None, one, one]), b"NULL")):
        _expect(lib, select(**kw), INV, fn, word, kw)
    fn = b"ivl_beam_commit_fwd"
    for kw, word in ((dict(G=0), b"G=0"), (dict(B=9), b"B=9"), (dict(hist_ld=0), b"hist_ld"), (dict(stride=0), b"token_stride"),
                     (dict(seen_ld=31), b"seen_ld"), (dict(ptrs=[one] * 4 + [None] + [one] * 3), b"NULL"),
                     (dict(tab=[None] + [one] * 5), b"NULL"), (dict(par=None), b"NULL")):
        _expect(lib, commit(**kw), INV, fn, word, kw)
    assert select(mask=0) == _lib.IVL_OK and commit(mask=0) == _lib.IVL_OK       # no group: nothing launched


# ---------------------------------------------------------------------------------------------
# host-side refusals
# ---------------------------------------------------------------------------------------------
def test_row_gather_plan_refuses_before_any_device_work():
    from infinitevl_amd import ops
    t = torch.zeros(6, 8)
    plan = ops.RowGatherPlan([t, torch.zeros(7, 3, dtype=torch.int64)])
    assert plan.n_rows == 6 and plan.plan.n_entries == 2
    par = torch.zeros(4, dtype=torch.int32)
    for args, word in (((0, 0, par), "n_rows"), ((0, 9, par), "n_rows"), ((-1, 4, par), "outside"), ((3, 4, par), "outside"),
                       ((0, 4, par.to(torch.int64)), "int32"), ((0, 3, par), "int32"), ((0, 4, [0, 0, 0, 0]), "int32"),
                       ((True, 4, par), "row0"), ((0, 4.0, par), "n_rows")):
        with pytest.raises(ValueError, match=word):
            plan.run(*args)
    with pytest.raises(ValueError, match="CPU"):
        plan.run(0, 4, par)
    for bad, word in (([], "non-empty"), ([t, 3], "non-empty"), ([torch.zeros(4, 4).t()], "contiguous"),
                      ([torch.zeros(64, 2)], "at most 63")):
        with pytest.raises(ValueError, match=word):
            ops.RowGatherPlan(bad)


def test_beam_width_refuses_more_than_twenty_candidates():
    from infinitevl_amd import ops
    assert ops.beam_width(1, 0) == 2 and ops.beam_width(4, 1) == 8 and ops.beam_width(4, 4) == 20 and ops.beam_width(8, 0) == 16
    for B, n in ((4, 5), (8, 2), (7, 2)):
        with pytest.raises(ValueError, match="exceed the 20"):
            ops.beam_width(B, n)
    for B in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="num_beams"):
            ops.beam_width(B, 0)


def test_graphed_beam_decode_refuses_on_the_host():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode
    stack, hc = fk.small_stack("cpu")
    cache = MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="no multiple"):
        GraphedBeamDecode(stack, cache, 3, hc.vocab_size, 16)
    with pytest.raises(ValueError, match="exceed the 20"):
        GraphedBeamDecode(stack, cache, 4, hc.vocab_size, 16, max_stop=5)
    dec = GraphedBeamDecode(stack, cache, 2, hc.vocab_size, 16, max_stop=1)
    assert (dec.G, dec.B, dec.K) == (2, 2, 4) and dec.beam["beam_done"].tolist() == [1, 1]
    x = fk.prompt(hc, 5, 1, "cpu")[0]
    for kw, word in ((dict(group=2, max_new_tokens=4), "group"), (dict(group=-1, max_new_tokens=4), "group"),
                     (dict(group=True, max_new_tokens=4), "group"), (dict(group=0, max_new_tokens=17), "history"),
                     (dict(group=0, max_new_tokens=0), "max_new_tokens"),
                     (dict(group=0, max_new_tokens=4, stop_token_ids=[1, 2]), "candidates per beam"),
                     (dict(group=0, max_new_tokens=4, stop_token_ids=[-1]), "stop_token_ids"),
                     (dict(group=0, max_new_tokens=4, early_stopping="never"), "early_stopping"),
                     (dict(group=0, max_new_tokens=4, length_penalty=math.inf), "length_penalty"),
                     (dict(group=0, max_new_tokens=4, repetition_penalty=0.0), "repetition_penalty")):
        with pytest.raises(ValueError, match=word):
            dec.admit(kw.pop("group"), x, **kw)
    with pytest.raises(TypeError):
        dec.admit(0, x)                        # max_new_tokens is required
    for call in (lambda: dec.fork(0, [1]), lambda: dec.extend(0, x), lambda: dec.admit_n([0, 1], x), lambda: dec.load([0], cache)):
        with pytest.raises(ValueError, match="not a stream of its own"):
            call()
    with pytest.raises(ValueError, match="group"):
        dec.result(5)
    with pytest.raises(ValueError, match="group"):
        dec.release(2)
    assert dec.beam["beam_done"].tolist() == [1, 1] and cache.slot_lengths == [0, 0, 0, 0]      # nothing was started

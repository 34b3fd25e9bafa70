"""CPU: the preconditions that make tests/test_gpu_lattice.py a test of the kernels and not of its inputs (tests/lattice.py).

For EVERY case the GPU file builds (lattice.gpu_case_list(); none skipped or filtered -- a case that fails here is a bug of the
generator, mended by changing its parameters):
  * the float64 expectation is representable: o survives bf16 (and fp16), the state survives bf16, at every scale probed;
  * the oracle's rounding models are exact on it: oracle.gdn.gdn_chunk with rounding=bf16, with mma_rounding=e4m3 on the kinds
    the fp8 kernel gets, and the fp32 token-by-token oracle.gdn.gdn_recurrent;
  * on "onehot_q" the oracle gives the same with the l2norm on (rounded to bf16 / fp16) as with it off;
  * the case is not degenerate (lattice.lattice_required).
And the report: lattice_mismatches catches an expectation computed with the wrong flag, the wrong scale and a one-token shift,
naming token and column.
"""
import pytest
import torch

import lattice as lat
from oracle import gdn as ogdn

BF, F16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
CASES = lat.gpu_case_list()
FP8_KINDS = ("memory", "still", "onehot_q")


def _id(c):
    return "-".join(str(x) for x in c)


_CACHE = {}


def _case(c):
    if c not in _CACHE:                                 # computed once, shared by the tests below, never written to
        case = lat.make(*c)
        _CACHE[c] = (case, lat.lattice_expected(case, 1.0))
    return _CACHE[c]


def _oracle_args(case):
    return tuple(case[n] for n in ("q", "k", "v", "g", "beta"))


def _assert_equal(exp, got, what):
    bad = lat.lattice_mismatches(exp[0], exp[1], got[0], got[1])
    assert not bad, (what, bad)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_expectation_is_representable_and_within_its_bound(c):
    case, (o, S) = _case(c)
    assert case["bound"] == (lat.BOUND_BF16 if c[0] == "half" else lat.BOUND_E4M3)
    for name in ("q", "k", "v", "beta"):
        x = case[name]
        assert torch.equal(x.to(BF).float(), x) and torch.equal(x.to(F16).float(), x), name
        if c[0] in FP8_KINDS:
            assert float(x.abs().max()) <= lat.BOUND_E4M3 and torch.equal(x.to(E4M3).float(), x), name
    assert set(case["g"].unique().tolist()) <= {0.0, lat.WIPE}
    for scale in lat.SCALES:
        os_ = o * scale
        assert torch.equal(os_.to(BF).double(), os_) and torch.equal(os_.to(F16).double(), os_), scale
    assert torch.equal(S.to(BF).double(), S) and torch.equal(S.float().double(), S)
    if case["h0"] is not None:
        assert torch.equal(case["h0"].to(BF).float(), case["h0"])
    if c[0] in FP8_KINDS:
        assert float(o.abs().max()) <= lat.BOUND_E4M3 and float(S.abs().max()) <= lat.BOUND_E4M3


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_oracle_rounding_models_are_exact_on_the_lattice(c):
    case, exp = _case(c)
    args = _oracle_args(case)
    for scale in ((1.0,) if c[2] > 1000 else (1.0, 0.125)):
        e = (exp[0] * scale, exp[1])
        kw = dict(scale=scale, initial_state=case["h0"], use_qk_l2norm_in_kernel=False)
        _assert_equal(e, ogdn.gdn_chunk(*args, rounding=BF, **kw), ("chunk bf16", scale))
        if c[0] in FP8_KINDS:
            _assert_equal(e, ogdn.gdn_chunk(*args, rounding=BF, mma_rounding=E4M3, **kw), ("chunk e4m3", scale))
        _assert_equal(e, ogdn.gdn_recurrent(*args, qk_round_dtype=BF, **kw), ("recurrent", scale))


@pytest.mark.parametrize("c", [c for c in CASES if c[0] == "onehot_q"], ids=_id)
def test_l2norm_is_a_no_op_on_unit_rows_in_the_oracle(c):
    case, exp = _case(c)
    args = _oracle_args(case)
    kw = dict(scale=0.5, initial_state=case["h0"], use_qk_l2norm_in_kernel=True)
    e = (exp[0] * 0.5, exp[1])
    _assert_equal(e, ogdn.gdn_chunk(*args, rounding=BF, **kw), "chunk bf16, l2norm on")
    _assert_equal(e, ogdn.gdn_chunk(*args, rounding=BF, mma_rounding=E4M3, **kw), "chunk e4m3, l2norm on")
    for dt in (BF, F16):
        _assert_equal(e, ogdn.gdn_recurrent(*args, qk_round_dtype=dt, **kw), ("recurrent, l2norm on", dt))


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_case_is_not_degenerate(c):
    case, exp = _case(c)
    f = lat.lattice_features(case, exp)
    missing = [n for n in lat.lattice_required(c[0], c[2]) if not f[n]]
    assert not missing, (missing, f)
    if c[0] == "still":
        assert torch.equal(exp[1], case["h0"].double())
        B, T, H = case["g"].shape
        if B * T * H >= 2 * lat.GDN_K:
            assert bool((case["q"] != 0).any(dim=(0, 1, 2)).all()), "every state row is read"
    elif case["g"].numel() >= 64:                       # (a call of 6 or 12 tokens cannot be asked to reach four blocks)
        ks = case["k"].abs().sum(dim=(0, 1, 2))
        assert all(bool((ks[32 * j:32 * j + 32] > 0).any()) for j in range(4)), "keys in all four 32-wide contraction blocks"


@pytest.mark.parametrize("T", [70, 129])
def test_cases_without_an_initial_state_are_exact_in_the_oracle_too(T):
    """the GPU file's h0=None forms: the same inputs from a zero state"""
    case = dict(lat.make("memory", 2, T, 3), h0=None)
    exp = lat.lattice_expected(case, 0.5)
    assert bool((exp[0] != 0).any()) and bool((exp[1] != 0).any())
    kw = dict(scale=0.5, initial_state=None, use_qk_l2norm_in_kernel=False)
    _assert_equal(exp, ogdn.gdn_chunk(*_oracle_args(case), rounding=BF, **kw), "chunk bf16")
    _assert_equal(exp, ogdn.gdn_chunk(*_oracle_args(case), rounding=BF, mma_rounding=E4M3, **kw), "chunk e4m3")
    _assert_equal(exp, ogdn.gdn_recurrent(*_oracle_args(case), **kw), "recurrent")


def test_long_case_carries_a_state_across_the_workspace_segment():
    """T = 4161: the state after token 4095 (what the chunk kernel carries from its first 64-chunk segment into the second) is
    not zero, differs from h0, and the 65 tokens behind it read it."""
    case = lat.make("memory", 1, lat.LONG_T, 1)
    cut = 64 * lat.CHUNK
    head = {n: (x[:, :cut] if n in ("q", "k", "v", "g", "beta") else x) for n, x in case.items()}
    _, s_mid = lat.lattice_expected(head)
    assert int((s_mid != 0).any(-1).sum()) >= 8 and not torch.equal(s_mid, case["h0"].double())
    tail = {n: (x[:, cut:] if n in ("q", "k", "v", "g", "beta") else x) for n, x in case.items()}
    o_with, _ = lat.lattice_expected(dict(tail, h0=s_mid.float()))
    o_without, _ = lat.lattice_expected(dict(tail, h0=None))
    assert int((o_with != o_without).any(-1).sum()) >= 8


def test_varlen_and_split_cases_are_cut_where_the_tests_say():
    flat = lat.varlen_case()
    seqs = lat.varlen_sequences(flat, lat.VARLEN_LENGTHS)
    assert [None if s is None else s["q"].shape[1] for s in seqs] == [70, 1, None, 64, 65]
    assert torch.equal(torch.cat([s["v"] for s in seqs if s is not None], 1), flat["v"])
    for s in seqs:
        if s is not None:
            o, S = lat.lattice_expected(s)
            assert bool((o != 0).any()) and not torch.equal(S, s["h0"].double())
    T, cut = lat.SPLIT
    assert cut % lat.CHUNK != 0 and (T - cut) % lat.CHUNK != 0 and T - cut > lat.CHUNK


def test_default_scale_leaves_the_lattice_and_rounds_once():
    case = lat.make("memory", 2, 65, 3)
    o, _ = lat.lattice_expected(case)
    e = lat.default_scale_expected(o)
    exact = o * (lat.GDN_K ** -0.5)
    assert not torch.equal(e.double(), exact), "128^-0.5 is no power of two: the scaled output is not representable"
    assert float(((e.double() - exact).abs() / exact.abs().clamp(min=1e-30)).max()) <= 2.0 ** -8     # half an ulp of bf16
    # the oracle's chunk model with the default scale, rounded to bf16, is this value
    got, _ = ogdn.gdn_chunk(*_oracle_args(case), initial_state=case["h0"], use_qk_l2norm_in_kernel=False, rounding=BF)
    assert torch.equal(got.to(BF), e)


# ---- the report catches what the GPU tests are for (the mutation check, on the CPU) -------------------------------------------
def _mutants():
    case = lat.make("memory", 2, 129, 3)
    exp = lat.lattice_expected(case, 0.5)
    args = _oracle_args(case)
    wrong_flag = ogdn.gdn_chunk(*args, scale=0.5, initial_state=case["h0"], use_qk_l2norm_in_kernel=True, rounding=BF)
    wrong_scale = ogdn.gdn_chunk(*args, scale=1.0, initial_state=case["h0"], use_qk_l2norm_in_kernel=False, rounding=BF)
    shifted = (torch.roll(exp[0], 1, dims=1), exp[1])
    one = exp[0].clone()
    one[1, 128, 2, 255] += 0.5                                           # one element of the ragged last chunk's only token
    state_one = exp[1].clone()
    state_one[1, 2, 127, 0] += 1.0
    return exp, {"l2norm on": wrong_flag, "scale 1.0 for 0.5": wrong_scale, "shift by one token": shifted,
                 "one element of o": (one, exp[1]), "one element of the state": (exp[0], state_one)}


def test_mismatch_report_names_token_and_column_for_each_wrong_expectation():
    exp, mutants = _mutants()
    assert lat.lattice_mismatches(exp[0], exp[1], exp[0].to(BF), exp[1].float()) == []
    for name, (o, s) in mutants.items():
        bad = lat.lattice_mismatches(exp[0], exp[1], o, s, limit=3)
        assert bad, name
        first = bad[0]
        assert ("token" in first and "chunk" in first and "row" in first and "column" in first) or "k row" in first, (name, first)
    bad = lat.lattice_mismatches(exp[0], exp[1], *mutants["one element of o"])
    assert bad[0].startswith("o[batch 1, token 128 (chunk 2, row 0), head 2, column 255]") and "1 of" in bad[1], bad
    bad = lat.lattice_mismatches(exp[0], exp[1], *mutants["one element of the state"])
    assert bad[0].startswith("state[batch 1, head 2, k row 127, v column 0]"), bad
    nan = exp[0].clone()
    nan[0, 5, 1, 7] = float("nan")
    assert lat.lattice_mismatches(exp[0], exp[1], nan, exp[1])[0].startswith("o[batch 0, token 5 (chunk 0, row 5), head 1, column 7]")

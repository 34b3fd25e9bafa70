"""CPU (-m "not gpu"): the sampling reference and its builders (tests/sampling.py) stand on their own -- the random stream's
check vectors, agreement with a sort-based HF-order implementation on tie-free rows, the top-p margin of every builder case --
and the host side of the feature: Sampler.set validation, ops.sample_tokens argument checks, the C entry point's error codes
and its presence in the library's dynamic symbol table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import sampling
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_u64_check_vectors():
    for (seed, ctr), want in sampling.U64_VECTORS:
        assert sampling.u64(seed, ctr) == want, (seed, ctr, hex(sampling.u64(seed, ctr)))
        assert int(sampling.u64_array(seed, [ctr])[0]) == want, (seed, ctr)
    ctrs = np.arange(300)
    for seed in (0, -1, 7, -(2 ** 63), 2 ** 63 - 1):
        assert [int(v) for v in sampling.u64_array(seed, ctrs)] == [sampling.u64(seed, int(c)) for c in ctrs]


@pytest.mark.parametrize("V", [97, 512, 4099])
def test_reference_matches_sorted_hf_order_on_tie_free_rows(V):
    # distinct bf16 values: a shuffled arithmetic ladder (steps of 1/16 are exact in bf16 up to 16)
    assert V <= 2 * 16 * 16 * 8 + 4
    g = torch.Generator().manual_seed(V)
    ladder = (torch.arange(V, dtype=torch.float32) - V // 2)
    x = (ladder * (2.0 ** -4 if V <= 512 else 2.0 ** -9))[torch.randperm(V, generator=g)].to(torch.bfloat16)
    # (V = 4099 at 2^-9: |x| < 4.01 needs 9 fractional bits below 4 -- bf16 has 8 significant bits, so the ladder is thinned)
    if V > 512:
        x = torch.unique(x)[torch.randperm(torch.unique(x).numel(), generator=g)]
    assert torch.unique(x).numel() == x.numel() > 90
    n = 0
    for tau in sampling.TAUS:
        for k in (0, 1, 7, 50, x.numel()):
            for p in sampling.PS + (0.3,):
                ref = sampling.reference(x, tau, k, p)
                if ref.margin < sampling.MARGIN:
                    continue
                n += 1
                assert np.array_equal(ref.P, sampling.hf_kept(x, tau, k, p)), (V, tau, k, p)
                assert ref.n_kept == ref.P.sum() >= 1 and ref.P[ref.argmax]
    assert n >= 50, n


def test_reference_draw_and_judge_agree():
    """the reference's own draws pass its judge; a neighbouring token, a wrong n_kept and a wrong prob do not"""
    for case in sampling.operator_cases(97)[:12] + sampling.adversarial_cases():
        ref = sampling.reference(case["x"], case["tau"], case["k"], case["p"])
        ctr = np.arange(64)
        tok = np.array([sampling.draw(ref, case["seed"], int(c)) for c in ctr])
        prob = ref.w[tok] / ref.Z
        sampling.judge(case["x"], case, ctr, tok, np.full(64, ref.n_kept), prob, where=case["name"])
        with pytest.raises(AssertionError):
            sampling.judge(ref, case, ctr, tok, np.full(64, ref.n_kept + 1), prob)
        if not ref.greedy and ref.n_kept > 3 and ref.w[ref.P].min() / ref.Z > 4 * sampling.EPS:
            other = np.flatnonzero(ref.P)
            wrong = other[(np.searchsorted(other, tok) + 2) % other.size]         # two kept tokens further on
            with pytest.raises(AssertionError):
                sampling.judge(ref, case, ctr, wrong, np.full(64, ref.n_kept), None)
            with pytest.raises(AssertionError):
                sampling.judge(ref, case, ctr, tok, None, prob * (1 + 2.0 ** -13) + 2.0 ** -37)


@pytest.mark.parametrize("V", sampling.OPERATOR_VS)
def test_every_operator_case_has_the_margin(V):
    cases = sampling.operator_cases(V)
    assert len(cases) == 1 + 3 * 5 * 3 and len({c["name"] for c in cases}) == len(cases)
    assert {(c["tau"], c["k"], c["p"]) for c in cases[1:]} == {(t, k, p) for t in sampling.TAUS for k in sampling.ks_for(V)
                                                               for p in sampling.PS}
    for c in cases:
        ref = sampling.reference(c["x"], c["tau"], c["k"], c["p"])
        assert c["x"].shape == (V,) and (ref.greedy or ref.margin >= sampling.MARGIN), c["name"]
        if not ref.greedy and 0 < c["k"] < V:
            assert ref.n_kept <= max(c["k"], int((sampling.logits64(c["x"]) >= np.sort(sampling.logits64(c["x"]))[V - c["k"]]).sum()))


def test_every_adversarial_case_has_the_margin_and_its_property():
    V = 4099
    cases = {c["name"]: c for c in sampling.adversarial_cases(V)}
    refs = {n: sampling.reference(c["x"], c["tau"], c["k"], c["p"]) for n, c in cases.items()}
    for n, r in refs.items():
        assert r.greedy or r.margin >= sampling.MARGIN, (n, r.margin)
    assert refs["adv-all-equal"].n_kept == V and refs["adv-all-equal-topk-topp"].n_kept == V      # ties stay together
    assert refs["adv-all-ninf"].n_kept == V and refs["adv-all-ninf-topk-topp"].n_kept == V
    assert refs["adv-all-nan-greedy"].argmax == 0
    assert refs["adv-nan-mixed-greedy"].argmax % 7 != 0 and torch.isnan(cases["adv-nan-mixed"]["x"][0])
    assert refs["adv-one-pinf"].n_kept == V and refs["adv-one-pinf-topk-topp"].n_kept == 1
    assert sampling.draw(refs["adv-one-pinf"], 11, 3) == V // 3
    assert refs["adv-ties-at-topk"].n_kept == 7 and refs["adv-ties-at-topk"].k == 3
    assert refs["adv-max-at-0-greedy"].argmax == 0 and refs["adv-max-at-last-greedy"].argmax == V - 1
    assert refs["adv-dup-max-greedy"].argmax == 41
    assert refs["adv-signed-zero-max-greedy"].argmax == 3 and refs["adv-signed-zero-max"].n_kept >= 2
    assert set(np.flatnonzero(refs["adv-signed-zero-max"].w == 1.0)) == {3, 4}
    deep = refs["adv-deep-tail"]
    assert (deep.w[deep.P] < 2.0 ** -40).mean() > 0.5


def test_sampler_set_validation():
    from infinitevl_amd.harness import Sampler
    s = Sampler(3, "cpu")
    assert s.temperature.tolist() == [0, 0, 0] and s.top_k.tolist() == [0, 0, 0] and s.top_p.tolist() == [1, 1, 1]
    assert (s.temperature.dtype, s.top_k.dtype, s.top_p.dtype, s.seed.dtype, s.counter.dtype) == \
        (torch.float32, torch.int32, torch.float32, torch.int64, torch.int64)
    s.counter[1] = 9
    s.set(1, temperature=0.7, top_k=50, top_p=0.9, seed=-5)
    assert (s.temperature[1].item(), s.top_k[1].item(), s.top_p[1].item(), s.seed[1].item(), s.counter[1].item()) == \
        (sampling.f32(0.7), 50, sampling.f32(0.9), -5, 0)
    s.set(2, temperature=1.0, seed=2 ** 64 - 1)
    assert s.seed[2].item() == -1
    saved = s.state()
    s.counter[2] = 4
    s.load_state(saved)
    assert s.counter.tolist() == [0, 0, 0]
    s.reset(1)
    assert (s.temperature[1].item(), s.top_k[1].item(), s.top_p[1].item(), s.seed[1].item()) == (0.0, 0, 1.0, 0)
    for bad in ({"temperature": -0.1}, {"temperature": float("nan")}, {"temperature": float("inf")}, {"top_k": -1},
                {"top_k": 1.5}, {"top_p": 0.0}, {"top_p": 1.0001}, {"top_p": float("nan")}, {"seed": 2 ** 64}, {"seed": 0.5}):
        with pytest.raises(ValueError):
            s.set(0, **bad)
    for row in (-1, 3, 0.0):
        with pytest.raises(ValueError):
            s.set(row)
    assert s.temperature[0].item() == 0.0 and s.top_p[0].item() == 1.0
    with pytest.raises(ValueError):
        Sampler(0, "cpu")


def test_sample_tokens_refuses_cpu_tensors_and_bad_arguments():
    from infinitevl_amd import ops
    S, V = 2, 16
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    t, k, p = torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S)
    sd, c = torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, k, p, sd, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg[:, None], t, k, p, sd, c, out=torch.zeros(S, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="bf16"):
        ops.sample_tokens(lg.float(), t, k, p, sd, c)
    with pytest.raises(ValueError, match="bf16"):
        ops.sample_tokens(lg[0], t, k, p, sd, c)
    with pytest.raises(ValueError, match="contiguous"):
        ops.sample_tokens(torch.zeros(V, S, dtype=torch.bfloat16).t(), t, k, p, sd, c)
    with pytest.raises(ValueError, match="temperature"):
        ops.sample_tokens(lg, t.double(), k, p, sd, c)
    with pytest.raises(ValueError, match="top_k"):
        ops.sample_tokens(lg, t, k.long(), p, sd, c)
    with pytest.raises(ValueError, match="top_p"):
        ops.sample_tokens(lg, t, k, p[:1], sd, c)
    with pytest.raises(ValueError, match="seed"):
        ops.sample_tokens(lg, t, k, p, sd.int(), c)
    with pytest.raises(ValueError, match="counter"):
        ops.sample_tokens(lg, t, k, p, sd, c.float())
    with pytest.raises(ValueError, match="out"):
        ops.sample_tokens(lg, t, k, p, sd, c, out=torch.zeros(S, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_kept"):
        ops.sample_tokens(lg, t, k, p, sd, c, n_kept=torch.zeros(S, dtype=torch.int64))
    with pytest.raises(ValueError, match="prob"):
        ops.sample_tokens(lg, t, k, p, sd, c, prob=torch.zeros(S + 1))


def test_entry_point_validates_and_is_exported(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    assert _lib.PROTOTYPES["ivl_sample_rows_fwd"] == (ctypes.c_int, [ctypes.POINTER(_lib.SampleArgs), ctypes.c_void_p])
    assert [n for n, _ in _lib.SampleArgs._fields_] == sampling.ARG_FIELDS
    assert lib.ivl_sample_rows_fwd(None, None) == INV and b"NULL" in lib.ivl_last_error()
    for name in ("logits", "temperature", "top_k", "top_p", "seed", "counter", "token"):     # every required pointer
        assert sampling.c_refused(lib, INV, b"NULL", V=16, **{name: None}), name
    assert sampling.c_refused(lib, INV, b"S=0", V=16, S=0)
    assert sampling.c_refused(lib, INV, b"V=0", V=0, ld=16)
    assert sampling.c_refused(lib, INV, b"ld=15", V=16, ld=15)
    assert sampling.c_refused(lib, UNS, b"2^23", V=1 << 23, ld=1 << 24)
    assert "ivl_sample_rows_fwd" in _lib.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "ivl_sample_rows_fwd" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.parametrize("logprobs", [None, 0, 2])
@pytest.mark.parametrize("history", [0, 5])
@pytest.mark.parametrize("max_stop", [0, 3])
@pytest.mark.parametrize("vocab_size", [None, 70])
def test_sampler_table_follows_its_configuration(monkeypatch, vocab_size, max_stop, history, logprobs):
    """Which per-row tensors a Sampler holds, which of them are state, what set() clears them to and under which keyword
    sample() hands each to ops.sample_tokens, as rules over the constructor's arguments."""
    from infinitevl_amd import ops
    from infinitevl_amd.harness import Sampler
    s = Sampler(3, "cpu", vocab_size=vocab_size, max_stop=max_stop, history=history, logprobs=logprobs)
    bitmap, ring, scored, top = vocab_size is not None, history > 0, logprobs is not None, bool(logprobs)
    inf = float("inf")
    # name: (exists, value of a fresh or cleared row, a step changes it, keyword of ops.sample_tokens), in row_tensors() order
    rules = {"temperature": (True, 0, False, None), "top_k": (True, 0, False, None), "top_p": (True, 1, False, None),
             "seed": (True, 0, False, None), "counter": (True, 0, True, None),
             "rep_penalty": (True, 1, False, "rep_penalty" if bitmap else None), "seen": (bitmap, 0, True, "seen"),
             "stop_ids": (max_stop > 0, -1, False, "stop_ids"), "budget": (True, -1, False, "budget"),
             "fill": (True, 0, False, "fill"), "n_new": (True, 0, True, "n_new"), "done": (True, 0, True, "done"),
             "history": (ring, 0, True, "history"), "logprob": (scored, 0, True, "logprob"),
             "cum_logprob": (scored, 0, True, "cum_logprob"), "top_ids": (top, -1, True, "top_ids"),
             "top_logprob": (top, -inf, True, "top_logprobs"), "lp_history": (scored and ring, 0, True, "lp_history"),
             "top_hist_ids": (top and ring, -1, True, "top_hist_ids"), "top_hist_lp": (top and ring, -inf, True, "top_hist_lp")}
    have = [n for n, r in rules.items() if r[0]]
    assert all(getattr(s, n) is None for n in rules if n not in have)
    assert len(have) == 10 + bitmap + (max_stop > 0) + ring + 2 * scored + 2 * top + (scored and ring) + 2 * (top and ring)
    assert [t.data_ptr() for t in s.row_tensors()] == [getattr(s, n).data_ptr() for n in have]
    for n in have:
        t = getattr(s, n)
        assert t.shape[0] == 3 and torch.equal(t, torch.full_like(t, rules[n][1])), n
    state = s.state()
    assert sorted(state) == sorted(n for n in have if rules[n][2])
    assert all(state[n].data_ptr() != getattr(s, n).data_ptr() for n in state)

    calls = []
    monkeypatch.setattr(ops, "sample_tokens", lambda *a, **k: calls.append((a, k)) or k["out"])
    V = vocab_size or 70
    token = torch.zeros(3, 1, dtype=torch.int64)
    assert s.sample(torch.zeros(3, V, dtype=torch.bfloat16), token) is token
    s.sample(torch.zeros(1, V, dtype=torch.bfloat16), token[1:2], row=1)
    assert s.controlled == (bitmap or ring or scored) and len(calls) == 2
    for (args, kw), rows, row0 in zip(calls, (3, 1), (0, 1)):
        def is_rows_of(t, name):
            whole = getattr(s, name)
            return tuple(t.shape) == (rows, *whole.shape[1:]) and \
                t.data_ptr() == whole.data_ptr() + row0 * whole.stride(0) * whole.element_size()
        assert len(args) == 6 and tuple(args[0].shape) == (rows, V)
        for t, n in zip(args[1:], ("temperature", "top_k", "top_p", "seed", "counter")):
            assert is_rows_of(t, n), n
        assert kw["out"].data_ptr() == token[row0:].data_ptr()
        given = {k: t for k, t in kw.items() if t is not None and k != "out"}
        want = {r[3]: n for n, r in rules.items() if r[0] and r[3] is not None} if s.controlled else {}
        assert sorted(given) == sorted(want)
        for k, t in given.items():
            assert is_rows_of(t, want[k]), k

    for n in have:
        if rules[n][2]:
            getattr(s, n)[1] = 7
    s.set(1)
    for n in have:
        t = getattr(s, n)
        assert torch.equal(t, torch.full_like(t, rules[n][1])), n

"""CPU (-m "not gpu"): the scores' reference (tests/logprobs.py) stands on its own -- against torch.log_softmax in float64 and the
special rows by hand -- and the host side of the feature: the header's declaration of the score group of
ivl_sample_args, the entry point's error codes on pointers that are never dereferenced, the ABI version, ops.sample_tokens' and
Sampler's new arguments."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import logprobs
import sampling
from conftest import ROOT

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def _bf(v):
    return torch.tensor(v, dtype=torch.float32).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 97, 4099])
def test_reference_is_log_softmax_in_float64(V):
    for seed, scale in ((1, 3.0), (2, 0.5), (3, 12.0)):
        x = sampling.random_row(V, seed, scale=scale)
        want = torch.log_softmax(x.double(), dim=-1).numpy()
        got = logprobs.reference(x)
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-12)
        assert abs(np.exp(got).sum() - 1.0) < 1e-12
        n = min(V, 20)
        vals, idx = torch.sort(x.double(), descending=True, stable=True)
        assert logprobs.top_list(x, 20).tolist() == idx[:n].tolist()
    d = logprobs.deep(4099)
    ref = logprobs.reference(d)
    assert np.isfinite(ref).all() and (ref < -27.7).sum() > 4000 and np.allclose(ref, torch.log_softmax(d.double(), -1).numpy(), atol=1e-12)


def test_reference_special_rows_by_hand():
    V = 97
    ref = logprobs.reference(logprobs.all_equal(V))
    assert np.array_equal(ref, np.full(V, -math.log(V))) and logprobs.top_list(logprobs.all_equal(V), 5).tolist() == [0, 1, 2, 3, 4]
    x = _bf([0.0, 1.0, INF, -2.0])                                   # one +inf: it holds all the mass
    assert logprobs.reference(x).tolist() == [-INF, -INF, 0.0, -INF] and logprobs.top_list(x, 3).tolist() == [2, 1, 0]
    x = _bf([INF, 1.0, INF])
    assert logprobs.reference(x).tolist() == [-math.log(2), -INF, -math.log(2)]
    x = _bf([-INF] * 5)                                              # all -inf: uniform
    assert np.array_equal(logprobs.reference(x), np.full(5, -math.log(5))) and logprobs.top_list(x, 9).tolist() == [0, 1, 2, 3, 4]
    x = _bf([float("nan"), 0.0, float("nan"), 0.0])                  # NaN = -inf
    assert logprobs.reference(x).tolist() == [-INF, -math.log(2), -INF, -math.log(2)]
    assert logprobs.top_list(x, 4).tolist() == [1, 3, 0, 2]
    assert np.array_equal(logprobs.reference(_bf([float("nan")] * 3)), np.full(3, -math.log(3)))
    x = _bf([1.0, 3.0, 2.0, 2.0, 0.0, 2.0, -0.0])                    # a tie across the 2nd .. 4th place; -0 ties with +0
    assert logprobs.top_list(x, 2).tolist() == [1, 2] and logprobs.top_list(x, 3).tolist() == [1, 2, 3]
    assert logprobs.top_list(x, 7).tolist() == [1, 2, 3, 5, 0, 4, 6]
    for n in (1, 5, 20):
        t = logprobs.ties_across(4099, n)
        srt = np.sort(t.double().numpy())[::-1]
        assert srt[n - 1] == srt[n] == 4.0 and (n == 1 or srt[n - 2] > 4.0), n     # the n-th place lies inside the tie


def test_judge_accepts_the_reference_and_refuses_what_is_off():
    x = logprobs.ties_across(97, 5)
    ref, ids = logprobs.reference(x), logprobs.top_list(x, 5)
    lps = ref[ids].astype(np.float32)
    logprobs.judge(x, ids[1], lps[1], ids, lps)
    with pytest.raises(AssertionError, match="logprob"):
        logprobs.judge(x, ids[1], lps[1] * (1 + 2.0 ** -16), ids, lps)
    swapped = ids.copy()
    swapped[[3, 4]] = swapped[[4, 3]]                                # the same values, the higher index first
    with pytest.raises(AssertionError, match="top ids"):
        logprobs.judge(x, ids[1], lps[1], swapped, lps)
    off = lps.copy()
    off[1] = np.nextafter(off[1], np.float32(0))                     # within the bound, yet not the bits of logprob
    with pytest.raises(AssertionError, match="!= logprob"):
        logprobs.judge(x, ids[1], lps[1], ids, off)
    tail_ids, tail_lps = np.array([0, -1, -1]), np.array([0.0, -INF, -INF], dtype=np.float32)
    logprobs.judge(_bf([2.0]), 0, 0.0, tail_ids, tail_lps)
    with pytest.raises(AssertionError, match="tail"):
        logprobs.judge(_bf([2.0]), 0, 0.0, np.array([0, 0, -1]), tail_lps)
    assert logprobs.close(-INF, -INF) and not logprobs.close(-1e30, -INF) and not logprobs.close(float("nan"), -1.0)


# ---------------------------------------------------------------------------------------------
# the C entry point
# ---------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_validates(lib):
    from infinitevl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    assert "IVL_API int ivl_sample_rows_fwd(const ivl_sample_args* args, void* stream);" in hdr
    assert _lib.PROTOTYPES["ivl_sample_rows_fwd"] == (ctypes.c_int, [ctypes.POINTER(_lib.SampleArgs), ctypes.c_void_p])
    fields = dict(_lib.SampleArgs._fields_)
    assert sampling.ARG_FIELDS[24:32] == ["logprob", "n_top", "top_ids", "top_logprobs", "cum_logprob", "lp_history", "top_hist_ids",
                                          "top_hist_lp"]
    assert fields["n_top"] is ctypes.c_int and fields["cum_logprob"] is ctypes.c_void_p
    assert lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12

    one, INV = sampling.ONE, _lib.IVL_ERR_INVALID_ARG

    def refused(word, **kw):
        return sampling.c_refused(lib, INV, word, **kw)

    assert refused(b"n_top", n_top=-1) and refused(b"n_top", n_top=21, top_ids=one, top_logprobs=one)
    assert refused(b"top_ids", n_top=5) and refused(b"top_ids", n_top=5, top_ids=one)
    assert refused(b"top_ids", n_top=5, top_logprobs=one)
    assert refused(b"n_new", lp_history=one, hist_ld=4)                                            # no n_new
    assert refused(b"hist_ld", lp_history=one, n_new=one, hist_ld=0)
    for ring in ("top_hist_ids", "top_hist_lp"):
        assert refused(b"n_new", **{ring: one}, n_top=5, top_ids=one, top_logprobs=one, hist_ld=4)       # no n_new
        assert refused(b"hist_ld", **{ring: one}, n_top=5, top_ids=one, top_logprobs=one, n_new=one, hist_ld=0)
        assert refused(b"n_top", **{ring: one}, n_new=one, hist_ld=4)                              # n_top == 0
    # whatever the controls refuse
    assert refused(b"rep_penalty needs seen", logprob=one, rep_penalty=one)
    assert refused(b"n_stop=", logprob=one, n_stop=17, stop_ids=one, done=one)
    assert refused(b"budget", logprob=one, budget=one, done=one) and refused(b"history", logprob=one, history=one, hist_ld=4)
    for name in ("logits", "temperature", "top_k", "top_p", "seed", "counter", "token"):          # with a score on
        assert refused(b"NULL", logprob=one, **{name: None}), name
    assert sampling.c_refused(lib, _lib.IVL_ERR_UNSUPPORTED, b"2^23", V=1 << 23, ld=1 << 24, logprob=one)


# ---------------------------------------------------------------------------------------------
# ops and Sampler
# ---------------------------------------------------------------------------------------------
def test_ops_check_the_score_arguments():
    from infinitevl_amd import ops
    S, V, H, N = 2, 40, 4, 5
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    t, k, p = torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S)
    sd, c = torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64)
    good = {"n_new": torch.zeros(S, dtype=torch.int64), "history": torch.zeros(S, H, dtype=torch.int64),
            "logprob": torch.zeros(S), "top_ids": torch.zeros(S, N, dtype=torch.int64), "top_logprobs": torch.zeros(S, N),
            "cum_logprob": torch.zeros(S, dtype=torch.float64), "lp_history": torch.zeros(S, H),
            "top_hist_ids": torch.zeros(S, H, N, dtype=torch.int64), "top_hist_lp": torch.zeros(S, H, N)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, k, p, sd, c, **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, k, p, sd, c, logprob=good["logprob"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # rings without a token history: their own length
        ops.sample_tokens(lg, t, k, p, sd, c, **{n: v for n, v in good.items() if n != "history"})
    with pytest.raises(TypeError):
        ops.sample_tokens(lg, t, k, p, sd, c, None, None, None, good["logprob"])              # keyword-only
    wrong = {"logprob": torch.zeros(S, dtype=torch.float64), "top_ids": torch.zeros(S, N, dtype=torch.int32),
             "top_logprobs": torch.zeros(S, N + 1), "cum_logprob": torch.zeros(S), "lp_history": torch.zeros(S, H + 1),
             "top_hist_ids": torch.zeros(S, H, N, dtype=torch.int32), "top_hist_lp": torch.zeros(S, H, N + 1)}
    for name, bad in wrong.items():
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, t, k, p, sd, c, **dict(good, **{name: bad}))
    for name, bad in (("top_ids", torch.zeros(S, 21, dtype=torch.int64)), ("top_ids", torch.zeros(S, 0, dtype=torch.int64)),
                      ("top_ids", torch.zeros(S, dtype=torch.int64)), ("logprob", torch.zeros(S + 1)),
                      ("lp_history", torch.zeros(S, 2 * H)[:, ::2])):
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, t, k, p, sd, c, **dict(good, **{name: bad}))
    for drop, named in ((("top_ids",), "top_ids"), (("top_logprobs",), "top_logprobs"), (("n_new", "history"), "n_new"),
                        (("top_ids", "top_logprobs"), "top_hist")):
        with pytest.raises(ValueError, match=named):
            ops.sample_tokens(lg, t, k, p, sd, c, **{n: v for n, v in good.items() if n not in drop})


def test_sampler_logprobs_argument_tensors_and_state():
    from infinitevl_amd.harness import Sampler
    for bad in (21, -1, 1.5, True, "5"):
        with pytest.raises(ValueError, match="logprobs"):
            Sampler(2, "cpu", logprobs=bad)
    plain = Sampler(2, "cpu", vocab_size=97, history=4)
    assert plain.n_logprobs is None and plain.logprob is None and plain.cum_logprob is None
    assert set(plain.state()) == {"counter", "seen", "n_new", "done", "history"}
    assert not Sampler(2, "cpu").controlled
    with pytest.raises(ValueError, match="logprobs"):
        plain.logprobs(0)
    s0 = Sampler(2, "cpu", logprobs=0)
    assert s0.controlled and s0.top_ids is None and s0.lp_history is None and tuple(s0.logprob.shape) == (2,)
    assert s0.cum_logprob.dtype == torch.float64 and set(s0.state()) == {"counter", "n_new", "done", "logprob", "cum_logprob"}
    with pytest.raises(ValueError, match="history"):
        s0.logprobs(0)
    h0 = Sampler(2, "cpu", history=4, logprobs=0)
    assert tuple(h0.lp_history.shape) == (2, 4) and h0.top_hist_ids is None
    with pytest.raises(ValueError, match="logprobs >= 1"):
        h0.top_logprobs(0)
    s = Sampler(2, "cpu", vocab_size=97, history=4, logprobs=3)
    assert (tuple(s.top_ids.shape), tuple(s.top_logprob.shape), tuple(s.top_hist_ids.shape), tuple(s.top_hist_lp.shape)) == \
        ((2, 3), (2, 3), (2, 4, 3), (2, 4, 3))
    assert (s.logprob.dtype, s.top_ids.dtype, s.top_logprob.dtype, s.lp_history.dtype, s.top_hist_ids.dtype, s.top_hist_lp.dtype) == \
        (torch.float32, torch.int64, torch.float32, torch.float32, torch.int64, torch.float32)
    assert set(s.state()) == {"counter", "seen", "n_new", "done", "history", "logprob", "cum_logprob", "top_ids", "top_logprob",
                              "lp_history", "top_hist_ids", "top_hist_lp"}
    # the accessors follow tokens(): aligned, same wrap rule
    s.n_new[0], s.history[0] = 2, torch.tensor([8, 9, 0, 0])
    s.lp_history[0] = torch.tensor([-1.0, -2.0, 0.0, 0.0])
    s.top_hist_ids[0] = torch.arange(12).view(4, 3)
    s.top_hist_lp[0] = -torch.arange(12.0).view(4, 3)
    assert s.tokens(0).tolist() == [8, 9] and s.logprobs(0).tolist() == [-1.0, -2.0]
    ids, lps = s.top_logprobs(0)
    assert ids.tolist() == [[0, 1, 2], [3, 4, 5]] and lps.tolist() == [[0.0, -1.0, -2.0], [-3.0, -4.0, -5.0]]
    s.n_new[0] = 6                                                     # wrapped: the last 4 of 6, oldest first
    s.lp_history[0] = torch.tensor([-4.0, -5.0, -2.0, -3.0])
    assert s.logprobs(0).tolist() == [-2.0, -3.0, -4.0, -5.0]
    assert s.top_logprobs(0)[0][:, 0].tolist() == [6, 9, 0, 3]
    # state round trip, then set() clears the row's scores and leaves the other row alone
    s.cum_logprob[:] = torch.tensor([-3.5, -1.25], dtype=torch.float64)
    s.logprob[:] = torch.tensor([-0.5, -0.25])
    saved = s.state()
    s.cum_logprob += 1
    s.lp_history.fill_(7)
    s.top_hist_ids.fill_(7)
    s.load_state(saved)
    assert s.cum_logprob.tolist() == [-3.5, -1.25] and s.logprobs(0).tolist() == [-2.0, -3.0, -4.0, -5.0]
    s.lp_history[1] = -9.0
    s.set(0, temperature=0.7)
    assert s.cum_logprob.tolist() == [0.0, -1.25] and s.logprob.tolist() == [0.0, -0.25]
    assert s.lp_history[0].tolist() == [0.0] * 4 and s.lp_history[1].tolist() == [-9.0] * 4
    assert (s.top_hist_ids[0] == -1).all() and (s.top_hist_lp[0] == -INF).all() and (s.top_ids[0] == -1).all()
    assert s.logprobs(0).numel() == 0
    done, n_new = s.poll()                                             # unchanged
    assert done.tolist() == [0, 0] and n_new.tolist() == [0, 0]
    with pytest.raises(ValueError, match="state"):
        plain.load_state(saved)

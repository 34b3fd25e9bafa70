"""CPU (-m "not gpu"): the generation controls' reference (tests/generation.py) stands on its own -- the penalty against HF's
RepetitionPenaltyLogitsProcessor bit for bit, the top-p margin of every builder case, the bitmap packing -- and the host side of
the feature: Sampler's new arguments and state, ops.sample_tokens / ops.mark_tokens argument checks, the two C entry points'
error codes on pointers that are never dereferenced, and their presence in the library's dynamic symbol table."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import generation
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


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", generation.FIXED_VS)
def test_every_fixed_case_has_the_margin(V):
    cases = generation.fixed_cases(V)
    assert len(cases) == 2 * (1 + 3 * 2 * 3) + 2 * 2 * 3 and len({c["name"] for c in cases}) == len(cases)
    assert {c["r"] for c in cases} == set(generation.RS)
    for c in cases:
        ref = generation.reference(c["x"], c["seen"], c["r"], c["tau"], c["k"], c["p"])
        assert c["x"].shape == (V,) and c["seen"].shape == (V,) and (ref.greedy or ref.margin >= sampling.MARGIN), c["name"]
    quarter = [c for c in cases if "quarter" in c["name"]]
    if V > 1:
        assert all(0 < c["seen"].sum() < V for c in quarter)
        # the penalty matters: it changes the kept set or the arg-max of some case
        assert any(generation.reference(c["x"], c["seen"], c["r"], c["tau"], c["k"], c["p"]).argmax !=
                   sampling.reference(c["x"], c["tau"], c["k"], c["p"]).argmax for c in cases)


def test_penalise_is_the_stated_arithmetic():
    c = generation.special_row()
    y = generation.penalise(c["x"], c["seen"], 1.3)
    x = c["x"]
    assert torch.isnan(y[0]) and torch.isnan(y[1])
    assert y[2] == float("inf") and y[3] == float("inf") and y[4] == -float("inf") and y[5] == -float("inf")
    assert y[6] == 0 and y[7] == 0 and y[7].view(torch.int16).item() == -32768           # -0 / r = -0: the class of +0
    unseen = torch.from_numpy(~c["seen"])
    assert torch.equal(y.view(torch.int16)[unseen], x.view(torch.int16)[unseen])
    assert torch.equal(generation.penalise(x, np.ones(97, dtype=bool), 1.0).view(torch.int16), x.view(torch.int16))
    # by hand: 3.0 / 1.3 = 2.3077 -> bf16 2.3125 (0x4014); -3.0 * 1.3 = -3.9 -> bf16 -3.90625 (0xC07A)
    h = generation.penalise(torch.tensor([3.0, -3.0], dtype=torch.bfloat16), np.ones(2, dtype=bool), 1.3)
    assert h.tolist() == [2.3125, -3.90625]
    # at most half a bf16 ulp (8 significant bits: 2^-8 relative) from the fp32 value HF keeps
    x = sampling.random_row(4099, 3)
    for r in (1.3, 0.8, 2.0):
        exact = np.where(x.float().numpy() < 0, x.float().numpy() * np.float32(r), x.float().numpy() / np.float32(r))
        got = generation.penalise(x, np.ones(4099, dtype=bool), r).float().numpy()
        assert (np.abs(got - exact) <= 2.0 ** -8 * np.abs(exact)).all()


def test_penalise_equals_the_hf_processor_rounded_to_bf16():
    tf = pytest.importorskip("transformers")
    for V, r, seed in ((97, 1.3, 1), (512, 0.8, 2), (4099, 2.0, 3), (4099, 1.3, 4)):
        x = sampling.random_row(V, seed, scale=4.0)
        seen = generation.random_seen(V, seed)
        ids = torch.from_numpy(np.flatnonzero(seen))[None]
        hf = tf.RepetitionPenaltyLogitsProcessor(penalty=r)(ids, x.float()[None].clone())[0]
        assert hf.dtype == torch.float32
        assert torch.equal(hf.to(torch.bfloat16).view(torch.int16), generation.penalise(x, seen, r).view(torch.int16)), (V, r)


def test_bitmap_packing_and_the_host_bookkeeping():
    seen = np.zeros(97, dtype=bool)
    seen[[0, 31, 32, 96]] = True
    w = generation.pack(seen, 5, beyond=True)
    assert w.tolist() == [0x80000001, 1, 0, 0xFFFFFFFF, 0xFFFFFFFF] and w.dtype == np.uint32
    assert generation.pack(seen, 4, beyond=False).tolist() == [0x80000001, 1, 0, 1]
    assert np.array_equal(generation.unpack(w)[:97], seen) and generation.unpack(w)[97:].all()
    assert generation.to_i32(w).dtype == torch.int32 and generation.to_i32(w)[0].item() == -2 ** 31 + 1
    b = generation.Book(16, stop_ids=(-1, 5), budget=3, hist_ld=2)
    b.push(4)
    b.push(7)
    assert (b.done, b.n_new, b.history) == (0, 2, [4, 7])
    b.push(5)                                                          # a stop id wins over the budget on the same token
    assert (b.done, b.n_new, b.history) == (1, 3, [5, 7]) and set(np.flatnonzero(b.seen)) == {4, 5, 7}
    b = generation.Book(16, stop_ids=(5,), budget=2)
    b.push(1)
    b.push(2)
    assert b.done == 2
    chain = generation.greedy_chain(sampling.random_row(4099, 5), 1.5, 16)
    assert len(set(chain)) == 16                                      # the evolving GPU test relies on it


# ---------------------------------------------------------------------------------------------
# Sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_without_controls_refuses_a_penalty_and_accepts_stop_ids_and_a_budget():
    from infinitevl_amd.harness import Sampler
    s = Sampler(3, "cpu")
    assert not s.controlled and s.seen is None and s.history is None
    with pytest.raises(ValueError, match="vocab_size"):
        s.set(0, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="vocab_size"):
        s.mark(0, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="history"):
        s.tokens(0)
    s.set(0, repetition_penalty=1.0)
    assert not s.controlled
    s.set(1, temperature=0.7, stop_token_ids=[2, 7], max_new_tokens=5, fill_token=9)
    assert s.controlled
    assert s.stop_ids[1].tolist() == [2, 7] + [-1] * 6 and s.budget.tolist() == [-1, 5, -1] and s.fill.tolist() == [0, 9, 0]
    s.reset(1)
    assert s.stop_ids[1].tolist() == [-1] * 8 and s.budget[1].item() == -1 and s.fill[1].item() == 0


def test_sampler_set_validation_of_the_controls():
    from infinitevl_amd.harness import Sampler
    s = Sampler(2, "cpu", vocab_size=97, max_stop=2, history=4)
    assert s.controlled and tuple(s.seen.shape) == (2, 4) and tuple(s.history.shape) == (2, 4) and tuple(s.stop_ids.shape) == (2, 2)
    assert (s.rep_penalty.dtype, s.seen.dtype, s.stop_ids.dtype, s.budget.dtype, s.fill.dtype, s.n_new.dtype, s.done.dtype,
            s.history.dtype) == (torch.float32, torch.int32, torch.int64, torch.int64, torch.int64, torch.int64, torch.int32,
                                 torch.int64)
    assert s.rep_penalty.tolist() == [1, 1] and s.budget.tolist() == [-1, -1] and s.done.tolist() == [0, 0]
    s.seen[1] = 5
    s.n_new[1], s.done[1], s.counter[1] = 3, 2, 7
    s.history[1] = 6
    s.seen[0] = 9
    s.set(1, temperature=0.7, repetition_penalty=1.3, stop_token_ids=(11,), max_new_tokens=1)
    assert s.rep_penalty[1].item() == sampling.f32(1.3) and s.stop_ids[1].tolist() == [11, -1] and s.budget[1].item() == 1
    assert s.seen[1].tolist() == [0] * 4 and s.history[1].tolist() == [0] * 4 and s.seen[0].tolist() == [9] * 4
    assert (s.n_new[1].item(), s.done[1].item(), s.counter[1].item()) == (0, 0, 0)
    for bad in ({"repetition_penalty": 0.0}, {"repetition_penalty": -1.3}, {"repetition_penalty": float("nan")},
                {"repetition_penalty": float("inf")}, {"stop_token_ids": [1, 2, 3]}, {"stop_token_ids": [-1]},
                {"stop_token_ids": [1.5]}, {"stop_token_ids": [True]}, {"max_new_tokens": 0}, {"max_new_tokens": 2.5},
                {"max_new_tokens": True}, {"fill_token": -1}, {"fill_token": 0.5}):
        with pytest.raises(ValueError):
            s.set(0, **bad)
    assert s.seen[0].tolist() == [9] * 4                                # a refused set() changes nothing
    for kw in ({"vocab_size": 0}, {"vocab_size": 1.5}, {"max_stop": 17}, {"max_stop": -1}, {"history": -1}, {"history": 1.5}):
        with pytest.raises(ValueError):
            Sampler(2, "cpu", **kw)
    assert Sampler(2, "cpu", max_stop=0).stop_ids is None
    with pytest.raises(ValueError, match="int64"):
        s.mark(0, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        s.mark(0, torch.zeros(2, 3, dtype=torch.int64))


def test_sampler_state_round_trip_of_every_control_tensor():
    from infinitevl_amd.harness import Sampler
    s = Sampler(2, "cpu", vocab_size=97, history=4)
    s.set(0, temperature=0.7, repetition_penalty=1.3, stop_token_ids=(3,), max_new_tokens=9)
    s.counter[0], s.n_new[0], s.done[1] = 4, 2, 1
    s.seen[0, 1], s.history[0, :2] = 0x10, torch.tensor([8, 9])
    saved = s.state()
    assert set(saved) == {"counter", "seen", "n_new", "done", "history"}
    want = {k: v.clone() for k, v in saved.items()}
    s.counter += 3
    s.n_new += 1
    s.done[0] = 2
    s.seen.fill_(-1)
    s.history.fill_(7)
    assert all(torch.equal(saved[k], want[k]) for k in want)          # the state is a copy
    s.load_state(saved)
    for k, t in (("counter", s.counter), ("seen", s.seen), ("n_new", s.n_new), ("done", s.done), ("history", s.history)):
        assert torch.equal(t, want[k]), k
    assert s.rep_penalty[0].item() == sampling.f32(1.3) and s.budget[0].item() == 9          # parameters are not state
    assert s.tokens(0).tolist() == [8, 9]
    s.n_new[0], s.history[0] = 6, torch.tensor([14, 15, 12, 13])      # wrapped: the last 4 of 6 tokens, oldest first
    assert s.tokens(0).tolist() == [12, 13, 14, 15]
    done, n_new = s.poll()
    assert done.tolist() == [0, 1] and n_new.tolist() == [6, 0] and not done.is_cuda
    with pytest.raises(ValueError, match="state"):
        Sampler(2, "cpu").load_state(saved)
    plain = Sampler(2, "cpu")
    assert set(plain.state()) == {"counter", "n_new", "done"}


# ---------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------
def test_ops_refuse_cpu_tensors_and_bad_control_arguments():
    from infinitevl_amd import ops
    S, V = 2, 40
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    t, k, p = torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S)
    sd, c = torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64)
    good = {"rep_penalty": torch.ones(S), "seen": torch.zeros(S, 2, dtype=torch.int32),
            "stop_ids": torch.full((S, 3), -1, dtype=torch.int64), "budget": torch.full((S,), -1, dtype=torch.int64),
            "fill": torch.zeros(S, dtype=torch.int64), "n_new": torch.zeros(S, dtype=torch.int64),
            "done": torch.zeros(S, dtype=torch.int32), "history": torch.zeros(S, 4, dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, k, p, sd, c, **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, k, p, sd, c, done=good["done"])
    with pytest.raises(TypeError):
        ops.sample_tokens(lg, t, k, p, sd, c, None, None, None, good["rep_penalty"])        # keyword-only
    wrong = {"rep_penalty": torch.ones(S, dtype=torch.float64), "seen": torch.zeros(S, 2, dtype=torch.int64),
             "stop_ids": torch.full((S, 3), -1, dtype=torch.int32), "budget": torch.zeros(S, dtype=torch.int32),
             "fill": torch.zeros(S + 1, dtype=torch.int64), "n_new": torch.zeros(S, dtype=torch.int32),
             "done": torch.zeros(S, dtype=torch.int64), "history": torch.zeros(S, 4, dtype=torch.int32)}
    for name, bad in wrong.items():
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, t, k, p, sd, c, **dict(good, **{name: bad}))
    for name, bad in (("seen", torch.zeros(S, 1, dtype=torch.int32)),                         # 32 bits for V = 40
                      ("seen", torch.zeros(S * 2, dtype=torch.int32)),
                      ("stop_ids", torch.full((S, 17), -1, dtype=torch.int64)),
                      ("stop_ids", torch.full((S, 0), -1, dtype=torch.int64)),
                      ("history", torch.zeros(S, 0, dtype=torch.int64))):
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, t, k, p, sd, c, **dict(good, **{name: bad}))
    for drop, named in ((("seen",), "rep_penalty"), (("done",), "done"), (("n_new",), "n_new"),
                        (("stop_ids", "done"), "budget"), (("budget", "n_new"), "history")):
        with pytest.raises(ValueError, match=named):
            ops.sample_tokens(lg, t, k, p, sd, c, **{n: v for n, v in good.items() if n not in drop})
    row, ids = torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mark_tokens(row, ids, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mark_tokens(row, ids[:0], 40)
    for a, kw in (((row.long(), ids, 40), "seen_row"), ((torch.zeros(2, 2, dtype=torch.int32), ids, 40), "seen_row"),
                  ((row, ids.int(), 40), "ids"), ((row, ids, 65), "vocab_size"), ((row, ids, 0), "vocab_size"),
                  ((row, ids, 40.0), "vocab_size")):
        with pytest.raises(ValueError, match=kw):
            ops.mark_tokens(*a)


def test_ops_refuse_a_padded_history_with_and_without_scores():
    """hist_ld is the ring's length AND its row pitch on the device (smp_after: history[s * hist_ld + n_new % hist_ld]), so a
    history whose rows lie further apart than they are long is refused on every path, before the device is looked at."""
    from infinitevl_amd import ops
    S, V, H = 2, 40, 4
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    tab = (torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S), torch.zeros(S, dtype=torch.int64),
           torch.zeros(S, dtype=torch.int64))
    n_new, padded = torch.zeros(S, dtype=torch.int64), torch.zeros(S, H + 2, dtype=torch.int64)[:, :H]
    assert padded.stride() == (H + 2, 1)
    for scores in ({}, {"logprob": torch.zeros(S)}, {"lp_history": torch.zeros(S, H)}):
        with pytest.raises(ValueError, match="history must be contiguous"):
            ops.sample_tokens(lg, *tab, n_new=n_new, history=padded, **scores)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                # one row, or rows that touch: nothing to refuse
            ops.sample_tokens(lg[:1], *(t[:1] for t in tab), n_new=n_new[:1], history=padded[:1],
                              **{k: v[:1] for k, v in scores.items()})
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sample_tokens(lg, *tab, n_new=n_new, history=padded.contiguous(), **scores)


# ---------------------------------------------------------------------------------------------
# the C entry points
# ---------------------------------------------------------------------------------------------
def test_entry_points_validate_and_are_exported(lib):
    from infinitevl_amd import _lib
    one, INV = sampling.ONE, _lib.IVL_ERR_INVALID_ARG
    assert sampling.ARG_FIELDS[13:24] == ["rep_penalty", "seen", "seen_ld", "stop_ids", "n_stop", "budget", "fill", "n_new", "done",
                                          "history", "hist_ld"]

    def refused(word, **kw):
        return sampling.c_refused(lib, INV, word, **kw)

    assert refused(b"rep_penalty needs seen", rep_penalty=one)
    assert refused(b"seen_ld", rep_penalty=one, seen=one, seen_ld=1)                                    # 32 bits for V = 64
    assert refused(b"seen_ld", seen=one, seen_ld=1)
    assert refused(b"n_stop=", n_stop=-1) and refused(b"n_stop=", n_stop=17, stop_ids=one, done=one)
    assert refused(b"n_stop=", n_stop=2, done=one) and refused(b"n_stop=", n_stop=2, stop_ids=one)
    assert refused(b"budget", budget=one, done=one) and refused(b"budget", budget=one, n_new=one)
    assert refused(b"history", history=one, hist_ld=4)
    assert refused(b"history", history=one, n_new=one, hist_ld=0)
    for name in ("logits", "temperature", "top_k", "top_p", "seed", "counter", "token"):               # with a control on
        assert refused(b"NULL", done=one, **{name: None}), name
    assert sampling.c_refused(lib, _lib.IVL_ERR_UNSUPPORTED, b"2^23", V=1 << 23, ld=1 << 24, done=one)
    one = ctypes.c_void_p(one)
    assert lib.ivl_token_mark_fwd(None, 64, one, 1, None) == INV
    assert lib.ivl_token_mark_fwd(one, 0, one, 1, None) == INV
    assert lib.ivl_token_mark_fwd(one, 64, one, -1, None) == INV
    assert lib.ivl_token_mark_fwd(one, 64, None, 1, None) == INV and b"ivl_token_mark_fwd" in lib.ivl_last_error()
    assert lib.ivl_token_mark_fwd(one, 64, None, 0, None) == _lib.IVL_OK                                 # n == 0: nothing launched
    assert lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("ivl_sample_rows_fwd", "ivl_token_mark_fwd"):
        assert name in _lib.EXPORTED_SYMBOLS and name in exported, name

"""GPU (-m gpu): the scores of the sampling launch (ops.sample_tokens logprob= / top_ids= / ... -> ivl_sample_rows_fwd) and
their use in the graphed decode steps, judged by tests/logprobs.py: float64 log-softmax of the (penalised) bf16 row, exact ids.

  * operator: V in {1, 97, 4099} and one row of 151936, n_top in {0, 1, 5, 20} (also > V), calls of 1 .. 4 rows in a +inf
    surround at odd ld and shifted bases; random, all-equal, tied across the N-th place, NaN / +-inf / all -inf, a wide row whose
    tail lies below the weight floor, penalised rows; greedy and sampled rows mixed; a finished row;
  * the token, counter, seen, n_new, done, history, n_kept and prob of every call bit-identical to the controlled entry's; the
    group all NULL is the controlled entry; the same call twice; a row alone and among four;
  * the rings and their wrap, cum_logprob = the sequential float64 sum of the logged fp32 values;
  * GraphedMultiStreamDecode / GraphedDecode with Sampler(logprobs=3): eager == replayed graph, every step judged, tokens equal to
    a sampler without logprobs, run_until_done."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import generation
import logprobs
import parity
import sampling
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
N_TOPS = (0, 1, 5, 20)


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


def _case(name, x, tau=0.0, k=0, p=1.0, seed=1, r=1.0, seen=None, done=0):
    V = x.shape[0]
    return {"name": name, "x": x, "tau": tau, "k": k, "p": p, "seed": seed, "r": r,
            "seen": np.zeros(V, dtype=bool) if seen is None else seen, "done": done}


def _run(cases, n_top, ld, shift, hist_ld=0, steps=1, scores=True):
    """`steps` calls on one set of logits whose state (bitmap, counter, n_new, done, rings) evolves.  scores=False: the same call
    without the score keywords = the controlled entry.  Returns the host copies: per step outputs and the final state."""
    from infinitevl_amd import ops
    S, V = len(cases), cases[0]["x"].shape[0]
    _, lg = _place([c["x"] for c in cases], ld, shift)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    tab = (dev([c["tau"] for c in cases], torch.float32), dev([c["k"] for c in cases], torch.int32),
           dev([c["p"] for c in cases], torch.float32), dev([c["seed"] for c in cases], torch.int64),
           torch.zeros(S, dtype=torch.int64, device=DEV))
    W = generation.words_for(V) + 1
    seen = torch.stack([generation.to_i32(generation.pack(c["seen"], W, beyond=True)) for c in cases]).to(DEV)
    ctl = {"rep_penalty": dev([c["r"] for c in cases], torch.float32), "seen": seen, "fill": dev([7] * S, torch.int64),
           "n_new": torch.zeros(S, dtype=torch.int64, device=DEV), "done": dev([c["done"] for c in cases], torch.int32)}
    if hist_ld:
        ctl["history"] = torch.full((S, hist_ld), -5, dtype=torch.int64, device=DEV)
    lp = {}
    if scores:
        lp = {"logprob": torch.full((S,), 9.0, device=DEV), "cum_logprob": torch.zeros(S, dtype=torch.float64, device=DEV)}
        if n_top:
            lp["top_ids"] = torch.full((S, n_top), -7, dtype=torch.int64, device=DEV)
            lp["top_logprobs"] = torch.full((S, n_top), 9.0, device=DEV)
        if hist_ld:
            lp["lp_history"] = torch.full((S, hist_ld), 9.0, device=DEV)
            if n_top:
                lp["top_hist_ids"] = torch.full((S, hist_ld, n_top), -7, dtype=torch.int64, device=DEV)
                lp["top_hist_lp"] = torch.full((S, hist_ld, n_top), 9.0, device=DEV)
    tok = torch.full((S, 1), -1, dtype=torch.int64, device=DEV)
    nk, pr = torch.full((S,), -1, dtype=torch.int32, device=DEV), torch.full((S,), -1.0, device=DEV)
    out = []
    for _ in range(steps):
        ops.sample_tokens(lg, *tab, out=tok, n_kept=nk, prob=pr, **ctl, **lp)
        step = {"token": tok[:, 0], "n_kept": nk, "prob": pr}
        step.update({k_: lp[k_] for k_ in ("logprob", "top_ids", "top_logprobs") if k_ in lp})
        out.append({k_: v.cpu().numpy().copy() for k_, v in step.items()})
    torch.cuda.synchronize()
    state = {"counter": tab[4], **{k_: ctl[k_] for k_ in ("seen", "n_new", "done", "history") if k_ in ctl},
             **{k_: v for k_, v in lp.items() if k_ not in ("logprob", "top_ids", "top_logprobs")}}
    return out, {k_: v.cpu().numpy().copy() for k_, v in state.items()}


CTL_KEYS = ("token", "n_kept", "prob")
CTL_STATE = ("counter", "seen", "n_new", "done", "history")


def _same_as_ctl(a, b, where):
    """token, n_kept, prob of every step and counter, seen, n_new, done, history: bit-identical"""
    (out_a, st_a), (out_b, st_b) = a, b
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        for k_ in CTL_KEYS:
            assert x[k_].tobytes() == y[k_].tobytes(), (where, i, k_)
    for k_ in CTL_STATE:
        assert (k_ in st_a) == (k_ in st_b) and (k_ not in st_a or st_a[k_].tobytes() == st_b[k_].tobytes()), (where, k_)


def _judge_steps(cases, n_top, out, where=""):
    """every step of every live row against the reference on the row penalised by the bitmap of that step"""
    seen = [c["seen"].copy() for c in cases]
    for i, step in enumerate(out):
        for s, c in enumerate(cases):
            w = f"{where}{c['name']} n_top={n_top} step {i}"
            if c["done"]:
                assert step["token"][s] == 7 and step["logprob"][s] == 0.0, w
                if n_top:
                    assert (step["top_ids"][s] == -1).all() and (step["top_logprobs"][s] == -INF).all(), w
                continue
            x = generation.penalise(c["x"], seen[s], c["r"])
            logprobs.judge(x, step["token"][s], step["logprob"][s], step["top_ids"][s] if n_top else None,
                           step["top_logprobs"][s] if n_top else None, where=w)
            seen[s][step["token"][s]] = True


def _rows(V):
    """every kind of row at one V: (name, x, sampling / penalty arguments)"""
    q = generation.random_seen(V, 40 + V)
    rows = [_case("random-greedy", sampling.random_row(V, 11)),
            _case("random-sampled", sampling.random_row(V, 12, scale=2.0), tau=0.7, k=50, p=0.9, seed=3),
            _case("all-equal", logprobs.all_equal(V), tau=1.0, seed=4),
            _case("ties-1", logprobs.ties_across(V, 1, 1)),
            _case("ties-5", logprobs.ties_across(V, 5, 2), tau=1.5, seed=5),
            _case("ties-20", logprobs.ties_across(V, 20, 3), tau=0.7, k=3, seed=6),
            _case("nan", logprobs.specials(V, "nan"), tau=0.7, p=0.5, seed=7),
            _case("pinf", logprobs.specials(V, "pinf"), tau=0.7, seed=8),
            _case("ninf-greedy", logprobs.specials(V, "ninf")),
            _case("ninf-sampled", logprobs.specials(V, "ninf"), tau=1.0, seed=9),
            _case("deep-greedy", logprobs.deep(V, 1)),
            _case("deep-sampled", logprobs.deep(V, 2), tau=1.5, k=0, p=0.9, seed=10),
            _case("pen-1.3", sampling.random_row(V, 13), tau=0.7, k=50, p=0.9, seed=11, r=1.3, seen=q),
            _case("pen-0.8-greedy", sampling.random_row(V, 14), r=0.8, seen=q),
            _case("pen-0.8-all-seen", sampling.random_row(V, 15, scale=5.0), tau=1.5, seed=12, r=0.8, seen=np.ones(V, dtype=bool))]
    return [dict(c, name=f"V{V}-{c['name']}") for c in rows]


# ---------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 97, 4099])
def test_operator_every_row_kind_and_n_top(V):
    rows = _rows(V)
    if V >= 4099:                                                     # the wide row does lie below the weight floor
        ref = logprobs.reference(rows[10]["x"])
        assert np.isfinite(ref).all() and (ref < -27.7 - 1.0).sum() > V - 10
    a = call = 0
    sizes = set()
    while a < len(rows):
        S = min((1, 4, 3, 2)[call % 4], len(rows) - a)
        grp = rows[a:a + S]
        ld, shift = _odd_ld(V) + 2 * (call % 3), (0, 1, 5, 8, 3)[call % 5]
        plain = _run(grp, 0, ld, shift, scores=False)
        for n_top in N_TOPS:
            got = _run(grp, n_top, ld, shift)
            _judge_steps(grp, n_top, got[0])
            _same_as_ctl(got, plain, (V, a, n_top))
            for s in range(S):                                        # no ring given: the sum is the one value
                assert got[1]["cum_logprob"][s] == np.float64(got[0][0]["logprob"][s]), (V, a, s)
        sizes.add(S)
        a, call = a + S, call + 1
    assert {1, 4} <= sizes


def test_single_row_of_the_model_vocabulary():
    V = 151936
    q = generation.random_seen(V, 5, frac=0.1)
    for c, n_top in ((_case("V151936-pen", sampling.random_row(V, 21), tau=0.7, k=50, p=0.9, seed=2, r=1.3, seen=q), 20),
                     (_case("V151936-deep-greedy", logprobs.deep(V, 3)), 5),
                     (_case("V151936-ties", logprobs.ties_across(V, 5, 4), tau=1.0, seed=3), 5)):
        got = _run([c], n_top, _odd_ld(V), 3)
        _judge_steps([c], n_top, got[0])
        _same_as_ctl(got, _run([c], 0, _odd_ld(V), 3, scores=False), c["name"])


def test_greedy_and_sampled_rows_mixed_with_finished_rows():
    V = 4099
    grp = [_case("mix-greedy", sampling.random_row(V, 31)),
           _case("mix-finished-1", sampling.random_row(V, 32), tau=0.7, seed=4, done=1),
           _case("mix-sampled", sampling.random_row(V, 33), tau=0.7, k=50, p=0.9, seed=5, r=1.3, seen=generation.random_seen(V, 6)),
           _case("mix-finished-2", sampling.random_row(V, 34), done=2)]
    for n_top in (0, 5):
        got = _run(grp, n_top, _odd_ld(V), 1, hist_ld=4, steps=2)
        _judge_steps(grp, n_top, got[0])
        _same_as_ctl(got, _run(grp, 0, _odd_ld(V), 1, hist_ld=4, steps=2, scores=False), n_top)
        st = got[1]
        assert st["n_new"].tolist() == [2, 0, 2, 0] and st["done"].tolist() == [0, 1, 0, 2]
        for s in (1, 3):                                              # a finished row: no ring write, no sum
            assert st["cum_logprob"][s] == 0.0 and (st["lp_history"][s] == 9.0).all()
            if n_top:
                assert (st["top_hist_ids"][s] == -7).all() and (st["top_hist_lp"][s] == 9.0).all()


def test_group_all_null_is_the_controlled_entry():
    from infinitevl_amd import _lib
    V = 4099
    grp = [c for c in _rows(V) if c["name"].split("-", 1)[1] in ("random-sampled", "pen-1.3", "ties-5", "pen-0.8-greedy")]
    want = _run(grp, 0, _odd_ld(V), 1, scores=False)
    S = len(grp)
    _, lg = _place([c["x"] for c in grp], _odd_ld(V), 1)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)
    tab = [dev([c["tau"] for c in grp], torch.float32), dev([c["k"] for c in grp], torch.int32),
           dev([c["p"] for c in grp], torch.float32), dev([c["seed"] for c in grp], torch.int64),
           torch.zeros(S, dtype=torch.int64, device=DEV)]
    W = generation.words_for(V) + 1
    seen = torch.stack([generation.to_i32(generation.pack(c["seen"], W, beyond=True)) for c in grp]).to(DEV)
    rp, fill = dev([c["r"] for c in grp], torch.float32), dev([7] * S, torch.int64)
    n_new, done = torch.zeros(S, dtype=torch.int64, device=DEV), torch.zeros(S, dtype=torch.int32, device=DEV)
    tok = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    nk, pr = torch.full((S,), -1, dtype=torch.int32, device=DEV), torch.full((S,), -1.0, device=DEV)
    # the score and constraint groups off: their pointers NULL, their scalars (and hist_ld, without a history) set all the same
    ptrs = dict(zip(("temperature", "top_k", "top_p", "seed", "counter"), tab), logits=lg, token=tok, n_kept=nk, prob=pr,
                rep_penalty=rp, seen=seen, fill=fill, n_new=n_new, done=done)
    a = _lib.SampleArgs(ld=lg.stride(0), S=S, V=V, token_stride=1, seen_ld=W, hist_ld=4, mask_ld=W, n_states=3,
                        **{k: t.data_ptr() for k, t in ptrs.items()})
    assert _lib.load().ivl_sample_rows_fwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    got = ([{"token": tok.cpu().numpy(), "n_kept": nk.cpu().numpy(), "prob": pr.cpu().numpy()}],
           {"counter": tab[4].cpu().numpy(), "seen": seen.cpu().numpy(), "n_new": n_new.cpu().numpy(), "done": done.cpu().numpy()})
    _same_as_ctl(got, want, "all-null")


def test_same_call_twice_and_row_alone_equals_row_of_four():
    V = 4099
    rows = {c["name"].split("-", 1)[1]: c for c in _rows(V)}
    grp = [rows["pen-1.3"], rows["ties-20"], rows["deep-sampled"], rows["random-greedy"]]
    a = _run(grp, 20, _odd_ld(V), 1, hist_ld=4, steps=3)
    b = _run(grp, 20, _odd_ld(V), 1, hist_ld=4, steps=3)
    for x, y in zip(a[0], b[0]):
        assert all(x[k_].tobytes() == y[k_].tobytes() for k_ in x)
    assert all(a[1][k_].tobytes() == b[1][k_].tobytes() for k_ in a[1])
    for s in range(4):                                                # alone, in another buffer at another alignment
        alone = _run(grp[s:s + 1], 20, V + 8, 0, hist_ld=4, steps=3)
        for x, y in zip(alone[0], a[0]):
            assert all(x[k_][0].tobytes() == y[k_][s].tobytes() for k_ in x), s
        assert all(alone[1][k_][0].tobytes() == a[1][k_][s].tobytes() for k_ in a[1]), s


def test_rings_wrap_and_the_sum_is_sequential_float64():
    V, H, steps, n_top = 97, 4, 6, 5
    grp = [_case("ring-sampled", sampling.random_row(V, 41, scale=1.0), tau=1.5, seed=6, r=1.3),
           _case("ring-greedy-pen", sampling.random_row(V, 42), r=1.5),      # the penalty moves the arg-max on: distinct tokens
           _case("ring-sampled-k", sampling.random_row(V, 43, scale=1.0), tau=1.0, k=20, seed=7)]
    out, st = _run(grp, n_top, _odd_ld(V), 5, hist_ld=H, steps=steps)
    _judge_steps(grp, n_top, out)
    _same_as_ctl((out, st), _run(grp, 0, _odd_ld(V), 5, hist_ld=H, steps=steps, scores=False), "rings")
    assert st["n_new"].tolist() == [steps] * 3
    for s in range(3):
        cum = np.float64(0.0)
        for i in range(steps):
            cum = cum + np.float64(out[i]["logprob"][s])
        assert st["cum_logprob"][s].tobytes() == cum.tobytes(), s
        for i in range(steps - H, steps):                             # the last H steps, step i at index i % H
            assert st["history"][s, i % H] == out[i]["token"][s]
            assert st["lp_history"][s, i % H].tobytes() == out[i]["logprob"][s].tobytes(), (s, i)
            assert st["top_hist_ids"][s, i % H].tolist() == out[i]["top_ids"][s].tolist(), (s, i)
            assert st["top_hist_lp"][s, i % H].tobytes() == out[i]["top_logprobs"][s].tobytes(), (s, i)
    assert len({out[i]["token"][1] for i in range(steps)}) == steps


# ---------------------------------------------------------------------------------------------
# 2. the graphed decode steps
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
    x = (torch.randn(1, T, hc.hidden_size, generator=g_) * 0.5).to(torch.bfloat16).to(DEV)
    return x, torch.randint(0, hc.vocab_size, (T,), generator=g_, dtype=torch.int64)


PROMPTS = ((130, 5), (70, 6))
HIST, N_LP, N_STEPS = 8, 3, 6
CONTROLS = {0: {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 1234, "repetition_penalty": 1.3},
            1: {"repetition_penalty": 1.5}}


class _Seen:
    """the host's copy of a row's bitmap and the judge of its next token's scores"""

    def __init__(self, V, r, prompt_ids):
        self.seen, self.r = np.zeros(V, dtype=bool), r
        self.seen[prompt_ids.numpy()] = True

    def judge(self, logits_row, token, lp, ids, lps, where):
        logprobs.judge(generation.penalise(logits_row, self.seen, self.r), token, lp, ids, lps, where=str(where))
        self.seen[token] = True


def _multistream(n_logprobs):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=2, device=DEV, dtype=torch.bfloat16)
    return GraphedMultiStreamDecode(stack, cache, sampler=Sampler(2, DEV, vocab_size=hc.vocab_size, history=HIST,
                                                                  logprobs=n_logprobs)), hc


def _latest(smp):
    return smp.logprob.cpu().numpy().copy(), smp.top_ids.cpu().numpy().copy(), smp.top_logprob.cpu().numpy().copy()


def _ms_run(graph, n_logprobs=N_LP, judge=True):
    dec, hc = _multistream(n_logprobs)
    smp, tracks = dec.sampler, {}
    toks = []
    for slot, (T, seed) in enumerate(PROMPTS):
        x, ids = _prompt(hc, T, seed)
        dec.admit(slot, x, sampling=CONTROLS[slot], prompt_ids=ids)
        tracks[slot] = _Seen(hc.vocab_size, CONTROLS[slot].get("repetition_penalty", 1.0), ids)
        if judge:                                                     # the first token is scored by the same launch
            lp, ti, tl = _latest(smp)
            tracks[slot].judge(dec.admit_logits[0, -1].cpu(), dec.token[slot, 0].item(), lp[slot], ti[slot], tl[slot], ("admit", slot))
    toks.append(dec.token[:, 0].tolist())
    for i in range(N_STEPS):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
        if judge:
            lg, (lp, ti, tl) = dec.logits[:, -1].cpu(), _latest(smp)
            for slot, t in tracks.items():
                t.judge(lg[slot], toks[-1][slot], lp[slot], ti[slot], tl[slot], ("graph" if graph else "eager", i, slot))
    return dec, toks


def test_multistream_eager_equals_graph_every_step_judged():
    (dec_g, toks_g), (dec_e, toks_e) = _ms_run(True), _ms_run(False)
    assert toks_g == toks_e
    _, toks_plain = _ms_run(True, n_logprobs=None, judge=False)       # the scores change no token
    assert toks_plain == toks_g
    for slot in (0, 1):
        want = [t[slot] for t in toks_g]
        for dec in (dec_g, dec_e):
            assert dec.sampler.tokens(slot).tolist() == want      # N_STEPS + 1 <= HIST: nothing has wrapped
        lp_g, lp_e = dec_g.sampler.logprobs(slot), dec_e.sampler.logprobs(slot)
        assert lp_g.dtype == torch.float32 and lp_g.shape == (min(HIST, N_STEPS + 1),)
        assert lp_g.numpy().tobytes() == lp_e.numpy().tobytes(), slot
        (ig, lg_), (ie, le) = dec_g.sampler.top_logprobs(slot), dec_e.sampler.top_logprobs(slot)
        assert ig.shape == (lp_g.shape[0], N_LP) and torch.equal(ig, ie) and lg_.numpy().tobytes() == le.numpy().tobytes(), slot
        # the sum over ALL N_STEPS + 1 tokens; the ring holds the last HIST of them
        assert dec_g.sampler.cum_logprob[slot].item() == dec_e.sampler.cum_logprob[slot].item() < 0.0
    assert N_STEPS + 1 <= HIST
    for slot in (0, 1):
        cum = np.float64(0.0)
        for v in dec_g.sampler.logprobs(slot).numpy():
            cum = cum + np.float64(v)
        assert dec_g.sampler.cum_logprob[slot].item() == cum


def test_run_until_done_returns_tokens_with_aligned_logprobs():
    dec, toks = _ms_run(True, judge=False)
    dec2, hc = _multistream(N_LP)
    for slot, (T, seed) in enumerate(PROMPTS):
        x, ids = _prompt(hc, T, seed)
        dec2.admit(slot, x, sampling=dict(CONTROLS[slot], max_new_tokens=N_STEPS + 1), prompt_ids=ids)
    out = dec2.run_until_done(40, poll_every=4)
    for slot in (0, 1):
        assert out[slot].tolist() == [t[slot] for t in toks]
        assert dec2.sampler.logprobs(slot).numpy().tobytes() == dec.sampler.logprobs(slot).numpy().tobytes()
        assert torch.equal(dec2.sampler.top_logprobs(slot)[0], dec.sampler.top_logprobs(slot)[0])
        assert dec2.sampler.logprobs(slot).shape[0] == out[slot].shape[0] == N_STEPS + 1
        # a finished row is not scored again: the sum stays that of its N_STEPS + 1 tokens
        assert dec2.sampler.cum_logprob[slot].item() == dec.sampler.cum_logprob[slot].item()


def test_graphed_decode_batch_two_with_logprobs():
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = _small()
    V = hc.vocab_size
    sp = {0: {"temperature": 1.5, "seed": 42, "repetition_penalty": 1.3}, 1: {"repetition_penalty": 1.5}}
    runs = []
    for graphed in (True, False):
        cache = stack.allocate_inference_cache(2)
        (x0, ids0), (x1, ids1) = _prompt(hc, 64, 31), _prompt(hc, 64, 32)
        with torch.no_grad():
            pid = torch.arange(64, device=DEV)[None, None, :].expand(3, 2, 64)
            _, lg = stack(inputs_embeds=torch.cat([x0, x1]), position_ids=pid, past_key_values=cache, logits_to_keep=1)
        smp = Sampler(2, DEV, vocab_size=V, history=HIST, logprobs=N_LP)
        tracks = {}
        for row, ids in ((0, ids0), (1, ids1)):
            smp.set(row, **sp[row])
            smp.mark(row, ids.to(DEV))
            tracks[row] = _Seen(V, sp[row]["repetition_penalty"], ids)
        dec = GraphedDecode(stack, cache, 2, sampler=smp)
        smp.sample(lg[:, -1], dec.token)
        toks = [dec.token[:, 0].tolist()]
        lp, ti, tl = _latest(smp)
        for row, t in tracks.items():
            t.judge(lg[row, -1].cpu(), toks[0][row], lp[row], ti[row], tl[row], ("b2 first", row))
        for i in range(4):
            if graphed:
                dec.step()
            else:
                with torch.no_grad():
                    dec.logits = dec._run()
                cache.advance(1)
            toks.append(dec.token[:, 0].tolist())
            lp, ti, tl = _latest(smp)
            for row, t in tracks.items():
                t.judge(dec.logits[row, -1].cpu(), toks[-1][row], lp[row], ti[row], tl[row], ("b2", graphed, i, row))
        assert smp.tokens(0).tolist() == [t[0] for t in toks] and smp.logprobs(1).shape == (5,)
        torch.cuda.synchronize()
        runs.append((toks, {k_: v.cpu() for k_, v in smp.state().items()}))
    assert runs[0][0] == runs[1][0]
    for k_ in runs[0][1]:
        assert runs[0][1][k_].numpy().tobytes() == runs[1][1][k_].numpy().tobytes(), k_

"""GPU (-m gpu): per-row sampling (ops.sample_tokens / ivl_sample_rows_fwd) and its use in the graphed decode steps, judged by
tests/sampling.py (float64 reference, derived bounds, builders whose cases carry the top-p margin):

  * operator: every (temperature, top-k, top-p) of the builders at V in {1, 97, 512, 4099, 151936}, mixed rows in calls of 1, 4
    and 6 rows, ld == V, odd ld and unaligned bases, 256 consecutive draws of each row judged one by one;
  * adversarial rows (equal logits, NaN, -inf, +inf, ties at the top-k threshold, the maximum at either end, twice, as +-0);
  * determinism: the same call twice, a row alone and as row 3 of 4, beside a co-running stream;
  * GraphedMultiStreamDecode / GraphedDecode with a Sampler: every token of every live slot judged against the step's logits,
    graph == eager across a capture, parameters changed between replays, sampler=None == the greedy classes."""
import functools

import numpy as np
import pytest
import torch

import parity
import sampling
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DRAWS = 256


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _operator_cases(V):
    return tuple(sampling.operator_cases(V))


@functools.lru_cache(maxsize=None)
def _adversarial_cases():
    return tuple(sampling.adversarial_cases())


def _table(cases):
    return (torch.tensor([c["tau"] for c in cases], dtype=torch.float32, device=DEV),
            torch.tensor([c["k"] for c in cases], dtype=torch.int32, device=DEV),
            torch.tensor([c["p"] for c in cases], dtype=torch.float32, device=DEV),
            torch.tensor([c["seed"] for c in cases], dtype=torch.int64, device=DEV),
            torch.zeros(len(cases), dtype=torch.int64, device=DEV))


def _place(cases, ld, shift):
    """the rows of `cases` in a buffer of +inf (an element read from outside a row would win every draw): row s at element
    shift + s * ld of a 256-byte aligned allocation"""
    S, V = len(cases), cases[0]["x"].shape[0]
    buf = torch.full((shift + S * ld + 8,), float("inf"), dtype=torch.bfloat16, device=DEV)
    lg = buf[shift:shift + S * ld].view(S, ld)[:, :V]
    lg.copy_(torch.stack([c["x"] for c in cases]).to(DEV))
    return buf, lg


def _draws(cases, ld, shift, n_draws, three_dim=False):
    """n_draws consecutive calls on one set of logits -> tokens, n_kept, prob [n_draws, S] and the counters (host)"""
    from infinitevl_amd import ops
    S = len(cases)
    buf, lg = _place(cases, ld, shift)
    tau, k, p, seed, ctr = _table(cases)
    tok = torch.full((n_draws, S), -1, dtype=torch.int64, device=DEV)
    nk = torch.full((n_draws, S), -1, dtype=torch.int32, device=DEV)
    pr = torch.full((n_draws, S), -1.0, dtype=torch.float32, device=DEV)
    for d in range(n_draws):
        out = ops.sample_tokens(lg[:, None] if three_dim else lg, tau, k, p, seed, ctr, out=tok[d], n_kept=nk[d], prob=pr[d])
        assert out.data_ptr() == tok[d].data_ptr()
    torch.cuda.synchronize()
    return tok.cpu().numpy(), nk.cpu().numpy(), pr.cpu().numpy(), ctr.cpu().tolist()


def _judge_rows(cases, tok, nk, pr, ctr):
    n = tok.shape[0]
    for s, c in enumerate(cases):
        sampling.judge(c["x"], c, np.arange(n), tok[:, s], nk[:, s], pr[:, s], where=c["name"])
        assert ctr[s] == (0 if not c["tau"] > 0 else n), (c["name"], ctr[s])


# ---------------------------------------------------------------------------------------------
# 1. operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sampling.OPERATOR_VS)
def test_operator_every_parameter_mix(V):
    cases = _operator_cases(V)
    sizes, lds = (1, 4, 6), (V, V + 3, V + 8, V + 1)              # V + 3 / V + 1: odd ld, so the rows of a call are unaligned
    a = call = 0
    seen_S = set()
    while a < len(cases):
        S = min(sizes[call % 3], len(cases) - a)
        ld, shift = lds[call % 4], (0, 1, 5, 8)[(call // 2) % 4]   # shift: the first row 2-byte aligned only
        rows = cases[a:a + S]
        tok, nk, pr, ctr = _draws(rows, ld, shift, N_DRAWS, three_dim=(call % 5 == 2 and ld == V))
        _judge_rows(rows, tok, nk, pr, ctr)
        seen_S.add(S)
        a, call = a + S, call + 1
    assert {1, 4, 6} <= seen_S


def test_operator_without_optional_outputs_and_new_out():
    from infinitevl_amd import ops
    rows = _operator_cases(4099)[:6]
    _, lg = _place(rows, 4099 + 3, 1)
    tau, k, p, seed, ctr = _table(rows)
    t0 = ops.sample_tokens(lg, tau, k, p, seed, ctr)
    assert t0.shape == (6,) and t0.dtype == torch.int64
    ctr2 = torch.zeros_like(ctr)
    out = torch.full((6, 1), -1, dtype=torch.int64, device=DEV)
    nk, pr = torch.zeros(6, dtype=torch.int32, device=DEV), torch.zeros(6, device=DEV)
    t1 = ops.sample_tokens(lg, tau, k, p, seed, ctr2, out=out, n_kept=nk, prob=pr)
    torch.cuda.synchronize()
    assert t1.data_ptr() == out.data_ptr() and torch.equal(t0, out[:, 0]) and torch.equal(ctr, ctr2)
    for s, c in enumerate(rows):
        sampling.judge(c["x"], c, 0, t0[s].item(), nk[s].item(), pr[s].item(), where=c["name"])


# ---------------------------------------------------------------------------------------------
# 2. adversarial rows
# ---------------------------------------------------------------------------------------------
def test_adversarial_rows():
    cases = _adversarial_cases()
    V = cases[0]["x"].shape[0]
    for a, S, ld, shift in ((0, 6, V + 1, 3), (6, 6, V, 0), (12, 4, V + 8, 1), (16, len(cases) - 16, V + 5, 0)):
        rows = cases[a:a + S]
        tok, nk, pr, ctr = _draws(rows, ld, shift, 64)
        assert ((tok >= 0) & (tok < V)).all(), [c["name"] for c in rows]
        _judge_rows(rows, tok, nk, pr, ctr)
    assert a + S == len(cases)


def test_all_equal_row_at_the_model_vocabulary():
    V = 151936
    x = torch.full((V,), 0.75, dtype=torch.bfloat16)
    rows = [{"name": f"equal-{i}", "x": x, "tau": t, "k": k, "p": p, "seed": 3 + i}
            for i, (t, k, p) in enumerate(((0.7, 0, 1.0), (0.7, 50, 0.9), (0.0, 0, 1.0), (1.5, 0, 0.5)))]
    tok, nk, pr, ctr = _draws(rows, V, 0, 64)
    _judge_rows(rows, tok, nk, pr, ctr)
    assert (nk[:, :2] == V).all() and (tok[:, 2] == 0).all() and len(np.unique(tok[:, 0])) > 32


# ---------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------
def test_same_call_twice_and_row_alone_equals_row_of_four():
    cases = _operator_cases(151936)
    rows = (cases[2], cases[11], cases[0], cases[24])          # row 3 samples with top-k 50 / top-p
    assert rows[3]["tau"] > 0
    a = _draws(rows, 151936 + 3, 1, 32)
    b = _draws(rows, 151936 + 3, 1, 32)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    for s in range(4):                                           # alone, in another buffer at another alignment
        alone = _draws(rows[s:s + 1], 151936, 0, 32)
        assert np.array_equal(alone[0][:, 0], a[0][:, s]) and np.array_equal(alone[1][:, 0], a[1][:, s])
        assert np.array_equal(alone[2][:, 0], a[2][:, s]) and alone[3][0] == a[3][s]


def test_same_tokens_beside_a_co_running_stream():
    cases = _operator_cases(151936)
    rows = cases[20:24]
    quiet = _draws(rows, 151936, 0, 32)
    side = torch.cuda.Stream()
    m = torch.randn(2048, 2048, device=DEV, dtype=torch.bfloat16)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(200):
            m = (m @ m).clamp_(-1, 1)
    busy = _draws(rows, 151936, 0, 32)
    side.synchronize()
    for x, y in zip(quiet, busy):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


# ---------------------------------------------------------------------------------------------
# 4. the graphed decode steps
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


SAMPLING = {0: {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 1234},
            1: {},                                                             # greedy
            2: {"temperature": 1.5, "top_k": 0, "top_p": 1.0, "seed": -77}}


def _judge_step(dec, live, draws, where):
    """live: {slot: Sampler.set arguments}; draws: {slot: draws made before this token}.  Judged against dec.logits; a row
    whose logits lack the top-p margin has its n_kept left to the operator tests, never its token."""
    lg = dec.logits[:, -1].cpu()
    toks = dec.token[:, 0].tolist()
    for slot, sp in live.items():
        params = {"tau": sp.get("temperature", 0.0), "k": sp.get("top_k", 0), "p": sp.get("top_p", 1.0), "seed": sp.get("seed", 0)}
        ref = sampling.reference(lg[slot], params["tau"], params["k"], params["p"])
        if ref.greedy:
            assert toks[slot] == ref.argmax == int(lg[slot].float().argmax()), (where, slot)
        else:
            _judge_token(ref, params, draws[slot], toks[slot], (where, slot))
            draws[slot] += 1


def _judge_token(ref, params, ctr, token, where):
    """sampling.judge on logits the model made: like a builder's case they must carry the top-p margin, and the run is
    deterministic (fixed weights, prompts and seeds; integer sampling), so the prompts' seeds are chosen such that they do"""
    assert ref.margin >= sampling.MARGIN, f"{where}: logits without the top-p margin ({ref.margin:.3e}): choose another prompt seed"
    sampling.judge(ref, params, ctr, token, where=str(where))


def _multistream(sampler_on):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=3, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(3, DEV) if sampler_on else None
    return GraphedMultiStreamDecode(stack, cache, sampler=smp), hc


def test_multistream_sampled_streams_join_and_leave():
    dec, hc = _multistream(True)
    live, draws, seq = {}, {}, {s: [] for s in range(3)}

    def admit(slot, T, seed, via_admit):
        sp = SAMPLING[slot]
        if via_admit:
            dec.admit(slot, _prompt(hc, T, seed), sampling=sp or None)
        else:
            dec.sampler.set(slot, **sp)
            dec.admit(slot, _prompt(hc, T, seed))
        live[slot], draws[slot] = sp, 0
        lg = dec.admit_logits                                     # the prompt's first token: one row of the table
        params = {"tau": sp.get("temperature", 0.0), "k": sp.get("top_k", 0), "p": sp.get("top_p", 1.0), "seed": sp.get("seed", 0)}
        ref = sampling.reference(lg[0, -1].cpu(), params["tau"], params["k"], params["p"])
        tok = dec.token[slot, 0].item()
        if ref.greedy:
            assert tok == ref.argmax
        else:
            _judge_token(ref, params, 0, tok, ("admit", slot))
            draws[slot] = 1

    def steps(n, where):
        for i in range(n):
            dec.step()
            _judge_step(dec, live, draws, (where, i))
            for s in live:
                seq[s].append(dec.token[s, 0].item())

    admit(0, 130, 5, True)
    admit(1, 70, 6, True)
    steps(5, "a")
    admit(2, 97, 7, False)
    steps(6, "b")
    dec.release(0)
    live.pop(0)
    assert dec.sampler.temperature[0].item() == 0.0 and dec.sampler.counter[0].item() == 0
    steps(3, "c")
    admit(0, 50, 8, True)
    steps(5, "d")
    torch.cuda.synchronize()
    assert dec.sampler.counter.tolist() == [draws[0], 0, draws[2]] and draws[2] == 1 + 6 + 3 + 5
    assert len(set(seq[2])) > 4                                   # tau = 1.5 on 512 tokens: not a constant stream


def test_multistream_graph_equals_eager_across_a_capture():
    runs = []
    for graph in (True, False):
        dec, hc = _multistream(True)
        for slot, (T, seed) in enumerate(((130, 5), (70, 6), (97, 7))):
            dec.admit(slot, _prompt(hc, T, seed), sampling=SAMPLING[slot] or None)
        toks = [dec.token[:, 0].tolist()]
        for _ in range(16):                                       # graph: the first step captures (warm-up + capture draw too)
            dec.step(graph=graph)
            toks.append(dec.token[:, 0].tolist())
        torch.cuda.synchronize()
        runs.append((toks, dec.sampler.counter.tolist()))
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1] == [17, 0, 17]


def test_parameter_change_between_replays_needs_no_recapture():
    dec, hc = _multistream(True)
    for slot, (T, seed) in enumerate(((130, 5), (70, 6), (97, 7))):
        dec.admit(slot, _prompt(hc, T, seed))                     # all greedy
    live, draws = {0: {}, 1: {}, 2: {}}, {0: 0, 1: 0, 2: 0}
    for i in range(3):
        dec.step()
        _judge_step(dec, live, draws, ("greedy", i))
    graph = dec.graph
    assert graph is not None and dec.sampler.counter.tolist() == [0, 0, 0]
    live[1] = {"temperature": 1.5, "top_k": 0, "top_p": 1.0, "seed": 99}
    dec.sampler.set(1, **live[1])
    picked = []
    for i in range(8):
        dec.step()
        _judge_step(dec, live, draws, ("sampled", i))
        picked.append(dec.token[1, 0].item() != int(dec.logits[1, -1].float().argmax()))
    assert dec.graph is graph and dec.sampler.counter.tolist() == [0, 8, 0]
    assert any(picked)                                            # tau = 1.5: not the arg-max every time
    dec.sampler.reset(1)
    live[1] = {}
    for i in range(2):
        dec.step()
        _judge_step(dec, live, draws, ("greedy again", i))
    assert dec.graph is graph


def test_graphed_decode_batch_two_with_sampler():
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = _small()
    sp = {0: {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 42}, 1: {}}
    runs = []
    for graphed in (True, False):
        cache = stack.allocate_inference_cache(2)
        x = torch.cat([_prompt(hc, 64, 31), _prompt(hc, 64, 32)])
        with torch.no_grad():
            pid = torch.arange(64, device=DEV)[None, None, :].expand(3, 2, 64)
            _, lg = stack(inputs_embeds=x, position_ids=pid, past_key_values=cache, logits_to_keep=1)
        smp = Sampler(2, DEV)
        smp.set(0, **sp[0])
        dec = GraphedDecode(stack, cache, 2, sampler=smp)
        smp.sample(lg[:, -1], dec.token)
        draws, toks = {0: 1, 1: 0}, [dec.token[:, 0].tolist()]
        for i in range(8):
            if graphed:
                dec.step()
            else:
                with torch.no_grad():
                    dec.logits = dec._run()
                cache.advance(1)
            _judge_step(dec, sp, draws, ("b2", graphed, i))
            toks.append(dec.token[:, 0].tolist())
        torch.cuda.synchronize()
        assert smp.counter.tolist() == [9, 0]
        runs.append(toks)
    assert runs[0] == runs[1]


def test_sampler_none_is_the_greedy_path():
    from infinitevl_amd.harness import Sampler
    outs = []
    for mode in ("none", "greedy-sampler"):
        dec, hc = _multistream(mode != "none")
        assert (dec.sampler is None) == (mode == "none")
        for slot, (T, seed) in enumerate(((130, 5), (70, 6), (97, 7))):
            dec.admit(slot, _prompt(hc, T, seed))
        toks = [dec.token[:, 0].tolist()]
        for _ in range(10):
            dec.step()
            lg = dec.logits[:, -1]
            if mode == "none":
                assert dec.token[:, 0].tolist() == lg.argmax(-1).tolist()
            toks.append(dec.token[:, 0].tolist())
        outs.append(toks)
    # a table left greedy draws the lowest-index arg-max: the tokens of the torch path wherever the maximum is unique
    assert outs[0] == outs[1]
    with pytest.raises(ValueError, match="sampler"):
        _multistream(False)[0].admit(0, _prompt(_small()[1], 8, 1), sampling={"temperature": 1.0})
    with pytest.raises(ValueError, match="rows"):
        from infinitevl_amd.cache import MultiStreamCache
        from infinitevl_amd.harness import GraphedMultiStreamDecode
        stack, hc = _small()
        GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=3, device=DEV, dtype=torch.bfloat16),
                                 sampler=Sampler(2, DEV))

"""GPU (-m gpu): the generation controls of the sampling launch (ops.sample_tokens keywords / the controls of ivl_sample_rows_fwd,
ops.mark_tokens) and their use in the graphed decode steps, judged by tests/generation.py: the float64 reference and the bounds
of tests/sampling.py on the penalised bf16 row, integer bookkeeping compared exactly.

  * fixed bitmaps: r in {1.3, 0.8} x every (temperature, top-k, top-p) of the builders at V in {1, 97, 4099}, a quarter / all /
    none of the bits set, calls of 1 and 4 rows in a +inf surround at odd ld and shifted bases, bitmap rows of ceil(V/32) + 1
    words whose guard word and bits >= V are preset to ones; 32 draws per row, each judged; the bitmap after a call = before + the
    token's bit;
  * evolving bitmaps: a greedy chain of 16 distinct tokens, 32 sampled draws judged against the host-tracked set;
  * equivalence: r = 1 with a bitmap, and every group off, against the control-free call bit for bit; a row alone and as row 3
    of 4; the same call twice;
  * stop ids, budget, n_new, the history ring and its wrap, finished rows; mark_tokens;
  * GraphedMultiStreamDecode / GraphedDecode with a controlled Sampler: eager == replayed graph across a capture, capture() leaves
    the control state alone, every live token judged, controls changed between replays, run_until_done."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import generation
import parity
import sampling
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DRAWS = 32
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _fixed_cases(V):
    return tuple(generation.fixed_cases(V))


def _odd_ld(V):
    return (V + 3) | 1


def _table(cases):
    return (torch.tensor([c["tau"] for c in cases], dtype=torch.float32, device=DEV),
            torch.tensor([c["k"] for c in cases], dtype=torch.int32, device=DEV),
            torch.tensor([c["p"] for c in cases], dtype=torch.float32, device=DEV),
            torch.tensor([c["seed"] for c in cases], dtype=torch.int64, device=DEV),
            torch.zeros(len(cases), dtype=torch.int64, device=DEV))


def _place(rows, ld, shift):
    """rows (bf16 [V] each) in a buffer of +inf (an element read from outside a row would win every draw): row s at element
    shift + s * ld of a 256-byte aligned allocation"""
    S, V = len(rows), rows[0].shape[0]
    buf = torch.full((shift + S * ld + 8,), INF, dtype=torch.bfloat16, device=DEV)
    lg = buf[shift:shift + S * ld].view(S, ld)[:, :V]
    lg.copy_(torch.stack(list(rows)).to(DEV))
    return buf, lg


def _bitmap(seens, V):
    """[S, ceil(V/32) + 1] int32 on the device: the guard word and the bits >= V are ones"""
    W = generation.words_for(V) + 1
    host = np.stack([generation.pack(s, W, beyond=True) for s in seens])
    return torch.stack([generation.to_i32(h) for h in host]).to(DEV), host


def _fixed_draws(cases, ld, shift, n_draws):
    """n_draws calls on one set of logits, the bitmap restored before each -> tokens, n_kept, prob [n_draws, S], the counters and
    the bitmap after every call (host)"""
    from infinitevl_amd import ops
    S, V = len(cases), cases[0]["x"].shape[0]
    _, lg = _place([c["x"] for c in cases], ld, shift)
    tau, k, p, seed, ctr = _table(cases)
    rp = torch.tensor([c["r"] for c in cases], dtype=torch.float32, device=DEV)
    saved, saved_host = _bitmap([c["seen"] for c in cases], V)
    seen = saved.clone()
    tok = torch.full((n_draws, S), -1, dtype=torch.int64, device=DEV)
    nk = torch.full((n_draws, S), -1, dtype=torch.int32, device=DEV)
    pr = torch.full((n_draws, S), -1.0, dtype=torch.float32, device=DEV)
    after = torch.zeros((n_draws,) + tuple(seen.shape), dtype=torch.int32, device=DEV)
    for d in range(n_draws):
        seen.copy_(saved)
        ops.sample_tokens(lg, tau, k, p, seed, ctr, out=tok[d], n_kept=nk[d], prob=pr[d], rep_penalty=rp, seen=seen)
        after[d].copy_(seen)
    torch.cuda.synchronize()
    return (tok.cpu().numpy(), nk.cpu().numpy(), pr.cpu().numpy(), ctr.cpu().tolist(),
            after.cpu().numpy().view(np.uint32), saved_host)


def _judge_fixed(cases, tok, nk, pr, ctr, after, saved_host):
    n = tok.shape[0]
    for s, c in enumerate(cases):
        generation.judge(c, np.arange(n), tok[:, s], nk[:, s], pr[:, s])
        assert ctr[s] == (0 if not c["tau"] > 0 else n), (c["name"], ctr[s])
        for d in range(n):                                        # the saved row with only the token's bit added
            want = saved_host[s].copy()
            want[tok[d, s] >> 5] |= np.uint32(1) << np.uint32(tok[d, s] & 31)
            assert np.array_equal(after[d, s], want), (c["name"], d, int(tok[d, s]))


# ---------------------------------------------------------------------------------------------
# 1. fixed bitmaps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", generation.FIXED_VS)
def test_fixed_bitmaps_every_parameter_mix(V):
    cases = _fixed_cases(V)
    a = call = 0
    sizes = set()
    while a < len(cases):
        S = min((1, 4)[call % 2], len(cases) - a)
        rows = cases[a:a + S]
        out = _fixed_draws(rows, _odd_ld(V) + 2 * (call % 3), (0, 1, 5, 8)[call % 4], N_DRAWS)
        _judge_fixed(rows, *out)
        sizes.add(S)
        a, call = a + S, call + 1
    assert {1, 4} <= sizes


def test_special_values_keep_their_class():
    c = generation.special_row()
    rows = [c, dict(c, tau=0.0, name="special-greedy"), dict(c, r=0.8, name="special-0.8"), dict(c, k=5, p=0.9, name="special-kp")]
    for r_ in rows:
        ref = generation.reference(r_["x"], r_["seen"], r_["r"], r_["tau"], r_["k"], r_["p"])
        assert ref.greedy or ref.margin >= sampling.MARGIN
    out = _fixed_draws(rows, _odd_ld(97), 5, N_DRAWS)
    _judge_fixed(rows, *out)
    assert set(np.unique(out[0])) <= {2, 3}                      # the two +inf tokens, seen or not


# ---------------------------------------------------------------------------------------------
# 2. evolving bitmaps
# ---------------------------------------------------------------------------------------------
def _evolve(x, r, tau, seed, n, seen0):
    from infinitevl_amd import ops
    V = x.shape[0]
    _, lg = _place([x], _odd_ld(V), 1)
    case = {"name": "evolving", "x": x, "seen": seen0, "r": r, "tau": tau, "k": 0, "p": 1.0, "seed": seed}
    tab = _table([case])
    rp = torch.tensor([r], dtype=torch.float32, device=DEV)
    seen, _ = _bitmap([seen0], V)
    tok = torch.full((n, 1), -1, dtype=torch.int64, device=DEV)
    for d in range(n):
        ops.sample_tokens(lg, *tab, out=tok[d], rep_penalty=rp, seen=seen)
    torch.cuda.synchronize()
    return case, tok[:, 0].tolist(), seen.cpu().numpy().view(np.uint32)[0], tab[4].item()


def test_evolving_bitmap_greedy_chain():
    x = sampling.random_row(4099, 5)
    chain = generation.greedy_chain(x, 1.5, 16)
    assert len(set(chain)) == 16
    _, toks, words, ctr = _evolve(x, 1.5, 0.0, 0, 16, np.zeros(4099, dtype=bool))
    assert toks == chain and ctr == 0
    want = np.zeros(4099, dtype=bool)
    want[chain] = True
    assert np.array_equal(words, generation.pack(want, generation.words_for(4099) + 1, beyond=True))


def test_evolving_bitmap_sampled_draws():
    x = sampling.random_row(4099, 6, scale=2.0)
    seen = generation.random_seen(4099, 8, frac=0.05)
    case, toks, words, ctr = _evolve(x, 1.3, 0.7, 21, N_DRAWS, seen.copy())
    assert ctr == N_DRAWS
    for d, t in enumerate(toks):                                  # p = 1: no top-p boundary, every draw is judged
        generation.judge(case, d, t, seen_bool=seen, where=f"evolving draw {d}")
        seen[t] = True
    assert np.array_equal(words, generation.pack(seen, generation.words_for(4099) + 1, beyond=True))
    assert len(set(toks)) > 8


# ---------------------------------------------------------------------------------------------
# 3. equivalence and determinism
# ---------------------------------------------------------------------------------------------
def _plain_draws(cases, ld, shift, n, how):
    """how: "old" = ops.sample_tokens without controls, "r1" = rep_penalty 1 with a bitmap, "null" = the entry point on an
    ivl_sample_args whose three groups are off -- every pointer NULL but `fill`, every scalar of theirs set all the same"""
    from infinitevl_amd import _lib, ops
    S, V = len(cases), cases[0]["x"].shape[0]
    _, lg = _place([c["x"] for c in cases], ld, shift)
    tab = _table(cases)
    tok = torch.full((n, S), -1, dtype=torch.int64, device=DEV)
    nk = torch.full((n, S), -1, dtype=torch.int32, device=DEV)
    pr = torch.full((n, S), -1.0, dtype=torch.float32, device=DEV)
    seen, _ = _bitmap([np.ones(V, dtype=bool)] * S, V)
    rp = torch.ones(S, dtype=torch.float32, device=DEV)
    fill = torch.full((S,), 7, dtype=torch.int64, device=DEV)
    for d in range(n):
        if how == "old":
            ops.sample_tokens(lg, *tab, out=tok[d], n_kept=nk[d], prob=pr[d])
        elif how == "r1":
            ops.sample_tokens(lg, *tab, out=tok[d], n_kept=nk[d], prob=pr[d], rep_penalty=rp, seen=seen)
        else:
            ptrs = dict(zip(("temperature", "top_k", "top_p", "seed", "counter"), tab), logits=lg, token=tok[d], n_kept=nk[d],
                        prob=pr[d], fill=fill)
            a = _lib.SampleArgs(ld=lg.stride(0) if S > 1 else V, S=S, V=V, token_stride=1, seen_ld=generation.words_for(V), hist_ld=4,
                                mask_ld=generation.words_for(V), n_states=3, **{k: t.data_ptr() for k, t in ptrs.items()})
            assert _lib.load().ivl_sample_rows_fwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return tok.cpu().numpy(), nk.cpu().numpy(), pr.cpu().numpy(), tab[4].cpu().tolist()


def test_r1_and_all_null_equal_the_control_free_entry_point():
    plain = [dict(c, r=1.0, seen=np.ones(4099, dtype=bool)) for c in sampling.operator_cases(4099)[:8:2] + _adv()]
    for a in range(0, len(plain), 4):
        rows = plain[a:a + 4]
        old = _plain_draws(rows, _odd_ld(4099), 1, N_DRAWS, "old")
        for how in ("r1", "null"):
            new = _plain_draws(rows, _odd_ld(4099), 1, N_DRAWS, how)
            for x, y in zip(old, new):
                assert np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y, (how, a)


def _adv():
    adv = {c["name"]: c for c in sampling.adversarial_cases()}
    return [adv[n] for n in ("adv-nan-mixed-topk-topp", "adv-ties-at-topk-topp", "adv-signed-zero-max", "adv-deep-tail-topp")]


def test_same_call_twice_and_row_alone_equals_row_of_four():
    cases = _fixed_cases(4099)
    rows = (cases[3], cases[0], cases[30], cases[11])
    assert rows[3]["tau"] > 0 and rows[3]["k"] == 50 and rows[3]["p"] < 1
    a = _fixed_draws(rows, _odd_ld(4099), 1, N_DRAWS)
    b = _fixed_draws(rows, _odd_ld(4099), 1, N_DRAWS)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    for s in range(4):                                            # alone, in another buffer at another alignment
        alone = _fixed_draws(rows[s:s + 1], 4099 + 8, 0, N_DRAWS)
        for i in range(3):
            assert np.array_equal(alone[i][:, 0], a[i][:, s]), (s, i)
        assert alone[3][0] == a[3][s] and np.array_equal(alone[4][:, 0], a[4][:, s])


# ---------------------------------------------------------------------------------------------
# 4. stop ids, budget, history, finished rows
# ---------------------------------------------------------------------------------------------
def test_stop_ids_budget_history_and_finished_rows():
    """Four rows whose token of each call is known: the call's logits have one peak per row, 20 above the rest (rows 1 and 3 sample
    at temperature 0.05: every other weight is exp(-400) = 0 in Q40, the draw is the peak and the counter moves)."""
    from infinitevl_amd import ops
    V, H, n_calls = 97, 4, 9
    plan = [[5, 6, 7, 8, 9, 10, 11, 12, 13],           # row 0 greedy: stop ids {-1, 8, 96}: done 1 at call 3
            [40, 41, 42, 43, 44, 45, 46, 47, 48],      # row 1 sampled: budget 3: done 2 at call 2
            [70, 96, 72, 73, 74, 75, 76, 77, 78],      # row 2 greedy: budget 2 and stop id 96 on the same token: done 1
            [1, 2, 3, 4, 1, 2, 0, 95, 33]]             # row 3 sampled: no stop, no budget: runs on, the history wraps twice
    stops = [[-1, 8, 96], [-1, -1, -1], [96, -1, -1], [-1, -1, -1]]
    budgets, fills = [-1, 3, 2, -1], [90, 91, 0, 93]
    books = [generation.Book(V, stops[s], budgets[s], fills[s], H) for s in range(4)]
    base = (torch.randn(4, V, generator=torch.Generator().manual_seed(3)) * 0.5).to(torch.bfloat16)
    tau = torch.tensor([0.0, 0.05, 0.0, 0.05], device=DEV)
    k, p = torch.zeros(4, dtype=torch.int32, device=DEV), torch.ones(4, device=DEV)
    seed, ctr = torch.arange(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    seen, _ = _bitmap([np.zeros(V, dtype=bool)] * 4, V)
    ctl = {"stop_ids": torch.tensor(stops, dtype=torch.int64, device=DEV), "budget": torch.tensor(budgets, dtype=torch.int64, device=DEV),
           "fill": torch.tensor(fills, dtype=torch.int64, device=DEV), "n_new": torch.zeros(4, dtype=torch.int64, device=DEV),
           "done": torch.zeros(4, dtype=torch.int32, device=DEV), "history": torch.full((4, H), -5, dtype=torch.int64, device=DEV),
           "seen": seen}
    tok = torch.full((4, 1), -1, dtype=torch.int64, device=DEV)
    nk, pr = torch.full((4,), -1, dtype=torch.int32, device=DEV), torch.full((4,), -1.0, device=DEV)
    draws = [0, 0, 0, 0]
    for call in range(n_calls):
        rows = base.clone()
        for s in range(4):
            rows[s, plan[s][call]] = 20.0
        _, lg = _place(list(rows), _odd_ld(V), 1)
        ops.sample_tokens(lg, tau, k, p, seed, ctr, out=tok, n_kept=nk, prob=pr, **ctl)
        torch.cuda.synchronize()
        for s, b in enumerate(books):
            if b.done:                                            # finished on entry: the fill token, nothing else moves
                assert (tok[s, 0].item(), nk[s].item(), pr[s].item()) == (fills[s], 0, 0.0), (call, s)
            else:
                kept = V if s in (1, 3) else 1                    # a sampled row keeps all V (the others at weight 0)
                assert (tok[s, 0].item(), nk[s].item(), pr[s].item()) == (plan[s][call], kept, 1.0), (call, s)
                b.push(plan[s][call])
                draws[s] += 1 if s in (1, 3) else 0
        assert ctl["done"].tolist() == [b.done for b in books], call
        assert ctl["n_new"].tolist() == [b.n_new for b in books], call
        assert ctr.tolist() == draws, call
        hist = ctl["history"].tolist()
        for s, b in enumerate(books):
            assert hist[s][:min(b.n_new, H)] == b.history[:min(b.n_new, H)] and hist[s][b.n_new:] == [-5] * max(0, H - b.n_new), (call, s)
        words = seen.cpu().numpy().view(np.uint32)
        for s, b in enumerate(books):
            assert np.array_equal(words[s], generation.pack(b.seen, generation.words_for(V) + 1, beyond=True)), (call, s)
    assert [b.done for b in books] == [1, 2, 1, 0] and [b.n_new for b in books] == [4, 3, 2, 9]
    assert books[3].history == [33, 2, 0, 95]
    # done without fill fills with 0; done alone is a legal control set
    done = torch.tensor([0, 1, 0, 2], dtype=torch.int32, device=DEV)
    ops.sample_tokens(lg, tau, k, p, seed, ctr, out=tok, done=done)
    assert tok[:, 0].tolist() == [plan[0][-1], 0, plan[2][-1], 0] and done.tolist() == [0, 1, 0, 2] and ctr.tolist() == draws


# ---------------------------------------------------------------------------------------------
# 5. mark_tokens
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [97, 4099])
def test_mark_tokens(V):
    from infinitevl_amd import ops
    W = generation.words_for(V)
    g = np.random.default_rng(V)
    first = g.integers(0, 2 ** 32, size=W + 2, dtype=np.uint64).astype(np.uint32)
    first[:W] &= generation.pack(generation.random_seen(V, 3, 0.1), W, beyond=False)         # bits >= V of the row start as zeros
    buf = generation.to_i32(first).to(DEV)
    row = buf[:W]                                                 # two guard words behind it
    ids = g.integers(-20, V + 80, size=3000 if V > 97 else 150)
    ids = np.concatenate([ids, [0, V - 1, V, -1, W * 32, W * 32 + 3, 2 ** 40, -2 ** 40, V - 1, 0]])   # the ends, duplicates, far outside
    want = generation.unpack(first)
    inside = ids[(ids >= 0) & (ids < V)]
    assert 0 < np.unique(inside).size < inside.size               # duplicates among them
    want[inside] = True
    ops.mark_tokens(row, torch.from_numpy(ids).to(DEV), V)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), generation.pack(want, W + 2, beyond=False))
    before = buf.clone()
    ops.mark_tokens(row, torch.zeros(0, dtype=torch.int64, device=DEV), V)                    # n = 0
    ops.mark_tokens(row, torch.tensor([[V, -3]], dtype=torch.int64, device=DEV), V)          # nothing inside
    assert torch.equal(buf, before)


# ---------------------------------------------------------------------------------------------
# 6. the graphed decode steps
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


PROMPTS = ((130, 5), (70, 6), (97, 7))
HIST = 32


def _controls(stop_id):
    """slot 0 samples with top-k / top-p under a penalty and ends on `stop_id`; slot 1 is greedy under a penalty with a budget of
    6; slot 2 samples at temperature 1.5 with a boosting penalty (< 1) and runs on"""
    return {0: {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 1234, "repetition_penalty": 1.3,
                "stop_token_ids": [] if stop_id is None else [stop_id], "fill_token": 3},
            1: {"repetition_penalty": 1.5, "max_new_tokens": 6, "fill_token": 4},
            2: {"temperature": 1.5, "seed": -77, "repetition_penalty": 0.8}}


class _Track:
    """the host's copy of a slot: its seen set and bookkeeping, and the judge of its next token"""

    def __init__(self, V, sp, prompt_ids):
        seen0 = np.zeros(V, dtype=bool)
        seen0[prompt_ids.numpy()] = True
        self.sp = sp
        self.book = generation.Book(V, sp.get("stop_token_ids", ()), sp.get("max_new_tokens") or -1, sp.get("fill_token", 0), HIST, seen0)
        self.draws = 0

    def judge(self, logits_row, token, where):
        if self.book.done:
            assert token == self.book.fill, where
            return
        sp = self.sp
        case = {"name": str(where), "x": logits_row, "seen": self.book.seen, "r": sp.get("repetition_penalty", 1.0),
                "tau": sp.get("temperature", 0.0), "k": sp.get("top_k", 0), "p": sp.get("top_p", 1.0), "seed": sp.get("seed", 0)}
        ref = generation.reference(case["x"], case["seen"], case["r"], case["tau"], case["k"], case["p"])
        # like a builder's case, logits the model made must carry the top-p margin: the run is deterministic (fixed weights,
        # prompts and seeds; integer sampling), so the prompts' seeds are chosen such that they do
        assert ref.greedy or ref.margin >= sampling.MARGIN, f"{where}: logits without the top-p margin ({ref.margin:.3e})"
        generation.judge(case, self.draws, token, where=str(where))
        self.draws += 0 if ref.greedy else 1
        self.book.push(token)


def _multistream(hist=HIST):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=3, device=DEV, dtype=torch.bfloat16)
    return GraphedMultiStreamDecode(stack, cache, sampler=Sampler(3, DEV, vocab_size=hc.vocab_size, history=hist)), hc


def _admit_all(dec, hc, controls, judge=True):
    tracks = {}
    for slot, (T, seed) in enumerate(PROMPTS):
        x, ids = _prompt(hc, T, seed)
        dec.admit(slot, x, sampling=controls[slot], prompt_ids=ids if slot != 1 else ids[None])
        tracks[slot] = _Track(hc.vocab_size, controls[slot], ids)
        if judge:
            tracks[slot].judge(dec.admit_logits[0, -1].cpu(), dec.token[slot, 0].item(), ("admit", slot))
    return tracks


def _state(smp):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in smp.state().items()}


def _check_books(smp, tracks, where):
    st = _state(smp)
    V = smp.vocab_size
    for slot, t in tracks.items():
        b = t.book
        assert (st["done"][slot].item(), st["n_new"][slot].item(), st["counter"][slot].item()) == (b.done, b.n_new, t.draws), (where, slot)
        assert st["history"][slot, :min(b.n_new, HIST)].tolist() == b.history[:min(b.n_new, HIST)], (where, slot)
        assert np.array_equal(st["seen"][slot].numpy().view(np.uint32), generation.pack(b.seen, generation.words_for(V), False)), (where, slot)


def _run(graph, stop_id, n_steps, judge=True, explicit_capture=False):
    dec, hc = _multistream()
    tracks = _admit_all(dec, hc, _controls(stop_id), judge)
    if explicit_capture:
        before = _state(dec.sampler)
        dec.capture()
        after = _state(dec.sampler)
        assert set(before) == {"counter", "seen", "n_new", "done", "history"}
        for k_ in before:                                         # the warm-up and the capture drew tokens: all of it is restored
            assert torch.equal(before[k_], after[k_]), k_
    toks = [dec.token[:, 0].tolist()]
    for i in range(n_steps):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
        if judge:
            lg = dec.logits[:, -1].cpu()
            for slot, t in tracks.items():
                t.judge(lg[slot], toks[-1][slot], ("graph" if graph else "eager", i, slot))
    if judge:
        _check_books(dec.sampler, tracks, "end")
    return dec, hc, tracks, toks, _state(dec.sampler)


@functools.lru_cache(maxsize=None)
def _stop_id():
    """the 5th token of slot 0 in an eager dry run without a stop id"""
    _, _, _, toks, _ = _run(False, None, 4, judge=False)
    return toks[4][0]


def test_multistream_eager_equals_graph_with_three_controlled_slots():
    stop = _stop_id()
    runs = [_run(graph, stop, 12, explicit_capture=graph) for graph in (True, False)]
    (dec, hc, tracks, toks_g, st_g), (_, _, _, toks_e, st_e) = runs
    assert toks_g == toks_e
    for k_ in st_g:
        assert torch.equal(st_g[k_], st_e[k_]), k_
    first = [t[0] for t in toks_g].index(stop)                   # the stream ends where the stop id first appears
    assert first <= 4 and tracks[0].book.done == 1 and tracks[0].book.n_new == first + 1
    assert [t[0] for t in toks_g[first + 1:]] == [3] * (12 - first)
    assert tracks[1].book.done == 2 and tracks[1].book.n_new == 6 and [t[1] for t in toks_g[6:]] == [4] * 7
    assert tracks[2].book.done == 0 and tracks[2].book.n_new == 13
    # the controls of a slot change between replays, without a recapture
    graph = dec.graph
    sp = {"repetition_penalty": 1.3, "stop_token_ids": [7, 9], "max_new_tokens": 3, "fill_token": 11}
    dec.sampler.set(2, **sp)
    tracks[2] = _Track(hc.vocab_size, sp, torch.zeros(0, dtype=torch.int64))
    for i in range(5):
        dec.step()
        lg = dec.logits[:, -1].cpu()
        for slot, t in tracks.items():
            t.judge(lg[slot], dec.token[slot, 0].item(), ("changed", i, slot))
    assert dec.graph is graph and tracks[2].book.done in (1, 2) and dec.token[2, 0].item() == 11
    _check_books(dec.sampler, tracks, "changed")
    dec.release(2)
    st = _state(dec.sampler)
    assert (st["done"][2].item(), st["n_new"][2].item(), int(st["seen"][2].abs().sum()), int(st["history"][2].abs().sum())) == (0, 0, 0, 0)
    assert dec.sampler.rep_penalty[2].item() == 1.0 and dec.sampler.budget[2].item() == -1


def test_run_until_done_returns_the_tokens_of_the_step_loop():
    stop = _stop_id()
    _, _, tracks, toks, _ = _run(True, stop, 12, judge=True)
    dec, hc = _multistream()
    _admit_all(dec, hc, _controls(stop), judge=False)
    out = dec.run_until_done(40, poll_every=4)
    done, n_new = dec.sampler.poll()
    assert done.tolist() == [1, 2, 0] and set(out) == {0, 1, 2}
    steps = n_new[2].item() - 1                                   # slot 2 runs on: one token per step after the admission's
    assert steps % 4 == 0 and 4 <= steps <= 8                     # polled every 4 steps; both ends fall within 5 steps
    for slot in (0, 1):
        b = tracks[slot].book
        assert out[slot].tolist() == b.history[:b.n_new], slot
    assert out[2].tolist() == [t[2] for t in toks[:steps + 1]]
    assert dec.run_until_done(0).keys() == out.keys()
    with pytest.raises(ValueError, match="history"):
        _multistream(hist=0)[0].run_until_done(4)


def test_graphed_decode_batch_two_with_controls():
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = _small()
    V = hc.vocab_size
    sp = {0: {"temperature": 1.5, "seed": 42, "repetition_penalty": 1.3, "max_new_tokens": 5, "fill_token": 2},
          1: {"repetition_penalty": 1.5}}
    runs = []
    for graphed in (True, False):
        cache = stack.allocate_inference_cache(2)
        (x0, ids0), (x1, ids1) = _prompt(hc, 64, 31), _prompt(hc, 64, 32)
        with torch.no_grad():
            pid = torch.arange(64, device=DEV)[None, None, :].expand(3, 2, 64)
            _, lg = stack(inputs_embeds=torch.cat([x0, x1]), position_ids=pid, past_key_values=cache, logits_to_keep=1)
        smp = Sampler(2, DEV, vocab_size=V, history=HIST)
        tracks = {}
        for row, ids in ((0, ids0), (1, ids1)):
            smp.set(row, **sp[row])
            smp.mark(row, ids.to(DEV))
            tracks[row] = _Track(V, sp[row], ids)
        dec = GraphedDecode(stack, cache, 2, sampler=smp)
        smp.sample(lg[:, -1], dec.token)
        toks = [dec.token[:, 0].tolist()]
        for row, t in tracks.items():
            t.judge(lg[row, -1].cpu(), toks[0][row], ("b2 first", row))
        for i in range(8):
            if graphed:
                dec.step()
            else:
                with torch.no_grad():
                    dec.logits = dec._run()
                cache.advance(1)
            toks.append(dec.token[:, 0].tolist())
            for row, t in tracks.items():
                t.judge(dec.logits[row, -1].cpu(), toks[-1][row], ("b2", graphed, i, row))
        _check_books(smp, tracks, ("b2", graphed))
        assert tracks[0].book.done == 2 and [t[0] for t in toks[5:]] == [2] * 4 and tracks[1].book.n_new == 9
        assert smp.tokens(0).tolist() == [t[0] for t in toks[:5]] and smp.tokens(1).tolist() == [t[1] for t in toks]
        runs.append((toks, _state(smp)))
    assert runs[0][0] == runs[1][0]
    for k_ in runs[0][1]:
        assert torch.equal(runs[0][1][k_], runs[1][1][k_]), k_


def _bytes_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().flatten().view(torch.uint8),
                                                                      b.contiguous().flatten().view(torch.uint8))


def test_admit_n_equals_admit_with_every_option_on():
    """admit_n(slots, ...) leaves every slot as admit(slot, ...) with that slot's dict would: sampling, prompt_ids, a grammar, a
    bias table and a bad-words table at once, on a sampler with every per-row option but guidance.  Tokens of the admission and of
    6 graphed steps, the sampler's state and every tensor a slot owns (cache rows, token, positions, sampler rows), byte for byte."""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.grammar import TokenFsm
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = _small()
    V = hc.vocab_size
    x, ids = _prompt(hc, 37, 21)
    fsm = TokenFsm.from_edges(V, 2, [(0, list(range(0, V, 2)), 1), (1, list(range(V)), 0)])   # every state allows >= V/2 tokens
    dicts = [dict(temperature=0.8, top_k=40, top_p=0.95, seed=5, repetition_penalty=1.2, min_p=0.01, frequency_penalty=0.3,
                  no_repeat_ngram_size=2, max_new_tokens=4, fill_token=3),
             dict(repetition_penalty=1.4, presence_penalty=0.5, min_new_tokens=3, stop_token_ids=[8, 9]),
             dict(temperature=1.3, seed=-9, top_k=0, min_p=0.02, no_repeat_ngram_size=3)]
    runs = []
    for n_way in (True, False):
        cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
        smp = Sampler(4, DEV, vocab_size=V, history=32, logprobs=2, grammar_states=8, penalties=True, bias_tables=2, bans=True,
                      ban_context=16, ban_tables=2, ban_seqs=8, ban_len=4)
        dec = GraphedMultiStreamDecode(stack, cache, sampler=smp)
        opts = dict(prompt_ids=ids, grammar=smp.load_grammar(fsm), logit_bias=smp.load_logit_bias({5: -INF, 12: 2.0, 100: -1.5}),
                    bad_words=smp.load_bad_words([[7], [20, 22], [1, 2, 3, 4]]))
        if n_way:
            dec.admit_n([0, 1, 2], x, sampling=dicts, **opts)
        else:
            for slot in range(3):
                dec.admit(slot, x, sampling=dicts[slot], **opts)
        toks = [dec.token[:3, 0].tolist()]
        for _ in range(6):
            dec.step()
            toks.append(dec.token[:3, 0].tolist())
        torch.cuda.synchronize()
        runs.append((toks, _state(smp), [t[:3].cpu() for t in dec._slot_tensors()]))
    (toks_n, st_n, rows_n), (toks_1, st_1, rows_1) = runs
    assert not (st_n["done"][:3] == 3).any() and st_n["done"][0].item() == 2, "no row meets a dead end; row 0 spends its budget"
    assert toks_n == toks_1
    assert set(st_n) == set(st_1)
    for k_ in st_n:
        assert _bytes_equal(st_n[k_], st_1[k_]), k_
    assert len(rows_n) == len(rows_1)
    for i, (a, b) in enumerate(zip(rows_n, rows_1)):
        assert _bytes_equal(a, b), i

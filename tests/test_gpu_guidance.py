"""GPU (-m gpu): guidance on paired rows -- ops.guide_logits (ivl_logit_guide_fwd, GUIDE-0 .. GUIDE-5) and ops.rows_follow in
front of and behind the sampling launch, and their use in the graphed multi-stream step -- judged by tests/guidance.py.

Every operator test runs ONE call of S = 6 rows over a buffer of random 16-bit patterns (NaN payloads, -0, +-inf) that starts one
element off a 16-byte boundary and has an odd ld, so the six row starts take different offsets inside their tiles; the whole
buffer -- the element in front, the columns V..ld, the partner rows, the rows that are off and a guard row behind -- is compared
as int16 with what the host says may change."""
import numpy as np
import pytest
import torch

import guidance as G
import test_gpu_adjust as tga

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F32 = torch.int32, torch.int64, torch.float32
NINF = -float("inf")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _dev(k):
    """the device tensors of a call k of tests/guidance.py: (buffer, the logits view [S,V], keywords of ops.guide_logits)"""
    S, V, ld = len(k["partner"]), k["V"], k["ld"]
    flat = np.concatenate([np.array([0x7FC5], dtype=np.int16), k["bits"].reshape(-1)])
    buf = torch.from_numpy(flat).to(DEV)
    assert buf.data_ptr() % 16 == 0
    lg = buf[1:].view(S + 1, ld)[:S, :V].view(torch.bfloat16)
    kw = dict(partner=torch.from_numpy(k["partner"]).to(DEV), scale=torch.from_numpy(k["scale"]).to(DEV),
              cut=torch.from_numpy(k["cut"]).to(DEV))
    if k.get("done") is not None:
        kw["done"] = torch.from_numpy(k["done"]).to(DEV)
    return buf, lg, kw


def _check(k, buf, kw, where):
    """judges the buffer after the call; returns (the rows' bits, elements that are not the correctly rounded value)"""
    S, V, ld = len(k["partner"]), k["V"], k["ld"]
    torch.cuda.synchronize()
    for name in ("partner", "scale", "cut", "done"):
        if k.get(name) is not None:
            assert np.array_equal(kw[name].cpu().numpy(), k[name], equal_nan=name != "partner"), f"{name} is only read"
    flat = buf.cpu().numpy()
    assert flat[0] == 0x7FC5, "the element in front of row 0"
    got = flat[1:].reshape(S + 1, ld)
    refs = G.reference(k["bits"], V, k["partner"], k["scale"], k["cut"], k.get("done"))
    assert sorted(refs) == sorted(k["leaders"]), (where, sorted(refs))
    keep = np.ones_like(got, dtype=bool)
    near = 0
    for r, ref in refs.items():
        keep[r, :V] = False
        bad, n = G.judge(got[r, :V], ref, k["scale"][r])
        near += n
        assert bad.size == 0, (where, "row", r, "of", V, bad[:5].tolist(), ref[bad[:5]].tolist(),
                               G.bf16_value(got[r, bad[:5]]).tolist(), float(k["scale"][r]), float(k["cut"][r]))
    assert (got[keep] == k["bits"][keep]).all(), (where, "a byte outside the leaders' first V columns changed",
                                                  np.argwhere((got != k["bits"]) & keep)[:5].tolist())
    return got, near


SIZES = (1, 7, 8, 9, 1023, 1024, 1025, 8191, 8193, 151936)


@pytest.mark.parametrize("V", SIZES)
def test_operator_against_the_judge(V):
    from infinitevl_amd import ops
    ld = V + 3 + (V % 2 == 1)                                            # odd
    combos = [(l, v) for l in G.LAYOUTS for v in G.VARIANTS]
    if V > 10000:
        combos = [(G.LAYOUTS[0], "plain"), (G.LAYOUTS[1], "harsh")]
    n0, near, total = ops.GUIDE_CALLS["guide"], 0, 0
    for j, (layout, variant) in enumerate(combos):
        k = G.call(V, ld, layout, variant, 7000 + 10 * SIZES.index(V) + j)
        for r in k["leaders"]:
            assert G.margin_ok(k["bits"][r, :V], k["cut"][r])
        buf, lg, kw = _dev(k)
        assert lg.data_ptr() % 16 == 2 and ld % 2 == 1
        assert ops.guide_logits(lg, **kw) is lg
        near += _check(k, buf, kw, (V, layout, variant))[1]
        total += 2 * V
    assert ops.GUIDE_CALLS["guide"] == n0 + len(combos)
    assert near <= max(2, 0.02 * total), ("elements that are the neighbour of the rounded value: a boundary is rare", near, total)


def _special(V, rows, partner, scale, cut, done=None, ld=None, seed=5):
    """a call whose rows are given as float64 arrays (None: random bits)"""
    S = len(rows)
    ld = ld or V + 5
    bits = G.random_bits(S + 1, ld, seed)
    for r, x in enumerate(rows):
        if x is not None:
            bits[r, :V] = G.to_bf16(np.asarray(x, dtype=np.float64))
    k = dict(V=V, ld=ld, bits=bits, partner=np.array(partner, dtype=np.int32), scale=np.array(scale, dtype=np.float32),
             cut=np.array(cut, dtype=np.float32), done=None if done is None else np.array(done, dtype=np.int32))
    k["leaders"] = [r for r in range(S) if G.guided(k["partner"], k["scale"], k["done"], r)]
    return k


def test_infinities_scales_zero_and_one_and_a_cut_that_leaves_the_maximum():
    from infinitevl_amd import ops
    V = 300
    rng = np.random.default_rng(3)
    c = G.bf16_value(G.logit_row(V, rng)).astype(np.float64)
    u = G.bf16_value(G.logit_row(V, rng)).astype(np.float64)
    u_part = np.where(rng.random(V) < 0.4, NINF, u)
    ninf = np.full(V, NINF)
    # rows: 0 <- 1 both all -inf; 2 <- 3 u partly -inf at s = 3; 4 <- 5 s = 0; 6 <- 7 s = 1; 8 <- 9 the cut leaves the maximum;
    # 10 <- 11 a leader over an all -inf partner
    rows = [ninf, ninf, c, u_part, c, u, c, u, c, u, c, ninf]
    partner = [1, -1, 3, -1, 5, -1, 7, -1, 9, -1, 11, -1]
    scale = [2.0, 1, 3.0, 1, 0.0, 1, 1.0, 1, 2.5, 1, 4.0, 1]
    tiny = -2.0 ** -12                                                   # every other bf16 value lies further below the maximum
    cut = [NINF, 0, NINF, 0, NINF, 0, NINF, 0, tiny, 0, NINF, 0]
    k = _special(V, rows, partner, scale, cut)
    assert k["leaders"] == [0, 2, 4, 6, 8, 10] and G.margin_ok(k["bits"][8, :V], np.float32(tiny))
    buf, lg, kw = _dev(k)
    ops.guide_logits(lg, **kw)
    got, _ = _check(k, buf, kw, "special")
    out = G.bf16_value(got[:, :V]).astype(np.float64)
    assert np.isneginf(out[0]).all()
    lc, lu = G.log_softmax64(c)[0], G.log_softmax64(u)[0]
    gone = np.isneginf(u_part)
    assert gone.sum() > 50 and (got[2, :V][gone] == G.to_bf16(lc)[gone]).mean() > 0.98, "u(v) = -inf: the leader's own log-probability"
    assert (got[4, :V] == G.to_bf16(lu)).mean() > 0.98 and (got[6, :V] == G.to_bf16(lc)).mean() > 0.98, "s = 0 is lu, s = 1 is lc"
    top = c == c.max()
    assert np.isneginf(out[8][~top]).all() and np.isfinite(out[8][top]).all() and top.sum() >= 1
    assert (got[10, :V] == G.to_bf16(lc)).mean() > 0.98


def test_rows_that_are_off_keep_every_bit():
    """GUIDE-0, each clause on a row of random bit patterns (NaN payloads) whose partner table entry would otherwise do: the
    partner out of range below and above, the row itself, a partner that is itself a leader, a scale that is not finite, done."""
    from infinitevl_amd import ops
    V, S = 1025, 8
    rng = np.random.default_rng(9)
    c, u = G.logit_row(V, rng), G.logit_row(V, rng)
    rows = [G.bf16_value(c), G.bf16_value(u)] + [None] * (S - 2)
    #          0 leads 1      2: below  3: above  4: itself  5 names the leader 0   6: inf      7: done
    partner = [1, -1, -7, S, 4, 0, 1, 1]
    scale = [2.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.inf, 1.0]
    k = _special(V, rows, partner, scale, [NINF] * S, done=[0, 0, 0, 0, 0, 0, 0, 3])
    assert k["leaders"] == [0]
    buf, lg, kw = _dev(k)
    ops.guide_logits(lg, **kw)
    _check(k, buf, kw, "off rows")
    k2 = {**k, "scale": k["scale"].copy()}
    k2["scale"][6] = np.nan
    buf, lg, kw = _dev(k2)
    ops.guide_logits(lg, **kw)
    _check(k2, buf, kw, "a NaN scale")
    # without `done` the finished row is one more leader of partner 1
    k3 = {**k, "done": None}
    k3["leaders"] = [0, 7]
    k3["bits"] = k["bits"].copy()
    k3["bits"][7, :V] = G.logit_row(V, rng)
    buf, lg, kw = _dev(k3)
    assert "done" not in kw
    ops.guide_logits(lg, **kw)
    _check(k3, buf, kw, "done = None")


# ---------------------------------------------------------------------------------------------
# bit contracts
# ---------------------------------------------------------------------------------------------
def test_same_bits_replayed_and_in_other_row_positions_among_other_neighbours():
    from infinitevl_amd import ops
    V = 8193
    c, u, s, cut = G.pair_rows(V, 77, 2.5, 0.05, u_ninf=0.01)
    c2, u2, s2, cut2 = G.pair_rows(V, 78, 1.5, 0.0)

    def run(S, at, other, ld, graph=False):
        """the pair in the rows at = (leader, partner) of S, the second pair in `other` (or None), the rest random and off"""
        bits = G.random_bits(S + 1, ld, 100 + S)
        partner, scale, cutv = np.full(S, -1, np.int32), np.ones(S, np.float32), np.full(S, NINF, np.float32)
        bits[at[0], :V], bits[at[1], :V] = c, u
        partner[at[0]], scale[at[0]], cutv[at[0]] = at[1], s, cut
        leaders = [at[0]]
        if other is not None:
            bits[other[0], :V], bits[other[1], :V] = c2, u2
            partner[other[0]], scale[other[0]], cutv[other[0]] = other[1], s2, cut2
            leaders.append(other[0])
        k = dict(V=V, ld=ld, bits=bits, partner=partner, scale=scale, cut=cutv, done=None, leaders=leaders)
        buf, lg, kw = _dev(k)
        if graph:
            fresh = buf.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.guide_logits(lg, **kw)                               # warm-up (the call is not idempotent: the buffer is put back)
            torch.cuda.current_stream().wait_stream(side)
            buf.copy_(fresh)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ops.guide_logits(lg, **kw)
            buf.copy_(fresh)
            g.replay()
        else:
            ops.guide_logits(lg, **kw)
        got, _ = _check(k, buf, kw, (S, at, other, ld, graph))
        return got[at[0], :V].copy()

    first = run(2, (0, 1), None, V + 3)
    assert (run(2, (0, 1), None, V + 3, graph=True) == first).all(), "replayed"
    assert (run(2, (1, 0), None, V + 8) == first).all(), "leader behind its partner, aligned rows"
    assert (run(6, (4, 2), (0, 5), V + 5) == first).all(), "other positions, another pair beside it"
    assert (run(63, (62, 0), (30, 31), V + 1, graph=True) == first).all(), "the most rows a call takes"


def test_rows_follow_moves_only_the_partners_token_and_done():
    from infinitevl_amd import ops
    S = 8
    #          0 -> 1   2 -> 6, 3 -> 6 (the lowest wins)   4 names the leader 0: not valid   5: itself   7 names 7's... out of range
    partner = np.array([1, -1, 6, 6, 0, 5, -1, S], dtype=np.int32)
    assert G.followers(partner) == {1: 0, 6: 2}
    tok = torch.arange(100, 100 + 2 * S, dtype=I64, device=DEV).view(S, 2)
    done = torch.tensor([2, 0, 1, 3, 0, 4, 0, 0], dtype=I32, device=DEV)
    t0, d0 = tok.clone(), done.clone()
    p = torch.from_numpy(partner).to(DEV)
    n0 = ops.GUIDE_CALLS["follow"]
    view = tok[:, :1]                                                    # [S,1] at stride 2: the odd columns are guards
    assert ops.rows_follow(view, p, done) is view
    want_t, want_d = t0.clone(), d0.clone()
    want_t[1, 0], want_t[6, 0], want_d[1], want_d[6] = t0[0, 0], t0[2, 0], d0[0], d0[2]
    assert torch.equal(tok, want_t) and torch.equal(done, want_d) and torch.equal(p.cpu(), torch.from_numpy(partner))
    # done = None: nothing of done is written; a 1-d token
    flat = torch.arange(50, 50 + S, dtype=I64, device=DEV)
    done.copy_(d0)
    ops.rows_follow(flat, p)
    want = torch.arange(50, 50 + S, dtype=I64)
    want[1], want[6] = 50, 52
    assert torch.equal(flat.cpu(), want) and torch.equal(done, d0)
    assert ops.GUIDE_CALLS["follow"] == n0 + 2
    # replayed: the same
    tok.copy_(t0)
    done.copy_(d0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rows_follow(view, p, done)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rows_follow(view, p, done)
    tok.copy_(t0)
    done.copy_(d0)
    g.replay()
    assert torch.equal(tok, want_t) and torch.equal(done, want_d)


# ---------------------------------------------------------------------------------------------
# end to end: the graphed multi-stream step on the small stack
# ---------------------------------------------------------------------------------------------
N_STEPS = 12
POS, NEG = (50, 5), (20, 6)                  # (tokens, seed) of the prompt and of the negative prompt
LEAD = dict(temperature=0.8, seed=7, top_k=40)
SCALE, BETA = 2.5, 0.05


def _decoder(guidance, holds=False, n_slots=4):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    stack, hc = tga._small()
    cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(n_slots, DEV, vocab_size=hc.vocab_size, history=32, logprobs=2, **({"guidance": True} if guidance else {}))
    return GraphedMultiStreamDecode(stack, cache, sampler=smp, holds=holds), hc


def _compose(c_row, u_row, scale, cut32, counter, sampling=LEAD):
    """what the composition predicts from the two raw logit rows [V]: (the guided row's bits, token, logprob)"""
    from infinitevl_amd import ops
    two = torch.stack([c_row, u_row]).contiguous()
    ops.guide_logits(two, partner=torch.tensor([1, -1], dtype=I32, device=DEV), scale=torch.tensor([scale, 1.0], dtype=F32, device=DEV),
                     cut=torch.tensor([cut32, NINF], dtype=F32, device=DEV))
    row = two[0:1].clone()
    lp = torch.zeros(1, dtype=F32, device=DEV)
    tok = ops.sample_tokens(row, torch.tensor([sampling.get("temperature", 0.0)], dtype=F32, device=DEV),
                            torch.tensor([sampling.get("top_k", 0)], dtype=I32, device=DEV),
                            torch.tensor([sampling.get("top_p", 1.0)], dtype=F32, device=DEV),
                            torch.tensor([sampling.get("seed", 0)], dtype=I64, device=DEV),
                            torch.tensor([counter], dtype=I64, device=DEV), logprob=lp)
    return two[0].clone(), int(tok.item()), lp.clone()


def _mirrored_run(graph):
    """slots: 0 the leader, 1 its partner, 2 a plain slot with the leader's prompt, 3 a plain slot with the negative prompt; the
    host overwrites the tokens of 2 and 3 with the leader's before every step, so their logits are the pair's RAW rows"""
    dec, hc = _decoder(True)
    dec.admit(2, tga._prompt(hc, *POS), sampling=dict())
    dec.admit(3, tga._prompt(hc, *NEG), sampling=dict())
    first = dec.admit_guided(0, 1, tga._prompt(hc, *POS), tga._prompt(hc, *NEG), guidance_scale=SCALE, plausibility=BETA,
                             sampling=LEAD).clone()
    log = dict(tok=[dec.token[:, 0].tolist()], lp=[dec.sampler.logprob[0:1].clone()], lg=[], first=first)
    for _ in range(N_STEPS):
        dec.token[2].copy_(dec.token[0])
        dec.token[3].copy_(dec.token[0])
        dec.step(graph=graph)
        log["tok"].append(dec.token[:, 0].tolist())
        log["lp"].append(dec.sampler.logprob[0:1].clone())
        log["lg"].append(dec.logits[:, -1].clone())
    return dec, hc, log


def test_the_guided_step_replayed_equals_eager_and_the_composition():
    from infinitevl_amd import ops
    n0 = dict(ops.GUIDE_CALLS)
    dec, hc, got = _mirrored_run(True)
    assert dec.graph is not None and ops.GUIDE_CALLS["guide"] > n0["guide"] and ops.GUIDE_CALLS["follow"] > n0["follow"]
    twin, _, eager = _mirrored_run(False)
    assert twin.graph is None
    assert got["tok"] == eager["tok"], "replayed steps equal the eager steps"
    assert all(tga._bytes(a) == tga._bytes(b) for a, b in zip(got["lp"], eager["lp"])), "logprobs, bit for bit"
    sg, se = dec.sampler.state(), twin.sampler.state()
    for name, v in sg.items():
        assert tga._bytes(v) == tga._bytes(se[name]), name
    cut32 = float(np.float32(np.log(BETA)))
    assert dec.sampler.guide_partner.tolist() == [1, -1, -1, -1] and dec.sampler.guide_cut[0].item() == cut32
    lead = [t[0] for t in got["tok"]]
    assert all(t[1] == t[0] for t in got["tok"]), "token[partner] == token[leader] at every step"
    assert len(set(lead)) > 3
    for i, lg in enumerate(got["lg"]):
        assert tga._bytes(lg[1]) == tga._bytes(lg[3]), (i, "the partner's logits are those of a plain slot fed the leader's tokens")
        row, tok, lp = _compose(lg[2], lg[3], SCALE, cut32, counter=i + 1)
        assert tga._bytes(row) == tga._bytes(lg[0]), (i, "the leader's row is the guided row")
        assert tok == lead[i + 1] and tga._bytes(lp) == tga._bytes(got["lp"][i + 1]), (i, tok, lead[i + 1])
    # the guided distribution is not the leader's own: somewhere the plain slot's arg-max row differs from the guided row
    assert any(tga._bytes(lg[0]) != tga._bytes(lg[2]) for lg in got["lg"])
    # ---- set_guidance between two replays: the next step obeys it, with the same graph object
    graph = dec.graph
    dec.set_guidance(0, guidance_scale=1.0, plausibility=0.5)
    assert dec.sampler.guide_scale[0].item() == 1.0 and dec.sampler._guide_params[0] == (1.0, 0.5)
    dec.token[2].copy_(dec.token[0])
    dec.token[3].copy_(dec.token[0])
    dec.step()
    lg = dec.logits[:, -1]
    new_cut = float(np.float32(np.log(0.5)))
    row, tok, lp = _compose(lg[2], lg[3], 1.0, new_cut, counter=N_STEPS + 1)
    old_row, _, _ = _compose(lg[2], lg[3], SCALE, cut32, counter=N_STEPS + 1)
    assert dec.graph is graph and tga._bytes(row) == tga._bytes(lg[0]) and tga._bytes(old_row) != tga._bytes(row)
    assert dec.token[0, 0].item() == tok == dec.token[1, 0].item() and tga._bytes(lp) == tga._bytes(dec.sampler.logprob[0:1])
    dec.set_guidance(0, plausibility=0.0)
    assert dec.sampler._guide_params[0] == (1.0, 0.0) and torch.isneginf(dec.sampler.guide_cut[0])
    with pytest.raises(ValueError, match="leads no guided pair"):
        dec.set_guidance(2, guidance_scale=2.0)


def test_the_first_token_is_guided_too():
    dec, hc = _decoder(True)
    dec.admit(2, tga._prompt(hc, *POS), sampling=dict())
    c = dec.admit_logits[0, -1].clone()
    dec.admit(3, tga._prompt(hc, *NEG), sampling=dict())
    u = dec.admit_logits[0, -1].clone()
    dec.admit_guided(0, 1, tga._prompt(hc, *POS), tga._prompt(hc, *NEG), guidance_scale=SCALE, plausibility=BETA, sampling=LEAD)
    row, tok, lp = _compose(c, u, SCALE, float(np.float32(np.log(BETA))), counter=0)
    assert tga._bytes(dec.admit_logits[0, -1]) == tga._bytes(row) and tuple(dec.admit_logits.shape) == (1, 1, hc.vocab_size)
    assert dec.token[0, 0].item() == tok == dec.token[1, 0].item() and tga._bytes(lp) == tga._bytes(dec.sampler.logprob[0:1])
    assert dec.sampler.temperature.tolist()[1] == 0.0 and dec.sampler.budget.tolist()[1] == -1 and not dec.sampler._ends[1]
    assert dec.position_ids[0, :2, 0].tolist() == [POS[0], NEG[0]]


def test_unguided_slots_beside_a_pair_and_a_sampler_without_guidance():
    from infinitevl_amd import ops
    free = dict(temperature=1.0, seed=11, top_k=50)

    def run(guidance):
        dec, hc = _decoder(guidance)
        if guidance:
            dec.admit_guided(0, 1, tga._prompt(hc, *POS), tga._prompt(hc, *NEG), guidance_scale=SCALE, sampling=LEAD)
        dec.admit(2, tga._prompt(hc, 33, 7), sampling=free)
        dec.admit(3, tga._prompt(hc, 40, 8), sampling=dict())
        toks = [dec.token[2:, 0].tolist()]
        for _ in range(N_STEPS):
            dec.step()
            toks.append(dec.token[2:, 0].tolist())
        return dec, toks

    n0 = dict(ops.GUIDE_CALLS)
    plain, base = run(False)
    assert ops.GUIDE_CALLS == n0, "a sampler built without guidance launches what it always did"
    dec, got = run(True)
    assert got == base and len({t[0] for t in got}) > 3
    assert tga._bytes(dec.sampler.logprob[2:]) == tga._bytes(plain.sampler.logprob[2:])
    # refusals of the decoder: a pair is not forked, loaded onto, admitted into or released by its partner
    hc = tga._small()[1]
    for call, word in ((lambda: dec.fork(0, [3]), "leads a guided pair"), (lambda: dec.fork(2, [1]), "is the partner"),
                       (lambda: dec.fork(1, [3]), "is the partner"),
                       (lambda: dec.admit_n([3, 1], tga._prompt(hc, 8, 1)), "is the partner"),
                       (lambda: dec.admit_n([0, 3], tga._prompt(hc, 8, 1)), "leads a guided pair"),
                       (lambda: dec.load([1], None), "is the partner"), (lambda: dec.load([0], None), "leads a guided pair"),
                       (lambda: dec.admit(1, tga._prompt(hc, 8, 1)), "is the partner"),
                       (lambda: dec.admit(0, tga._prompt(hc, 8, 1)), "leads a guided pair"),
                       (lambda: dec.release(1), "is the partner"),
                       (lambda: dec.extend(1, tga._prompt(hc, 8, 1)), "is the partner"),
                       (lambda: dec.extend(0, tga._prompt(hc, 8, 1)), "negative_embeds"),
                       (lambda: dec.extend(2, tga._prompt(hc, 8, 1), negative_embeds=tga._prompt(hc, 8, 1)), "leads none"),
                       (lambda: dec.admit_guided(2, 1, tga._prompt(hc, 8, 1), tga._prompt(hc, 8, 1), guidance_scale=2.0), "is the partner"),
                       (lambda: dec.admit_guided(2, 2, tga._prompt(hc, 8, 1), tga._prompt(hc, 8, 1), guidance_scale=2.0), "distinct"),
                       (lambda: dec.admit_guided(2, 3, tga._prompt(hc, 8, 1), tga._prompt(hc, 8, 1), guidance_scale=float("inf")), "finite"),
                       (lambda: plain.admit_guided(0, 1, tga._prompt(hc, 8, 1), tga._prompt(hc, 8, 1), guidance_scale=2.0), "guidance=True")):
        with pytest.raises(ValueError, match=word):
            call()
    assert dec.token[2:, 0].tolist() == got[-1] and sorted(dec._live) == [0, 1, 2, 3], "nothing was written"
    # release of the leader frees both slots; a plain stream in the former partner slot runs unguided
    graph = dec.graph
    dec.release(0)
    assert sorted(dec._live) == [2, 3] and dec.sampler.guide_partner.tolist() == [-1] * 4 and dec.sampler._partner == {}
    assert dec.token[:2, 0].tolist() == [0, 0]
    plain.release(2)
    plain.admit(1, tga._prompt(hc, 33, 7), sampling=free)
    dec.release(2)
    dec.admit(1, tga._prompt(hc, 33, 7), sampling=free)
    for _ in range(4):
        dec.step()
        plain.step()
        assert dec.token[1, 0].item() == plain.token[1, 0].item() and dec.token[3, 0].item() == plain.token[3, 0].item()
    assert dec.graph is graph


def test_beam_search_refuses_a_guidance_sampler():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode, Sampler
    stack, hc = tga._small()
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
    smp = Sampler(4, DEV, vocab_size=hc.vocab_size, max_stop=0, history=8, logprobs=4, score_rings=False, guidance=True)
    with pytest.raises(ValueError, match="guidance"):
        GraphedBeamDecode(stack, cache, num_beams=2, vocab_size=hc.vocab_size, history=8, sampler=smp)


def test_holds_a_budget_freezes_both_rows_extend_continues_hold_and_resume_round_trip():
    def start():
        dec, hc = _decoder(True, holds=True)
        dec.admit_guided(0, 1, tga._prompt(hc, *POS), tga._prompt(hc, *NEG), guidance_scale=SCALE, plausibility=BETA,
                         sampling=dict(max_new_tokens=4))
        dec.admit(2, tga._prompt(hc, 33, 7), sampling=dict())
        return dec, hc

    dec, hc = start()
    smp, pos = dec.sampler, dec.cache.pos_rows
    p0 = pos[:3].tolist()
    out = dec.run_until_done(16, poll_every=2)
    assert smp.done.tolist()[:3] == [2, 2, 0] and len(out[0]) == 4, "the follow launch copies the leader's done code"
    frozen = pos[:3].tolist()
    # the first token came from the prefill: three steps drew the other three, and the step that ended the leader still ran
    assert [frozen[i] - p0[i] for i in range(3)][:2] == [3, 3], (p0, frozen)
    before = dec.position_ids[:, :2].clone()
    for _ in range(3):
        dec.step()
    assert pos[:2].tolist() == frozen[:2] and pos[2].item() == frozen[2] + 3, "both rows of the pair stopped together"
    assert torch.equal(dec.position_ids[:, :2], before)
    # extend with both halves: the next turn of both streams
    graph = dec.graph
    with pytest.raises(ValueError, match="negative_embeds"):
        dec.extend(0, tga._prompt(hc, 10, 22))
    t = dec.extend(0, tga._prompt(hc, 10, 22), negative_embeds=tga._prompt(hc, 6, 23), max_new_tokens=3)
    assert smp.done.tolist()[:2] == [0, 0] and int(smp.n_new[0]) == 1 and dec.token[1, 0].item() == t.item()
    assert pos[:2].tolist() == [frozen[0] + 10, frozen[1] + 6]
    assert dec.position_ids[0, :2, 0].tolist() == [int(before[0, 0, 0]) + 10, int(before[0, 1, 0]) + 6]
    dec.step()
    assert dec.graph is graph and dec.token[1, 0].item() == dec.token[0, 0].item() and smp.done.tolist()[:2] == [0, 0]
    assert pos[:2].tolist() == [frozen[0] + 11, frozen[1] + 7]
    # hold / resume: the pair sits a step out and goes on as a twin that never held
    twin, _ = start()
    twin.run_until_done(16, poll_every=2)
    for _ in range(3):
        twin.step()
    twin.extend(0, tga._prompt(hc, 10, 22), negative_embeds=tga._prompt(hc, 6, 23), max_new_tokens=3)
    twin.step()
    assert twin.token[:2, 0].tolist() == dec.token[:2, 0].tolist()
    with pytest.raises(ValueError, match="is the partner"):
        dec.hold(1)
    dec.hold(0)
    assert smp.done.tolist()[:2] == [4, 4] and sorted(dec._held) == [0, 1]
    parked, at = dec.token[:2].clone(), pos[:2].tolist()
    dec.step()
    dec.step()
    assert pos[:2].tolist() == at and smp.done.tolist()[:2] == [4, 4]
    with pytest.raises(ValueError, match="is the partner"):
        dec.resume(1)
    dec.resume(0)
    assert smp.done.tolist()[:2] == [0, 0] and torch.equal(dec.token[:2], parked) and not dec._held
    dec.step()
    twin.step()
    assert dec.token[:2, 0].tolist() == twin.token[:2, 0].tolist() and smp.done.tolist()[:2] == twin.sampler.done.tolist()[:2] == [2, 2]
    assert smp.tokens(0).tolist() == twin.sampler.tokens(0).tolist() and len(smp.tokens(0)) == 3

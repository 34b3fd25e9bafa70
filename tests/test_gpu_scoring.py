"""GPU (-m gpu): scoring given tokens -- ivl_linear_logprob_m256_fwd (the 256-row GEMM with a log-sum-exp epilogue + the per-row
combine), ops.linear_logprob, harness.score_sequence and GraphedMultiStreamDecode.score.

The float64 reference (tests/scoring.py) works on the kernel's OWN logits: the plain ivl_linear_m256_fwd on the same inputs.
Tolerance |err| <= 1e-5 + 2^-22 |ref| for logprob and lse (derived in scoring.tolerance); top1, infinities, ignored rows and
n_scored are exact.  Largest observed |err| / tolerance on the MI355X: 0.104 (logprob) and 0.080 (lse) at (130, 151936, 256),
0.056 end to end, 0.045 against the sampling launch (allowed 2); DESIGN 4.12 records them."""
import math

import pytest
import torch

import fork as fk
import scoring

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@pytest.fixture(scope="module")
def small():
    return fk.small_stack(DEV)


def bf(x):
    return x.to(torch.bfloat16)


def plain(x, w, bias):
    """The logits the plain 256-row kernel writes for x [M,K] (M <= 256)."""
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().ivl_linear_m256_fwd(ops._p(x), ops._p(w), ops._p(bias), ops._p(y), M, N, K, 0, ops._stream(x)))
    return y


def score(x, w, t, bias=None):
    from infinitevl_amd import ops
    return ops.linear_logprob(x, w, t, bias, top1=True, lse=True)


def _inputs(M, N, K, seed, with_bias=False, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(M, K, generator=g)).to(DEV)
    w = bf(torch.randn(N, K, generator=g) * scale * K ** -0.5).to(DEV)
    b = bf(torch.randn(N, generator=g)).to(DEV) if with_bias else None
    t = torch.randint(0, N, (M,), generator=g).to(DEV)
    return x, w, b, t


def lowest_argmax(y):
    yf = y.float()
    return (yf == yf.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)


@pytest.mark.parametrize("M,N,K,with_bias", [(256, 1000, 128, False), (200, 4100, 64, False), (1, 64, 64, False),
                                             (130, 151936, 256, False), (256, 1000, 128, True)])
def test_linear_logprob_vs_float64(M, N, K, with_bias):
    """(256, 1000): a masked column tail; (130, 151936): the full vocabulary's 2374 partials per row."""
    x, w, b, t = _inputs(M, N, K, M + N + K + int(with_bias), with_bias)
    lp, top1, lse = score(x, w, t, b)
    y = plain(x, w, b)
    ref_lp, ref_top1, ref_lse = scoring.ref_logprob(y, t)
    r1 = scoring.judge(lp, ref_lp, "logprob")
    r2 = scoring.judge(lse, ref_lse, "lse")
    print(f"  ({M}, {N}, {K}, bias={with_bias}): max |err| / tolerance: logprob {r1:.3f}, lse {r2:.3f}")
    assert torch.equal(top1.cpu(), ref_top1) and torch.equal(top1, lowest_argmax(y))
    assert lp.dtype == torch.float32 and lse.dtype == torch.float32 and top1.dtype == torch.int64
    assert bool((lp <= 0).all())


def test_top1_ties_across_column_blocks_take_the_lowest_index():
    """Weight rows c and c + 64 * 3 are equal, so their logits are bit-equal and a row whose maximum they are has the tie in two
    different partials; a second pair ties inside one lane group's neighbour (c, c + 16)."""
    M, N, K = 96, 1000, 128
    x, w, _, t = _inputs(M, N, K, 11)
    v = bf(torch.randn(K, generator=torch.Generator().manual_seed(12))).to(DEV)
    w[70] = v
    w[70 + 192] = w[70]
    w[70 + 192 + 64 * 9] = w[70]
    w[401] = -v
    w[401 + 16] = w[401]
    w[401 - 64 * 3] = w[401]
    lp, top1, lse = score(x, w, t)
    y = plain(x, w, None)
    assert torch.equal(y[:, 70], y[:, 262]) and torch.equal(y[:, 401], y[:, 209])
    want = lowest_argmax(y)
    assert torch.equal(top1, want)
    assert int((want == 70).sum()) >= 10 and int((want == 209).sum()) >= 10, want.tolist()   # the ties ARE the maxima
    assert not bool(((top1 == 262) | (top1 == 838) | (top1 == 401) | (top1 == 417)).any())
    ref_lp, _, ref_lse = scoring.ref_logprob(y, t)
    scoring.judge(lp, ref_lp, "logprob")
    scoring.judge(lse, ref_lse, "lse")


def test_ignored_targets_give_zero_bits_and_still_a_top1():
    M, N, K = 200, 4100, 64
    x, w, _, t = _inputs(M, N, K, 21)
    t[::3] = -100
    t[1::7] = N
    t[5] = -1
    t[6] = 1 << 40
    lp, top1, lse = score(x, w, t)
    ignored = (t < 0) | (t >= N)
    assert int(ignored.sum()) > 60
    assert bool((lp.view(torch.int32)[ignored] == 0).all())               # +0.0, bit for bit
    assert bool((lp[~ignored] < 0).all())
    y = plain(x, w, None)
    assert torch.equal(top1, lowest_argmax(y))
    ref_lp, _, ref_lse = scoring.ref_logprob(y, t)
    scoring.judge(lp, ref_lp, "logprob")
    scoring.judge(lse, ref_lse, "lse")


def test_edges_are_judged_by_the_conventions():
    """(8, 256, 64).  Call A: bias entries of -inf (a target on one of them), one x row with a NaN (the whole row NaN: -log N,
    top1 0).  Call B: two +inf bias entries as well (targets on one of them, on a finite column, on a -inf column)."""
    M, N, K = 8, 256, 64
    x, w, _, _ = _inputs(M, N, K, 31)
    x[3, 17] = float("nan")
    bias = bf(torch.randn(N, generator=torch.Generator().manual_seed(32))).to(DEV)
    bias[[5, 64, 130, 255]] = -INF
    t = torch.tensor([5, 9, 130, 77, 255, 0, 64, 200], device=DEV)
    lp, top1, lse = score(x, w, t, bias)
    y = plain(x, w, bias)
    assert bool(torch.isnan(y[3].float()).all()) and bool(torch.isinf(y[:, 5].float())[[0, 1, 2, 4, 5, 6, 7]].all())
    ref_lp, ref_top1, ref_lse = scoring.ref_logprob(y, t)
    scoring.judge(lp, ref_lp, "A logprob")
    scoring.judge(lse, ref_lse, "A lse")
    assert torch.equal(top1.cpu(), ref_top1)
    assert lp[0].item() == -INF and lp[2].item() == -INF and lp[4].item() == -INF and lp[6].item() == -INF   # targets at -inf
    assert top1[3].item() == 0 and lse[3].item() == -INF
    assert abs(lp[3].item() + math.log(N)) <= 1e-6                          # the all -inf row: -logf((float)N)
    assert math.isfinite(lp[1].item()) and math.isfinite(lp[7].item())

    bias[[9, 200]] = INF
    lp, top1, lse = score(x, w, t, bias)
    y = plain(x, w, bias)
    ref_lp, ref_top1, ref_lse = scoring.ref_logprob(y, t)
    scoring.judge(lp, ref_lp, "B logprob")
    scoring.judge(lse, ref_lse, "B lse")
    assert torch.equal(top1.cpu(), ref_top1)
    rows = [0, 1, 2, 4, 5, 6, 7]
    assert top1[rows].tolist() == [9] * 7 and bool((lse[rows] == INF).all())
    assert abs(lp[1].item() + math.log(2.0)) <= 1e-6 and abs(lp[7].item() + math.log(2.0)) <= 1e-6   # one of two +inf columns
    assert lp[5].item() == -INF and lp[0].item() == -INF                     # a finite / a -inf logit below a +inf maximum
    assert top1[3].item() == 0 and abs(lp[3].item() + math.log(N)) <= 1e-6   # NaN + inf = NaN: still the all -inf row


def test_purity_row_position_runs_and_graph_replay():
    """The outputs of a row are a pure function of (x[r], W, bias, target[r]): row 37 of a 256-row call == the same row as an
    M = 1 call; two runs agree; a captured-graph replay into zeroed outputs agrees -- all bit for bit."""
    from infinitevl_amd import _lib, ops
    M, N, K = 256, 4100, 128
    x, w, b, t = _inputs(M, N, K, 41, with_bias=True)
    a = score(x, w, t, b)
    one = score(x[37:38].clone(), w, t[37:38].clone(), b)
    for u, v in zip(a, one):
        assert torch.equal(u[37:38], v)
    mid = score(x[30:131].clone(), w, t[30:131].clone(), b)                # another M, another position of the row
    for u, v in zip(a, mid):
        assert torch.equal(u[30:131], v)
    again = score(x, w, t, b)
    for u, v in zip(a, again):
        assert torch.equal(u, v)
    lib = _lib.load()
    ws = ops.get_workspace(lib.ivl_linear_logprob_workspace_bytes(M, N), x.device, "logprob")
    lp, lse = torch.empty(M, dtype=torch.float32, device=DEV), torch.empty(M, dtype=torch.float32, device=DEV)
    top1 = torch.empty(M, dtype=torch.int64, device=DEV)

    def launch():
        _lib.check(lib.ivl_linear_logprob_m256_fwd(ops._p(x), ops._p(w), ops._p(b), ops._p(t), ops._p(lp), ops._p(top1), ops._p(lse),
                                                   M, N, K, ops._p(ws), ws.numel(), ops._stream(x)))
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for o in (lp, top1, lse):
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lp, a[0]) and torch.equal(top1, a[1]) and torch.equal(lse, a[2])


def test_consistent_with_the_sampling_launch():
    """Greedy rows of the sampling launch on the same logits: its token is top1 and its logprob (integer weights with a 2^-40
    floor: at most N 2^-40 relative on Z) and this one are within the tolerance of the same real number, so within twice it of
    each other."""
    from infinitevl_amd import ops
    M, N, K = 64, 4100, 128
    x, w, _, _ = _inputs(M, N, K, 51)
    y = plain(x, w, None)
    z = lambda dt, v=0: torch.full((M,), v, dtype=dt, device=DEV)
    s_lp = torch.empty(M, dtype=torch.float32, device=DEV)
    tok = ops.sample_tokens(y, z(torch.float32), z(torch.int32), z(torch.float32, 1.0), z(torch.int64), z(torch.int64),
                            logprob=s_lp)
    lp, top1, _ = score(x, w, tok.view(M).clone())
    assert torch.equal(top1, tok.view(M))
    ratio = scoring.judge(lp, s_lp.double(), "logprob vs the sampling launch", scale=2.0)
    print(f"  max |logprob - sampling logprob| / tolerance = {ratio:.3f} (allowed 2)")


def test_ops_linear_logprob_shapes_and_refusals():
    from infinitevl_amd import ops
    x, w, _, _ = _inputs(600, 512, 256, 61)                                 # three pieces: 256 + 256 + 88 rows
    t = torch.randint(0, 512, (600,), generator=torch.Generator().manual_seed(62)).to(DEV)
    lp, top1 = ops.linear_logprob(x.view(2, 300, 256), w, t.view(2, 300), top1=True)
    assert lp.shape == (2, 300) and top1.shape == (2, 300)
    only = ops.linear_logprob(x, w, t)
    assert torch.equal(only, lp.view(600))
    refs = [scoring.ref_logprob(plain(x[a:a + 256], w, None), t[a:a + 256]) for a in (0, 256, 512)]
    scoring.judge(only, torch.cat([r[0] for r in refs]), "logprob over three pieces")
    assert torch.equal(top1.view(600).cpu(), torch.cat([r[1] for r in refs]))
    with pytest.raises(ValueError):
        ops.linear_logprob(x.float(), w, t)
    with pytest.raises(ValueError):
        ops.linear_logprob(x.t().contiguous().t(), w, t)                    # not contiguous
    with pytest.raises(ValueError):
        ops.linear_logprob(x, w, t.to(torch.int32))
    with pytest.raises(ValueError):
        ops.linear_logprob(x[:, :200].contiguous(), w[:, :200].contiguous(), t)   # K % 64: the kernel refuses the shape


# ---- end to end ------------------------------------------------------------------------------
def _labels(T, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (1, T), generator=g)
    labels = ids.clone()
    labels[0, 250:262] = -100                           # a run of ignored labels across the boundary at 256
    labels[0, 511:513] = -100                           # the target of the LAST position of the second chunk is ignored
    labels[0, :5] = -100
    return ids.to(DEV), labels.to(DEV)


def test_score_sequence_equals_chunked_hidden_states_plain_kernel_float64(small):
    """vocab 512, hidden 256, T = 600 in chunks of 256: boundaries at 256 and 512 and a ragged tail of 88."""
    from infinitevl_amd.harness import score_sequence
    stack, hc = small
    T, chunk, nxt = 600, 256, 5
    ids, labels = _labels(T, hc.vocab_size, 71)
    with torch.no_grad():
        res = score_sequence(stack, stack.allocate_inference_cache(1), input_ids=ids, labels=labels, chunk=chunk, next_label=nxt)
        cache = stack.allocate_inference_cache(1)
        logits = []
        for a in range(0, T, chunk):
            h, none = stack(input_ids=ids[:, a:a + chunk], past_key_values=cache, logits_to_keep=0)
            assert none is None
            logits.append(plain(h[0].contiguous(), stack.embed_tokens.weight, None))
    y = torch.cat(logits)
    hand = torch.tensor(scoring.shifted_by_hand(labels[0].tolist(), nxt))
    assert torch.equal(res.targets.cpu()[0], hand)
    ref_lp, ref_top1, _ = scoring.ref_logprob(y, hand)
    ratio = scoring.judge(res.logprobs[0], ref_lp, "score_sequence logprobs")
    print(f"  end to end: max |err| / tolerance = {ratio:.3f}")
    assert torch.equal(res.top1.cpu()[0], ref_top1)
    n = int((hand >= 0).sum())
    assert n == T - 12 - 2 - 4 and res.n_scored.item() == n and res.n_scored.dtype == torch.int64
    assert bool((res.logprobs[0].cpu()[hand < 0].view(torch.int32) == 0).all())
    assert res.nll.dtype == torch.float64 and res.nll.item() == -res.logprobs.double().sum().item()
    assert abs(res.nll.item() + ref_lp.sum().item()) <= scoring.tolerance(ref_lp).sum().item()
    assert res.perplexity.item() == pytest.approx(math.exp(-ref_lp.sum().item() / n), rel=2e-5)     # exp of nll / n: 1.1e-5 at most
    acc = (ref_top1 == hand).sum().item() / n
    assert res.accuracy.item() == pytest.approx(acc, abs=1e-12)
    # no next_label: the last position is not scored, everything before it is unchanged
    with torch.no_grad():
        res2 = score_sequence(stack, stack.allocate_inference_cache(1), input_ids=ids, labels=labels[0], chunk=chunk)
    assert res2.logprobs.shape == (T,) and res2.n_scored.item() == n - 1 and res2.logprobs[-1].item() == 0.0
    assert torch.equal(res2.logprobs[:-1], res.logprobs[0, :-1]) and torch.equal(res2.top1, res.top1[0])


def test_decoder_score_on_a_forked_slot_equals_score_sequence_and_leaves_the_source(small):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, score_sequence
    stack, hc = small
    cache = MultiStreamCache(config=hc, n_slots=3, device=DEV, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(stack, cache)
    dec.PREFILL_CHUNK = 128                               # (this object only) several calls for a 300-token candidate
    dec.admit(0, fk.prompt(hc, 130, 81, DEV)[0])
    T = 300
    cand, cand_ids = fk.prompt(hc, T, 82, DEV)
    labels = cand_ids.to(DEV)
    labels[100:140] = -100
    b1 = stack.allocate_inference_cache(1)
    cache.store(0, b1)                                    # a B = 1 cache carrying the same stream
    before = [t[0].clone() for t in cache.row_tensors()] + [dec.token[0].clone(), dec.position_ids[:, 0].clone()]
    dec.fork(0, [1])
    got = dec.score(1, cand, labels, next_label=3)
    pos = torch.arange(130, 130 + T, device=DEV)[None, None].expand(3, 1, T)
    want = score_sequence(stack, b1, inputs_embeds=cand, labels=labels, position_ids=pos, chunk=128, next_label=3)
    torch.cuda.synchronize()
    for name in ("logprobs", "top1", "targets", "n_scored", "nll"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.n_scored.item() == T - 40 and bool((got.logprobs[got.targets >= 0] < 0).all())
    after = [t[0] for t in cache.row_tensors()] + [dec.token[0], dec.position_ids[:, 0]]
    for i, (u, v) in enumerate(zip(before, after)):
        assert torch.equal(u, v), ("the source slot changed", i)
    assert cache.slot_lengths[:2] == [130, 130 + T] and dec.position_ids[:, 1, 0].tolist() == [130 + T] * 3
    assert dec.token[1].item() == 0
    dec.release(1)
    assert cache.slot_lengths[1] == 0
    with pytest.raises(ValueError, match="holds no stream"):
        dec.score(2, cand, labels)


def test_score_sequence_runs_in_constant_memory_at_the_full_vocabulary():
    """T = 4096 at vocab 151936 in ONE call of 4096 tokens: the peak of allocated memory rises by less than ONE [256, 151936]
    bf16 tensor (77.8 MB) over the same call unscored (expected: the 9.7 MB workspace and a few [T] vectors)."""
    from infinitevl_amd import ops
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack, score_sequence
    lt = ["sliding_attention", "linear_attention"]
    cfg = InfiniteVLTextConfig(vocab_size=151936, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                               num_attention_heads=2, num_key_value_heads=1, head_dim=128, sliding_window=96, layer_types=lt,
                               num_linear_heads=2, num_linear_key_value_heads=2, linear_head_dim=128, rope_theta=1e6)
    stack = InfiniteVLTextStack(cfg).to(DEV, torch.bfloat16).eval()
    stack.init_weights_(seed=0)
    stack.fuse_()
    T = 4096
    ids = torch.randint(0, cfg.vocab_size, (1, T), generator=torch.Generator().manual_seed(91)).to(DEV)

    def peak(fn):
        cache = stack.allocate_inference_cache(1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(cache)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    with torch.no_grad():
        unscored = lambda c: stack(input_ids=ids, past_key_values=c, logits_to_keep=0)[0]
        peak(unscored)                                                      # (the stack's own workspaces exist from here on)
        ops._WORKSPACES.pop((torch.cuda.current_device(), "logprob"), None)   # the scoring workspace counts as part of the rise
        p_plain, _ = peak(unscored)
        p_score, res = peak(lambda c: score_sequence(stack, c, input_ids=ids, labels=ids, chunk=T))
    one_piece = 256 * cfg.vocab_size * 2
    print(f"  peak over the call: unscored {p_plain / 1e6:.1f} MB, scored {p_score / 1e6:.1f} MB, rise {(p_score - p_plain) / 1e6:.1f} MB "
          f"(one [256, vocab] bf16 tensor: {one_piece / 1e6:.1f} MB)")
    assert p_score - p_plain < one_piece
    assert res.n_scored.item() == T - 1 and math.isfinite(res.nll.item()) and res.nll.item() > 0

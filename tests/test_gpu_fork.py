"""GPU (-m gpu): a stream's state forked into other slots in one launch.

  1. ops.RowCopyPlan (ivl_rows_copy_fwd) against torch indexing, bit for bit: rows of 8 B to 1 MiB + 48 B, unaligned views, a
     column slice; separate tensors and rows inside one tensor; guard bytes and every other row untouched;
  2. MultiStreamCache.fork after the ring has wrapped;
  3. a forked slot decodes exactly as a slot that prefilled the same prompt itself;
  4. a fork between replays: no recapture, the graph equals the eager run;
  5. admit_n: one prefill, n independent sampled answers == n admissions;
  6. the streaming demo's branch: load from a B = 1 stream cache, extend with a question, decode; the source stays untouched;
  7. store + load == fork;
  8. the model's real width: one launch is not slower than the per-tensor copy_ loop;
  9. admit refuses an empty prompt before any state is touched;
 10. capture() of each of the four graphed classes leaves every tensor the object owns as it was."""
import statistics

import pytest
import torch

import fork as fk
from conftest import rms_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@pytest.fixture(scope="module")
def small():
    return fk.small_stack(DEV)


def _decoder(small, n_slots, sampler=None):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = small
    cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=torch.bfloat16)
    return GraphedMultiStreamDecode(stack, cache, sampler=sampler), cache


# ---------------------------------------------------------------------------------------------
# 1. the operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_rows, dst_rows", [((1, 3), [1]), ((2, 1), [0, 2, 4]), ((4, 0), [1, 2, 3, 4])], ids=["to1", "to024", "to1234"])
@pytest.mark.parametrize("inside", [False, True], ids=["separate", "same_tensor"])
def test_rows_copy_bit_equal_to_indexing(inside, src_rows, dst_rows):
    """Between separate tensors the source row is one of the destination rows too: that destination sits at the source's offset
    in a 16-byte line whatever the row stride, so `to1` takes the 16-byte path with its byte head and tail for every pair, and
    the other sets mix it with destinations at other offsets.  Inside one tensor the source row is not a destination."""
    from infinitevl_amd import ops
    src_row = src_rows[1] if inside else src_rows[0]
    src_raw = fk.raw_buffers(1, DEV)
    dst_raw = src_raw if inside else fk.raw_buffers(2, DEV)
    want_raw = [r.clone() for r in dst_raw]
    src0 = [t.clone() for t in fk.typed_views([r.clone() for r in src_raw])]       # the source rows before the call
    for want, s in zip(fk.typed_views(want_raw), src0):
        for d in dst_rows:
            want[d] = s[src_row]
    src_before = [r.clone() for r in src_raw]
    plan = ops.RowCopyPlan(list(zip(fk.typed_views(src_raw), fk.typed_views(dst_raw))))
    assert plan.n_entries == len(fk.SPECS) and plan.same == [inside] * len(fk.SPECS) and plan.max_row_bytes == 2 ** 20 + 48
    assert plan.n_pieces == 1 + 1 + 1 + 1 + 2 + 2 + 65 + 1
    plan.run(src_row, dst_rows)
    torch.cuda.synchronize()
    for (name, *_), got, want, s_now, s_was in zip(fk.SPECS, dst_raw, want_raw, src_raw, src_before):
        assert torch.equal(got, want), name            # destination rows == the source row; other rows, gaps and guards unchanged
        if not inside:
            assert torch.equal(s_now, s_was), name


# ---------------------------------------------------------------------------------------------
# 2. the cache
# ---------------------------------------------------------------------------------------------
def test_cache_fork_after_the_ring_wrapped(small):
    _, hc = small
    dec, cache = _decoder(small, 4)
    dec.admit(0, fk.prompt(hc, 130, 11, DEV)[0])       # capacity 95: the ring has wrapped
    dec.admit(3, fk.prompt(hc, 40, 12, DEV)[0])
    rows3 = [t[3].clone() for t in cache.row_tensors()]
    assert cache.slot_lengths == [130, 0, 0, 40]
    cache.fork(0, [1, 2])
    torch.cuda.synchronize()
    for d in (1, 2):
        fk.assert_rows_equal(cache, 0, d)
    assert cache.pos_rows.tolist() == [130, 130, 130, 40] and cache.slot_lengths == [130, 130, 130, 40]
    for t, was in zip(cache.row_tensors(), rows3):
        assert torch.equal(t[3], was)
    assert any(bool(t[0].any()) for t in cache.row_tensors()[:-1])


# ---------------------------------------------------------------------------------------------
# 3. fork == re-prefill
# ---------------------------------------------------------------------------------------------
def test_forked_slots_decode_as_slots_that_prefilled_themselves(small):
    _, hc = small
    x = fk.prompt(hc, 130, 21, DEV)[0]
    X, xc = _decoder(small, 3)
    Y, yc = _decoder(small, 3)
    for s in range(3):
        X.admit(s, x)
    Y.admit(0, x)
    Y.fork(0, [1, 2])
    torch.cuda.synchronize()
    for s in (1, 2):                                   # the precondition: prefill is deterministic
        fk.assert_rows_equal(xc, 0, s, "precondition")
    assert torch.equal(X.token, Y.token) and torch.equal(X.position_ids, Y.position_ids)
    assert yc.slot_lengths == xc.slot_lengths == [130] * 3
    for i in range(8):
        X.step()
        Y.step()
        assert torch.equal(Y.logits, X.logits), i
        assert torch.equal(Y.token, X.token), i
    assert yc.slot_lengths == xc.slot_lengths == [138] * 3


# ---------------------------------------------------------------------------------------------
# 4. no recapture
# ---------------------------------------------------------------------------------------------
def _fork_schedule(small, graph):
    _, hc = small
    dec, cache = _decoder(small, 4)
    dec.admit(0, fk.prompt(hc, 130, 31, DEV)[0])
    dec.admit(1, fk.prompt(hc, 70, 32, DEV)[0])
    out, first = [], None
    for i in range(9):
        if i == 3:
            first = dec.graph
            dec.fork(0, [2, 3])
        dec.step(graph=graph)
        out.append((dec.logits.clone(), dec.token.clone()))
    torch.cuda.synchronize()
    return dec, first, out


def test_fork_between_replays_without_recapture(small):
    dec, first, got = _fork_schedule(small, True)
    assert first is not None and dec.graph is first
    _, none, want = _fork_schedule(small, False)
    assert none is None
    for i, ((lg, tk), (lw, tw)) in enumerate(zip(got, want)):
        assert torch.equal(lg, lw) and torch.equal(tk, tw), i


# ---------------------------------------------------------------------------------------------
# 5. admit_n
# ---------------------------------------------------------------------------------------------
def test_admit_n_equals_n_admissions(small):
    from infinitevl_amd.harness import Sampler
    _, hc = small
    x, ids = fk.prompt(hc, 130, 41, DEV)
    sampling = [{"temperature": 0.8, "seed": s, "repetition_penalty": 1.3} for s in (1, 2, 3)]

    def build():
        return _decoder(small, 3, sampler=Sampler(3, DEV, vocab_size=hc.vocab_size, history=32, logprobs=3))[0]

    A, B = build(), build()
    first = A.admit_n([0, 1, 2], x, sampling=sampling, prompt_ids=ids)
    for s in range(3):
        B.admit(s, x, sampling=sampling[s], prompt_ids=ids)
    assert torch.equal(first, B.token) and first.shape == (3, 1)
    toks = [A.token[:, 0].tolist()]
    for i in range(12):
        A.step()
        B.step()
        assert torch.equal(A.token, B.token), i
        toks.append(A.token[:, 0].tolist())
    torch.cuda.synchronize()
    a, b = A.sampler, B.sampler
    for ta, tb in zip(a.row_tensors(), b.row_tensors()):          # parameters, seen bitmaps, counters, histories, score rings
        assert ta.cpu().numpy().tobytes() == tb.cpu().numpy().tobytes()
    assert a.n_new.tolist() == [13] * 3 and a._ends == b._ends
    for s in range(3):
        assert a.tokens(s).tolist() == [t[s] for t in toks] == b.tokens(s).tolist()
        assert a.logprobs(s).numpy().tobytes() == b.logprobs(s).numpy().tobytes() and a.logprobs(s).numel() == 13
    assert a.cum_logprob.cpu().numpy().tobytes() == b.cum_logprob.cpu().numpy().tobytes()
    seqs = {tuple(t[s] for t in toks) for s in range(3)}
    assert len(seqs) >= 2                                          # the draws really are independent


# ---------------------------------------------------------------------------------------------
# 6. the demo's flow
# ---------------------------------------------------------------------------------------------
def _source_snapshot(cache):
    out = []
    for layer in cache.layers:
        out.append(([t.clone() for t in layer.carried_tensors()],
                    {k: v for k, v in vars(layer).items() if k in ("size", "cumulative_length", "seq_len", "start")},
                    layer._pos_dev.clone() if hasattr(layer, "_pos_dev") else None))
    return out


def test_load_from_a_stream_cache_then_extend(small):
    stack, hc = small
    frames = [fk.prompt(hc, 64, 50 + i, DEV)[0] for i in range(2)]
    questions = {1: fk.prompt(hc, 7, 61, DEV)[0], 2: fk.prompt(hc, 12, 62, DEV)[0]}
    calls = [(frames[0], 0), (frames[1], 64)]

    def feed(cache, x, start):
        T = x.shape[1]
        pid = torch.arange(start, start + T, device=DEV)[None, None, :].expand(3, 1, T)
        with torch.no_grad():
            return stack(inputs_embeds=x, position_ids=pid, past_key_values=cache, logits_to_keep=1)[1]

    video = stack.allocate_inference_cache(1)
    for x, start in calls:
        feed(video, x, start)
    before = _source_snapshot(video)
    dec, cache = _decoder(small, 3)
    dec.load([1, 2], video, next_position=128)
    assert cache.slot_lengths == [0, 128, 128] and dec.position_ids[:, 1:, 0].tolist() == [[128, 128]] * 3
    for s, q in questions.items():
        dec.extend(s, q)
    # the control: the same three calls on each slot's view, by hand
    ctl, ccache = _decoder(small, 3)
    for s, q in questions.items():
        ccache.admit(s)
        view = ccache.slot_view(s)
        for x, start in calls:
            feed(view, x, start)
        lg = feed(view, q, 128)
        ctl.token[s].copy_(lg[0, -1].argmax(-1, keepdim=True))
        ctl.position_ids[:, s].fill_(128 + q.shape[1])
    assert torch.equal(dec.admit_logits, lg)                     # the latest extend's
    assert torch.equal(dec.token, ctl.token) and torch.equal(dec.position_ids, ctl.position_ids)
    assert cache.slot_lengths == ccache.slot_lengths == [0, 135, 140]
    for i in range(8):
        dec.step()
        ctl.step()
        assert torch.equal(dec.logits, ctl.logits), i
    torch.cuda.synchronize()
    for (ts, host, pos), (ts0, host0, pos0) in zip(_source_snapshot(video), before):      # questions never touched the video
        assert host == host0 and all(torch.equal(a, b) for a, b in zip(ts, ts0))
        assert pos is None or torch.equal(pos, pos0)
    assert video.get_seq_length() == 128


# ---------------------------------------------------------------------------------------------
# 7. store then load
# ---------------------------------------------------------------------------------------------
def test_store_then_load_equals_fork(small):
    stack, hc = small
    dec, cache = _decoder(small, 4)
    dec.admit(0, fk.prompt(hc, 130, 71, DEV)[0])
    for _ in range(2):
        dec.step()
    n = cache.slot_lengths[0]
    assert n == 132
    b1 = stack.allocate_inference_cache(1)
    cache.store(0, b1)
    cache.load([1], b1)
    cache.fork(0, [2])
    torch.cuda.synchronize()
    fk.assert_rows_equal(cache, 1, 2)
    fk.assert_rows_equal(cache, 0, 1)
    assert cache.pos_rows.tolist()[:3] == [n] * 3
    # the stored cache is a complete B = 1 cache: counters as import_carried(n) leaves them, and a plain forward counts on
    ref = stack.allocate_inference_cache(1)
    for layer in ref.layers:
        layer.import_carried(n)
    for a, b in zip(b1.layers, ref.layers):
        assert {k: v for k, v in vars(a).items() if k in ("size", "cumulative_length", "seq_len", "start")} == \
               {k: v for k, v in vars(b).items() if k in ("size", "cumulative_length", "seq_len", "start")}
    assert b1.layers[0]._pos_dev.tolist() == [n] and b1.get_seq_length() == n
    with torch.no_grad():
        pid = torch.full((3, 1, 1), n, device=DEV, dtype=torch.int64)
        _, lg = stack(input_ids=dec.token[0:1], position_ids=pid, past_key_values=b1)
    assert b1.get_seq_length() == n + 1 and b1.layers[0]._pos_dev.tolist() == [n + 1]
    dec.step(graph=False)                                         # the same token in the slot it came from
    assert rms_rel(lg[0, -1].float().cpu(), dec.logits[0, -1].float().cpu()) < 4e-3


# ---------------------------------------------------------------------------------------------
# 9. a refused admission
# ---------------------------------------------------------------------------------------------
def test_admit_refuses_an_empty_prompt_before_it_touches_anything(small):
    _, hc = small
    dec, cache = _decoder(small, 2)
    dec.admit(0, fk.prompt(hc, 5, 81, DEV)[0])
    rows = [t.clone() for t in cache.row_tensors()]
    with pytest.raises(ValueError, match=r"admit: inputs_embeds must be \[1,T,hidden\]"):
        dec.admit(1, torch.zeros(1, 0, hc.hidden_size, dtype=torch.bfloat16, device=DEV))
    assert cache.slot_lengths == [5, 0] and dec._live == {0}
    for t, was in zip(cache.row_tensors(), rows):
        assert torch.equal(t, was)


# ---------------------------------------------------------------------------------------------
# 10. capture() has no side effects
# ---------------------------------------------------------------------------------------------
def _graphed_step(small):
    """The T and the once-fed B = 1 cache of the capture test in tests/test_gpu_parity.py."""
    from infinitevl_amd.harness import GraphedStep
    stack, hc = small
    T = 70
    cache = stack.allocate_inference_cache(1, zero_init=True)
    with torch.no_grad():
        stack(inputs_embeds=fk.prompt(hc, T, 91, DEV)[0], past_key_values=cache)
    gs = GraphedStep(stack, cache, 1, T)
    gs.inputs_embeds.copy_(fk.prompt(hc, T, 92, DEV)[0])
    return gs


def _graphed_decode(small):
    from infinitevl_amd.harness import GraphedDecode, Sampler
    stack, hc = small
    cache = stack.allocate_inference_cache(2, zero_init=True)
    with torch.no_grad():
        stack(inputs_embeds=torch.cat([fk.prompt(hc, 5, 93 + b, DEV)[0] for b in range(2)]), past_key_values=cache)
    smp = Sampler(2, DEV, vocab_size=hc.vocab_size, history=8)
    for b in range(2):
        smp.set(b, temperature=0.8, seed=b + 1, repetition_penalty=1.3)
    dec = GraphedDecode(stack, cache, 2, sampler=smp)
    dec.token.copy_(torch.tensor([[7], [300]]))
    return dec


def _graphed_multistream(small):
    from infinitevl_amd.harness import Sampler
    _, hc = small
    dec, _ = _decoder(small, 4, sampler=Sampler(4, DEV, vocab_size=hc.vocab_size, history=8, logprobs=2))
    for slot, T in ((0, 5), (2, 100)):                 # below the window of 96 and past it: that slot's ring has wrapped
        x, ids = fk.prompt(hc, T, 95 + slot, DEV)
        dec.admit(slot, x, sampling=dict(temperature=0.8, seed=slot + 1, repetition_penalty=1.3), prompt_ids=ids)
    return dec


def _graphed_beam(small):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode
    stack, hc = small
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=torch.bfloat16)
    dec = GraphedBeamDecode(stack, cache, 2, hc.vocab_size, 16)
    x, ids = fk.prompt(hc, 100, 99, DEV)
    dec.admit(1, x, prompt_ids=ids, max_new_tokens=12, stop_token_ids=[3], repetition_penalty=1.3)
    return dec


def _owned(obj):
    """Every tensor the graphed object owns on the host, by name, and the host counters of its cache."""
    out, cache = {}, obj.cache
    if hasattr(cache, "row_tensors"):
        out.update({f"cache.{i}": t for i, t in enumerate(cache.row_tensors())})
        host = list(cache.slot_lengths)
    else:
        snap = _source_snapshot(cache)
        out.update({f"cache.{i}.{j}": t for i, (ts, _, _) in enumerate(snap) for j, t in enumerate(ts)})
        out.update({f"cache.{i}.pos": pos for i, (_, _, pos) in enumerate(snap) if pos is not None})
        host = [h for _, h, _ in snap]
    out["position_ids"] = obj.position_ids
    for name in ("token", "stop_ids"):
        if getattr(obj, name, None) is not None:
            out[name] = getattr(obj, name)
    if getattr(obj, "sampler", None) is not None:
        out.update({f"sampler.{i}": t for i, t in enumerate(obj.sampler.row_tensors())})
    out.update({f"beam.{k}": t for k, t in getattr(obj, "beam", {}).items()})
    return {k: t.cpu() for k, t in out.items()}, host


@pytest.mark.parametrize("build, eager", [(_graphed_step, False), (_graphed_decode, False), (_graphed_multistream, True),
                                          (_graphed_beam, True)], ids=["step", "decode", "multistream", "beam"])
def test_capture_leaves_every_tensor_as_it_was(small, build, eager):
    """The warm-up runs and the captured run themselves advance the cache, the positions, the token, the sampler's state and
    the beam tables: all of it is back afterwards, bit for bit, and the graph then steps as the eager step does (where the
    class offers one; the other two have their own graph-against-eager tests)."""
    obj = build(small)
    torch.cuda.synchronize()
    before, host = _owned(obj)
    obj.capture()
    torch.cuda.synchronize()
    after, host_after = _owned(obj)
    assert obj.graph is not None and host_after == host and after.keys() == before.keys()
    for k, was in before.items():
        assert torch.equal(after[k], was), k
    if eager:
        ref = build(small)
        for i in range(3):
            obj.step()
            ref.step(graph=False)
            assert torch.equal(obj.token, ref.token), i


# ---------------------------------------------------------------------------------------------
# 8. the model's real width
# ---------------------------------------------------------------------------------------------
def test_real_width_fork_is_not_slower_than_the_copy_loop():
    """One launch against 378 copy_ launches, each timed with events over 5 interleaved repetitions; the medians are compared."""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(sliding_window=4096)
    with torch.device(DEV):
        torch.set_default_dtype(torch.bfloat16)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(torch.bfloat16).eval()
    model.init_weights_(seed=0)
    model.fuse_()
    cache = MultiStreamCache(config=cfg, n_slots=4, device=DEV, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(model, cache)
    gen = torch.Generator(device=DEV).manual_seed(5)
    T = 4096 + 700
    dec.admit(0, (torch.randn(1, T, cfg.hidden_size, generator=gen, device=DEV) * 0.5).to(torch.bfloat16))
    rows = cache.row_tensors()
    assert len(rows) == 126 + 1
    cache.fork(0, [1, 2, 3])
    torch.cuda.synchronize()
    for d in (1, 2, 3):
        fk.assert_rows_equal(cache, 0, d)
    assert cache.pos_rows.tolist() == [T] * 4 and cache.slot_lengths == [T] * 4

    def loop():
        for t in rows:
            for d in (1, 2, 3):
                t[d].copy_(t[0])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    loop()
    torch.cuda.synchronize()
    t_fork, t_loop = [], []
    for _ in range(5):
        t_fork.append(timed(lambda: cache.fork(0, [1, 2, 3])))
        t_loop.append(timed(loop))
    m_fork, m_loop = statistics.median(t_fork), statistics.median(t_loop)
    print(f"fork to 3 slots: {m_fork * 1e3:.1f} us, copy_ loop: {m_loop * 1e3:.1f} us ({t_fork} / {t_loop})")
    assert m_fork <= m_loop, (t_fork, t_loop)

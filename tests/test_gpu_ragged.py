"""GPU (-m gpu): the ragged frame step at operator level -- a token count per batch row, read on the device.

  * ops.gdn_chunk_fused(n_rows=) (ivl_gdn_chunk_fused_rows_fwd, RAG-1..4): row b against row b of the unmasked two-launch call over
    T = n_b tokens on the same B, bit for bit (output, recurrent state, the three conv states); NaN in the masked tokens and in every
    state of a row that sits the call out; one captured call serves changing counts;
  * ops.swa_forward_rows(n_rows=) (ivl_swa_rows_n_fwd, RAG-5..10): o[b, :n_b] against the unmasked call on zero-filled masked inputs, the
    ring row against the T = n_b call, NaN in masked inputs and unread ring slots, capture and replay;
  * the stack (GraphedRaggedStep on the small model of test_gpu_frames.py, 4 slots, window 96, T = 130): every n = T is the unmasked
    stepper bit for bit; lengths [5, 0, 130, 64] against the unmasked step on zeros, the idle slot byte-equal; three ticks, one graph."""
import functools

import pytest
import torch

import frames
import ragged
from frames import CASES, D, words
from ragged import NAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = D ** -0.5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


# ---------------------------------------------------------------------------------------------
# GDN
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gdn_inputs(B, T, H):
    return ragged.gdn_inputs(B, T, H, DEV)


@functools.lru_cache(maxsize=None)
def _gdn_ref(B, T, H, n):
    """the unmasked call over n tokens of every row (computed once per n, shared by the cases)"""
    out = ragged.gdn_unmasked(_gdn_inputs(B, T, H), H, n)
    torch.cuda.synchronize()
    return out


GDN_CASES = [
    (3, 130, 2, (130, 130, 130)),        # three chunks, a partial last one; every row whole: also THE unmasked T = 130 call
    (3, 130, 2, (0, 64, 130)),
    (3, 130, 2, (1, 3, 65)),             # conv states that mix old and new inputs
    (3, 130, 2, (129, 2, 0)),
    (3, 70, 12, (70, 5, 0)),             # B * H * 4 > 128: the 64-column scan workgroups
]


@pytest.mark.parametrize("B,T,H,lengths", GDN_CASES)
def test_gdn_rows_equal_the_unmasked_call_of_their_length(B, T, H, lengths):
    from infinitevl_amd import ops
    inp = _gdn_inputs(B, T, H)
    calls = ops.RAGGED_CALLS
    got = ragged.gdn_ragged(inp, H, lengths)
    torch.cuda.synchronize()
    assert ops.RAGGED_CALLS == calls + 1
    refs = {n: _gdn_ref(B, T, H, n) for n in set(lengths) if n > 0}
    ragged.assert_rag1(inp, H, lengths, got, refs, tag=str(lengths))


def test_gdn_rows_ignore_their_neighbours():
    """RAG-2: row 1 (n = 64) next to other rows, other lengths and other garbage behind its own tokens: the same bits"""
    B, T, H = 3, 130, 2
    inp = _gdn_inputs(B, T, H)
    a = ragged.gdn_ragged(inp, H, (0, 64, 130))
    proj, cols, cw, cs, A32, dt32, h0 = inp
    proj2, _, _, cs2, _, _, h02 = ragged.gdn_inputs(B, T, H, DEV, seed=1)      # what the other rows hold; the weights are the call's
    proj2[1, :64] = proj[1, :64]                                     # row 1: the same valid tokens, inf behind them
    proj2[1, 64:] = float("inf")
    for s2, s in zip(cs2, cs):
        s2[1] = s[1]
    h02[1] = h0[1]
    b = ragged.gdn_ragged((proj2, cols, cw, cs2, A32, dt32, h02), H, (130, 64, 7), poison=False)
    torch.cuda.synchronize()
    assert torch.equal(words(a[0][1, :64]), words(b[0][1, :64]))
    assert torch.equal(words(a[2][1]), words(b[2][1]))
    for x, y in zip(a[1], b[1]):
        assert torch.equal(words(x[1]), words(y[1]))


def test_gdn_counts_are_clamped_on_the_device():
    B, T, H = 3, 130, 2
    inp = _gdn_inputs(B, T, H)
    from infinitevl_amd import ops
    proj, cols, cw, cs, A32, dt32, h0 = inp
    so, ht = [c.clone() for c in cs], h0.clone()
    before = [s.clone() for s in so] + [ht.clone()]
    n_rows = torch.tensor([-5, 64, 9000], dtype=torch.int32, device=DEV)
    o = ops.gdn_chunk_fused(proj, cols, cw, so, so, A32, dt32, H, ragged.K, ragged.V, initial_state=ht, final_state_out=ht, n_rows=n_rows)
    torch.cuda.synchronize()
    refs = {n: _gdn_ref(B, T, H, n) for n in (64, 130)}
    ragged.assert_rag1(inp, H, (0, 64, 130), (o, so, ht, before), refs, tag="clamped")


def test_gdn_without_counts_is_the_unmasked_call():
    from infinitevl_amd import ops
    B, T, H = 3, 130, 2
    proj, cols, cw, cs, A32, dt32, h0 = _gdn_inputs(B, T, H)
    lib = ops._lib.load()
    so, ht = [c.clone() for c in cs], h0.clone()
    o = torch.empty(B, T, H, ragged.V, dtype=ragged.BF, device=DEV)
    ws = torch.empty(lib.ivl_gdn_chunk_workspace_bytes(B, T, H, ragged.K, ragged.V), dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()      # noqa: E731
    rc = lib.ivl_gdn_chunk_fused_rows_fwd(p(proj), proj.shape[-1], *cols, p(cw[0]), p(cw[1]), p(cw[2]), p(so[0]), p(so[1]), p(so[2]), p(so[0]),
                                          p(so[1]), p(so[2]), p(A32), p(dt32), p(o), p(ht), ops._lib.IVL_BF16, p(ht), ops._lib.IVL_BF16, B, T, H,
                                          ragged.K, ragged.V, 4, ragged.K ** -0.5, ops._lib.IVL_BF16, p(ws), ws.numel(), None, None)
    torch.cuda.synchronize()
    assert rc == 0
    ro, rso, rht = _gdn_ref(B, T, H, T)
    assert torch.equal(o, ro) and torch.equal(ht, rht) and all(torch.equal(x, y) for x, y in zip(so, rso))


def test_gdn_replay_reads_the_counts():
    """RAG-4: one captured call, two length vectors: each replay equals the eager call with those counts"""
    from infinitevl_amd import ops
    B, T, H = 3, 130, 2
    proj, cols, cw, cs, A32, dt32, h0 = _gdn_inputs(B, T, H)
    so, ht = [c.clone() for c in cs], h0.clone()
    n_rows = torch.tensor([T] * B, dtype=torch.int32, device=DEV)

    def call():
        return ops.gdn_chunk_fused(proj, cols, cw, so, so, A32, dt32, H, ragged.K, ragged.V, initial_state=ht, final_state_out=ht, n_rows=n_rows)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    ops.prepare_gdn_capture(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = call()
    for lengths in ((0, 64, 130), (129, 2, 0)):
        n_rows.copy_(torch.tensor(lengths, dtype=torch.int32))
        for x, y in zip(so + [ht], cs + [h0]):
            x.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        eager = ragged.gdn_ragged(_gdn_inputs(B, T, H), H, lengths, poison=False)
        torch.cuda.synchronize()
        for b, n in enumerate(lengths):
            assert torch.equal(words(o[b, :n]), words(eager[0][b, :n])), (lengths, b)
        assert torch.equal(ht, eager[2]) and all(torch.equal(x, y) for x, y in zip(so, eager[1])), lengths


# ---------------------------------------------------------------------------------------------
# SWA: shapes a (64-row form), c (prefill, 3 splits, rope pre-pass) and d (tail tile, T > C) of tests/frames.py
# ---------------------------------------------------------------------------------------------
# per case: length vectors, one count per row, from {0, 1, 63, 64, 65, T - 1, T} (a count above T is clamped to T)
SWA_LENGTHS = {
    "a": [(0, 1, 39, 40, 17, 63)],                                   # T = 40
    "c": [(0, 63, 256), (64, 65, 255), (1, 256, 0)],                 # T = 256
    "d": [(0, 1, 63, 64, 65, 129, 130, 96)],                         # T = 130, C = 95: n_b > C (96, 129, 130) and n_b < C < T (1 .. 65)
}


@functools.lru_cache(maxsize=None)
def _swa_inputs(name):
    return frames.case_tensors(name, DEV, nan_unread=True)


def _rows_call(name, q, k, v, kc, vc, pos_rows, rope, n_rows=None):
    from infinitevl_amd import ops
    T, C, _ = CASES[name]
    kr, vr = kc.clone(), vc.clone()
    o = ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=kr, v_cache=vr, pos_rows=pos_rows, rope=rope, append=True,
                             n_rows=n_rows)
    return o, kr, vr


@functools.lru_cache(maxsize=None)
def _swa_short(name, use_rope, n):
    """rings after ivl_swa_rows_fwd with T = n on the first n tokens of every row (RAG-6's reference, once per n)"""
    q, k, v, kc, vc, pos_rows, rope = _swa_inputs(name)
    rope_n = (rope[0][:, :, :n].contiguous(), rope[1][:, :, :n].contiguous(), rope[2]) if use_rope else None
    _, kr, vr = _rows_call(name, q[:, :n].contiguous(), k[:, :n].contiguous(), v[:, :n].contiguous(), kc, vc, pos_rows, rope_n)
    torch.cuda.synchronize()
    return kr, vr


def _masked(x, lengths, value):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, n:] = value
    return x


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("name,lengths", [(n, l) for n in sorted(SWA_LENGTHS) for l in SWA_LENGTHS[n]])
def test_swa_rows_n(name, lengths, use_rope):
    from infinitevl_amd import ops
    T, C, positions = CASES[name]
    q, k, v, kc, vc, pos_rows, rope = _swa_inputs(name)
    rope = rope if use_rope else None
    nb = [min(n, T) for n in lengths]
    n_rows = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    calls = ops.RAGGED_CALLS
    o, kr, vr = _rows_call(name, _masked(q, nb, NAN), _masked(k, nb, NAN), _masked(v, nb, NAN), kc, vc, pos_rows, rope, n_rows)
    o0, _, _ = _rows_call(name, _masked(q, nb, 0), _masked(k, nb, 0), _masked(v, nb, 0), kc, vc, pos_rows, rope)
    torch.cuda.synchronize()
    assert ops.RAGGED_CALLS == calls + 1
    assert pos_rows.tolist() == positions                           # RAG-8
    for b, n in enumerate(nb):
        assert torch.isfinite(o[b, :n].float()).all(), (name, b, n)              # RAG-9
        assert torch.equal(words(o[b, :n]), words(o0[b, :n])), (name, "o", b, n)  # RAG-5
        if n == 0:                                                   # RAG-7
            assert torch.equal(words(kr[b]), words(kc[b])) and torch.equal(words(vr[b]), words(vc[b])), (name, "ring of an idle row", b)
        else:                                                        # RAG-6
            ks, vs = _swa_short(name, use_rope, n)
            assert torch.equal(words(kr[b]), words(ks[b])), (name, "k ring", b, n)
            assert torch.equal(words(vr[b]), words(vs[b])), (name, "v ring", b, n)


def test_swa_replay_reads_the_counts():
    """RAG-10: capture case c, change the counts in place, replay == the eager call with those counts"""
    name = "c"
    T, C, positions = CASES[name]
    q, k, v, kc, vc, pos_rows, rope = _swa_inputs(name)
    from infinitevl_amd import ops
    kr, vr = kc.clone(), vc.clone()
    n_rows = torch.tensor([T] * len(positions), dtype=torch.int32, device=DEV)

    def call():
        return ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=kr, v_cache=vr, pos_rows=pos_rows, rope=rope, append=True,
                                    n_rows=n_rows)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = call()
    for lengths in SWA_LENGTHS[name][:2]:
        n_rows.copy_(torch.tensor(lengths, dtype=torch.int32))
        kr.copy_(kc)
        vr.copy_(vc)
        graph.replay()
        torch.cuda.synchronize()
        o2, k2, v2 = _rows_call(name, q, k, v, kc, vc, pos_rows, rope, torch.tensor(lengths, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        for b, n in enumerate(lengths):
            assert torch.equal(words(o[b, :n]), words(o2[b, :n])), (lengths, b)
        assert torch.equal(words(kr), words(k2)) and torch.equal(words(vr), words(v2)), lengths


# ---------------------------------------------------------------------------------------------
# the stack: the small model of test_gpu_frames.py -- 4 slots, window 96, T = 130
# ---------------------------------------------------------------------------------------------
T_STACK, N_SLOTS, PROMPTS = 130, 4, [5, 70, 130, 33]


@functools.lru_cache(maxsize=None)
def _small():
    import fork
    return fork.small_stack(DEV)


def _bf_randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.5).to(ragged.BF).to(DEV)


def _admitted():
    """a fresh cache with four streams of PROMPTS tokens, and the positions of their next frame"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = _small()
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=ragged.BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    for s, L in enumerate(PROMPTS):
        dec.admit(s, _bf_randn((1, L, hc.hidden_size), 100 + s))
    start = torch.tensor(PROMPTS, dtype=torch.int64, device=DEV)
    pid = (start[None, :, None] + torch.arange(T_STACK, device=DEV)[None, None, :]).expand(3, N_SLOTS, T_STACK).contiguous()
    return stack, hc, cache, dec, pid


def _rows_of(cache):
    return [t.clone() for t in cache.row_tensors()]


@pytest.mark.parametrize("graph", [True, False])
def test_stack_all_lengths_T_is_the_unmasked_step(graph):
    """every n = T: logits, hidden, every row tensor, pos_rows and position_ids bit-equal to GraphedMultiStreamStep"""
    from infinitevl_amd.harness import GraphedMultiStreamStep, GraphedRaggedStep
    out = []
    for cls in (GraphedMultiStreamStep, GraphedRaggedStep):
        stack, hc, cache, _, pid = _admitted()
        st = cls(stack, cache, T_STACK)
        x = _bf_randn((N_SLOTS, T_STACK, hc.hidden_size), 200)
        h, lg = st.step(x, pid, graph=graph)
        torch.cuda.synchronize()
        out.append((h.clone(), lg.clone(), _rows_of(cache), cache.pos_rows.clone(), st.position_ids.clone(), list(cache.slot_lengths)))
    a, b = out
    assert torch.equal(words(a[0]), words(b[0])) and torch.equal(words(a[1]), words(b[1]))
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        assert torch.equal(ragged.words(x), ragged.words(y)), ("row tensor", i)
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and a[5] == b[5] == [L + T_STACK for L in PROMPTS]


def test_stack_ragged_step_and_a_slot_that_sits_out():
    """lengths [5, 0, 130, 64] with NaN in the masked embeddings: hidden[s, :n_s] bit-equal to the unmasked step on zeros there (the
    same GEMM shapes: the same rows); slot 1 keeps every byte; three ticks on one graph, slot_lengths == pos_rows"""
    from infinitevl_amd.harness import GraphedMultiStreamStep, GraphedRaggedStep
    lengths = [5, 0, 130, 64]
    stack, hc, cache, _, pid = _admitted()
    x = _bf_randn((N_SLOTS, T_STACK, hc.hidden_size), 201)
    x0, xn = x.clone(), x.clone()
    for s, n in enumerate(lengths):
        x0[s, n:] = 0
        xn[s, n:] = NAN
    ref_h, _ = GraphedMultiStreamStep(stack, cache, T_STACK).step(x0, pid, graph=False)
    ref_h = ref_h.clone()
    stack, hc, cache, _, pid = _admitted()
    before = _rows_of(cache)
    st = GraphedRaggedStep(stack, cache, T_STACK)
    h, lg = st.step(xn, pid, lengths=lengths)
    torch.cuda.synchronize()
    for s, n in enumerate(lengths):
        assert torch.isfinite(h[s, :n].float()).all(), s
        assert torch.equal(words(h[s, :n]), words(ref_h[s, :n])), ("hidden", s, n)
    for i, (was, now) in enumerate(zip(before, cache.row_tensors())):
        assert torch.equal(ragged.words(was[1]), ragged.words(now[1])), ("slot 1 sat the tick out: row tensor", i)
    assert cache.pos_rows.tolist() == [L + n for L, n in zip(PROMPTS, lengths)] == list(cache.slot_lengths)
    assert st.position_ids[:, :, 0].tolist() == [[L + n for L, n in zip(PROMPTS, lengths)]] * 3
    assert torch.isfinite(lg[[0, 2, 3]].float()).all()
    g0, total = st.graph, list(lengths)
    for tick, ln in enumerate(([130, 7, 0, 1], [0, 130, 65, 63])):
        st.step(_bf_randn((N_SLOTS, T_STACK, hc.hidden_size), 210 + tick), None, lengths=ln)
        total = [a + b for a, b in zip(total, ln)]
    torch.cuda.synchronize()
    assert st.graph is g0                                            # changing the counts never recaptures
    assert cache.pos_rows.tolist() == [L + n for L, n in zip(PROMPTS, total)] == list(cache.slot_lengths)


def test_extend_frames_with_lengths_against_per_slot_extend():
    """extend_frames(lengths=) on one decoder against extend() slot by slot, of the same tokens, on a second one: the same greedy tokens
    and positions; the slot that took nothing keeps its pending token, its three positions and its sampler row"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedRaggedStep, Sampler
    stack, hc = _small()
    lengths = [5, 0, 130, 64]
    decs = []
    for _ in range(2):
        cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=ragged.BF)
        dec = GraphedMultiStreamDecode(stack, cache, sampler=Sampler(N_SLOTS, DEV, vocab_size=hc.vocab_size, history=8))
        for s, L in enumerate(PROMPTS):                           # slot 1 SAMPLES (its row holds a live RNG state), the others are greedy
            dec.admit(s, _bf_randn((1, L, hc.hidden_size), 100 + s),
                      sampling=dict(temperature=0.8, top_k=20, seed=6) if s == 1 else dict(temperature=0.0))
        decs.append(dec)
    a, b = decs
    x = _bf_randn((N_SLOTS, T_STACK, hc.hidden_size), 220)
    xn = x.clone()
    for s, n in enumerate(lengths):
        xn[s, n:] = NAN
    pending, pos1, n_new1 = a.token.clone(), a.position_ids.clone(), a.sampler.n_new.clone()
    rows1 = [t.clone() for t in a.sampler.row_tensors()]
    a.extend_frames(GraphedRaggedStep(stack, a.cache, T_STACK), xn, lengths=lengths)
    for s, n in enumerate(lengths):
        if n > 0:
            b.extend(s, x[s:s + 1, :n])
    torch.cuda.synchronize()
    assert torch.equal(a.position_ids, b.position_ids) and torch.equal(a.cache.pos_rows, b.cache.pos_rows)
    assert a.position_ids[:, :, 0].tolist() == [[L + n for L, n in zip(PROMPTS, lengths)]] * 3
    assert list(a.cache.slot_lengths) == [L + n for L, n in zip(PROMPTS, lengths)]
    assert int(a.token[1, 0]) == int(pending[1, 0]) and torch.equal(a.position_ids[:, 1], pos1[:, 1])
    assert (a.sampler.n_new - n_new1).tolist() == [1, 0, 1, 1]
    for i, (was, now) in enumerate(zip(rows1, a.sampler.row_tensors())):          # the idle slot's WHOLE sampler row: RNG state, history,
        assert torch.equal(ragged.words(was[1]), ragged.words(now[1])), ("sampler row tensor", i)      # counters, done code, parameters
    # the same greedy tokens wherever the two paths' logits agree on the winner by more than their rounding (a frame step's GEMMs have
    # other shapes than a B = 1 call's: test_gpu_frames.py gates that distance; here the tokens)
    for s in (0, 2, 3):
        lg = a.admit_logits[s, -1].float()
        top2 = lg.topk(2).values
        print(f"slot {s}: tokens {int(a.token[s, 0])} / {int(b.token[s, 0])}, margin {float(top2[0] - top2[1]):.3e}")
        assert int(a.token[s, 0]) == int(lg.argmax())
        assert int(a.token[s, 0]) == int(b.token[s, 0]), s
    # ... and its next draw is the one it would have made: a decode step of both decoders gives slot 1 the same sampled token
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert int(a.token[1, 0]) == int(b.token[1, 0]), "the idle slot's RNG moved"


# ---------------------------------------------------------------------------------------------
# three ragged ticks against the CPU oracle and the eager B = 1 slot_view path on the same valid tokens (the gate of test_gpu_frames.py)
# ---------------------------------------------------------------------------------------------
TICKS = [[5, 0, 130, 64], [130, 7, 0, 1], [0, 130, 65, 63]]          # every slot sits one tick out and resumes (slot 3: never idle)


@functools.lru_cache(maxsize=None)
def _tick_inputs():
    import test_gpu_frames as tgf
    _, hc, _, _ = tgf._small()
    prompts = [_bf_randn((1, L, hc.hidden_size), 100 + s) for s, L in enumerate(PROMPTS)]
    xs = [_bf_randn((N_SLOTS, T_STACK, hc.hidden_size), 230 + k) for k in range(len(TICKS))]
    return prompts, xs


@functools.lru_cache(maxsize=None)
def _tick_oracle():
    """[slot][tick] -> logits of the tick's last valid token by oracle.model.text_stack (None where the slot sat the tick out)"""
    import test_gpu_frames as tgf
    from oracle import model as omodel
    _, hc, oc, params = tgf._small()
    prompts, xs = _tick_inputs()
    emb, out = params["embed_tokens.weight"], []
    for s, L in enumerate(PROMPTS):
        ocache = omodel.new_cache(oc, cache_dtype=ragged.BF)
        omodel.text_stack(params, prompts[s].float().cpu(), torch.arange(L)[None, None, :].expand(3, 1, L), oc, ocache, act_dtype=ragged.BF,
                          kernel_rounding=ragged.BF)
        row, at = [], L
        for k, ln in enumerate(TICKS):
            n = ln[s]
            if n == 0:
                row.append(None)
                continue
            pid = torch.arange(at, at + n)[None, None, :].expand(3, 1, n)
            h = omodel.text_stack(params, xs[k][s:s + 1, :n].float().cpu(), pid, oc, ocache, act_dtype=ragged.BF, kernel_rounding=ragged.BF)
            row.append(h[0, -1] @ emb.T)
            at += n
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def _tick_slot_view():
    """the same through the eager B = 1 path: every slot's valid tokens on its slot_view, slot by slot"""
    import test_gpu_frames as tgf
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc, _, _ = tgf._small()
    prompts, xs = _tick_inputs()
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=ragged.BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    out = []
    for s, L in enumerate(PROMPTS):
        dec.admit(s, prompts[s])
        row, at = [], L
        for k, ln in enumerate(TICKS):
            n = ln[s]
            if n == 0:
                row.append(None)
                continue
            pid = torch.arange(at, at + n, device=DEV)[None, None, :].expand(3, 1, n)
            with torch.no_grad():
                _, lg = stack(inputs_embeds=xs[k][s:s + 1, :n].contiguous(), position_ids=pid, past_key_values=cache.slot_view(s), logits_to_keep=1)
            row.append(lg[0, -1].float().cpu())
            at += n
        out.append(row)
    torch.cuda.synchronize()
    return out


def test_three_ragged_ticks_against_the_oracle_and_the_slot_view_path():
    """Per slot and tick, the logits of the last valid token: rms_rel to the CPU oracle below 2e-2 and at most 1.25 x that of the eager
    B = 1 slot_view path on the same tokens (test_gpu_frames._gate).  NaN behind the counts; every slot but one sits a tick out and
    resumes; one graph; slot_lengths == pos_rows after every tick."""
    import test_gpu_frames as tgf
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedRaggedStep
    stack, hc, _, _ = tgf._small()
    prompts, xs = _tick_inputs()
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=ragged.BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    for s, x in enumerate(prompts):
        dec.admit(s, x)
    st = GraphedRaggedStep(stack, cache, T_STACK)
    start = torch.tensor(PROMPTS, dtype=torch.int64, device=DEV)
    pid = (start[None, :, None] + torch.arange(T_STACK, device=DEV)[None, None, :]).expand(3, N_SLOTS, T_STACK).contiguous()
    got, graphs, at = [], [], list(PROMPTS)
    for k, ln in enumerate(TICKS):
        x = xs[k].clone()
        for s, n in enumerate(ln):
            x[s, n:] = NAN
        _, lg = st.step(x, pid if k == 0 else None, lengths=ln)      # (later ticks: the positions the graph advanced by the counts)
        torch.cuda.synchronize()
        got.append(lg[:, -1].float().cpu())
        graphs.append(st.graph)
        at = [a + n for a, n in zip(at, ln)]
        assert cache.pos_rows.tolist() == at == list(cache.slot_lengths), k
        assert st.position_ids[:, :, 0].tolist() == [at] * 3, k
    assert graphs[0] is not None and all(g is graphs[0] for g in graphs)
    olg, one = _tick_oracle(), _tick_slot_view()
    judged = 0
    for s in range(N_SLOTS):
        for k, ln in enumerate(TICKS):
            if ln[s] == 0:
                continue
            assert torch.isfinite(got[k][s]).all(), (s, k)
            tgf._gate(f"ragged tick {k} slot {s} n {ln[s]}", olg[s][k], got[k][s], one[s][k])
            judged += 1
    assert judged == 9

"""GPU (-m gpu): the multi-stream frame step -- T tokens for every slot of a MultiStreamCache in one captured step.

  * ops.swa_forward_rows (ivl_swa_rows_fwd): one ring position per batch row at every T.  ROWS-1: row b is bit-equal to row b of
    ops.swa_forward on the same tensors with every row at pos_rows[b] (output and ring after the append); close to the oracle;
    ring slots a row never wrote are never read; the positions are read when a captured call is replayed (ROWS-3);
  * GraphedMultiStreamStep: graph == eager bit for bit, a slot does not notice its neighbours, streams join and leave without a
    recapture, and the step is as close to the oracle as the B = 1 slot_view path on the same inputs;
  * GraphedMultiStreamDecode.extend_frames against extend() slot by slot;
  * the model's real width."""
import functools

import pytest
import torch

import fork
import frames
import parity
from conftest import rms_rel
from frames import BF, CASES, D, HKV, HQ, words
from oracle import model as omodel
from oracle import swa as oswa

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
# the operator
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(name, nan_unread=False):
    return frames.case_tensors(name, DEV, nan_unread=nan_unread)


@functools.lru_cache(maxsize=None)
def _rows(name, use_rope, append=True, nan_unread=False):
    """(o, k ring, v ring) of ONE ops.swa_forward_rows call on clones of the case's rings; pos_rows must come back unchanged"""
    from infinitevl_amd import ops
    T, C, positions = CASES[name]
    q, k, v, kc, vc, pos_rows, rope = _inputs(name, nan_unread)
    kr, vr = kc.clone(), vc.clone()
    before = ops.ROWS_STEP_CALLS
    o = ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=kr, v_cache=vr, pos_rows=pos_rows,
                             rope=rope if use_rope else None, append=append)
    torch.cuda.synchronize()
    assert ops.ROWS_STEP_CALLS == before + 1
    assert pos_rows.tolist() == positions                       # never written
    return o, kr, vr


@functools.lru_cache(maxsize=None)
def _reference(name, use_rope, append=True, nan_unread=False):
    """Row b of (o, k ring, v ring) from ops.swa_forward on the same B-row tensors and cloned rings with pos_dev = [p_b]."""
    from infinitevl_amd import ops
    T, C, positions = CASES[name]
    q, k, v, kc, vc, _, rope = _inputs(name, nan_unread)
    o_ref, k_ref, v_ref = [], [], []
    for b, p in enumerate(positions):
        kr, vr = kc.clone(), vc.clone()
        pos_dev = torch.tensor([p], dtype=torch.int64, device=DEV)
        o = ops.swa_forward(q, k, v, window=C + 1, scaling=SCALE, k_cache=kr, v_cache=vr, pos_dev=pos_dev,
                            rope=rope if use_rope else None, append=append)
        o_ref.append(o[b])
        k_ref.append(kr[b])
        v_ref.append(vr[b])
    torch.cuda.synchronize()
    return torch.stack(o_ref), torch.stack(k_ref), torch.stack(v_ref)


def _assert_rows1(name, use_rope, append=True, nan_unread=False):
    got, ref = _rows(name, use_rope, append, nan_unread), _reference(name, use_rope, append, nan_unread)
    for b, p in enumerate(CASES[name][2]):
        for what, g, r in zip(("o", "k ring", "v ring"), got, ref):
            assert torch.equal(words(g[b]), words(r[b])), (name, use_rope, what, b, p)


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_rows1_bit_equal_to_the_scalar_position(name, use_rope):
    from infinitevl_amd import ops
    before = ops.SWA_RING256_CALLS
    _assert_rows1(name, use_rope)
    assert ops.SWA_RING256_CALLS == before                      # neither side took the 256-row form
    T, C, positions = CASES[name]
    if T > C:                                                    # ROWS-4: the ring holds exactly the last C tokens of every row
        q, k, v, kc, vc, _, rope = _inputs(name)
        _, kr, vr = _rows(name, use_rope)
        for b, p in enumerate(positions):
            slots = torch.tensor([(p + t) % C for t in range(T - C, T)], device=DEV)
            assert torch.equal(vr[b][:, slots], v[b, T - C:].transpose(0, 1)), (name, b)


def test_rows1_without_append_leaves_the_ring():
    _assert_rows1("a", True, append=False)
    _, _, _, kc, vc, _, _ = _inputs("a")
    _, kr, vr = _rows("a", True, append=False)
    assert torch.equal(kr, kc) and torch.equal(vr, vc)
    o_app, _, _ = _rows("a", True)
    assert torch.equal(_rows("a", True, append=False)[0], o_app)


def test_packed_shape_equals_the_decode_rows_call():
    """case f: T = 4 packs (4 x 8 rows): the launches of ivl_swa_decode_rows_fwd"""
    from infinitevl_amd import ops
    C, T, positions = 4095, 4, [0, 2, 4093, 4095, 9001]
    B = len(positions)
    g = torch.Generator().manual_seed(4)
    kc, vc = (torch.randn(B, HKV, C, D, generator=g).to(BF).to(DEV) for _ in range(2))
    q = torch.randn(B, T, HQ, D, generator=g).to(BF).to(DEV)
    k, v = (torch.randn(B, T, HKV, D, generator=g).to(BF).to(DEV) for _ in range(2))
    pos_rows = torch.tensor(positions, dtype=torch.int64, device=DEV)
    pid = (pos_rows[None, :, None] + torch.arange(T, device=DEV)[None, None, :]).expand(3, B, T)
    cos, sin = frames.rope_tables(pid)
    for rope in (None, (cos, sin, frames.SECTIONS)):
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        o1 = ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=k1, v_cache=v1, pos_rows=pos_rows, rope=rope, append=True)
        o2 = ops.swa_forward(q, k, v, window=C + 1, scaling=SCALE, k_cache=k2, v_cache=v2, pos_rows=pos_rows, rope=rope, append=True)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(v1, v2), rope is not None


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("T", [1, 4])
def test_packed_rows_forms_share_one_launch_plan(T, use_rope, append):
    """On a packed shape the three pos_rows entry points run ONE launch plan, the pack branch of ivl_swa_fwd's: ivl_swa_decode_rows_fwd,
    ivl_swa_rows_fwd and ivl_swa_decode_rows_hold_fwd under a mask of zeros give the same bits in o and in both rings, and every row
    is the B = 1 scalar-position call at its position, bit for bit.  With row 1 held its ring row keeps its bits and rows 0 and 2 do
    not notice.  Ring of 95 under window 96 (3 splits); the rows: an empty ring row, a half-full one, a wrapped one."""
    from infinitevl_amd import ops
    C, positions = 95, [0, 40, 200]
    B = len(positions)
    g = torch.Generator().manual_seed(40 + T)
    kc, vc = (torch.randn(B, HKV, C, D, generator=g).to(BF).to(DEV) for _ in range(2))
    q = torch.randn(B, T, HQ, D, generator=g).to(BF).to(DEV)
    k, v = (torch.randn(B, T, HKV, D, generator=g).to(BF).to(DEV) for _ in range(2))
    pos_rows = torch.tensor(positions, dtype=torch.int64, device=DEV)
    pid = (pos_rows[None, :, None] + torch.arange(T, device=DEV)[None, None, :]).expand(3, B, T) + \
        torch.tensor([0, 3, 11], device=DEV)[:, None, None]
    cos, sin = frames.rope_tables(pid)
    kw = dict(window=C + 1, scaling=SCALE, append=append)
    names = ("o", "k ring", "v ring")

    def run(fn, **extra):
        kr, vr = kc.clone(), vc.clone()
        o = fn(q, k, v, k_cache=kr, v_cache=vr, pos_rows=pos_rows, rope=(cos, sin, frames.SECTIONS) if use_rope else None, **kw, **extra)
        torch.cuda.synchronize()
        return o, kr, vr

    calls, holds = ops.ROWS_STEP_CALLS, ops.HOLD_CALLS["swa_forward"]
    dec = run(ops.swa_forward)                                                                   # ivl_swa_decode_rows_fwd
    rows = run(ops.swa_forward_rows)                                                             # ivl_swa_rows_fwd
    hold0 = run(ops.swa_forward, frozen=torch.zeros(B, dtype=torch.int32, device=DEV))           # ivl_swa_decode_rows_hold_fwd
    assert ops.ROWS_STEP_CALLS == calls + 1 and ops.HOLD_CALLS["swa_forward"] == holds + 1
    assert pos_rows.tolist() == positions
    for what, a, b_, c in zip(names, dec, rows, hold0):
        assert torch.equal(words(a), words(b_)), (what, "ivl_swa_rows_fwd")
        assert torch.equal(words(a), words(c)), (what, "ivl_swa_decode_rows_hold_fwd")
    for b, p in enumerate(positions):                                                            # the B = 1 call with a scalar position
        kr, vr = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        rope1 = (cos[:, b:b + 1].contiguous(), sin[:, b:b + 1].contiguous(), frames.SECTIONS) if use_rope else None
        o1 = ops.swa_forward(q[b:b + 1], k[b:b + 1], v[b:b + 1], k_cache=kr, v_cache=vr, pos=p, rope=rope1, **kw)
        torch.cuda.synchronize()
        for what, got, ref in zip(names, dec, (o1, kr, vr)):
            assert torch.equal(words(got[b]), words(ref[0])), (what, b, p)
        slots = torch.tensor([(p + t) % C for t in range(T)], device=DEV)
        assert torch.equal(dec[2][b][:, slots], vc[b][:, slots]) == (not append), (b, p)         # the append took its slots, or none
    held = run(ops.swa_forward, frozen=torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV))
    assert torch.equal(words(held[1][1]), words(kc[1])) and torch.equal(words(held[2][1]), words(vc[1]))      # HOLD-1
    for b in (0, 2):                                                                             # HOLD-2
        for what, got, ref in zip(names, held, dec):
            assert torch.equal(words(got[b]), words(ref[b])), (what, b)


@pytest.mark.parametrize("name", ["c", "d"])
def test_rows_against_the_oracle(name):
    from infinitevl_amd import ops
    T, C, positions = CASES[name]
    q, k, v, kc, vc, _, rope = _inputs(name)
    o, _, _ = _rows(name, True)
    qq, kk = q.clone(), k.clone()
    ops.apply_mrope_inplace(qq, kk, rope[0], rope[1], rope[2])
    for b, p in enumerate(positions):
        n_ring = min(p, C)
        keys = torch.cat([frames.chronological(kc[b], p, C), kk[b].transpose(0, 1)], 1)[None].float().cpu()      # [1,Hkv,S,d]
        vals = torch.cat([frames.chronological(vc[b], p, C), v[b].transpose(0, 1)], 1)[None].float().cpu()
        ref = oswa.swa_attention(qq[b:b + 1].float().cpu().transpose(1, 2), keys, vals, n_ring, C + 1, SCALE)
        err = rms_rel(ref, o[b:b + 1].float().cpu())
        print(f"oracle case {name} row {b} pos {p}: rms_rel {err:.3e}")
        assert err <= 5e-3, (name, b, p, err)


@pytest.mark.parametrize("name", ["a", "c"])
def test_unread_slots_may_hold_nan(name):
    for use_rope in (False, True):
        _assert_rows1(name, use_rope, nan_unread=True)
        o = _rows(name, use_rope, nan_unread=True)[0]
        assert torch.isfinite(o.float()).all(), (name, use_rope)
        assert torch.equal(o, _rows(name, use_rope)[0]), (name, use_rope)         # the same q, keys and read slots: the same bits


def test_replay_reads_the_positions():
    """ROWS-3: capture case c, change pos_rows in place, replay == the eager call at the new positions"""
    from infinitevl_amd import ops
    T, C, positions = CASES["c"]
    q, k, v, kc, vc, pos0, rope = _inputs("c")
    pos_rows, kr, vr = pos0.clone(), kc.clone(), vc.clone()

    def call():
        return ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=kr, v_cache=vr, pos_rows=pos_rows, rope=rope, append=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = call()
    for new in (positions, [4095, 17, 9000]):
        pos_rows.copy_(torch.tensor(new, dtype=torch.int64))
        kr.copy_(kc)
        vr.copy_(vc)
        graph.replay()
        torch.cuda.synchronize()
        k2, v2 = kc.clone(), vc.clone()
        o2 = ops.swa_forward_rows(q, k, v, window=C + 1, scaling=SCALE, k_cache=k2, v_cache=v2,
                                  pos_rows=torch.tensor(new, dtype=torch.int64, device=DEV), rope=rope, append=True)
        torch.cuda.synchronize()
        assert torch.equal(o, o2) and torch.equal(kr, k2) and torch.equal(vr, v2), new
        assert pos_rows.tolist() == new


# ---------------------------------------------------------------------------------------------
# the stack: 4 slots (window 96), three streams at lengths 5, 70 and 130, one idle slot, three frame steps
# ---------------------------------------------------------------------------------------------
LENGTHS = [5, 70, 130]
N_SLOTS, N_STEPS = 4, 3


@functools.lru_cache(maxsize=None)
def _small():
    stack, hc = fork.small_stack(DEV)
    _, oc = parity.small_configs(96)
    params = parity.bf16_params(omodel.random_params(oc, seed=3, vocab=hc.vocab_size))
    return stack, hc, oc, params


def _bf_randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.5).to(BF).to(DEV)


@functools.lru_cache(maxsize=None)
def _streams(T, variant=0):
    """(prompts [1,L,hidden] of slots 0..2, frames [N_STEPS] of [4,T,hidden]).  variant 1: slots 0 and 2 hold other streams at other
    lengths and get other frames; slot 1 is the same stream."""
    _, hc, _, _ = _small()
    lengths = LENGTHS if variant == 0 else [33, LENGTHS[1], 97]
    prompts = [_bf_randn((1, L, hc.hidden_size), 100 + s + (50 * variant if s != 1 else 0)) for s, L in enumerate(lengths)]
    xs = []
    for k in range(N_STEPS):
        x = _bf_randn((N_SLOTS, T, hc.hidden_size), 200 + k)
        if variant:
            y = _bf_randn((N_SLOTS, T, hc.hidden_size), 300 + k)
            y[1] = x[1]
            x = y
        x[3].zero_()                                             # the idle slot
        xs.append(x)
    return prompts, xs, lengths


def _first_positions(lengths, T):
    start = torch.tensor(list(lengths) + [0], dtype=torch.int64, device=DEV)
    return (start[None, :, None] + torch.arange(T, device=DEV)[None, None, :]).expand(3, N_SLOTS, T).contiguous()


@functools.lru_cache(maxsize=None)
def _frame_run(T, graph, variant=0):
    """Three frame steps; slot 3 is admitted after the first step and released after the second.  Returns per-step logits
    [4,vocab], the cache's row tensors, pos_rows, slot_lengths and whether stepper.graph stayed the same object."""
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep
    stack, hc, _, _ = _small()
    prompts, xs, lengths = _streams(T, variant)
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    for s, x in enumerate(prompts):
        dec.admit(s, x)
    stepper = GraphedMultiStreamStep(stack, cache, T)
    logits, graphs, calls = [], [], ops.ROWS_STEP_CALLS
    for k in range(N_STEPS):
        _, lg = stepper.step(xs[k], _first_positions(lengths, T) if k == 0 else None, graph=graph)
        logits.append(lg[:, -1].float().cpu())
        graphs.append(stepper.graph)
        if k == 0:
            assert cache.pos_rows.tolist() == [L + T for L in lengths] + [T]
            dec.admit(3, _bf_randn((1, 20, hc.hidden_size), 77))
        if k == 1:
            dec.release(3)
    torch.cuda.synchronize()
    n_sliding = sum(t == "sliding_attention" for t in hc.layer_types)
    if not graph:
        assert ops.ROWS_STEP_CALLS - calls == N_STEPS * n_sliding          # every sliding layer of every step ran ivl_swa_rows_fwd
        assert stepper.graph is None
    else:
        assert graphs[0] is not None and all(g is graphs[0] for g in graphs)      # admit / release: no recapture
    assert torch.equal(stepper.position_ids, _first_positions(lengths, T) + N_STEPS * T)
    return logits, [t.clone() for t in cache.row_tensors()], cache.pos_rows.tolist(), list(cache.slot_lengths)


@functools.lru_cache(maxsize=None)
def _oracle_logits(T):
    """[slot][step] -> logits of the frame's last token by oracle.model.text_stack (bf16 rounding), slots 0..2"""
    _, hc, oc, params = _small()
    prompts, xs, lengths = _streams(T)
    emb = params["embed_tokens.weight"]
    out = []
    for s, L in enumerate(lengths):
        ocache = omodel.new_cache(oc, cache_dtype=BF)
        pid = torch.arange(L)[None, None, :].expand(3, 1, L)
        omodel.text_stack(params, prompts[s].float().cpu(), pid, oc, ocache, act_dtype=BF, kernel_rounding=BF)
        row = []
        for k in range(N_STEPS):
            pid = torch.arange(L + k * T, L + (k + 1) * T)[None, None, :].expand(3, 1, T)
            h = omodel.text_stack(params, xs[k][s:s + 1].float().cpu(), pid, oc, ocache, act_dtype=BF, kernel_rounding=BF)
            row.append(h[0, -1] @ emb.T)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def _slot_view_logits(T):
    """[slot][step] -> the same logits through the eager B = 1 path: every slot's frame on its slot_view, slot by slot"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc, _, _ = _small()
    prompts, xs, lengths = _streams(T)
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    out = []
    for s, L in enumerate(lengths):
        dec.admit(s, prompts[s])
        row = []
        for k in range(N_STEPS):
            pid = torch.arange(L + k * T, L + (k + 1) * T, device=DEV)[None, None, :].expand(3, 1, T)
            with torch.no_grad():
                _, lg = stack(inputs_embeds=xs[k][s:s + 1], position_ids=pid, past_key_values=cache.slot_view(s), logits_to_keep=1)
            row.append(lg[0, -1].float().cpu())
        out.append(row)
    torch.cuda.synchronize()
    return out


def _gate(what, olg, got, one):
    """the stack gate: e_new < 2e-2 (this file's stack bound against the oracle) and e_new <= 1.25 e_one (the model's own distance:
    the B = 1 slot_view path on the same inputs)"""
    e_new, e_one = rms_rel(olg, got), rms_rel(olg, one)
    print(f"{what}: e_new {e_new:.3e} e_one {e_one:.3e} ratio {e_new / e_one:.3f}")
    assert e_new < 2e-2, (what, e_new)
    assert e_new <= 1.25 * e_one, (what, e_new, e_one)


@pytest.mark.parametrize("T", [40, 130])
def test_stack_graph_equals_eager(T):
    g, e = _frame_run(T, True), _frame_run(T, False)
    for k, (a, b) in enumerate(zip(g[0], e[0])):
        assert torch.equal(a, b), (T, "logits of step", k)
    for i, (a, b) in enumerate(zip(g[1], e[1])):
        assert torch.equal(words(a) if a.dtype == BF else a, words(b) if b.dtype == BF else b), (T, "row tensor", i)
    want = [L + N_STEPS * T for L in LENGTHS] + [T]              # slot 3: released after the second step, then one more frame
    for run in (g, e):
        assert run[2] == want and run[3] == want, (T, run[2], run[3])


@pytest.mark.parametrize("T", [40, 130])
def test_stack_a_slot_does_not_notice_its_neighbours(T):
    a, b = _frame_run(T, True), _frame_run(T, True, variant=1)
    for k in range(N_STEPS):
        assert torch.equal(a[0][k][1], b[0][k][1]), (T, "slot 1 logits of step", k)
        assert not torch.equal(a[0][k][0], b[0][k][0])                             # (the neighbours do hold other streams)
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(words(x[1]) if x.dtype == BF else x[1], words(y[1]) if y.dtype == BF else y[1]), (T, "row tensor", i)
    assert a[2][1] == b[2][1] == LENGTHS[1] + N_STEPS * T


@pytest.mark.parametrize("T", [40, 130])
def test_stack_is_as_close_to_the_oracle_as_the_slot_view_path(T):
    got, olg, one = _frame_run(T, True)[0], _oracle_logits(T), _slot_view_logits(T)
    for s in range(3):
        for k in range(N_STEPS):
            _gate(f"T {T} slot {s} step {k}", olg[s][k], got[k][s], one[s][k])


def test_frame_step_does_not_read_a_hold_mask():
    """a cache that keeps a hold mask: the T > 1 call reads none of it -- frozen slots take the frame too, the same bits"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep
    T = 40
    stack, hc, _, _ = _small()
    prompts, xs, lengths = _streams(T)
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    for s, x in enumerate(prompts):
        dec.admit(s, x)
    cache.enable_holds(torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=DEV))
    stepper = GraphedMultiStreamStep(stack, cache, T)
    for graph in (False, True):
        _, lg = stepper.step(xs[0] if not graph else xs[1], _first_positions(lengths, T) if not graph else None, graph=graph)
        torch.cuda.synchronize()
        k = int(graph)
        if not graph:
            assert torch.equal(lg[:, -1].float().cpu(), _frame_run(T, True)[0][0])
        assert cache.pos_rows.tolist() == [L + (k + 1) * T for L in lengths] + [(k + 1) * T]
        assert cache.sync_lengths() == cache.pos_rows.tolist()


# ---------------------------------------------------------------------------------------------
# extend_frames against extend() slot by slot
# ---------------------------------------------------------------------------------------------
def test_extend_frames_draws_every_row_in_the_sampling_launch():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep, Sampler
    T = 40
    stack, hc, _, _ = _small()
    prompts, xs, lengths = _streams(T)
    cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=BF)
    smp = Sampler(N_SLOTS, DEV, vocab_size=hc.vocab_size, history=8)
    dec = GraphedMultiStreamDecode(stack, cache, sampler=smp)
    for s, x in enumerate(prompts):
        dec.admit(s, x, sampling=dict(temperature=0.8, top_k=20, seed=6) if s == 1 else dict(temperature=0.0))
    n_before, pending = smp.n_new.clone(), dec.token.clone()
    dec.extend_frames(GraphedMultiStreamStep(stack, cache, T), xs[0])
    torch.cuda.synchronize()
    assert (smp.n_new[:3] - n_before[:3]).tolist() == [1, 1, 1]                     # one draw per row, counted in the launch
    best = dec.admit_logits[:, -1].float().argmax(-1)
    for s in (0, 2):                                                                 # the greedy rows
        assert int(dec.token[s, 0]) == int(best[s]), s
        assert int(smp.tokens(s)[-1]) == int(dec.token[s, 0])
    top20 = dec.admit_logits[1, -1].float().topk(20).indices.tolist()
    assert int(dec.token[1, 0]) in top20                                            # the sampling row drew inside its top-k
    assert pending.shape == dec.token.shape and dec.position_ids[0, :3, 0].tolist() == [L + T for L in lengths]



def test_extend_frames_against_per_slot_extend():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep
    T = 40
    stack, hc, _, _ = _small()
    prompts, xs, lengths = _streams(T)
    prompts = list(prompts) + [_bf_randn((1, 33, hc.hidden_size), 78)]              # here the fourth slot holds a stream too
    decs = []
    for _ in range(2):
        cache = MultiStreamCache(config=hc, n_slots=N_SLOTS, device=DEV, dtype=BF)
        dec = GraphedMultiStreamDecode(stack, cache)
        for s, x in enumerate(prompts):
            dec.admit(s, x)
        decs.append(dec)
    a, b = decs
    assert torch.equal(a.token, b.token) and torch.equal(a.position_ids, b.position_ids)
    stepper = GraphedMultiStreamStep(stack, a.cache, T)
    x = xs[0].clone()
    x[3] = _bf_randn((T, hc.hidden_size), 79)
    tok = a.extend_frames(stepper, x)
    assert tok is a.token and tuple(a.admit_logits.shape) == (N_SLOTS, 1, hc.vocab_size)
    assert torch.equal(a.token[:, 0], a.admit_logits[:, -1].argmax(-1))
    one = []
    for s in range(N_SLOTS):
        b.extend(s, x[s:s + 1])
        one.append(b.admit_logits[0, -1].float().cpu())
    torch.cuda.synchronize()
    want = [L + T for L in lengths + [33]]
    assert torch.equal(a.position_ids, b.position_ids) and a.position_ids[0, :, 0].tolist() == want
    assert torch.equal(a.cache.pos_rows, b.cache.pos_rows) and a.cache.pos_rows.tolist() == want
    assert a.cache.slot_lengths == b.cache.slot_lengths == want
    olg = _oracle_logits(T)
    for s in range(3):
        _gate(f"extend_frames slot {s}", olg[s][0], a.admit_logits[s, -1].float().cpu(), one[s])
    # M-RoPE positions that are not text-like: every slot's next position is its own maximum + 1
    g_step = stepper.graph
    a.step()
    g_dec = a.graph
    assert g_dec is not None and stepper.graph is g_step
    pid = a.position_ids + torch.arange(T, device=DEV)
    pid[1, 2] += 7                                                                   # slot 2: its height axis runs ahead
    before = a.position_ids[0, :, 0].tolist()
    a.extend_frames(stepper, xs[1], pid)
    a.step()
    torch.cuda.synchronize()
    assert a.graph is g_dec and stepper.graph is g_step                              # neither graph was recaptured
    nxt = [p + T + 1 for p in before]                                                # (+ 1: the decode step behind the frame)
    nxt[2] += 7
    assert a.position_ids[0, :, 0].tolist() == nxt and a.position_ids[2, :, 0].tolist() == nxt
    assert a.cache.pos_rows.tolist() == [w + 1 + T + 1 for w in want]


# ---------------------------------------------------------------------------------------------
# the model's real width
# ---------------------------------------------------------------------------------------------
def test_real_width_two_slots_one_frame():
    """sliding_window 4096, slots at 3996 (the frame crosses the fill point) and 5000 (full ring), one T = 256 step, per slot against
    the B = 1 path on the same tokens.

    The bound test_gpu_multistream.py::test_real_width_staggered_slots_and_ring256_admission applies to that comparison (4e-3)
    does NOT hold for a 256-token frame, and cannot: the two slots make the projections 512-row GEMMs, whose tiles round in another
    order than the 256-row call's, and this random-weight 36-layer model amplifies a last-bit difference to percents.  Measured
    on the MI355X (logits of the frame's last token, rms_rel against the B = 1 path in one call): the frame step 6.99e-2 (slot 0) /
    7.37e-2 (slot 1); the B = 1 path AGAINST ITSELF with the same 256 tokens split into two calls of 128: 6.64e-2 / 7.29e-2.  So the
    gate is 1.25 x the B = 1 path's own distance, measured here on the same tokens.  What is not a matter of rounding is pinned
    exactly: with ONE slot (the same GEMM shapes as the B = 1 call) the frame step equals the B = 1 path bit for bit."""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, GraphedMultiStreamStep, InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(sliding_window=4096)
    with torch.device(DEV):
        torch.set_default_dtype(BF)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(BF).eval()
    model.init_weights_(seed=0)
    model.fuse_()
    T, lengths = 256, [3996, 5000]
    gen = torch.Generator(device=DEV).manual_seed(5)
    prompts = [(torch.randn(1, L, cfg.hidden_size, generator=gen, device=DEV) * 0.5).to(BF) for L in lengths]
    frame = (torch.randn(2, T, cfg.hidden_size, generator=gen, device=DEV) * 0.5).to(BF)
    start = torch.tensor(lengths, device=DEV)
    pid = (start[None, :, None] + torch.arange(T, device=DEV)[None, None, :]).expand(3, 2, T)

    def frame_step(slots):
        cache = MultiStreamCache(config=cfg, n_slots=len(slots), device=DEV, dtype=BF)
        dec = GraphedMultiStreamDecode(model, cache)
        for i, s in enumerate(slots):
            dec.admit(i, prompts[s])
        _, lg = GraphedMultiStreamStep(model, cache, T).step(frame[slots], pid[:, slots])
        torch.cuda.synchronize()
        assert cache.pos_rows.tolist() == [lengths[s] + T for s in slots]
        return lg[:, -1].float().cpu()

    got = frame_step([0, 1])
    assert torch.isfinite(got).all()
    for s, x in enumerate(prompts):
        with torch.no_grad():
            c1 = model.allocate_inference_cache(1)
            for a in range(0, lengths[s], 4096):
                b = min(lengths[s], a + 4096)
                p1 = torch.arange(a, b, device=DEV)[None, None, :].expand(3, 1, b - a)
                model(inputs_embeds=x[:, a:b], position_ids=p1, past_key_values=c1)
            c2 = c1.clone()
            _, lg1 = model(inputs_embeds=frame[s:s + 1], position_ids=pid[:, s:s + 1], past_key_values=c1)
            for a, b in ((0, T // 2), (T // 2, T)):
                _, lg2 = model(inputs_embeds=frame[s:s + 1, a:b], position_ids=pid[:, s:s + 1, a:b], past_key_values=c2)
        one, two = lg1[0, -1].float().cpu(), lg2[0, -1].float().cpu()
        err, own = rms_rel(one, got[s]), rms_rel(one, two)
        print(f"real width slot {s} (length {lengths[s]}): rms_rel vs the B = 1 path {err:.3e}; the B = 1 path in two calls {own:.3e}")
        assert err <= 1.25 * own, (s, err, own)
        if s == 0:
            assert torch.equal(frame_step([0])[0], one), "one slot: the B = 1 path's GEMM shapes, the same bits"

"""GPU (-m gpu): per-slot hold in the multi-stream decode step (HOLD-1..3 of include/ivl_hip.h).

  1-3  the three operators: a frozen row is untouched bit for bit (whatever it holds, NaN included), running rows equal the
       unmasked entry point bit for bit, and a captured call follows a mask changed after the capture;
  4    hold / resume in the captured step: the held slot's stream continues five steps later as if nothing happened, the
       neighbours never notice, the graph is never recaptured;
  5    a finished slot freezes where it ended (its rows equal the reference's right after the replay that ended it);
  6    extend() on a finished slot starts the next turn from exactly there;
  7    more than four slots (the 16-row projections);  8  under an adapter table and over packed mxfp4 weights.
Every comparison is bitwise."""
import ctypes

import pytest
import torch

import parity
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _bf(x):
    return x.to(BF)


def _same(a, b):
    """bitwise equality (NaN payloads included)"""
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _mask(bits):
    return torch.tensor(bits, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------
# 1. GDN step operator
# ---------------------------------------------------------------------------------------------
def _gdn_inputs(state_dtype, seed):
    B, H, K, V = 3, 2, 128, 256
    Dq, Dv = H * K, H * V
    cols = (0, Dq, 2 * Dq, 2 * Dq + Dv, 2 * Dq + 2 * Dv, 2 * Dq + 2 * Dv + H)      # q k v g a b
    ld = cols[5] + H
    ld += (-ld) % 8
    g_ = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g_)                                    # noqa: E731
    return dict(B=B, H=H, K=K, V=V, cols=cols, state=_bf(r(B, H, K, V)).to(DEV, state_dtype),
                conv=[_bf(r(B, D, 4)).to(DEV) for D in (Dq, Dq, Dv)], cw=[_bf(r(D, 1, 4) * 0.5).to(DEV) for D in (Dq, Dq, Dv)],
                A32=r(H).to(DEV), dt32=r(H).to(DEV), wn=_bf(r(V)).to(DEV), proj=_bf(r(B, 1, ld)).to(DEV))


def _gdn_call(x, proj, state, conv, frozen):
    from infinitevl_amd import ops
    y = ops.gdn_decode_step(proj, x["cols"], x["cw"], conv, x["A32"], x["dt32"], x["wn"], 1e-5, state, x["H"], x["K"], x["V"],
                            x["K"] ** -0.5, **({} if frozen is None else {"frozen": frozen}))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("state_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bits", [[0, 1, 0], [1, 1, 1]])
@pytest.mark.parametrize("poison", [False, True])
def test_gdn_step_frozen_rows_are_untouched_and_running_rows_do_not_notice(state_dtype, bits, poison):
    from infinitevl_amd import ops
    x = _gdn_inputs(state_dtype, 11)
    st_ref, cv_ref = x["state"].clone(), [c.clone() for c in x["conv"]]
    y_ref = _gdn_call(x, x["proj"], st_ref, cv_ref, None)                           # ivl_gdn_decode_step_fwd
    proj, st, cv = x["proj"].clone(), x["state"].clone(), [c.clone() for c in x["conv"]]
    frozen_rows = [b for b, f in enumerate(bits) if f]
    if poison:                                                                       # a frozen row may hold anything at all
        for b in frozen_rows:
            proj[b] = float("nan")
            st[b] = float("nan")
            for c in cv:
                c[b] = float("inf")
    st0, cv0 = st.clone(), [c.clone() for c in cv]
    before = ops.HOLD_CALLS["gdn_decode_step"]
    y = _gdn_call(x, proj, st, cv, _mask(bits))
    assert ops.HOLD_CALLS["gdn_decode_step"] == before + 1
    for b, f in enumerate(bits):
        if f:                                                                        # HOLD-1
            assert _same(st[b], st0[b]), b
            assert all(_same(c[b], c0[b]) for c, c0 in zip(cv, cv0)), b
        else:                                                                        # HOLD-2
            assert _same(y[b], y_ref[b]) and _same(st[b], st_ref[b]), b
            assert all(_same(c[b], cr[b]) for c, cr in zip(cv, cv_ref)), b


@pytest.mark.parametrize("state_dtype", [torch.bfloat16, torch.float32])
def test_gdn_step_rows_with_a_null_mask_is_the_old_entry(state_dtype):
    from infinitevl_amd import _lib, ops
    x = _gdn_inputs(state_dtype, 12)
    st_ref, cv_ref = x["state"].clone(), [c.clone() for c in x["conv"]]
    y_ref = _gdn_call(x, x["proj"], st_ref, cv_ref, None)
    st, cv = x["state"].clone(), [c.clone() for c in x["conv"]]
    y = torch.empty_like(y_ref)
    p, c = x["proj"], x["cols"]
    rc = _lib.load().ivl_gdn_decode_step_rows_fwd(
        p.data_ptr(), p.shape[-1], *c, *(w.data_ptr() for w in x["cw"]), *(s.data_ptr() for s in cv), x["A32"].data_ptr(),
        x["dt32"].data_ptr(), x["wn"].data_ptr(), 1e-5, st.data_ptr(), ops._DT_CODE[st.dtype], y.data_ptr(), x["B"], x["H"], x["K"],
        x["V"], x["K"] ** -0.5, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert _same(y, y_ref) and _same(st, st_ref) and all(_same(a, b) for a, b in zip(cv, cv_ref))
    # and a mask of zeros runs the hold kernel to the same bits
    st2, cv2 = x["state"].clone(), [c_.clone() for c_ in x["conv"]]
    y2 = _gdn_call(x, x["proj"], st2, cv2, _mask([0, 0, 0]))
    assert _same(y2, y_ref) and _same(st2, st_ref) and all(_same(a, b) for a, b in zip(cv2, cv_ref))


# ---------------------------------------------------------------------------------------------
# 2. SWA rows operator
# ---------------------------------------------------------------------------------------------
def _rope(pid):
    from infinitevl_amd import ops
    inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, device=DEV, dtype=torch.float32) / 128))
    return ops.rope_tables(pid, inv_freq, 1.0)


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("fused_rope", [False, True])
def test_swa_rows_hold_each_row_in_turn(T, fused_rope):
    from infinitevl_amd import ops
    C, Hq, Hkv, d = 95, 16, 2, 128
    W = C + 1
    positions = [17, C + 5, 3 * C + 1]                         # one below C, one past a wrap, one after several
    B = len(positions)
    g_ = torch.Generator().manual_seed(5 + T + 7 * fused_rope)
    r = lambda *s: _bf(torch.randn(*s, generator=g_)).to(DEV)   # noqa: E731
    kc, vc, q, k, v = r(B, Hkv, C, d), r(B, Hkv, C, d), r(B, T, Hq, d), r(B, T, Hkv, d), r(B, T, Hkv, d)
    pos_rows = torch.tensor(positions, dtype=torch.int64, device=DEV)
    rope = None
    if fused_rope:
        pid = (pos_rows[None, :, None] + torch.arange(T, device=DEV)[None, None, :]).expand(3, B, T) + \
            torch.tensor([0, 3, 11], device=DEV)[:, None, None]
        cos, sin = _rope(pid.contiguous())
        rope = (cos, sin, (16, 24, 24))
    kw = dict(window=W, scaling=d ** -0.5, pos_rows=pos_rows, rope=rope, append=True)
    k_ref, v_ref = kc.clone(), vc.clone()
    o_ref = ops.swa_forward(q, k, v, k_cache=k_ref, v_cache=v_ref, **kw)      # ivl_swa_decode_rows_fwd
    torch.cuda.synchronize()
    for t in range(T):                                                       # the append did take the slots the test watches
        for b, p in enumerate(positions):
            assert not _same(k_ref[b, :, (p + t) % C], kc[b, :, (p + t) % C])
    for fb in range(B):
        bits = [int(b == fb) for b in range(B)]
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        q2[fb], k2[fb], v2[fb] = float("nan"), float("nan"), float("nan")     # the frozen row's inputs are never read
        kr, vr = kc.clone(), vc.clone()
        before = ops.HOLD_CALLS["swa_forward"]
        o = ops.swa_forward(q2, k2, v2, k_cache=kr, v_cache=vr, frozen=_mask(bits), **kw)
        torch.cuda.synchronize()
        assert ops.HOLD_CALLS["swa_forward"] == before + 1
        assert pos_rows.tolist() == positions
        for b in range(B):
            if b == fb:                                                      # HOLD-1: the whole ring row, K and V
                assert _same(kr[b], kc[b]) and _same(vr[b], vc[b]), (fb, b)
            else:                                                            # HOLD-2
                assert _same(o[b], o_ref[b]), (fb, b)
                assert _same(kr[b], k_ref[b]) and _same(vr[b], v_ref[b]), (fb, b)
    # every row frozen: nothing moves; no row frozen: the bits of the unmasked entry
    kr, vr = kc.clone(), vc.clone()
    ops.swa_forward(q, k, v, k_cache=kr, v_cache=vr, frozen=_mask([1, 1, 1]), **kw)
    torch.cuda.synchronize()
    assert _same(kr, kc) and _same(vr, vc)
    o = ops.swa_forward(q, k, v, k_cache=kr, v_cache=vr, frozen=_mask([0, 0, 0]), **kw)
    torch.cuda.synchronize()
    assert _same(o, o_ref) and _same(kr, k_ref) and _same(vr, v_ref)


def test_swa_frozen_needs_pos_rows():
    from infinitevl_amd import ops
    z = torch.zeros(2, 1, 16, 128, dtype=BF, device=DEV)
    kv = torch.zeros(2, 1, 2, 128, dtype=BF, device=DEV)
    kc = torch.zeros(2, 2, 95, 128, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="frozen goes with pos_rows"):
        ops.swa_forward(z, kv, kv, window=96, scaling=1.0, k_cache=kc, v_cache=kc.clone(), frozen=_mask([0, 1]))
    with pytest.raises(ValueError, match="int32"):
        ops.swa_forward(z, kv, kv, window=96, scaling=1.0, k_cache=kc, v_cache=kc.clone(),
                        pos_rows=torch.zeros(2, dtype=torch.int64, device=DEV), frozen=torch.zeros(2, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------------------------
# 3. rows_advance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [1, 3])
def test_rows_advance_moves_running_rows_only(delta):
    from infinitevl_amd import ops
    S, bits = 5, [0, 1, 0, 0, 1]
    pos0 = torch.tensor([0, 7, 94, 95, 2 ** 40], dtype=torch.int64, device=DEV)
    pid0 = torch.arange(3 * S, dtype=torch.int64, device=DEV).reshape(3, S, 1) * 10
    run = torch.tensor([1 - b for b in bits], dtype=torch.int64, device=DEV)
    pos, pid = pos0.clone(), pid0.clone()
    ops.rows_advance(pos, pid, _mask(bits), delta)
    assert torch.equal(pos, pos0 + delta * run) and torch.equal(pid, pid0 + delta * run[None, :, None])
    pos, pid = pos0.clone(), pid0.clone()
    ops.rows_advance(pos, None, _mask(bits), delta)
    ops.rows_advance(None, pid, _mask(bits), delta)
    assert torch.equal(pos, pos0 + delta * run) and torch.equal(pid, pid0 + delta * run[None, :, None])
    pos, pid = pos0.clone(), pid0.clone()
    ops.rows_advance(pos, pid, None, delta)                                          # no mask: every row
    assert torch.equal(pos, pos0 + delta) and torch.equal(pid, pid0 + delta)
    with pytest.raises(ValueError, match=r"\[3, S\]"):
        ops.rows_advance(pos, pid[:, :4], None, delta)


def test_a_captured_rows_advance_follows_a_mask_changed_after_the_capture():
    from infinitevl_amd import ops
    S = 5
    pos = torch.zeros(S, dtype=torch.int64, device=DEV)
    pid = torch.zeros(3, S, 1, dtype=torch.int64, device=DEV)
    mask = _mask([0, 1, 0, 0, 1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rows_advance(pos, pid, mask, 1)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.rows_advance(pos, pid, mask, 1)
    pos.zero_()
    pid.zero_()
    g.replay()
    assert pos.tolist() == [1, 0, 1, 1, 0]
    mask.copy_(_mask([1, 0, 0, 1, 0]))                                                # after the capture
    g.replay()
    assert pos.tolist() == [1, 1, 2, 1, 1] and all(pid[a, :, 0].tolist() == [1, 1, 2, 1, 1] for a in range(3))


# ---------------------------------------------------------------------------------------------
# the small stack
# ---------------------------------------------------------------------------------------------
def _small(window=96, seed=3):
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(window)
    params = parity.bf16_params(omodel.random_params(oc, seed=seed, vocab=hc.vocab_size))
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, params)
    stack = stack.to(DEV, torch.bfloat16).eval().fuse_()
    return stack, hc, oc, params


def _prompt(hc, T, seed):
    g_ = torch.Generator().manual_seed(seed)
    return _bf(torch.randn(1, T, hc.hidden_size, generator=g_) * 0.5).to(DEV)


def _decoder(stack, hc, n_slots, holds, history=64, **smp):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode, Sampler
    cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=BF)
    sampler = Sampler(n_slots, DEV, vocab_size=hc.vocab_size, history=history, **smp)
    kw = {"holds": True} if holds else {}                      # (the reference runs are built exactly as before the feature)
    return GraphedMultiStreamDecode(stack, cache, sampler=sampler, **kw)


def _rows(dec, slot):
    return [t[slot].clone() for t in dec._slot_tensors()]


def _hold_and_resume(stack, hc, lengths, held, adapters=None):
    """Run A: 12 steps with `held` held for steps 4..8; run B: the same decoder with nothing held.  The assertions of test 4."""
    from infinitevl_amd import ops
    n = len(lengths)
    sampling = [{} for _ in range(n)]
    sampling[held] = dict(temperature=0.8, top_k=20, seed=7)                 # the held row draws: its random counter must wait too
    sampling[(held + 1) % n] = dict(temperature=1.1, top_p=0.9, seed=3)
    runs = {}
    for leg in ("A", "B"):
        dec = _decoder(stack, hc, n, holds=True)
        for s_, T in enumerate(lengths):
            dec.admit(s_, _prompt(hc, T, 40 + s_), sampling=sampling[s_],
                      **({"adapter": adapters[s_]} if adapters is not None else {}))
        before = dict(ops.HOLD_CALLS)
        toks, logits, graph, snap = [], [], None, None
        for step in range(1, 13):
            if leg == "A" and step == 4:
                snap = _rows(dec, held)                                      # after step 3
                pending = dec.token[held].clone()
                dec.hold(held)
            dec.step()
            graph = graph or dec.graph
            toks.append(dec.token[:, 0].tolist())
            logits.append(dec.logits[:, -1].clone())
            if leg == "A" and step == 8:
                torch.cuda.synchronize()
                names = dec._slot_tensors()
                now = _rows(dec, held)
                i_tok = [i for i, t in enumerate(names) if t is dec.token][0]
                i_done = [i for i, t in enumerate(names) if t is dec.sampler.done][0]
                for i, (a, b) in enumerate(zip(now, snap)):
                    if i not in (i_tok, i_done):
                        assert _same(a, b), ("held row moved", i)
                assert int(now[i_done]) == 4 and int(snap[i_done]) == 0
                dec.resume(held)
                assert all(_same(a, b) for a, b in zip(_rows(dec, held), snap)), "resume puts the pending token and the code back"
                assert torch.equal(dec.token[held], pending)
        torch.cuda.synchronize()
        assert dec.graph is graph, "never a recapture"
        assert all(ops.HOLD_CALLS[k] > before[k] for k in before), (before, ops.HOLD_CALLS)      # the hold kernels did run
        runs[leg] = (toks, logits, dec)
    (ta, la, dec_a), (tb, lb, dec_b) = runs["A"], runs["B"]
    others = [s_ for s_ in range(n) if s_ != held]
    for i in range(12):
        assert [ta[i][s_] for s_ in others] == [tb[i][s_] for s_ in others], i
        assert _same(la[i][others], lb[i][others]), i
    for i in range(3):                                                       # steps 1..3: before the hold
        assert ta[i][held] == tb[i][held] and _same(la[i][held], lb[i][held])
    for i in range(3, 7):                                                    # B's steps 4..7 are A's steps 9..12
        assert ta[i + 5][held] == tb[i][held], i
        assert _same(la[i + 5][held], lb[i][held]), i
    assert len({tuple(t) for t in tb}) > 1, "the streams do move"
    assert dec_a.cache.sync_lengths() == [T + (7 if s_ == held else 12) for s_, T in enumerate(lengths)]
    with pytest.raises(ValueError, match="is not held"):
        dec_a.resume(held)
    return dec_a


# ---------------------------------------------------------------------------------------------
# 4. hold and resume in the captured step
# ---------------------------------------------------------------------------------------------
def test_hold_and_resume_in_the_captured_step():
    stack, hc, _, _ = _small()
    dec = _hold_and_resume(stack, hc, [130, 50, 130], held=1)                # slot 0 / 2: a full, wrapped ring; slot 1: not full
    dec.release(2)
    with pytest.raises(ValueError, match="holds no stream"):
        dec.hold(2)
    dec.sampler.done[0] = 2
    with pytest.raises(ValueError, match="not running"):
        dec.hold(0)


def test_a_held_slot_that_is_admitted_again_runs():
    """admit / admit_n on a held slot start a new stream there: the host's code 4 goes with the note, with or without sampling"""
    stack, hc, _, _ = _small()
    dec = _decoder(stack, hc, 3, holds=True)
    for s_ in range(3):
        dec.admit(s_, _prompt(hc, 30 + s_, 80 + s_))
    dec.step()
    dec.hold(1)
    dec.hold(2)
    dec.step()
    dec.admit(1, _prompt(hc, 25, 90))                                        # no sampling: the row is not set afresh
    dec.admit_n([2], _prompt(hc, 26, 91))
    assert dec.sampler.poll()[0].tolist() == [0, 0, 0] and not dec._held
    for _ in range(3):
        dec.step()
    assert dec.cache.sync_lengths() == [30 + 5, 25 + 3, 26 + 3]
    dec.hold(1)                                                              # and it can be held again
    dec.resume(1)
    with pytest.raises(ValueError, match="is not held"):
        dec.resume(2)


def test_an_unfused_stack_is_refused_not_corrupted():
    """a GDN layer that cannot take the masked step raises when the cache keeps a mask: no quiet unmasked path"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(96)
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, parity.bf16_params(omodel.random_params(oc, seed=3, vocab=hc.vocab_size)))
    stack = stack.to(DEV, BF).eval()                                         # never fuse_()d
    cache = MultiStreamCache(config=hc, n_slots=2, device=DEV, dtype=BF)
    cache.enable_holds(_mask([0, 1]))
    before = [t.clone() for t in cache.row_tensors()]
    with pytest.raises(RuntimeError, match="does not reach the masked"), torch.no_grad():
        stack(input_ids=torch.zeros(2, 1, dtype=torch.int64, device=DEV), position_ids=torch.zeros(3, 2, 1, dtype=torch.int64, device=DEV),
              past_key_values=cache, logits_to_keep=1)
    torch.cuda.synchronize()
    gdn = [i for i, l in enumerate(stack.layers) if hasattr(l.self_attn, "holds_ok")]
    assert gdn and all(_same(a, b) for a, b in zip(cache.row_tensors(), before) if a.dim() == 4 and a.shape[-1] == 256), \
        "no recurrent state was written"


def test_hold_needs_holds():
    stack, hc, _, _ = _small()
    dec = _decoder(stack, hc, 3, holds=False)
    dec.admit(0, _prompt(hc, 20, 1))
    with pytest.raises(ValueError, match="holds=True"):
        dec.hold(0)
    with pytest.raises(ValueError, match="holds=True"):
        dec.resume(0)
    assert dec.cache.hold_mask is None


# ---------------------------------------------------------------------------------------------
# 5. a finished row freezes where it ended; 6. the second turn
# ---------------------------------------------------------------------------------------------
LENGTHS5 = [130, 50, 77]
BUDGETS5 = [3, 7, None]


def _cache_rows(dec, slot):
    return [t[slot].clone() for t in dec.cache.row_tensors()] + [dec.position_ids[:, slot].clone()]


def _finished_run(stack, hc):
    dec = _decoder(stack, hc, 3, holds=True)
    for s_, (T, n) in enumerate(zip(LENGTHS5, BUDGETS5)):
        dec.admit(s_, _prompt(hc, T, 60 + s_), sampling=dict(max_new_tokens=n))
    out = dec.run_until_done(32, poll_every=16)
    torch.cuda.synchronize()
    return dec, out


def test_a_finished_row_freezes_where_it_ended():
    """Fails on the code before holds by construction: the keyword does not exist, and without the mask the rows of a finished
    slot keep moving for the rest of the 16 replays between two polls."""
    stack, hc, _, _ = _small()
    dec, out = _finished_run(stack, hc)
    ref = _decoder(stack, hc, 3, holds=False)
    for s_, (T, n) in enumerate(zip(LENGTHS5, BUDGETS5)):
        ref.admit(s_, _prompt(hc, T, 60 + s_), sampling=dict(max_new_tokens=n))
    ended, replays = {}, {}
    for i in range(1, 17):
        ref.step()
        done, _ = ref.sampler.poll()
        for s_ in range(3):
            if s_ not in ended and int(done[s_]) != 0:
                ended[s_], replays[s_] = _cache_rows(ref, s_), i
    assert replays == {0: 2, 1: 6}                             # the first token is the admission's; budget n ends in replay n - 1
    ended[2], replays[2] = _cache_rows(ref, 2), 16             # never ends: 16 replays in both runs
    done, n_new = dec.sampler.poll()
    assert done.tolist() == [2, 2, 0] and n_new.tolist() == [3, 7, 17]
    for s_ in range(3):
        got = _cache_rows(dec, s_)
        assert len(got) == len(ended[s_])
        for i, (a, b) in enumerate(zip(got, ended[s_])):
            assert _same(a, b), (s_, i)
    assert dec.cache.sync_lengths() == [T + replays[s_] for s_, T in enumerate(LENGTHS5)]
    assert dec.cache.pos_rows.tolist() == dec.cache.slot_lengths
    for s_ in range(3):
        assert out[s_].tolist() == ref.sampler.tokens(s_).tolist()[:len(out[s_])]
    # the reference's finished rows did move on: the mask is what holds them
    assert not all(_same(a, b) for a, b in zip(_cache_rows(ref, 0), ended[0]))


def test_second_turn_on_a_finished_slot():
    stack, hc, _, _ = _small()
    dec, _ = _finished_run(stack, hc)
    more = _prompt(hc, 20, 99)
    first = dec.extend(0, more, max_new_tokens=4).clone()
    got_tok, got_lg = [int(first)], [dec.admit_logits[0, -1].clone()]
    assert dec.sampler.poll()[0].tolist() == [0, 2, 0]
    for _ in range(3):
        dec.step()
        got_tok.append(int(dec.token[0]))
        got_lg.append(dec.logits[0, -1].clone())
    done, n_new = dec.sampler.poll()
    assert int(done[0]) == 2 and int(n_new[0]) == 4
    assert dec.sampler.tokens(0).tolist() == got_tok, "the second answer only"
    # a fresh decoder without holds: the same prompt, as many replays as slot 0 ran (2), the same extension
    ref = _decoder(stack, hc, 3, holds=False)
    ref.admit(0, _prompt(hc, LENGTHS5[0], 60))
    for _ in range(2):
        ref.step()
    ref_tok, ref_lg = [int(ref.extend(0, more))], [ref.admit_logits[0, -1].clone()]
    for _ in range(3):
        ref.step()
        ref_tok.append(int(ref.token[0]))
        ref_lg.append(ref.logits[0, -1].clone())
    torch.cuda.synchronize()
    assert got_tok == ref_tok
    for i, (a, b) in enumerate(zip(got_lg, ref_lg)):
        assert _same(a, b), i
    assert dec.cache.sync_lengths()[0] == LENGTHS5[0] + 2 + 20 + 3
    # the same turn ended by a stop id instead (the second token of the answer above): extend(stop_token_ids=) on a finished slot
    dec2, _ = _finished_run(stack, hc)
    stop = ref_tok[1]
    k = ref_tok.index(stop)
    dec2.extend(0, more, max_new_tokens=None, stop_token_ids=[stop])
    assert dec2.sampler._ends[0] and int(dec2.sampler.budget[0]) == -1
    out = dec2.run_until_done(8, poll_every=8)
    assert out[0].tolist() == ref_tok[:k + 1] and int(dec2.sampler.poll()[0][0]) == 1
    assert dec2.cache.get_seq_length(slot=0) == LENGTHS5[0] + 2 + 20 + k, "frozen from the replay after the stop id"
    with pytest.raises(ValueError, match="stop_token_ids"):
        dec2.extend(0, more, stop_token_ids=[-1])
    # the frozen neighbour is still where it ended, the running one ran on
    assert dec.cache.slot_lengths[1] == LENGTHS5[1] + 6 and dec.cache.slot_lengths[2] == LENGTHS5[2] + 16 + 3


# ---------------------------------------------------------------------------------------------
# 7. more than four slots; 8. adapters and packed copies
# ---------------------------------------------------------------------------------------------
def test_hold_and_resume_on_six_slots_with_the_16_row_projections():
    from infinitevl_amd import ops
    stack, hc, _, _ = _small(seed=5)
    stack.use_wide_decode(True)
    before = sum(ops.M16_CALLS.values())
    _hold_and_resume(stack, hc, [130, 50, 70, 41, 130, 50], held=4)
    assert sum(ops.M16_CALLS.values()) > before, "the 16-row projections ran"


def _adapter_state(stack, r, seed, scale=0.05):
    g_ = torch.Generator().manual_seed(seed)
    sd = {}
    for name in stack._lora_names:
        w = stack.get_submodule(name).weight
        sd[f"base_model.model.model.language_model.{name}.lora_A.weight"] = (torch.randn(r, w.shape[1], generator=g_) * scale).to(BF)
        sd[f"base_model.model.model.language_model.{name}.lora_B.weight"] = (torch.randn(w.shape[0], r, generator=g_) * scale).to(BF)
    return sd


def test_hold_and_resume_under_an_adapter_table():
    stack, hc, _, _ = _small(seed=6)
    stack.enable_adapters(2, 8)
    h = stack.load_adapter(_adapter_state(stack, 8, 9), alpha=16, rank=8)
    _hold_and_resume(stack, hc, [130, 50, 130], held=1, adapters=[None, h, None])


def test_hold_and_resume_over_packed_mxfp4_weights():
    from infinitevl_amd import ops
    stack, hc, _, _ = _small(seed=7)
    stack.quantize_weights_(lm_head=True, fmt="mxfp4").use_packed_weights(True)
    before = sum(ops.W4_CALLS.values())
    _hold_and_resume(stack, hc, [130, 50, 130], held=1)
    assert sum(ops.W4_CALLS.values()) > before, "the packed projections ran"

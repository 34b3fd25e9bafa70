"""GPU (-m gpu): independent streams in the rows (slots) of one cache.

  * ops.swa_forward(pos_rows=...) (ivl_swa_decode_rows_fwd): one ring position per batch row; every row bit-equal to the
    existing B = 1 decode step at that row's position (output and ring after the append), and close to the oracle;
  * MultiStreamCache + GraphedMultiStreamDecode: streams join (admit) and leave (release) between decode steps; every stream
    matches the same stream run alone through the B = 1 path and the oracle;
  * the captured step equals the eager step bit for bit, across admissions and releases;
  * the model's real width, with one slot admitted through two 4096-token calls (the second takes the 256-row attention)."""
import pytest
import torch

import parity
from conftest import rms_rel
from oracle import model as omodel
from oracle import swa as oswa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# 1. operator: per-row positions == B = 1 scalar position, bit for bit
# ---------------------------------------------------------------------------------------------
def _rope(pid, dev=DEV):
    from infinitevl_amd import ops
    inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, device=dev, dtype=torch.float32) / 128))
    cos, sin = ops.rope_tables(pid, inv_freq, 1.0)
    return cos, sin


@pytest.mark.parametrize("C", [95, 4095])
@pytest.mark.parametrize("fused_rope", [False, True])
def test_rows_decode_bit_equal_to_scalar_path_and_oracle(C, fused_rope):
    from infinitevl_amd import ops
    W, Hq, Hkv, d = C + 1, 16, 2, 128
    positions = [0, 1, 37, C - 1, C, 3 * C + 17]
    B = len(positions)
    g_ = torch.Generator().manual_seed(C + 7 * fused_rope)
    kc = _bf(torch.randn(B, Hkv, C, d, generator=g_)).to(DEV)
    vc = _bf(torch.randn(B, Hkv, C, d, generator=g_)).to(DEV)
    q = _bf(torch.randn(B, 1, Hq, d, generator=g_)).to(DEV)
    k = _bf(torch.randn(B, 1, Hkv, d, generator=g_)).to(DEV)
    v = _bf(torch.randn(B, 1, Hkv, d, generator=g_)).to(DEV)
    pos_rows = torch.tensor(positions, dtype=torch.int64, device=DEV)
    rope = None
    if fused_rope:
        pid = pos_rows[None, :, None].expand(3, B, 1) + torch.tensor([0, 3, 11], device=DEV)[:, None, None]
        cos, sin = _rope(pid.contiguous())
        rope = (cos, sin, (16, 24, 24))
    kr, vr = kc.clone(), vc.clone()
    o = ops.swa_forward(q, k, v, window=W, scaling=d ** -0.5, k_cache=kr, v_cache=vr, pos_rows=pos_rows, rope=rope,
                        append=True)
    torch.cuda.synchronize()
    assert pos_rows.tolist() == positions                      # the kernel never advances the positions
    for b, p in enumerate(positions):
        k1, v1 = kc[b:b + 1].clone(), vc[b:b + 1].clone()
        pos_dev = torch.tensor([p], dtype=torch.int64, device=DEV)
        rope1 = None if rope is None else (rope[0][:, b:b + 1].contiguous(), rope[1][:, b:b + 1].contiguous(), rope[2])
        o1 = ops.swa_forward(q[b:b + 1], k[b:b + 1], v[b:b + 1], window=W, scaling=d ** -0.5, k_cache=k1, v_cache=v1,
                             pos_dev=pos_dev, rope=rope1, append=True)
        torch.cuda.synchronize()
        assert torch.equal(o[b:b + 1], o1), (C, p)
        assert torch.equal(kr[b:b + 1], k1) and torch.equal(vr[b:b + 1], v1), (C, p)
        # oracle: the ring before the call in chronological order ++ the new key as the append stored it (rotated if fused)
        n_ring = min(p, C)
        slots = torch.tensor([(p - n_ring + j) % C for j in range(n_ring)], dtype=torch.long, device=DEV)
        keys = torch.cat([kc[b][:, slots], k1[0][:, p % C:p % C + 1]], 1)[None].float().cpu()      # [1,Hkv,S,d]
        vals = torch.cat([vc[b][:, slots], v1[0][:, p % C:p % C + 1]], 1)[None].float().cpu()
        qq = q[b:b + 1]
        if fused_rope:
            qq, kk = qq.clone(), k[b:b + 1].clone()
            ops.apply_mrope_inplace(qq, kk, rope1[0], rope1[1], rope[2])
            assert torch.equal(kk[0, 0], k1[0, :, p % C])                   # the fused append stored the rotated key
        ref = oswa.swa_attention(qq.float().cpu().transpose(1, 2), keys, vals, n_ring, W, d ** -0.5)
        assert rms_rel(ref.reshape(1, 1, Hq, d), o1.float().cpu()) <= 5e-3, (C, p)


def test_rows_decode_refuses_unsupported_shapes():
    from infinitevl_amd import ops
    B, Hq, Hkv, d, C = 2, 16, 2, 128, 95
    kc = torch.zeros(B, Hkv, C, d, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(B, 9, Hq, d, dtype=torch.bfloat16, device=DEV)          # 9 x 8 = 72 packed rows
    k = torch.zeros(B, 9, Hkv, d, dtype=torch.bfloat16, device=DEV)
    pos_rows = torch.zeros(B, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="T \\* Hq/Hkv <= 64"):
        ops.swa_forward(q, k, k, window=C + 1, scaling=1.0, k_cache=kc, v_cache=kc.clone(), pos_rows=pos_rows)
    with pytest.raises(ValueError, match="excludes"):
        ops.swa_forward(q[:, :1], k[:, :1], k[:, :1], window=C + 1, scaling=1.0, k_cache=kc, v_cache=kc.clone(),
                        pos_rows=pos_rows, pos_dev=pos_rows[:1])
    with pytest.raises(ValueError, match="bf16"):
        ops.swa_forward(q[:, :1], k[:, :1], k[:, :1], window=C + 1, scaling=1.0, k_cache=kc, v_cache=kc.clone(),
                        pos_rows=pos_rows, mma_dtype="fp8_e4m3")


# ---------------------------------------------------------------------------------------------
# 2-3. small stack: streams joining and leaving
# ---------------------------------------------------------------------------------------------
def _small(window=96, seed=3):
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(window)
    params = parity.bf16_params(omodel.random_params(oc, seed=seed, vocab=hc.vocab_size))
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, params)
    stack = stack.to(DEV, torch.bfloat16).eval().fuse_()
    return stack, hc, oc, params


def _run_schedule(stack, hc, schedule, n_slots, graph=True, seed=11, check_capture=False):
    """schedule: list of ("admit", slot, name, T) | ("release", slot) | ("steps", n).  Returns
    {name: {"prompt": x, "tokens": [input token per step], "logits": [logits per step]}} and the decoder."""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(stack, cache)
    g_ = torch.Generator().manual_seed(seed)
    streams, owner = {}, {}
    for ev in schedule:
        if ev[0] == "admit":
            _, slot, name, T = ev
            x = _bf(torch.randn(1, T, hc.hidden_size, generator=g_) * 0.5).to(DEV)
            dec.admit(slot, x)
            streams[name] = {"prompt": x, "tokens": [], "logits": []}
            owner[slot] = name
        elif ev[0] == "release":
            dec.release(ev[1])
            owner.pop(ev[1])
        else:
            for _ in range(ev[1]):
                if graph and dec.graph is None and check_capture:
                    before = cache.clone()
                    pos_before = list(cache.slot_lengths)
                    dec.capture()
                    torch.cuda.synchronize()
                    for a, b in zip(before.layers, cache.layers):
                        for ta, tb in zip(a.carried_tensors(), b.carried_tensors()):
                            assert torch.equal(ta, tb)
                    assert torch.equal(before.pos_rows, cache.pos_rows) and cache.slot_lengths == pos_before
                toks = dec.token[:, 0].tolist()
                dec.step(graph=graph)
                lg = dec.logits[:, -1].float().cpu()
                for slot, name in owner.items():
                    streams[name]["tokens"].append(toks[slot])
                    streams[name]["logits"].append(lg[slot].clone())
    torch.cuda.synchronize()
    return streams, dec


SCHEDULE = [("admit", 0, "A", 130), ("steps", 5), ("admit", 1, "B", 70), ("steps", 6), ("admit", 2, "C", 200), ("steps", 4),
            ("release", 0), ("admit", 0, "D", 50), ("steps", 5)]


def test_streams_join_and_leave_vs_alone_and_oracle():
    stack, hc, oc, params = _small()
    streams, _ = _run_schedule(stack, hc, SCHEDULE, n_slots=3)
    emb = params["embed_tokens.weight"]
    assert set(streams) == {"A", "B", "C", "D"}
    for name, s in streams.items():
        assert len(s["logits"]) >= 5, name
        T = s["prompt"].shape[1]
        with torch.no_grad():
            # alone through the existing B = 1 path (the same input tokens: a greedy divergence must not hide a state bug)
            cache = stack.allocate_inference_cache(1)
            pid = torch.arange(T, device=DEV)[None, None, :].expand(3, 1, T)
            stack(inputs_embeds=s["prompt"], position_ids=pid, past_key_values=cache)
            ocache = omodel.new_cache(oc, cache_dtype=torch.bfloat16)
            omodel.text_stack(params, s["prompt"].float().cpu(), pid.cpu(), oc, ocache, act_dtype=torch.bfloat16,
                              kernel_rounding=torch.bfloat16)
            for i, (tok, got) in enumerate(zip(s["tokens"], s["logits"])):
                p = T + i
                pid1 = torch.full((3, 1, 1), p, device=DEV, dtype=torch.int64)
                _, lg1 = stack(input_ids=torch.tensor([[tok]], device=DEV), position_ids=pid1, past_key_values=cache)
                err = rms_rel(lg1[0, -1].float().cpu(), got)
                assert err < 4e-3, (name, i, err)
                h = omodel.text_stack(params, emb[tok].reshape(1, 1, -1), pid1.cpu(), oc, ocache, act_dtype=torch.bfloat16,
                                      kernel_rounding=torch.bfloat16)
                olg = h[0, -1] @ emb.T
                err_o = rms_rel(olg, got)
                assert err_o < 2e-2, (name, i, err_o)


def test_graph_equals_eager_with_admissions_and_releases():
    stack, hc, _, _ = _small()
    sched = [("admit", 0, "A", 130), ("admit", 2, "B", 97), ("steps", 8), ("admit", 1, "C", 200), ("steps", 10),
             ("release", 2), ("steps", 4), ("admit", 2, "D", 61), ("steps", 9), ("release", 0), ("admit", 0, "E", 33),
             ("steps", 9)]
    assert sum(e[1] for e in sched if e[0] == "steps") == 40
    g_streams, _ = _run_schedule(stack, hc, sched, n_slots=3, graph=True, check_capture=True)
    e_streams, _ = _run_schedule(stack, hc, sched, n_slots=3, graph=False)
    assert set(g_streams) == set(e_streams)
    for name in g_streams:
        assert g_streams[name]["tokens"] == e_streams[name]["tokens"], name
        for a, b in zip(g_streams[name]["logits"], e_streams[name]["logits"]):
            assert torch.equal(a, b), name


# ---------------------------------------------------------------------------------------------
# 4. the model's real width
# ---------------------------------------------------------------------------------------------
def test_real_width_staggered_slots_and_ring256_admission():
    from infinitevl_amd import ops
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
    n_sliding = sum(t == "sliding_attention" for t in cfg.layer_types)
    assert n_sliding == 9
    lengths = [4096, 4096 + 700, 8192, 4096 + 2300]          # slot 2: two 4096-token calls
    cache = MultiStreamCache(config=cfg, n_slots=4, device=DEV, dtype=torch.bfloat16)
    dec = GraphedMultiStreamDecode(model, cache)
    gen = torch.Generator(device=DEV).manual_seed(5)
    prompts = [_bf(torch.randn(1, T, cfg.hidden_size, generator=gen, device=DEV) * 0.5) for T in lengths]
    for slot, x in enumerate(prompts):
        before = ops.SWA_RING256_CALLS
        dec.admit(slot, x)
        if slot == 2:
            assert ops.SWA_RING256_CALLS - before == n_sliding, ops.SWA_RING256_CALLS - before
        assert cache.slot_lengths[slot] == lengths[slot]
    toks, logits = [], []
    for _ in range(16):
        toks.append(dec.token[:, 0].tolist())
        dec.step()
        logits.append(dec.logits[:, -1].float().cpu())
    torch.cuda.synchronize()
    for slot, x in enumerate(prompts):
        T = x.shape[1]
        with torch.no_grad():
            c1 = model.allocate_inference_cache(1)
            for a in range(0, T, 4096):
                b = min(T, a + 4096)
                pid = torch.arange(a, b, device=DEV)[None, None, :].expand(3, 1, b - a)
                model(inputs_embeds=x[:, a:b], position_ids=pid, past_key_values=c1)
            for i in range(16):
                pid1 = torch.full((3, 1, 1), T + i, device=DEV, dtype=torch.int64)
                _, lg1 = model(input_ids=torch.tensor([[toks[i][slot]]], device=DEV), position_ids=pid1, past_key_values=c1)
                err = rms_rel(lg1[0, -1].float().cpu(), logits[i][slot])
                assert err < 4e-3, (slot, i, err)

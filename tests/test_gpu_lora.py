"""GPU (-m gpu): per-row LoRA adapters in the decode step -- ivl_lora_add_small_m_fwd behind ops.lora_add, and the model with an
adapter table.

  * the exact-integer probe, the ties variant and the randn judge of tests/lora.py over the smallest shapes that can go wrong:
    K 8 .. 11008 plain and 512 .. 4096 NORM, N 1 .. 600, 1 / 2 / 6 segments with borders off any multiple of 8 and untouched
    columns in front and behind, R 8 / 16 / 64 with true rank 3 inside R = 8, M = 1 .. 4, three adapters, every index pattern;
    guard bytes around y and t_ws; untouched rows and columns keep the bits of y0 (which holds -0.0);
  * bit-equalities: the NORM form == the plain form on the materialised add_rmsnorm output; row m among others == row m alone;
    eager == replayed, also after the indices changed between replays;
  * the model: (a) a table with every slot at -1 changes no bit (bf16, e4m3, mxfp4; eager and graphed) (b) B = 0 equals the base
    (c) a slot among slots with other adapters == the stream alone (d) set_adapter between replays == a fresh capture, no
    recapture (e) packed copies on / off (f) fork / release (g) one step at the real width.
"""
import pytest
import torch

import lora
import parity
import rowwise as rw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 64
SENTINEL = 24576.0
SEG6 = (5, 101, 203, 301, 399, 501, 595)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)
    return rep


# ---- ops.lora_add as the `run` of tests/lora.py (CPU tensors in, CPU tensors out) -------------------------------------------------------
_TABLES = {}


def _table(c):
    """the case's tables on the device (one LoraTable per case, t_ws inside guard elements)"""
    from infinitevl_amd import ops
    if id(c) not in _TABLES:
        t = ops.LoraTable(c["n_adapters"], c["R"], DEV)
        t.register("p", c["N"], c["K"], c["seg_cols"])
        p = t.proj["p"]
        p.A.copy_(c["A"])
        p.B.copy_(c["B"])
        t.scaling.copy_(c["s"])
        buf = torch.full((2 * GUARD + 4 * lora.T_LD,), SENTINEL, dtype=BF, device=DEV)
        p.t_ws = buf[GUARD:GUARD + 4 * lora.T_LD].view(4, lora.T_LD)
        _TABLES[id(c)] = (t, buf, c, {k: c[k].to(DEV) for k in ("nw",) if k in c})
    return _TABLES[id(c)]


def _guards_ok(buf, n):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "a store outside the buffer"


def run_lora(c, x, res, y0, idx):
    from infinitevl_amd import ops
    t, tbuf, _, dev = _table(c)
    M, N = y0.shape
    ybuf = torch.full((2 * GUARD + M * N,), SENTINEL, dtype=BF, device=DEV)
    y = ybuf[GUARD:GUARD + M * N].view(M, N)
    y.copy_(y0)
    t.proj["p"].t_ws.fill_(lora.T_SENTINEL)
    xd = x.to(DEV)
    if c["norm"]:
        xd = ops.PreNorm(xd, None if res is None else res.to(DEV), dev["nw"], c["eps"])
    rows = torch.tensor(idx, dtype=torch.int32, device=DEV)
    n0 = ops.LORA_CALLS["small_m"]
    out = ops.lora_add(y, xd, t, "p", rows)
    torch.cuda.synchronize()
    assert out is y and ops.LORA_CALLS["small_m"] == n0 + 1
    _guards_ok(ybuf, M * N)
    _guards_ok(tbuf, 4 * lora.T_LD)
    return y.cpu(), t.proj["p"].t_ws[:M].cpu()


PROBE = [dict(K=8, N=1, seg_cols=(0, 1), R=8),
         dict(K=8, N=7, seg_cols=(0, 7), R=8, rank=3),
         dict(K=72, N=257, seg_cols=(3, 100, 250), R=8, rank=3),
         dict(K=72, N=255, seg_cols=(0, 255), R=64),
         dict(K=520, N=600, seg_cols=SEG6, R=16),
         dict(K=520, N=256, seg_cols=(0, 129, 256), R=16),
         dict(K=2056, N=257, seg_cols=(1, 257), R=16),
         dict(K=4096, N=255, seg_cols=(3, 100, 250), R=64),
         dict(K=11008, N=7, seg_cols=(0, 7), R=8, rank=3),
         dict(K=512, N=256, seg_cols=(1, 131, 255), R=16, norm=True),
         dict(K=520, N=600, seg_cols=SEG6, R=8, rank=3, norm=True),
         dict(K=2048, N=257, seg_cols=(3, 100, 250), R=64, norm=True),
         dict(K=4096, N=7, seg_cols=(0, 7), R=16, norm=True),
         dict(K=72, N=257, seg_cols=(3, 100, 250), R=8, variant="ties"),
         dict(K=520, N=600, seg_cols=SEG6, R=16, variant="ties"),
         dict(K=2056, N=255, seg_cols=(0, 255), R=64, variant="ties")]
RANDN = [dict(K=520, N=257, seg_cols=(3, 100, 250), R=16, variant="randn"),
         dict(K=4096, N=600, seg_cols=SEG6, R=8, rank=3, variant="randn"),
         dict(K=11008, N=255, seg_cols=(0, 130, 255), R=64, variant="randn")]


def _id(a):
    return "-".join(f"{k}{len(v) - 1 if k == 'seg_cols' else v}" for k, v in a.items())


@pytest.mark.parametrize("args", PROBE, ids=[_id(a) for a in PROBE])
def test_exact_integer_probe(args):
    rep = _passes(lora.check_probe(run_lora, lora.case(**args)))
    assert rep.probed > 0
    _TABLES.clear()


@pytest.mark.parametrize("args", RANDN, ids=[_id(a) for a in RANDN])
def test_randn_judge(args):
    rep = _passes(lora.check_randn(run_lora, lora.case(**args)))
    assert rep.judged > 0 and rep.decided <= lora.WINDOW_MAX * rep.judged
    _TABLES.clear()


# ---- bit-equalities ---------------------------------------------------------------------------------------------------------------------
def _randn_setup(K, N=257, seg_cols=(3, 100, 250), R=16):
    c = lora.case(K=K, N=N, seg_cols=seg_cols, R=R, variant="randn")
    t, _, _, _ = _table(c)
    return c, t


def _add(t, x, y0, idx):
    from infinitevl_amd import ops
    y = y0.clone()
    t.proj["p"].t_ws.fill_(lora.T_SENTINEL)
    ops.lora_add(y, x, t, "p", torch.tensor(idx, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    return y, t.proj["p"].t_ws[:y.shape[0]].clone()


@pytest.mark.parametrize("K", [512, 520, 2048, 4096])
def test_norm_form_equals_the_plain_form_on_the_materialised_norm(K):
    from infinitevl_amd import ops
    c, t = _randn_setup(K)
    g_ = rw.gen(K)
    x, res = c["x"].to(DEV), torch.randn(4, K, generator=g_).to(BF).to(DEV)
    nw = rw.weight(K, g_).to(DEV)
    y0 = c["y0"].to(DEV)
    idx = [1, -1, 0, 2]
    for r_ in (res, None):
        xn, _ = ops.add_rmsnorm(x, r_, nw, 1e-6)
        ya, ta = _add(t, xn, y0, idx)
        yb, tb = _add(t, ops.PreNorm(x, r_, nw, 1e-6), y0, idx)
        assert torch.equal(lora.bits(ya), lora.bits(yb)) and torch.equal(lora.bits(ta), lora.bits(tb))
        assert not torch.equal(ya, y0)
    _TABLES.clear()


def test_row_among_others_equals_the_row_alone_and_eager_equals_replayed():
    from infinitevl_amd import ops
    c, t = _randn_setup(2056, N=600, seg_cols=SEG6)
    x, y0 = c["x"].to(DEV), c["y0"].to(DEV)
    idx = [0, 2, -1, 1]
    y, tw = _add(t, x, y0, idx)
    for m in range(4):
        ym, tm = _add(t, x[m:m + 1], y0[m:m + 1], idx[m:m + 1])
        assert torch.equal(lora.bits(ym[0]), lora.bits(y[m])) and torch.equal(lora.bits(tm[0]), lora.bits(tw[m])), m
    # one captured launch pair follows the indices on the device
    rows = torch.tensor(idx, dtype=torch.int32, device=DEV)
    ys = y0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.lora_add(ys, x, t, "p", rows)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    ys.copy_(y0)
    with torch.cuda.graph(g):
        ops.lora_add(ys, x, t, "p", rows)
    for idx2 in (idx, [2, 2, 1, -1], [-1, -1, -1, -1]):
        rows.copy_(torch.tensor(idx2, dtype=torch.int32))
        ys.copy_(y0)
        g.replay()
        torch.cuda.synchronize()
        ye, _ = _add(t, x, y0, idx2)
        assert torch.equal(lora.bits(ys), lora.bits(ye)), idx2
    assert torch.equal(lora.bits(ys), lora.bits(y0)), "all -1: nothing is touched"
    _TABLES.clear()


def test_more_than_four_rows_take_the_library_path_and_agree_with_the_kernel():
    from infinitevl_amd import ops
    c, t = _randn_setup(520)
    x, y0 = c["x"].to(DEV), c["y0"].to(DEV)
    h = ops.LoraHandle(1, 16, float(c["s"][1]))
    t._slots[1] = h
    yk, _ = _add(t, x, y0, [1, 1, 1, 1])
    n0 = dict(ops.LORA_CALLS)
    y8 = torch.cat([y0, y0])
    ops.lora_add(y8, torch.cat([x, x]), t, "p", h)
    assert ops.LORA_CALLS["torch"] == n0["torch"] + 1 and ops.LORA_CALLS["small_m"] == n0["small_m"]
    # the library GEMMs round t and d like the kernel does but sum in their own order: equal within the d window's neighbours
    err = (y8[:4].double() - yk.double()).abs()
    assert bool((err <= 2.0 ** -6 * (yk.double().abs() + 1.0)).all()) and float((err == 0).double().mean()) > 0.5
    _TABLES.clear()


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _small_stack(fmt=None, seed=2):
    """2 layers (one SWA, one Gated DeltaNet), hidden 512 = the smallest K of the NORM form, 4 heads of the real head shapes"""
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, _ = parity.small_configs(window=96, n_layers=2, heads=4)
    with torch.device(DEV):
        stack = InfiniteVLTextStack(hc)
    stack = stack.to(BF).eval().init_weights_(seed=seed).fuse_()
    if fmt is not None:
        stack.quantize_weights_(lm_head=True, fmt=fmt)
    return stack, hc


def _prompts(hc, n, T=40, seed=4):
    g_ = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, T + 3 * i, hc.hidden_size, generator=g_) * 0.5).to(BF).to(DEV) for i in range(n)]


def _adapter_state(stack, r, seed, zero_b=False, scale=0.05):
    """a peft state dict over all ten target modules"""
    g_ = rw.gen(seed)
    sd = {}
    for name in stack._lora_names:
        w = stack.get_submodule(name).weight
        sd[f"base_model.model.model.language_model.{name}.lora_A.weight"] = (torch.randn(r, w.shape[1], generator=g_) * scale).to(BF)
        B = torch.zeros(w.shape[0], r) if zero_b else torch.randn(w.shape[0], r, generator=g_) * scale
        sd[f"base_model.model.model.language_model.{name}.lora_B.weight"] = B.to(BF)
    return sd


def _cache_tensors(cache):
    names = ("_buf_keys", "_buf_values", "conv_state_q", "conv_state_k", "conv_state_v", "recurrent_state")
    return [getattr(layer, n) for layer in cache.layers for n in names if getattr(layer, n, None) is not None]


def _decode(stack, cache0, lg, B, steps, graph, adapters=None):
    from infinitevl_amd.harness import GraphedDecode
    dec = GraphedDecode(stack, cache0.clone(), B, adapters=adapters)
    dec.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
    toks, logits = [], []
    for _ in range(steps):
        if graph:
            dec.step()
            out = dec.logits
        else:
            with torch.no_grad():
                out = dec._run()
        toks.append(dec.token[:, 0].tolist())
        logits.append(out[:, -1].clone())
    torch.cuda.synchronize()
    return toks, torch.stack(logits), [t.clone() for t in _cache_tensors(dec.cache)], dec


@pytest.mark.parametrize("fmt", [None, "e4m3", "mxfp4"])
def test_a_table_with_every_slot_at_minus_one_changes_no_bit(fmt):
    """(a): decode logits, tokens and caches, eager and graphed; 8 lora_add calls per step (4 projections x 2 layers)"""
    from infinitevl_amd import ops
    stack, hc = _small_stack(fmt)
    B, steps = 2, 6
    x = torch.cat([p[:, :40] for p in _prompts(hc, B)])
    with torch.no_grad():
        cache0 = stack.allocate_inference_cache(B, zero_init=True)
        _, lg = stack(inputs_embeds=x, past_key_values=cache0)
    n0 = dict(ops.LORA_CALLS)
    base = _decode(stack, cache0, lg, B, steps, graph=True)
    assert ops.LORA_CALLS == n0, "no table: no call"
    stack.enable_adapters(3, 16)
    h = stack.load_adapter(_adapter_state(stack, 16, 7), alpha=32, rank=16)          # loaded, but no row names it
    with torch.no_grad():
        cache1 = stack.allocate_inference_cache(B, zero_init=True)
        _, lg1 = stack(inputs_embeds=x, past_key_values=cache1)
    assert torch.equal(lg1, lg) and all(torch.equal(a, b) for a, b in zip(_cache_tensors(cache0), _cache_tensors(cache1))), "prefill"
    n1 = dict(ops.LORA_CALLS)
    for graph in (False, True):
        n2 = ops.LORA_CALLS["small_m"]
        got = _decode(stack, cache0, lg, B, steps, graph=graph)
        if not graph:
            assert ops.LORA_CALLS["small_m"] - n2 == 8 * steps
        assert got[0] == base[0] and torch.equal(lora.bits(got[1]), lora.bits(base[1])), graph
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got[2], base[2])), graph
    assert ops.LORA_CALLS["torch"] == n1["torch"] + 0 and bool(torch.isfinite(base[1].float()).all())
    # and the adapter does something once a row names it
    got = _decode(stack, cache0, lg, B, steps, graph=True, adapters=[None, h])
    assert torch.equal(lora.bits(got[1][:, 0]), lora.bits(base[1][:, 0])) and not torch.equal(got[1][:, 1], base[1][:, 1])


def test_an_adapter_with_zero_b_equals_the_base_as_values():
    """(b)"""
    stack, hc = _small_stack()
    x = _prompts(hc, 1)[0]
    with torch.no_grad():
        cache0 = stack.allocate_inference_cache(1, zero_init=True)          # (compared by value: no stale NaN in unused ring slots)
        _, lg = stack(inputs_embeds=x, past_key_values=cache0)
    base = _decode(stack, cache0, lg, 1, 6, graph=True)
    stack.enable_adapters(2, 8)
    h = stack.load_adapter(_adapter_state(stack, 4, 9, zero_b=True), alpha=8, rank=4)
    with torch.no_grad():
        cache1 = stack.allocate_inference_cache(1)
        _, lg1 = stack(inputs_embeds=x, past_key_values=cache1, adapters=h)
    assert torch.equal(lg1, lg)
    got = _decode(stack, cache0, lg, 1, 6, graph=True, adapters=h)
    assert got[0] == base[0] and torch.equal(got[1], base[1]) and all(torch.equal(a, b) for a, b in zip(got[2], base[2]))


def _multistream(stack, hc, prompts, adapters, steps, graph=True):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    cache = MultiStreamCache(config=hc, n_slots=len(prompts), device=DEV, dtype=BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    first = [dec.admit(s, p, adapter=a).clone() for s, (p, a) in enumerate(zip(prompts, adapters))]
    toks, logits = [], []
    for _ in range(steps):
        dec.step(graph=graph)
        toks.append(dec.token[:, 0].tolist())
        logits.append(dec.logits[:, -1].clone())
    torch.cuda.synchronize()
    return first, toks, torch.stack(logits), dec


@pytest.mark.parametrize("fmt", [None, "mxfp4"])
def test_a_slot_among_other_adapters_equals_the_stream_alone_and_packed_copies_change_nothing(fmt):
    """(c) and (e)"""
    stack, hc = _small_stack(fmt)
    stack.enable_adapters(3, 16)
    h0 = stack.load_adapter(_adapter_state(stack, 16, 11), alpha=32, rank=16)
    h1 = stack.load_adapter(_adapter_state(stack, 4, 12), alpha=8, rank=4, use_rslora=True)
    prompts, adapters = _prompts(hc, 3), [h0, h1, None]
    first, toks, logits, dec = _multistream(stack, hc, prompts, adapters, 8)
    assert dec.adapter_ids.tolist() == [0, 1, -1] and bool(torch.isfinite(logits.float()).all())
    for s in range(3):
        f1, t1, l1, _ = _multistream(stack, hc, prompts[s:s + 1], adapters[s:s + 1], 8)
        assert torch.equal(f1[0], first[s]) and [t[0] for t in t1] == [t[s] for t in toks], s
        assert torch.equal(lora.bits(l1[:, 0]), lora.bits(logits[:, s])), s
    fe, te, le, _ = _multistream(stack, hc, prompts, adapters, 8, graph=False)
    assert te == toks and torch.equal(lora.bits(le), lora.bits(logits)), "eager == replayed"
    _, tb, lb, _ = _multistream(stack, hc, prompts, [None, None, None], 8)
    assert not torch.equal(lb[:, 0], logits[:, 0]) and not torch.equal(lb[:, 1], logits[:, 1])
    assert torch.equal(lora.bits(lb[:, 2]), lora.bits(logits[:, 2])), "the adapter-less slot keeps the base model's bits"
    if fmt is not None:
        stack.use_packed_weights(False)
        _, t2, l2, _ = _multistream(stack, hc, prompts, adapters, 8)
        stack.use_packed_weights(True)
        assert t2 == toks and torch.equal(lora.bits(l2), lora.bits(logits))


def test_set_adapter_between_replays_equals_a_fresh_capture_without_a_recapture():
    """(d), and attaching / replacing the table recaptures"""
    stack, hc = _small_stack()
    stack.enable_adapters(2, 16)
    h0 = stack.load_adapter(_adapter_state(stack, 16, 11), alpha=32, rank=16)
    h1 = stack.load_adapter(_adapter_state(stack, 8, 12), alpha=16, rank=8)
    prompts = _prompts(hc, 2)
    _, _, _, dec = _multistream(stack, hc, prompts, [h0, None], 4)
    g0 = dec.graph
    dec.set_adapter(0, h1)
    dec.set_adapter(1, h0)
    toks, logits = [], []
    for _ in range(4):
        dec.step()
        toks.append(dec.token[:, 0].tolist())
        logits.append(dec.logits[:, -1].clone())
    assert dec.graph is g0 and dec.adapter_ids.tolist() == [1, 0]
    _, _, _, dec2 = _multistream(stack, hc, prompts, [h0, None], 4, graph=False)
    assert dec2.graph is None
    dec2.set_adapter(0, h1)
    dec2.set_adapter(1, h0)
    for i in range(4):
        dec2.step()                                       # captured now, under the new ids
        assert dec2.token[:, 0].tolist() == toks[i] and torch.equal(lora.bits(dec2.logits[:, -1]), lora.bits(logits[i])), i
    # loading another adapter into the table: no recapture; another table: recapture
    stack.unload_adapter(h1)
    h2 = stack.load_adapter(_adapter_state(stack, 8, 13), alpha=16, rank=8)
    dec2.set_adapter(0, h2)
    dec2.step()
    g2 = dec2.graph
    assert not dec2._stale()
    stack.enable_adapters(2, 8)
    assert dec2._stale()
    with pytest.raises(ValueError, match="not an adapter loaded"):
        dec2.set_adapter(0, h2)
    dec2.set_adapter(0, None)
    dec2.set_adapter(1, None)
    dec2.step()
    assert dec2.graph is not g2 and not dec2._stale()
    stack.enable_adapters(0)
    assert dec2._stale()
    dec2.step()
    assert dec2._captured_lora is None


def test_fork_carries_the_adapter_and_release_clears_it():
    """(f)"""
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = _small_stack()
    stack.enable_adapters(2, 16)
    h0 = stack.load_adapter(_adapter_state(stack, 16, 11), alpha=32, rank=16)
    h1 = stack.load_adapter(_adapter_state(stack, 8, 12), alpha=16, rank=8)
    cache = MultiStreamCache(config=hc, n_slots=4, device=DEV, dtype=BF)
    dec = GraphedMultiStreamDecode(stack, cache)
    assert dec.adapter_ids.tolist() == [-1] * 4 and dec.adapter_ids.dtype == torch.int32
    dec.admit(0, _prompts(hc, 1)[0], adapter=h0)
    dec.fork(0, [1, 2])
    dec.fork(0, [3], adapter=h1)
    assert dec.adapter_ids.tolist() == [0, 0, 0, 1] and dec._slot_adapter == [h0, h0, h0, h1]
    for _ in range(3):
        dec.step()
    lg = dec.logits[:, -1]
    assert torch.equal(lora.bits(lg[0]), lora.bits(lg[1])) and torch.equal(lora.bits(lg[0]), lora.bits(lg[2]))
    assert not torch.equal(lg[0], lg[3])
    g0 = dec.graph
    dec.release(1)
    dec.fork(0, [1], adapter=None)
    assert dec.adapter_ids.tolist() == [0, -1, 0, 1] and dec._slot_adapter[1] is None
    dec.release(3)
    assert dec.adapter_ids.tolist() == [0, -1, 0, -1]
    x = _prompts(hc, 1, T=5, seed=9)[0]
    dec.extend(2, x)                                      # under the slot's adapter
    dec.step()
    assert dec.graph is g0
    with pytest.raises(ValueError, match="not an adapter loaded"):
        dec.admit(3, x, adapter=h1._replace(index=7))


def test_real_width_layers_take_a_step():
    """(g): one SWA and one Gated DeltaNet layer at the 3B model's widths, four slots, a rank-16 adapter over all ten modules"""
    from infinitevl_amd import ops
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=2048, num_hidden_layers=2, sliding_window=256)
    assert cfg.layer_types == ["sliding_attention", "linear_attention"] and cfg.hidden_size == 2048
    with torch.device(DEV):
        torch.set_default_dtype(BF)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(BF).eval().init_weights_(seed=0).fuse_().quantize_weights_(fmt="mxfp4").enable_adapters(2, 16)
    h = model.load_adapter(_adapter_state(model, 16, 3, scale=0.02), alpha=32, rank=16)
    x = (torch.randn(4, 8, cfg.hidden_size, device=DEV) * 0.5).to(BF)
    with torch.no_grad():
        cache0 = model.allocate_inference_cache(4)
        _, lg = model(inputs_embeds=x, past_key_values=cache0)
        tok = lg[:, -1].argmax(-1, keepdim=True)
        ids = torch.tensor([0, -1, 0, -1], dtype=torch.int32, device=DEV)
        n0 = ops.LORA_CALLS["small_m"]
        _, base = model(input_ids=tok, past_key_values=cache0.clone())
        _, got = model(input_ids=tok, past_key_values=cache0.clone(), adapters=ids)
    torch.cuda.synchronize()
    assert ops.LORA_CALLS["small_m"] == n0 + 16 and bool(torch.isfinite(got.float()).all())
    assert torch.equal(lora.bits(got[1]), lora.bits(base[1])) and torch.equal(lora.bits(got[3]), lora.bits(base[3]))
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[2], base[2])

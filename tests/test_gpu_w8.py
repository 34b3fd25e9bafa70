"""GPU (-m gpu): the weight-only e4m3 entry points of the decode step and the model on them.  No tolerance anywhere.

  * THE EXACT-INTEGER PROBE of tests/projections.py ("index" and "ties") with per-row scales 2^e, e in -3 .. 3 (tests/w8.py):
    expected = bf16(2^e sum + bias) bit for bit, plain / GLU / NORM over projections.SMALL_M (every instantiation, K = 8 .. 4104,
    N = 5 .. 8195, M = 1 .. 4).  The GDN form has no integer input (its prologue is the gated norm): with the probe's ternary
    weights and scales it must equal the gated-norm launch followed by the (probed) plain w8 entry point, bit for bit, over
    projections.GDN_OUT;
  * BIT-EQUALITY WITH THE bf16 KERNELS: gaussian x, gaussian weights quantised by ops.quantize_rows_e4m3; each w8 entry point
    against its bf16 twin on W' = dequantize(codes, scale): torch.equal on y, h_out and the conv states, the same case lists;
  * THE MODEL: the smallest stack whose decode step reaches all four entry points (counted through ops.W8_CALLS against the
    expected launches per step); 16 steps of GraphedDecode and GraphedMultiStreamDecode at 1, 2 and 4 rows with the packed copies
    on and off -- logits and tokens bit-equal, eager equal to replayed; a 5-slot step takes the bf16 fallback and is equal too;
    one step at the model's real width, lm_head both ways.
"""
import pytest
import torch

import parity
import projections as pj
import rowwise as rw
import w8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 64
SENTINEL = 24576.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


_ON_DEV = {}


@pytest.fixture(autouse=True)
def _fresh_uploads():
    _ON_DEV.clear()
    yield
    _ON_DEV.clear()


def _dev(t):
    if t is None:
        return None
    key = (t.data_ptr(), tuple(t.shape), t.dtype)
    if key not in _ON_DEV:
        _ON_DEV[key] = (t, t.to(DEV))
    return _ON_DEV[key][1]


def _out(rows, cols):
    buf = torch.full((rows * cols + GUARD,), SENTINEL, dtype=BF, device=DEV)
    buf[:rows * cols] = float("nan")
    return buf[:rows * cols].view(rows, cols), buf


def _guard_ok(buf):
    assert bool((buf[-GUARD:] == SENTINEL).all()), "a store went past the end of the output"


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)
    return rep


def _id(c):
    return "-".join(str(v) if not isinstance(v, tuple) else "M" + "".join(map(str, v)) for v in c)


# ---- the entry points as `run` callables (CPU tensors in, CPU tensors out) ------------------------------------------------------------
def run_w8(x, codes, scale, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = codes.shape[0] // 2 if glu else codes.shape[0]
    xd, cd, sd, bd = _dev(x), _dev(codes), _dev(scale), _dev(bias)
    y, buf = _out(M, N)
    fn = _lib.load().ivl_linear_swiglu_small_m_w8_fwd if glu else _lib.load().ivl_linear_small_m_w8_fwd
    _lib.check(fn(ops._p(xd), ops._p(cd), ops._p(sd), ops._p(bd), ops._p(y), M, N, K, ops._stream(xd)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    return y.cpu()


def run_bf16(x, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    y, buf = _out(M, N)
    fn = _lib.load().ivl_linear_swiglu_small_m_fwd if glu else _lib.load().ivl_linear_small_m_fwd
    _lib.check(fn(ops._p(xd), ops._p(wd), ops._p(bd), ops._p(y), M, N, K, ops._stream(xd)))
    torch.cuda.synchronize()
    return y.cpu()


def run_w8_norm(x, res, nw, eps, codes, scale, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = codes.shape[0] // 2 if glu else codes.shape[0]
    xd, rd, nwd, cd, sd, bd = _dev(x), _dev(res), _dev(nw), _dev(codes), _dev(scale), _dev(bias)
    y, buf = _out(M, N)
    h, hbuf = _out(M, K) if res is not None else (None, None)
    _lib.check(_lib.load().ivl_norm_linear_small_m_w8_fwd(ops._p(xd), ops._p(rd), ops._p(nwd), float(eps), ops._p(h), ops._p(cd), ops._p(sd),
                                                          ops._p(bd), ops._p(y), M, N, K, 1 if glu else 0, ops._stream(xd)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    if hbuf is not None:
        _guard_ok(hbuf)
    return y.cpu(), (None if h is None else h.cpu())


def run_bf16_norm(x, res, nw, eps, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    xd, rd, nwd, wd, bd = _dev(x), _dev(res), _dev(nw), _dev(w), _dev(bias)
    y, _ = _out(M, N)
    h = _out(M, K)[0] if res is not None else None
    _lib.check(_lib.load().ivl_norm_linear_small_m_fwd(ops._p(xd), ops._p(rd), ops._p(nwd), float(eps), ops._p(h), ops._p(wd), ops._p(bd),
                                                       ops._p(y), M, N, K, 1 if glu else 0, ops._stream(xd)))
    torch.cuda.synchronize()
    return y.cpu(), (None if h is None else h.cpu())


# ---- the exact-integer probe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glu,norm,N,K,Ms,variant", pj.SMALL_M, ids=[_id(c) for c in pj.SMALL_M])
def test_w8_exact_integer_probe(glu, norm, N, K, Ms, variant):
    """expected = bf16(2^e sum + bias), bit for bit (GLU through rowwise.silu_ref on the exact [g | u]); with the bias and without
    (ties: without, so that ties stay ties), NORM with a residual and without (h_out bit for bit)"""
    if norm:
        c = pj.norm_case(N, K, glu, Ms)
        _passes(w8.check_norm_linear(run_w8_norm, c, Ms, w8.probe_exponents(c, Ms)))
    else:
        c = pj.int_case(4, N, K, glu, variant, Ms)
        _passes(w8.check_linear(run_w8, c, Ms, w8.probe_exponents(c, Ms)))


def _gdn_run(c, M, wb, weight, pw):
    """one ops.gdn_out_linear call on fresh copies of the case's buffers -> (y, conv state q, conv state k) on the CPU"""
    from infinitevl_amd import ops
    Dv = c["H"] * 256
    proj = c["proj"][:M].to(DEV).view(M, 1, c["ld"])
    o_raw = c["o_raw"][:M].to(DEV).view(M, 1, Dv)
    cq, ck = c["cq"][:M].to(DEV), c["ck"][:M].to(DEV)
    y = ops.gdn_out_linear(o_raw, proj, c["col_g"], c["col_q"], c["col_k"], _dev(c["nw"]), c["eps"], cq, ck, weight,
                           _dev(c["bias"]) if wb else None, c["H"], w8=pw)
    torch.cuda.synchronize()
    return y.cpu(), cq.cpu(), ck.cpu()


@pytest.mark.parametrize("H,N", pj.GDN_OUT)
def test_w8_gdn_out_with_probe_weights_equals_gated_norm_plus_plain_w8(H, N):
    from infinitevl_amd import ops
    c = pj.gdn_out_case(H, N)
    Dv = H * 256
    g_ = rw.gen(H * 13 + N)
    wt = pj.ternary(N, Dv, 0.5, g_)
    e = torch.randint(-3, 4, (N,), generator=g_)
    codes, scale = w8.ternary_codes(wt), rw._pow2(e).float()
    c["bias"] = torch.randint(-4, 5, (N,), generator=g_).to(BF)
    wdq = ops.dequantize_rows_e4m3(codes, scale).to(DEV)
    before = dict(ops.W8_CALLS)
    for M in (1, 2, 3, 4):
        for wb in (False, True):
            pw = ops.PackedWeight(wdq, _dev(codes), _dev(scale))
            y, cq, ck = _gdn_run(c, M, wb, wdq, pw)
            proj = c["proj"][:M].to(DEV)
            gate = torch.empty(M, Dv, dtype=BF, device=DEV).copy_(proj[:, c["col_g"]:c["col_g"] + Dv])
            xn = ops.rmsnorm_swish_gate_strided(c["o_raw"][:M].to(DEV).view(M, 1, H, 256), gate, Dv, _dev(c["nw"]), c["eps"])
            torch.cuda.synchronize()
            y_ref = run_w8(xn.view(M, Dv).cpu(), codes, scale, c["bias"] if wb else None, False)
            assert bool(torch.isfinite(y.float()).all()) and torch.equal(y.view(M, N), y_ref), (M, wb)
            p = c["proj"][:M]
            assert torch.equal(cq, pj.conv_shift_ref(c["cq"][:M], p[:, c["col_q"]:c["col_q"] + H * 128])), (M, wb, "q")
            assert torch.equal(ck, pj.conv_shift_ref(c["ck"][:M], p[:, c["col_k"]:c["col_k"] + H * 128])), (M, wb, "k")
    assert ops.W8_CALLS["gdn_out_linear"] - before["gdn_out_linear"] == 8


# ---- bit-equality with the bf16 kernels on W' -------------------------------------------------------------------------------------------
def _gauss(glu, norm, N, K):
    from infinitevl_amd import ops
    c = pj.randn_case(4, N, K, glu)
    g_ = rw.gen(N + K + 1)
    c["w"][0] *= 1e-3                                    # rows of very different scales
    c["w"][-1] *= 64.0
    codes, exp, scale = ops.quantize_rows_e4m3(c["w"])
    assert len(exp.unique()) >= 2 or c["w"].shape[0] < 3
    c.update(codes=codes, scale=scale, wq=ops.dequantize_rows_e4m3(codes, scale))
    if norm:
        c.update(res=torch.randn(4, K, generator=g_).to(BF), nw=rw.weight(K, g_), eps=1e-6)
    return c


@pytest.mark.parametrize("glu,norm,N,K,Ms,variant", pj.SMALL_M, ids=[_id(c) for c in pj.SMALL_M])
def test_w8_equals_the_bf16_kernel_on_the_dequantised_weight(glu, norm, N, K, Ms, variant):
    c = _gauss(glu, norm, N, K)
    for M in Ms:
        for wb in (False, True):
            b = c["bias"] if wb else None
            if norm:
                for wr in (False, True):
                    r = c["res"][:M] if wr else None
                    y, h = run_w8_norm(c["x"][:M], r, c["nw"], c["eps"], c["codes"], c["scale"], b, glu)
                    y0, h0 = run_bf16_norm(c["x"][:M], r, c["nw"], c["eps"], c["wq"], b, glu)
                    assert bool(torch.isfinite(y.float()).all()) and torch.equal(y, y0), (M, wb, wr)
                    assert (h is None and h0 is None) or torch.equal(h, h0), (M, wb, wr)
            else:
                y, y0 = run_w8(c["x"][:M], c["codes"], c["scale"], b, glu), run_bf16(c["x"][:M], c["wq"], b, glu)
                assert bool(torch.isfinite(y.float()).all()) and torch.equal(y, y0), (M, wb)


@pytest.mark.parametrize("H,N", pj.GDN_OUT)
def test_w8_gdn_out_equals_the_bf16_kernel_on_the_dequantised_weight(H, N):
    from infinitevl_amd import ops
    c = pj.gdn_out_case(H, N)
    codes, _, scale = ops.quantize_rows_e4m3(c["w"])
    wdq = ops.dequantize_rows_e4m3(codes, scale).to(DEV)
    pw = ops.PackedWeight(wdq, _dev(codes), _dev(scale))
    for M in (1, 2, 3, 4):
        for wb in (False, True):
            a, b = _gdn_run(c, M, wb, wdq, pw), _gdn_run(c, M, wb, wdq, None)
            assert bool(torch.isfinite(a[0].float()).all())
            for got, ref, what in zip(a, b, ("y", "conv state q", "conv state k")):
                assert torch.equal(got, ref), (M, wb, what)
            assert not torch.equal(a[1], c["cq"][:M]), "the conv states were shifted"


def test_ops_route_and_refuse_a_stale_copy():
    """ops.linear with a packed copy: <= 4 rows take the w8 entry point, 5 rows the library GEMM on W'; a written weight raises"""
    from infinitevl_amd import ops
    c = _gauss(False, False, 7, 520)
    wd = c["wq"].to(DEV)
    pw = ops.PackedWeight(wd, c["codes"].to(DEV), c["scale"].to(DEV))
    x = torch.cat([c["x"], c["x"][:1]]).to(DEV)
    n0 = ops.W8_CALLS["linear"]
    y4 = ops.linear(x[None, :4], wd, w8=pw)
    assert ops.W8_CALLS["linear"] == n0 + 1 and torch.equal(y4, ops.linear(x[None, :4], wd))
    y5 = ops.linear(x[None], wd, w8=pw)
    assert ops.W8_CALLS["linear"] == n0 + 1 and torch.equal(y5, ops.linear(x[None], wd))
    wd.mul_(2.0)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(x[None, :4], wd, w8=pw)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(x[None], wd, w8=pw)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _small_stack(lm_head=True):
    """2 layers (one SWA, one Gated DeltaNet), hidden 512 = the smallest K of the NORM form, 4 heads of the real head shapes"""
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, _ = parity.small_configs(window=96, n_layers=2, heads=4)
    assert hc.layer_types == ["sliding_attention", "linear_attention"] and hc.hidden_size == 512
    with torch.device(DEV):
        stack = InfiniteVLTextStack(hc)
    stack = stack.to(BF).eval().init_weights_(seed=2).fuse_()
    return stack.quantize_weights_(lm_head=lm_head), hc


def _prompts(hc, n, T=40, seed=4):
    g_ = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, T + 3 * i, hc.hidden_size, generator=g_) * 0.5).to(BF).to(DEV) for i in range(n)]


def _delta(before):
    from infinitevl_amd import ops
    return {k: ops.W8_CALLS[k] - before[k] for k in before}


def test_decode_step_reaches_all_four_entry_points_with_the_expected_counts():
    """per step of the 2-layer stack: q|k|v, GDN in-projection and 2 x gate|up behind a norm; attention o_proj, GDN o_proj, 2 x
    down_proj and lm_head plain.  The split GDN step moves its o_proj to the GDN form; without the fused norms the four normed
    projections become 2 plain + 2 SwiGLU calls.  Every variant computes the same logits, packed or not."""
    from infinitevl_amd import ops
    stack, hc = _small_stack()
    x = _prompts(hc, 1)[0]
    with torch.no_grad():
        cache0 = stack.allocate_inference_cache(1)
        _, lg = stack(inputs_embeds=x, past_key_values=cache0)
    tok = lg[:, -1].argmax(-1, keepdim=True)
    expect = {(False, True): dict(linear=5, linear_swiglu=0, norm_linear=4, gdn_out_linear=0),
              (True, True): dict(linear=4, linear_swiglu=0, norm_linear=4, gdn_out_linear=1),
              (True, False): dict(linear=6, linear_swiglu=2, norm_linear=0, gdn_out_linear=1)}
    logits, reached = [], set()
    try:
        for (split, prenorm), want in expect.items():
            ops._SPLIT_DECODE, ops._PRENORM = split, prenorm
            for on in (True, False):
                stack.use_packed_weights(on)
                cache = cache0.clone()
                before = dict(ops.W8_CALLS)
                with torch.no_grad():
                    _, lg1 = stack(input_ids=tok, past_key_values=cache)
                torch.cuda.synchronize()
                d = _delta(before)
                assert d == (want if on else dict.fromkeys(want, 0)), (split, prenorm, on, d)
                reached |= {k for k, v in d.items() if v}
                logits.append(lg1)
    finally:
        ops._SPLIT_DECODE, ops._PRENORM = False, True
    assert reached == set(ops.W8_CALLS)
    assert bool(torch.isfinite(logits[0].float()).all()) and all(torch.equal(logits[0], l_) for l_ in logits[1:])


@pytest.mark.parametrize("B", [1, 2, 4])
def test_graphed_decode_is_bit_equal_with_the_packed_copies_on_and_off(B):
    from infinitevl_amd.harness import GraphedDecode
    stack, hc = _small_stack()
    x = torch.cat([p[:, :40] for p in _prompts(hc, B)])
    with torch.no_grad():
        cache0 = stack.allocate_inference_cache(B)
        _, lg = stack(inputs_embeds=x, past_key_values=cache0)
    runs = {}
    for leg in ("on", "off", "eager"):
        stack.use_packed_weights(leg != "off")
        dec = GraphedDecode(stack, cache0.clone(), B)
        dec.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
        toks, logits = [], []
        for _ in range(16):
            if leg == "eager":
                with torch.no_grad():
                    out = dec._run()
            else:
                dec.step()
                out = dec.logits
            toks.append(dec.token[:, 0].tolist())
            logits.append(out[:, -1].clone())
        torch.cuda.synchronize()
        runs[leg] = (toks, logits)
    stack.use_packed_weights(True)
    assert bool(torch.isfinite(torch.stack(runs["on"][1]).float()).all())
    for leg in ("off", "eager"):
        assert runs[leg][0] == runs["on"][0], leg
        assert all(torch.equal(a, b) for a, b in zip(runs[leg][1], runs["on"][1])), leg


def test_a_graph_captured_before_the_switch_is_recaptured():
    from infinitevl_amd.harness import GraphedDecode
    stack, hc = _small_stack()
    with torch.no_grad():
        cache = stack.allocate_inference_cache(1)
        _, lg = stack(inputs_embeds=_prompts(hc, 1)[0], past_key_values=cache)
    dec = GraphedDecode(stack, cache, 1)
    dec.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
    dec.step()
    g0 = dec.graph
    assert dec._captured_w8 and not dec._stale()
    dec.step()
    assert dec.graph is g0
    stack.use_packed_weights(False)
    assert dec._stale()
    dec.step()
    assert dec.graph is not g0 and not dec._captured_w8 and not dec._stale()
    stack.use_packed_weights(True)


@pytest.mark.parametrize("n_slots", [1, 2, 4, 5])
def test_multistream_decode_is_bit_equal_with_the_packed_copies_on_and_off(n_slots):
    """1, 2, 4 slots stream the packed copies; 5 slots are more rows than the weight-stream kernels take: the step runs the
    library GEMMs on W' (W8_CALLS unchanged) and is equal too"""
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = _small_stack()
    prompts = _prompts(hc, n_slots)
    runs = {}
    for leg in ("on", "off", "eager"):
        stack.use_packed_weights(leg != "off")
        cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=BF)
        dec = GraphedMultiStreamDecode(stack, cache)
        for s, p in enumerate(prompts):
            dec.admit(s, p)
        before = dict(ops.W8_CALLS)
        toks, logits = [], []
        for _ in range(16):
            dec.step(graph=leg != "eager")
            toks.append(dec.token[:, 0].tolist())
            logits.append(dec.logits[:, -1].clone())
        torch.cuda.synchronize()
        if leg == "eager":
            d = _delta(before)
            assert (sum(d.values()) == 0) == (n_slots > 4), (n_slots, d)
            assert n_slots > 4 or d == dict(linear=16 * 5, linear_swiglu=0, norm_linear=16 * 4, gdn_out_linear=0), d
        runs[leg] = (toks, logits)
    stack.use_packed_weights(True)
    assert bool(torch.isfinite(torch.stack(runs["on"][1]).float()).all())
    for leg in ("off", "eager"):
        assert runs[leg][0] == runs["on"][0], leg
        assert all(torch.equal(a, b) for a, b in zip(runs[leg][1], runs["on"][1])), leg


def test_real_width_step_is_bit_equal_lm_head_both_ways():
    from infinitevl_amd import ops
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(sliding_window=4096)
    assert cfg.num_hidden_layers == 36
    with torch.device(DEV):
        torch.set_default_dtype(BF)
        model = InfiniteVLTextStack(cfg)
        torch.set_default_dtype(torch.float32)
    model = model.to(BF).eval().init_weights_(seed=0).fuse_()
    x = (torch.randn(1, 8, cfg.hidden_size, device=DEV) * 0.5).to(BF)
    n_gdn = sum(t == "linear_attention" for t in cfg.layer_types)
    for lm_head in (False, True):
        model.quantize_weights_(lm_head=lm_head)
        with torch.no_grad():
            cache0 = model.allocate_inference_cache(1)
            _, lg = model(inputs_embeds=x, past_key_values=cache0)
            tok = lg[:, -1].argmax(-1, keepdim=True)
            out = []
            for on in (True, False):
                model.use_packed_weights(on)
                cache = cache0.clone()
                before = dict(ops.W8_CALLS)
                _, lg1 = model(input_ids=tok, past_key_values=cache)
                torch.cuda.synchronize()
                d = _delta(before)
                if on:
                    assert d == dict(linear=2 * 36 + int(lm_head), linear_swiglu=0, norm_linear=2 * 36, gdn_out_linear=0), d
                else:
                    assert sum(d.values()) == 0
                out.append((lg1, [t.clone() for layer in cache.layers for t in (getattr(layer, "recurrent_state", None),) if t is not None]))
        model.use_packed_weights(True)
        assert len(out[0][1]) == n_gdn and bool(torch.isfinite(out[0][0].float()).all())
        assert torch.equal(out[0][0], out[1][0]), lm_head
        assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))

"""GPU (-m gpu): the weight-only MXFP4 entry points of the decode step and the model on them.  No tolerance anywhere.

  * THE EXACT PROBE of tests/w4.py over w4.PROBE (the list tests/test_w4_cpu.py evaluates the probe's conditions on): ternary
    weights as the e2m1 codes {0x2, 0x0, 0xA} with per-block exponents ("index") or one exponent per row ("ties"), and all 16 codes
    drawn uniformly ("codes"); expected = bf16_RNE(float64 sum + bias) bit for bit.  The codes reach the kernels through
    w4.shuffle_ref, the test's own restatement of the layout;
  * BIT-EQUALITY WITH THE bf16 KERNELS: gaussian x, gaussian weights quantised by ops.quantize_rows_mxfp4 and shuffled by
    ops.mxfp4_shuffle; each w4 entry point against its bf16 twin on W': torch.equal on y, h_out and the conv states.  Plain and
    GLU (the bias through the C entry point) at K = 512 .. 11008, NORM at K = 512 .. 4096, M = 1 .. 4, N for every rows-per-wave
    branch with a column tail (the large N at K = 512); the GDN form at H = 2, 3, 5, 16;
  * THE MODEL: the tiny stack of test_gpu_w8.py with quantize_weights_(fmt="mxfp4", lm_head=True): decode logits bit-equal with
    the packed copies on and off, eager and replayed in GraphedDecode and GraphedMultiStreamDecode; W4_CALLS moves and W8_CALLS
    does not; switching the format recaptures; a prefill of the same tokens is unaffected.
"""
import pytest
import torch

import parity
import projections as pj
import rowwise as rw
import w4

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


def _d(t):
    return None if t is None else t.to(DEV)


# ---- the entry points on device tensors -------------------------------------------------------------------------------------------------
def w4_linear(x, wq, sq, bias, glu, R, K):
    """x [M,K], shuffled wq / sq of R weight rows, bias or None (all on the device) -> y [M, N] on the CPU"""
    from infinitevl_amd import _lib, ops
    M = x.shape[0]
    N = R // 2 if glu else R
    y, buf = _out(M, N)
    fn = _lib.load().ivl_linear_swiglu_small_m_w4_fwd if glu else _lib.load().ivl_linear_small_m_w4_fwd
    _lib.check(fn(ops._p(x), ops._p(wq), ops._p(sq), ops._p(bias), ops._p(y), M, N, K, ops._stream(x)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    return y.cpu()


def bf16_linear(x, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    y, _ = _out(M, N)
    fn = _lib.load().ivl_linear_swiglu_small_m_fwd if glu else _lib.load().ivl_linear_small_m_fwd
    _lib.check(fn(ops._p(x), ops._p(w), ops._p(bias), ops._p(y), M, N, K, ops._stream(x)))
    torch.cuda.synchronize()
    return y.cpu()


def w4_norm_linear(x, res, nw, eps, wq, sq, bias, glu, R, K):
    from infinitevl_amd import _lib, ops
    M = x.shape[0]
    N = R // 2 if glu else R
    y, buf = _out(M, N)
    h, hbuf = _out(M, K) if res is not None else (None, None)
    _lib.check(_lib.load().ivl_norm_linear_small_m_w4_fwd(ops._p(x), ops._p(res), ops._p(nw), float(eps), ops._p(h), ops._p(wq), ops._p(sq),
                                                          ops._p(bias), ops._p(y), M, N, K, 1 if glu else 0, ops._stream(x)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    if hbuf is not None:
        _guard_ok(hbuf)
    return y.cpu(), (None if h is None else h.cpu())


def bf16_norm_linear(x, res, nw, eps, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    y, _ = _out(M, N)
    h = _out(M, K)[0] if res is not None else None
    _lib.check(_lib.load().ivl_norm_linear_small_m_fwd(ops._p(x), ops._p(res), ops._p(nw), float(eps), ops._p(h), ops._p(w), ops._p(bias),
                                                       ops._p(y), M, N, K, 1 if glu else 0, ops._stream(x)))
    torch.cuda.synchronize()
    return y.cpu(), (None if h is None else h.cpu())


# ---- the exact probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glu,norm,N,K,Ms,variant", w4.PROBE, ids=[_id(c) for c in w4.PROBE])
def test_w4_exact_probe(glu, norm, N, K, Ms, variant):
    """expected = bf16(float64 sum + bias), bit for bit (GLU through rowwise.silu_ref on the exact [g | u]); with the bias and
    without (ties: without), NORM with a residual and without (h_out bit for bit)"""
    c = w4.probe_case(glu, norm, N, K, Ms, variant)
    R = c["nib"].shape[0]
    wq, sq = (_d(t) for t in w4.shuffle_ref(w4.pack(c["nib"]), c["e8m0"]))
    if norm:
        def run(x, res, nw, eps, nib, e8m0, bias, glu_):
            return w4_norm_linear(_d(x), _d(res), _d(nw), eps, wq, sq, _d(bias), glu_, R, K)
        _passes(w4.check_norm_linear(run, c, Ms))
    else:
        def run(x, nib, e8m0, bias, glu_):
            return w4_linear(_d(x), wq, sq, _d(bias), glu_, R, K)
        _passes(w4.check_linear(run, c, Ms))


# ---- bit-equality with the bf16 kernels on W' -------------------------------------------------------------------------------------------
K_PLAIN = (512, 544, 2016, 2048, 2080, 4096, 11008)
K_NORM = (512, 544, 2048, 2080, 4096)
EQUAL = ([(glu, False, N, K) for glu, N in ((False, 5), (True, 7)) for K in K_PLAIN]
         + [(glu, True, N, K) for glu, N in ((False, 5), (True, 7)) for K in K_NORM]
         + [(glu, norm, N, 512) for norm in (False, True) for glu, N in ((False, 4099), (False, 8197), (True, 4099))])


def _gauss(glu, norm, N, K):
    from infinitevl_amd import ops
    c = pj.randn_case(4, N, K, glu)
    g_ = rw.gen(N + K + 2)
    c["w"][0] *= 1e-3                                    # rows and blocks of very different scales
    c["w"][-1] *= 64.0
    c["w"][1, :32] = 0.0
    c["w"][2, 32:64] *= 256.0
    codes, e8m0, exp = ops.quantize_rows_mxfp4(c["w"])
    assert len(exp.unique()) >= 4
    c.update(codes=codes, e8m0=e8m0, wq=ops.dequantize_rows_mxfp4(codes, e8m0))
    if norm:
        c.update(res=torch.randn(4, K, generator=g_).to(BF), nw=rw.weight(K, g_), eps=1e-6)
    return c


@pytest.mark.parametrize("glu,norm,N,K", EQUAL, ids=[_id(c) for c in EQUAL])
def test_w4_equals_the_bf16_kernel_on_the_dequantised_weight(glu, norm, N, K):
    from infinitevl_amd import ops
    c = _gauss(glu, norm, N, K)
    R = c["codes"].shape[0]
    wq, sq = ops.mxfp4_shuffle(_d(c["codes"]), _d(c["e8m0"]))
    wd, x4, bias = _d(c["wq"]), _d(c["x"]), _d(c["bias"])
    res4, nw = (_d(c["res"]), _d(c["nw"])) if norm else (None, None)
    for M in (1, 2, 3, 4):
        x = x4[:M].contiguous()
        for b in (None, bias):
            if norm:
                for r in (None, res4[:M].contiguous()):
                    y, h = w4_norm_linear(x, r, nw, c["eps"], wq, sq, b, glu, R, K)
                    y0, h0 = bf16_norm_linear(x, r, nw, c["eps"], wd, b, glu)
                    assert bool(torch.isfinite(y.float()).all()) and torch.equal(y, y0), (M, b is not None, r is not None)
                    assert (h is None and h0 is None) or torch.equal(h, h0), (M, b is not None)
            else:
                y, y0 = w4_linear(x, wq, sq, b, glu, R, K), bf16_linear(x, wd, b, glu)
                assert bool(torch.isfinite(y.float()).all()) and torch.equal(y, y0), (M, b is not None)
                assert bool((y != 0).any())


def _gdn_run(c, M, wb, weight, pw):
    """one ops.gdn_out_linear call on fresh copies of the case's buffers -> (y, conv state q, conv state k) on the CPU"""
    from infinitevl_amd import ops
    Dv = c["H"] * 256
    proj = c["proj"][:M].to(DEV).view(M, 1, c["ld"])
    o_raw = c["o_raw"][:M].to(DEV).view(M, 1, Dv)
    cq, ck = c["cq"][:M].to(DEV), c["ck"][:M].to(DEV)
    y = ops.gdn_out_linear(o_raw, proj, c["col_g"], c["col_q"], c["col_k"], _d(c["nw"]), c["eps"], cq, ck, weight,
                           _d(c["bias"]) if wb else None, c["H"], w8=pw)
    torch.cuda.synchronize()
    return y.cpu(), cq.cpu(), ck.cpu()


@pytest.mark.parametrize("H,N", [(H, N) for H in (2, 3, 5, 16) for N in (7, 2048)])
def test_w4_gdn_out_equals_the_bf16_kernel_on_the_dequantised_weight(H, N):
    from infinitevl_amd import ops
    c = pj.gdn_out_case(H, N)
    wd = c["w"].to(DEV)
    pw = ops.PackedWeight.of(wd, fmt="mxfp4")
    assert pw.fmt == "mxfp4" and not torch.equal(wd.cpu(), c["w"])
    n4, n8 = dict(ops.W4_CALLS), dict(ops.W8_CALLS)
    for M in (1, 2, 3, 4):
        for wb in (False, True):
            a, b = _gdn_run(c, M, wb, wd, pw), _gdn_run(c, M, wb, wd, None)
            assert bool(torch.isfinite(a[0].float()).all())
            for got, ref, what in zip(a, b, ("y", "conv state q", "conv state k")):
                assert torch.equal(got, ref), (M, wb, what)
            assert not torch.equal(a[1], c["cq"][:M]), "the conv states were shifted"
    assert ops.W4_CALLS["gdn_out_linear"] - n4["gdn_out_linear"] == 8 and ops.W8_CALLS == n8


def test_ops_route_on_the_format_and_refuse_a_stale_copy():
    """ops.linear with an mxfp4 copy: <= 4 rows take the w4 entry point (W8_CALLS stays), 5 rows the library GEMM on W'"""
    from infinitevl_amd import ops
    c = _gauss(False, False, 7, 544)
    wd = c["w"].to(DEV)
    pw = ops.PackedWeight.of(wd, fmt="mxfp4")
    assert torch.equal(wd.cpu(), c["wq"])
    x = torch.cat([c["x"], c["x"][:1]]).to(DEV)
    n4, n8 = ops.W4_CALLS["linear"], dict(ops.W8_CALLS)
    y4 = ops.linear(x[None, :4], wd, w8=pw)
    assert ops.W4_CALLS["linear"] == n4 + 1 and ops.W8_CALLS == n8 and torch.equal(y4, ops.linear(x[None, :4], wd))
    y5 = ops.linear(x[None], wd, w8=pw)
    assert ops.W4_CALLS["linear"] == n4 + 1 and torch.equal(y5, ops.linear(x[None], wd))
    wd.mul_(2.0)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(x[None, :4], wd, w8=pw)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _small_stack(fmt="mxfp4"):
    """the stack of test_gpu_w8.py: 2 layers (one SWA, one Gated DeltaNet), hidden 512, 4 heads of the real head shapes"""
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, _ = parity.small_configs(window=96, n_layers=2, heads=4)
    with torch.device(DEV):
        stack = InfiniteVLTextStack(hc)
    stack = stack.to(BF).eval().init_weights_(seed=2).fuse_()
    return stack.quantize_weights_(lm_head=True, fmt=fmt), hc


def _prompts(hc, n, T=40, seed=4):
    g_ = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, T + 3 * i, hc.hidden_size, generator=g_) * 0.5).to(BF).to(DEV) for i in range(n)]


def test_model_decode_is_bit_equal_eager_graphed_and_prefill_is_unaffected():
    """eager steps and GraphedDecode replays, packed copies on and off: the same logits and tokens; every w4 entry point the
    step uses is counted and no w8 one; a prefill of the same tokens reads the bf16 weight and does not notice the switch"""
    from infinitevl_amd import ops
    from infinitevl_amd.harness import GraphedDecode
    stack, hc = _small_stack()
    B = 2
    x = torch.cat([p[:, :40] for p in _prompts(hc, B)])
    prefill = {}
    for on in (True, False):
        stack.use_packed_weights(on)
        with torch.no_grad():
            cache0 = stack.allocate_inference_cache(B)
            _, lg = stack(inputs_embeds=x, past_key_values=cache0)
        prefill[on] = lg.clone()
    assert torch.equal(prefill[True], prefill[False])
    runs = {}
    for leg in ("on", "off", "eager"):
        stack.use_packed_weights(leg != "off")
        dec = GraphedDecode(stack, cache0.clone(), B)
        dec.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
        n4, n8 = dict(ops.W4_CALLS), dict(ops.W8_CALLS)
        toks, logits = [], []
        for _ in range(8):
            if leg == "eager":
                with torch.no_grad():
                    out = dec._run()
            else:
                dec.step()
                out = dec.logits
            toks.append(dec.token[:, 0].tolist())
            logits.append(out[:, -1].clone())
        torch.cuda.synchronize()
        d4 = {k: ops.W4_CALLS[k] - n4[k] for k in n4}
        assert ops.W8_CALLS == n8, leg
        if leg == "eager":                                   # per step: 5 plain (2 o_proj, 2 down_proj, lm_head) + 4 behind a norm
            assert d4 == dict(linear=8 * 5, linear_swiglu=0, norm_linear=8 * 4, gdn_out_linear=0), d4
        if leg == "off":
            assert sum(d4.values()) == 0, d4
        runs[leg] = (toks, logits)
    stack.use_packed_weights(True)
    assert bool(torch.isfinite(torch.stack(runs["on"][1]).float()).all())
    for leg in ("off", "eager"):
        assert runs[leg][0] == runs["on"][0], leg
        assert all(torch.equal(a, b) for a, b in zip(runs[leg][1], runs["on"][1])), leg


def test_split_decode_reaches_the_gdn_form_and_the_unfused_norm_the_swiglu_form():
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
    n8 = dict(ops.W8_CALLS)
    try:
        for (split, prenorm), want in expect.items():
            ops._SPLIT_DECODE, ops._PRENORM = split, prenorm
            for on in (True, False):
                stack.use_packed_weights(on)
                cache = cache0.clone()
                before = dict(ops.W4_CALLS)
                with torch.no_grad():
                    _, lg1 = stack(input_ids=tok, past_key_values=cache)
                torch.cuda.synchronize()
                d = {k: ops.W4_CALLS[k] - before[k] for k in before}
                assert d == (want if on else dict.fromkeys(want, 0)), (split, prenorm, on, d)
                reached |= {k for k, v in d.items() if v}
                logits.append(lg1)
    finally:
        ops._SPLIT_DECODE, ops._PRENORM = False, True
        stack.use_packed_weights(True)
    assert reached == set(ops.W4_CALLS) and ops.W8_CALLS == n8
    assert bool(torch.isfinite(logits[0].float()).all()) and all(torch.equal(logits[0], l_) for l_ in logits[1:])


@pytest.mark.parametrize("n_slots", [1, 4])
def test_multistream_decode_is_bit_equal_with_the_packed_copies_on_and_off(n_slots):
    from infinitevl_amd import ops
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    stack, hc = _small_stack()
    prompts = _prompts(hc, n_slots)
    runs = {}
    n8 = dict(ops.W8_CALLS)
    for leg in ("on", "off", "eager"):
        stack.use_packed_weights(leg != "off")
        cache = MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=BF)
        dec = GraphedMultiStreamDecode(stack, cache)
        for s, p in enumerate(prompts):
            dec.admit(s, p)
        before = dict(ops.W4_CALLS)
        toks, logits = [], []
        for _ in range(8):
            dec.step(graph=leg != "eager")
            toks.append(dec.token[:, 0].tolist())
            logits.append(dec.logits[:, -1].clone())
        torch.cuda.synchronize()
        if leg == "eager":
            d = {k: ops.W4_CALLS[k] - before[k] for k in before}
            assert d == dict(linear=8 * 5, linear_swiglu=0, norm_linear=8 * 4, gdn_out_linear=0), d
        runs[leg] = (toks, logits)
    stack.use_packed_weights(True)
    assert ops.W8_CALLS == n8
    assert bool(torch.isfinite(torch.stack(runs["on"][1]).float()).all())
    for leg in ("off", "eager"):
        assert runs[leg][0] == runs["on"][0], leg
        assert all(torch.equal(a, b) for a, b in zip(runs[leg][1], runs["on"][1])), leg


def test_switching_the_format_recaptures():
    from infinitevl_amd import ops
    from infinitevl_amd.harness import GraphedDecode
    stack, hc = _small_stack()
    with torch.no_grad():
        cache = stack.allocate_inference_cache(1)
        _, lg = stack(inputs_embeds=_prompts(hc, 1)[0], past_key_values=cache)
    dec = GraphedDecode(stack, cache, 1)
    dec.token.copy_(lg[:, -1].argmax(-1, keepdim=True))
    dec.step()
    g0 = dec.graph
    assert dec._captured_w8 and dec._captured_fmt == "mxfp4" and not dec._stale()
    dec.step()
    assert dec.graph is g0
    stack.quantize_weights_(lm_head=True, fmt="e4m3")      # re-rounds W' onto the e4m3 grid and repacks
    assert dec._stale()
    n8 = ops.W8_CALLS["linear"]
    dec.step()
    assert dec.graph is not g0 and dec._captured_fmt == "e4m3" and not dec._stale() and ops.W8_CALLS["linear"] > n8
    stack.use_packed_weights(False)
    assert dec._stale()
    dec.step()
    assert dec._captured_fmt is None and not dec._captured_w8

"""GPU (-m gpu): the opt-in 64-row weight-stream projections (ivl_linear_m64*_fwd, ops.linear_m64, use_wide_decode(max_rows=);
DESIGN 4.18).  The contracts are those of include/ivl_hip.h.

KERNEL LEVEL, through ops.linear_m64, at the rows of wide64.MS64 -- the first row of a second x tile, both sides of each tile boundary,
the full operand:
  1. the exact-integer probe of tests/projections.py in the three formats, plain and GLU, bias on and off, "index" and "ties", at
     K in wide64.KS x N in wide64.NS and where a wave owns two column tiles (wide64.PAIRS);
  2. C2, row for row: row m of an M-row call torch.equal linear_m16 on that row alone, also among NaN / +-Inf / 1e38 rows; rows >= M of
     a poisoned y untouched;
  3. C3 / C4: packed = bf16 on W', GLU = plain + ops.silu_mul, at 33 and 64 rows;
  4. C1: eight calls of mixed shapes and formats captured in one graph, two replays equal to the eager results.
MODEL LEVEL, on the small stack of tests/test_gpu_multistream.py with 4 layers and a 24-slot cache:
  5. dispatch and counters;   6. a stream has the same logits alone or among 23 neighbours, graphed or eager, and in a 16-slot cache on
  the 16-row kernel;   7. slots 0, 16, 17, 23 of a 24-slot run against the CPU oracle;   8. recapture when max_rows flips;
  9. packed copies on and off.
"""
import os

import pytest
import torch

import fork as fk
import parity
import projections as pj
import wide64
from conftest import rms_rel
from oracle import model as omodel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
FORMATS = ("bf16", "e4m3", "mxfp4")
MS64 = wide64.MS64
ORACLE_BOUND = 2e-2          # tests/test_gpu_multistream.py, test_streams_join_and_leave_vs_alone_and_oracle: `err_o < 2e-2`
N_SLOTS = 24


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


# ---- the entry points on device tensors -------------------------------------------------------------------------------------------------
def _packed(wd, fmt, exact_of=None):
    """the packed copy of the device weight `wd` in `fmt` (None for bf16), WITHOUT touching wd; exact_of: assert that dequantising gives
    back that weight (the probe's ternary weights are exact in both formats)"""
    from infinitevl_amd import ops
    if fmt == "bf16":
        return None
    if fmt == "e4m3":
        codes, _, scale = ops.quantize_rows_e4m3(wd)
        back = ops.dequantize_rows_e4m3(codes, scale)
        pw = ops.PackedWeight(wd, codes, scale)
    else:
        codes, e8m0, _ = ops.quantize_rows_mxfp4(wd)
        back = ops.dequantize_rows_mxfp4(codes, e8m0)
        pw = ops.PackedWeight(wd, *ops.mxfp4_shuffle(codes, e8m0), fmt="mxfp4")
    if exact_of is not None:
        assert torch.equal(back, exact_of), f"{fmt}: the weight is not exact in the format"
    return pw


def _runner(w, fmt):
    """run(x, w, bias, glu) -> y on the CPU, for projections.check_linear: the case's weight lives on the device once; every call must
    move M64_CALLS[fmt] by one and nothing else"""
    from infinitevl_amd import ops
    wd = w.to(DEV)
    pw = _packed(wd, fmt, exact_of=wd)

    def run(x, w_, bias, glu):
        assert w_ is w
        before, before16 = dict(ops.M64_CALLS), dict(ops.M16_CALLS)
        y = ops.linear_m64(x.to(DEV), wd, None if bias is None else bias.to(DEV), glu=glu, w8=pw)
        assert {k: ops.M64_CALLS[k] - before[k] for k in before} == {k: int(k == fmt) for k in before} and ops.M16_CALLS == before16
        return y.cpu()
    return run


# ---- 1. the exact-integer probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, N", wide64.kernel_cases(), ids=lambda v: str(v))
def test_exact_integer_probe_in_the_three_formats(K, N):
    probed = 0
    for glu, variant in wide64.variants(K):
        c = pj.int_case(wide64.ROWS, N, K, glu, variant, Ms=MS64)             # (asserts the probe's conditions, on the CPU)
        for fmt in FORMATS:
            rep = pj.check_linear(_runner(c["w"], fmt), c, MS64)
            assert rep.ok(), (fmt, glu, variant, str(rep))
            probed += rep.probed
    print(f"K={K} N={N}: {probed} elements bit for bit")


@pytest.mark.parametrize("K, N", wide64.PAIRS)
def test_exact_integer_probe_where_a_wave_owns_two_column_tiles(K, N):
    c = pj.int_case(wide64.ROWS, N, K, False, "index", Ms=MS64)
    for fmt in FORMATS:
        rep = pj.check_linear(_runner(c["w"], fmt), c, MS64)
        assert rep.ok(), (fmt, str(rep))


# ---- 2. C2: row m of an M-row call is linear_m16 on that row alone ----------------------------------------------------------------------
def _gauss(R, K, seed, rows=wide64.ROWS):
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g_).to(BF).to(DEV)
    w = (torch.randn(R, K, generator=g_) * K ** -0.5).to(BF).to(DEV)
    return x, w, torch.randn(R, generator=g_).to(BF).to(DEV)


def _raw(fmt, x, wd, pw, bias, glu, M, y):
    """the C entry point itself, into the caller's y"""
    from infinitevl_amd import _lib, ops
    lib = _lib.load()
    R, K = wd.shape
    N = R // 2 if glu else R
    bp = ops._p(bias) if bias is not None else None
    if fmt == "bf16":
        rc = lib.ivl_linear_m64_fwd(ops._p(x), ops._p(wd), bp, ops._p(y), M, N, K, int(glu), ops._stream(x))
    else:
        fn = lib.ivl_linear_m64_w4_fwd if fmt == "mxfp4" else lib.ivl_linear_m64_w8_fwd
        rc = fn(ops._p(x), ops._p(pw.codes), ops._p(pw.scale), bp, ops._p(y), M, N, K, int(glu), ops._stream(x))
    _lib.check(rc)


POISON = (float("nan"), float("inf"), float("-inf"), 1e38)


@pytest.mark.parametrize("N, K", wide64.ROW_CASES)
@pytest.mark.parametrize("glu", [False, True])
def test_row_m_of_an_m_row_call_is_the_16_row_kernel_on_that_row_alone(N, K, glu):
    from infinitevl_amd import ops
    R = 2 * N if glu else N
    x, w, bias_ = _gauss(R, K, 5 * N + K + glu)
    poison = torch.tensor(POISON, dtype=torch.float32).repeat(16)[:, None].expand(64, K).to(BF).to(DEV)     # row r: POISON[r % 4]
    for fmt in FORMATS:
        wd = w.clone()
        pw = None if fmt == "bf16" else ops.PackedWeight.of(wd, fmt=fmt)
        for bias in (None, bias_):
            f64 = lambda xx: ops.linear_m64(xx, wd, bias, glu=glu, w8=pw)     # noqa: E731
            alone = torch.stack([ops.linear_m16(x[m:m + 1], wd, bias, glu=glu, w8=pw)[0] for m in range(wide64.ROWS)])
            assert tuple(alone.shape) == (64, N) and bool(torch.isfinite(alone.float()).all()) and float(alone.float().abs().max()) > 0
            for M in MS64:
                y = f64(x[:M])
                assert tuple(y.shape) == (M, N)
                bad = (y != alone[:M]).any(1).nonzero().flatten().tolist()
                assert not bad and torch.equal(y, alone[:M]), (fmt, bias is not None, M, "rows that differ", bad)
                for m in sorted({0, 16, M - 1}):                              # the same row among rows of NaN, +Inf, -Inf and 1e38
                    other = poison[:M].clone()
                    other[m] = x[m]
                    assert torch.equal(f64(other)[m], alone[m]), (fmt, bias is not None, M, m, "among poisoned rows")
            for M in (1, 16, 17, 33, 49):                                     # rows >= M of y are never written, nor anything behind y
                buf = torch.full((64 * N + 64,), 24576.0, dtype=BF, device=DEV)
                y = buf[:64 * N].view(64, N)
                _raw(fmt, x, wd, pw, bias, glu, M, y)
                torch.cuda.synchronize()
                assert torch.equal(y[:M], alone[:M]) and bool((buf[M * N:] == 24576.0).all()), (fmt, M)


# ---- 3. C3 / C4 -------------------------------------------------------------------------------------------------------------------------
def _silu_mul(gate_up):
    """ops.silu_mul (ivl_silu_mul_fwd: element-wise, I % 8 == 0) on a fused [M, 2I] output of any I: gate and up are moved to the
    halves of a zero-padded [M, 2I'] buffer, I' the next multiple of 8 -- the same operation on the same pairs of elements"""
    from infinitevl_amd import ops
    M, I = gate_up.shape[0], gate_up.shape[1] // 2
    Ip = -(-I // 8) * 8
    buf = torch.zeros(M, 2 * Ip, dtype=BF, device=gate_up.device)
    buf[:, :I], buf[:, Ip:Ip + I] = gate_up[:, :I], gate_up[:, I:]
    return ops.silu_mul(buf)[:, :I]


@pytest.mark.parametrize("N, K", [(17, 2080), (4100, 2048), (64, 11008)])
@pytest.mark.parametrize("fmt", ["e4m3", "mxfp4"])
def test_packed_equals_bf16_on_w_prime_and_glu_equals_plain_plus_gate(N, K, fmt):
    from infinitevl_amd import ops
    x, w, bias = _gauss(2 * N, K, N + K)
    w0 = w.clone()
    pw = ops.PackedWeight.of(w, fmt=fmt)                                      # rounds w to W' in place
    assert pw.fmt == fmt and not torch.equal(w, w0)
    for M in (33, 64):
        for b in (None, bias):
            plain = ops.linear_m64(x[:M], w, b)                               # the fused weight as a plain [2N, K] projection
            assert torch.equal(ops.linear_m64(x[:M], w, b, w8=pw), plain), (M, "C3, plain")
            glu = ops.linear_m64(x[:M], w, b, glu=True)
            assert torch.equal(ops.linear_m64(x[:M], w, b, glu=True, w8=pw), glu), (M, "C3, GLU")
            assert torch.equal(glu, _silu_mul(plain)), (M, "C4")
            assert tuple(glu.shape) == (M, N) and bool(torch.isfinite(glu.float()).all()) and float(glu.float().abs().max()) > 0.0
    torch.cuda.synchronize()


# ---- 4. C1 ------------------------------------------------------------------------------------------------------------------------------
def test_eight_calls_replayed_from_a_graph_equal_the_eager_results():
    from infinitevl_amd import ops
    calls = []
    for i, (N, K, glu, fmt, M) in enumerate([(100, 2080, False, "bf16", 64), (100, 2080, True, "e4m3", 17), (17, 4128, False, "mxfp4", 33),
                                              (4100, 2048, True, "bf16", 48), (4100, 2048, False, "e4m3", 49), (64, 11008, True, "mxfp4", 64),
                                              (8209, 96, False, "bf16", 31), (16, 96, True, "mxfp4", 32)]):
        x, w, bias = _gauss(2 * N if glu else N, K, 100 + i)
        pw = None if fmt == "bf16" else ops.PackedWeight.of(w, fmt=fmt)
        calls.append((x[:M].contiguous(), w, bias, glu, pw))
    run = lambda: [ops.linear_m64(x, w, b, glu=glu, w8=pw) for x, w, b, glu, pw in calls]      # noqa: E731
    eager = run()
    again = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again)), "two eager runs"
    assert all(bool(torch.isfinite(a.float()).all()) for a in eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for rep in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, outs)), rep


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def _small(seed=3):
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(96)
    params = parity.bf16_params(omodel.random_params(oc, seed=seed, vocab=hc.vocab_size))
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, params)
    return stack.to(DEV, BF).eval().fuse_(), hc, oc, params


@pytest.fixture(scope="module")
def small():
    """the bf16 stack; every test leaves its switch off"""
    return _small()


def _decoder(stack, hc, n_slots=N_SLOTS, **kw):
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedMultiStreamDecode
    return GraphedMultiStreamDecode(stack, MultiStreamCache(config=hc, n_slots=n_slots, device=DEV, dtype=BF), **kw)


def _prompt(hc, T, seed):
    return fk.prompt(hc, T, seed, DEV)[0]


def _counters():
    from infinitevl_amd import ops
    return dict(ops.M64_CALLS), dict(ops.M16_CALLS), dict(ops.W8_CALLS), dict(ops.W4_CALLS)


def _delta(before, which=0):
    from infinitevl_amd import ops
    now = (ops.M64_CALLS, ops.M16_CALLS)[which]
    return {k: now[k] - before[which][k] for k in now}


PER_STEP = 4 * 4 + 1         # q|k|v or the GDN in-projection, o_proj, gate|up, down_proj in each of 4 layers, and lm_head
ZERO = dict.fromkeys(FORMATS, 0)


def _admit_all(dec, hc, seed0, n=N_SLOTS):
    # 70 rows and more: no prefill is a call of 17..64 rows
    for s_ in range(n):
        dec.admit(s_, _prompt(hc, 70 + 3 * s_, seed0 + s_))


# ---- 5. dispatch ------------------------------------------------------------------------------------------------------------------------
def test_dispatch_follows_max_rows_and_the_packed_format():
    from infinitevl_amd import ops
    stack, hc, _, _ = _small(seed=5)
    assert len(stack.layers) == 4 and stack.layers[1].self_attn._fused_w.shape[0] == 1544, "the GDN in-projection has a column tail"
    try:
        for fmt in FORMATS:
            if fmt != "bf16":
                stack.quantize_weights_(lm_head=True, fmt=fmt)
            for setting in ("off", "wide16", "wide64"):
                stack.use_wide_decode(setting != "off", **({"max_rows": 64} if setting == "wide64" else {}))
                dec = _decoder(stack, hc)
                _admit_all(dec, hc, 50)
                before = _counters()
                for _ in range(3):
                    dec.step()
                torch.cuda.synchronize()
                runs = dec._warmup + 1                                         # the python calls of graphed steps are those of the capture
                want = dict(ZERO)
                if setting == "wide64":
                    want[fmt] = PER_STEP * runs
                assert _delta(before) == want, (fmt, setting, _delta(before))
                before2 = _counters()
                for _ in range(2):
                    dec.step(graph=False)
                want2 = dict(ZERO)
                if setting == "wide64":
                    want2[fmt] = PER_STEP * 2
                assert _delta(before2) == want2, (fmt, setting, "eager")
                # 24 rows are neither the 16-row kernel's nor the small-M kernels': their counters never move
                assert _delta(before, 1) == ZERO and (ops.W8_CALLS, ops.W4_CALLS) == before[2:], (fmt, setting)
                assert bool(torch.isfinite(dec.logits.float()).all())
        # a bound below the row count: 24 rows under max_rows=20 stay with the library
        stack.use_wide_decode(True, max_rows=20)
        dec = _decoder(stack, hc)
        _admit_all(dec, hc, 50)
        before = _counters()
        dec.step(graph=False)
        assert _delta(before) == ZERO and _delta(before, 1) == ZERO
        # while an adapter table is attached no projection of more than 16 rows takes the kernel, lm_head included, in every setting
        stack.enable_adapters(1, 8)
        for adapters in (False, True):
            stack.use_wide_decode(True, adapters=adapters, max_rows=64)
            dec = _decoder(stack, hc)
            _admit_all(dec, hc, 50)
            before = _counters()
            dec.step(graph=False)
            torch.cuda.synchronize()
            assert _delta(before) == ZERO and _delta(before, 1) == ZERO and bool(torch.isfinite(dec.logits.float()).all()), adapters
        stack.enable_adapters(0)
        before = _counters()
        dec.step(graph=False)
        assert _delta(before)["mxfp4"] == PER_STEP, "detached: on the kernel"
    finally:
        stack.use_wide_decode(False)


# ---- 6. slot and neighbours, across cache sizes -----------------------------------------------------------------------------------------
def test_a_stream_has_the_same_logits_alone_or_among_23_neighbours_and_in_a_16_slot_cache(small):
    """follows from C2 only if every other launch of the step is row-independent too: the 16-slot leg runs the 16-row kernel"""
    stack, hc, _, _ = small
    stack.use_wide_decode(True, max_rows=64)
    try:
        x = _prompt(hc, 130, 11)
        out = {}
        for leg, n_slots, slot, crowd, graph in (("alone", 24, 3, False, True), ("crowd", 24, 20, True, True),
                                                 ("alone eager", 24, 3, False, False), ("crowd eager", 24, 20, True, False),
                                                 ("16 slots", 16, 3, False, True)):
            dec = _decoder(stack, hc, n_slots)
            if crowd:
                for s_ in range(n_slots):
                    if s_ != slot:
                        dec.admit(s_, _prompt(hc, 33 + 5 * s_, 200 + s_))
            dec.admit(slot, x)
            before = _counters()
            toks, logits = [], []
            for _ in range(12):
                toks.append(int(dec.token[slot, 0]))
                dec.step(graph=graph)
                logits.append(dec.logits[slot, -1].clone())
            torch.cuda.synchronize()
            d64, d16 = _delta(before)["bf16"], _delta(before, 1)["bf16"]
            assert (d64 > 0 and d16 == 0) if n_slots == 24 else (d64 == 0 and d16 > 0), (leg, d64, d16)
            out[leg] = (toks, logits)
        assert bool(torch.isfinite(torch.stack(out["alone"][1]).float()).all())
        for leg in ("crowd", "alone eager", "crowd eager", "16 slots"):
            assert out[leg][0] == out["alone"][0], leg
            for i, (a, b) in enumerate(zip(out[leg][1], out["alone"][1])):
                assert torch.equal(a, b), (leg, "step", i, int((a != b).sum()))
    finally:
        stack.use_wide_decode(False)


# ---- 7. the oracle ----------------------------------------------------------------------------------------------------------------------
def test_streams_of_a_24_slot_run_match_the_oracle(small):
    """the measure and the bound of test_gpu_multistream.py's streams (rms_rel of the logits against the CPU oracle fed the same
    tokens, below 2e-2), for the streams in slots 0, 16, 17 and 23 of a full 24-slot run over 4 steps (printed per step).  Measured on
    the MI355X: 1.01e-2 .. 1.943e-2 over the 4 streams x 4 steps (largest: slot 17, step 3)."""
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_multistream.py")).read()
    assert "assert err_o < 2e-2" in src and ORACLE_BOUND == 2e-2, "the bound is that test's"
    stack, hc, oc, params = small
    emb = params["embed_tokens.weight"]
    stack.use_wide_decode(True, max_rows=64)
    checked, steps = (0, 16, 17, 23), 4
    try:
        dec = _decoder(stack, hc)
        prompts = [_prompt(hc, 40 + 5 * s_, 300 + s_) for s_ in range(N_SLOTS)]
        for s_, x in enumerate(prompts):
            dec.admit(s_, x)
        before = _counters()
        toks, logits = [], []
        for _ in range(steps):
            toks.append(dec.token[:, 0].tolist())
            dec.step()
            logits.append(dec.logits[:, -1].float().cpu())
        torch.cuda.synchronize()
        assert _delta(before)["bf16"] == PER_STEP * (dec._warmup + 1) and _delta(before, 1) == ZERO
    finally:
        stack.use_wide_decode(False)
    worst = 0.0
    for s_ in checked:
        x = prompts[s_]
        T = x.shape[1]
        pid = torch.arange(T)[None, None, :].expand(3, 1, T)
        ocache = omodel.new_cache(oc, cache_dtype=BF)
        omodel.text_stack(params, x.float().cpu(), pid, oc, ocache, act_dtype=BF, kernel_rounding=BF)
        for i in range(steps):
            pid1 = torch.full((3, 1, 1), T + i, dtype=torch.int64)
            h = omodel.text_stack(params, emb[toks[i][s_]].reshape(1, 1, -1), pid1, oc, ocache, act_dtype=BF, kernel_rounding=BF)
            err_o = rms_rel(h[0, -1] @ emb.T, logits[i][s_])
            worst = max(worst, err_o)
            print(f"slot {s_} step {i}: rms_rel against the oracle {err_o:.3e}")
            assert err_o < ORACLE_BOUND, (s_, i, err_o)
    print(f"largest rms_rel against the oracle over 4 streams x 4 steps: {worst:.3e} (bound {ORACLE_BOUND})")


# ---- 8. recapture -----------------------------------------------------------------------------------------------------------------------
def test_a_graph_is_recaptured_when_max_rows_flips_and_not_otherwise(small):
    stack, hc, _, _ = small
    stack.use_wide_decode(True, max_rows=64)
    try:
        dec = _decoder(stack, hc)
        _admit_all(dec, hc, 90)
        dec.step()
        g0 = dec.graph
        assert dec._captured_wide and dec._captured_wide_rows == 64 and not dec._stale()
        dec.step()
        stack.use_wide_decode(True, max_rows=64)                               # the same setting again
        dec.step()
        assert dec.graph is g0
        stack.use_wide_decode(True)
        assert dec._stale()
        before = _counters()
        dec.step()
        g1 = dec.graph
        assert g1 is not g0 and dec._captured_wide and dec._captured_wide_rows == 16 and not dec._stale() and _delta(before) == ZERO
        dec.step()
        stack.use_wide_decode(True, max_rows=16)
        dec.step()
        assert dec.graph is g1
        stack.use_wide_decode(True, max_rows=64)
        assert dec._stale()
        before = _counters()
        dec.step()
        assert dec.graph is not g1 and dec._captured_wide_rows == 64 and _delta(before)["bf16"] == PER_STEP * (dec._warmup + 1)
        torch.cuda.synchronize()
    finally:
        stack.use_wide_decode(False)


# ---- 9. packed on and off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["e4m3", "mxfp4"])
def test_the_24_slot_run_is_bit_equal_with_the_packed_copies_on_and_off(fmt):
    from infinitevl_amd import ops
    stack, hc, _, _ = _small(seed=7)
    stack.quantize_weights_(lm_head=True, fmt=fmt).use_wide_decode(True, max_rows=64)
    prompts = [_prompt(hc, 70 + 3 * i, 70 + i) for i in range(N_SLOTS)]
    runs = {}
    for leg in ("on", "off", "eager"):
        stack.use_packed_weights(leg != "off")
        dec = _decoder(stack, hc)
        for s_, p in enumerate(prompts):
            dec.admit(s_, p)
        before = _counters()
        toks, logits = [], []
        for _ in range(12):
            dec.step(graph=leg != "eager")
            toks.append(dec.token[:, 0].tolist())
            logits.append(dec.logits[:, -1].clone())
        torch.cuda.synchronize()
        d = _delta(before)
        key = "bf16" if leg == "off" else fmt
        assert d[key] > 0 and all(v == 0 for k, v in d.items() if k != key), (leg, d)
        assert _delta(before, 1) == ZERO and (ops.W8_CALLS, ops.W4_CALLS) == before[2:]
        runs[leg] = (toks, logits)
    assert bool(torch.isfinite(torch.stack(runs["on"][1]).float()).all())
    for leg in ("off", "eager"):
        assert runs[leg][0] == runs["on"][0], leg
        assert all(torch.equal(a, b) for a, b in zip(runs[leg][1], runs["on"][1])), leg

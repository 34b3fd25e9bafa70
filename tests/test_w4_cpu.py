"""CPU: weight-only MXFP4 for the decode step -- the quantiser, the shuffled layout, the judges of tests/w4.py, the C ABI's refusals,
PackedWeight's formats and quantize_weights_(fmt="mxfp4") on a small stack.  No tolerance anywhere.

  * ops.quantize_rows_mxfp4 against the independent restatement of tests/w4.py (equal codes and exponents) on gaussian rows, rows
    with zero blocks, blocks whose amax is exactly 6 2^e (= 0.75 2^x) and 4 2^e and the next bf16 above each, every tie point of
    the e2m1 grid in both signs and -0.0; W' is bf16-exact, amax / 2^e lies in (3, 6], |w - W'| <= 2^e (half the widest gap);
  * mxfp4_shuffle: the byte offsets of the header's formula directly, the padding bytes, unshuffle(shuffle) = identity;
  * the judge bites: the honest fp32 emulation of the stated order passes the probe in all three variants, each of five wrong
    ones is reported;
  * the four entry points are declared and exported and refuse what their w8 twins refuse, K % 32 != 0 and misaligned wq / sq,
    on the host, before anything is launched;
  * PackedWeight: the format field, from_mxfp4, stale detection through a view; quantize_weights_(fmt="mxfp4").
"""
import ctypes
import os
import subprocess

import pytest
import torch

import rowwise as rw
import w4
from conftest import ROOT

BF = torch.bfloat16
TIES = ((0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6))       # (w / 2^e, the code it rounds to)


# ---- the quantiser --------------------------------------------------------------------------------------------------------------------
def _quantiser_inputs():
    g_ = rw.gen(11)
    K = 96
    w = torch.cat([torch.randn(6, K, generator=g_) * 0.02, torch.randn(2, K, generator=g_) * 0.02 * 1e-3,
                   torch.randn(2, K, generator=g_) * 30.0]).to(BF)
    w[1, 32:64] = 0.0                                      # zero blocks
    w[2] = 0.0
    w[3, 0:32] = -0.0
    edge = []
    for j in (-20, -9, -1, 0, 3, 11):
        for top in (6.0, 4.0):                             # 6 2^j = 0.75 2^(j + 3): the end of an exponent's range; 4 2^j: m = 0.5
            t = torch.tensor([top * 2.0 ** j], dtype=torch.float64)
            for amax in (t, rw.next_bf16(t)):
                r = (torch.randn(K, generator=g_) * float(amax) * 0.4).clamp(-float(amax), float(amax)).to(BF)
                for b in range(K // 32):
                    r[32 * b + int(torch.randint(0, 32, (1,), generator=g_))] = float(amax) * (1 if (j + b) % 2 else -1)
                edge.append(r)
    return torch.cat([w, torch.stack(edge)])


def test_quantiser_equals_the_restatement_and_keeps_its_promises():
    from infinitevl_amd import ops
    w = _quantiser_inputs()
    codes, e8m0, exp = ops.quantize_rows_mxfp4(w)
    rc, rs, re_ = w4.quantize_ref(w)
    N, K = w.shape
    assert codes.dtype == torch.uint8 and e8m0.dtype == torch.uint8 and exp.dtype == torch.int32
    assert tuple(codes.shape) == (N, K // 2) and tuple(e8m0.shape) == (N, K // 32) and tuple(exp.shape) == (N, K // 32)
    assert torch.equal(exp, re_), (exp - re_).nonzero()
    assert torch.equal(e8m0, rs) and torch.equal(codes, rc), (codes != rc).nonzero()[:5]
    assert torch.equal(e8m0.to(torch.int32) - 127, exp)
    assert int(exp[1, 1]) == 0 and bool((codes[1, 16:32] == 0).all()) and bool((exp[2] == 0).all()), "zero blocks"
    assert bool((codes[3, :16] == 0x88).all()) and int(exp[3, 0]) == 0, "-0.0 keeps its sign bit"
    amax = w.double().view(N, -1, 32).abs().amax(2)
    ratio = amax / rw._pow2(exp.to(torch.int64))
    assert bool(((ratio > 3.0) & (ratio <= 6.0))[amax > 0].all()), ratio
    assert {float(r) for r in ratio[10:].flatten()} >= {6.0, 4.0}, "the edge rows sit on both ends"
    wd = w4.dequantize_ref(w4.unpack(codes), e8m0)
    assert torch.equal(rw.round_bf16(wd), wd), "W' is bf16-exact"
    wq = ops.dequantize_rows_mxfp4(codes, e8m0)
    assert wq.dtype == BF and torch.equal(wq.double(), wd)
    assert bool((torch.signbit(wq) == torch.signbit(w)).all()), "signs survive, zeros included"
    s = rw._pow2(exp.to(torch.int64)).repeat_interleave(32, 1)
    err, a = (w.double() - wd).abs(), w.double().abs()
    assert bool((err <= s).all()) and bool((err <= 0.25 * s)[a <= 2.0 * s].all())
    assert torch.equal(w4.encode_e2m1(wd / s), w4.unpack(codes)), "W' with the same exponents: the codes come back"


@pytest.mark.parametrize("e", [-7, 0, 5])
def test_every_tie_goes_to_the_even_mantissa_bit_in_both_signs(e):
    from infinitevl_amd import ops
    vals = [v for v, _ in TIES] + [-v for v, _ in TIES] + [-0.0, 0.0, -0.125, 6.0]
    want = [c for _, c in TIES] + [c | 8 for _, c in TIES] + [8, 0, 8, 7]
    w = torch.zeros(1, 32, dtype=torch.float64)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    w = (w * 2.0 ** e).to(BF)
    assert torch.equal(w.double(), torch.tensor(vals + [0.0] * (32 - len(vals)), dtype=torch.float64)[None] * 2.0 ** e), "exact in bf16"
    codes, e8m0, exp = ops.quantize_rows_mxfp4(w)
    assert int(exp) == e and int(e8m0) == e + 127
    assert w4.unpack(codes)[0, :len(vals)].tolist() == want
    assert torch.equal(codes, w4.quantize_ref(w)[0])
    assert [float(w4.decode_e2m1(torch.tensor(c))) for c in range(8)] == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert torch.equal(w4.decode_e2m1(torch.arange(8, 16)), -w4.decode_e2m1(torch.arange(8))) and tuple(ops.E2M1_VALUES) == tuple(w4.E2M1.tolist())


def test_quantiser_refusals():
    from infinitevl_amd import ops
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.quantize_rows_mxfp4(torch.zeros(2, 40, dtype=BF))
    bad = torch.ones(1, 32)
    for v in (float("inf"), float("nan")):
        bad[0, 3] = v
        with pytest.raises(ValueError, match="non-finite"):
            ops.quantize_rows_mxfp4(bad.to(BF))
    for big in (2.0 ** 120, 2.0 ** -120):
        with pytest.raises(ValueError, match="100"):
            ops.quantize_rows_mxfp4(torch.full((1, 32), big).to(BF))
    with pytest.raises(ValueError, match="bf16"):
        ops.quantize_rows_mxfp4(torch.zeros(2, 32))
    with pytest.raises(ValueError, match="mxfp4_shuffle"):
        ops.mxfp4_shuffle(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))


# ---- the layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 512, 2016, 2048, 2080, 4096, 11008])
def test_shuffle_puts_every_byte_where_the_header_says(K):
    from infinitevl_amd import ops
    g_ = rw.gen(K)
    N = 3
    codes = torch.randint(1, 256, (N, K // 2), generator=g_).to(torch.uint8)         # no 0x00: padding can be told apart
    e8m0 = torch.randint(0, 127, (N, K // 32), generator=g_).to(torch.uint8)         # no 127
    wq, sq = ops.mxfp4_shuffle(codes, e8m0)
    Kp = 2048 * ((K + 2047) // 2048)
    assert wq.dtype == torch.uint8 and sq.dtype == torch.uint8 and tuple(wq.shape) == (N, Kp // 2) and tuple(sq.shape) == (N, Kp // 32)
    assert wq.is_contiguous() and sq.is_contiguous()
    for t in range(Kp // 2048):                            # the formula itself: chunk 256 t + l + 64 u at byte 1024 t + 16 l + 4 u
        for l in range(64):
            for u in range(4):
                c = 256 * t + l + 64 * u
                got = wq[:, 1024 * t + 16 * l + 4 * u:1024 * t + 16 * l + 4 * u + 4]
                assert torch.equal(got, codes[:, 4 * c:4 * c + 4] if 8 * c < K else torch.zeros(N, 4, dtype=torch.uint8)), (t, l, u)
                if l % 4 == 0:                             # block 64 t + (l >> 2) + 16 u at byte 64 t + 4 (l >> 2) + u
                    i = 64 * t + (l >> 2) + 16 * u
                    assert c // 4 == i
                    got = sq[:, 64 * t + 4 * (l >> 2) + u]
                    assert torch.equal(got, e8m0[:, i] if 32 * i < K else torch.full((N,), 127, dtype=torch.uint8)), (t, l, u)
    assert int((wq == 0).sum()) == N * (Kp - K) // 2 and int((sq == 127).sum()) == N * (Kp - K) // 32, "padding: 0x0 and 127"
    rq, rs = w4.shuffle_ref(codes, e8m0)
    assert torch.equal(wq, rq) and torch.equal(sq, rs)
    back = ops.mxfp4_unshuffle(wq, sq, K)
    assert torch.equal(back[0], codes) and torch.equal(back[1], e8m0)
    if K % 2048 == 0:
        full = ops.mxfp4_unshuffle(wq, sq)
        assert torch.equal(full[0], codes) and torch.equal(full[1], e8m0)
    with pytest.raises(ValueError, match="mxfp4_unshuffle"):
        ops.mxfp4_unshuffle(wq, sq, Kp + 32)


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def _check(case, wrong=""):
    glu, norm, N, K, Ms, variant = case
    c = w4.probe_case(*case)
    if norm:
        return w4.check_norm_linear(lambda *a: w4.emu_w4_norm_linear(*a, wrong=wrong), c, Ms)
    return w4.check_linear(lambda *a: w4.emu_w4_linear(*a, wrong=wrong), c, Ms)


def test_probe_conditions_hold_and_the_honest_emulation_passes():
    """the same case list as the GPU test: the seeds are chosen here, on the scaled float64 sums"""
    probed = 0
    for case in w4.PROBE:
        rep = _check(case)
        assert rep.ok(), str(rep)
        probed += rep.probed
    assert {c[5] for c in w4.PROBE} == {"index", "ties", "codes"} and {c[1] for c in w4.PROBE} == {False, True}
    print(f"{len(w4.PROBE)} cases, {probed} elements bit for bit")
    c = w4.probe_case(False, False, 5, 2080, (1, 2, 3, 4), "index")
    e = c["e8m0"].to(torch.int64) - 127
    assert int(e.min()) == -2 and int(e.max()) == 2 and bool((e[:, :-1] != e[:, 1:]).any()), "per-block exponents"
    assert set(c["nib"].unique().tolist()) == {0x0, 0x2, 0xA}
    t = w4.probe_case(False, False, 5, 544, (1, 2, 3, 4), "ties")
    et = t["e8m0"].to(torch.int64) - 127
    assert bool((et == et[:, :1]).all()) and len(et[:, 0].unique()) > 1, "one exponent per row, different between rows"


@pytest.mark.parametrize("wrong", w4.WRONG)
def test_wrong_emulation_is_reported(wrong):
    hits = [c for c in w4.PROBE if c[2] < 100 and not _check(c, wrong=wrong).ok()]
    print(f"{wrong}: reported in {len(hits)} cases, e.g. {hits[:3]}")
    assert hits, wrong


def test_emulated_chain_on_scaled_weights_is_the_chain_on_w_prime():
    """the chain over decode(code) 2^e IS the bf16 kernel's chain on W' (the weights are the same fp32 numbers): the reason the w4
    kernels can equal the bf16 kernels on the dequantised weight"""
    from infinitevl_amd import ops
    import w8
    g_ = rw.gen(3)
    x = torch.randn(2, 544, generator=g_).to(BF)
    w = (torch.randn(6, 544, generator=g_) * 0.02).to(BF)
    codes, e8m0, _ = ops.quantize_rows_mxfp4(w)
    a = w8.emu_chain(x, w4.dequantize_ref(w4.unpack(codes), e8m0).float())
    b = w8.emu_chain(x, ops.dequantize_rows_mxfp4(codes, e8m0).float())
    assert torch.equal(a, b)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NAMES = ("ivl_linear_small_m_w4_fwd", "ivl_linear_swiglu_small_m_w4_fwd", "ivl_norm_linear_small_m_w4_fwd",
         "ivl_gdn_out_linear_small_m_w4_fwd")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_entry_points_are_declared_and_exported(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in _lib.PROTOTYPES and name in exported and hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[name.replace("_w4", "_w8")][1]), "the w8 twin's argument list"
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12


def test_refusals_come_before_any_launch(lib):
    """never-dereferenced pointers on a machine that may have no GPU: every refusal is decided on the host"""
    from infinitevl_amd import _lib
    p, odd16, odd4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1002)
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    lin, glu, nrm, gdn = (getattr(lib, n) for n in NAMES)
    for fn in (lin, glu):
        assert fn(p, p, p, None, p, 5, 16, 64, None) == UNS and fn(p, p, p, None, p, 0, 16, 64, None) == UNS          # M
        assert fn(p, p, p, None, p, 1, 16, 60, None) == INV and fn(p, p, p, None, p, 1, 0, 64, None) == INV           # K % 8, N
        for K in (40, 8, 2056):
            assert fn(p, p, p, None, p, 1, 16, K, None) == INV and b"multiple of 32" in lib.ivl_last_error(), K       # K % 32
        assert fn(p, p, None, None, p, 1, 16, 64, None) == INV and b"NULL" in lib.ivl_last_error()                    # sq
        assert fn(p, None, p, None, p, 1, 16, 64, None) == INV and fn(None, p, p, None, p, 1, 16, 64, None) == INV
        assert fn(p, p, p, None, None, 1, 16, 64, None) == INV
        assert fn(p, odd16, p, None, p, 1, 16, 64, None) == INV and b"aligned" in lib.ivl_last_error()                # wq
        assert fn(p, p, odd4, None, p, 1, 16, 64, None) == INV and b"aligned" in lib.ivl_last_error()                 # sq
    n_ok = (p, None, p, 1e-6, None, p, p, None, p)
    assert nrm(*n_ok, 5, 16, 512, 0, None) == UNS and nrm(*n_ok, 1, 16, 516, 0, None) == INV
    for K in (32, 256, 480, 4128, 8192):
        assert nrm(*n_ok, 1, 16, K, 0, None) == UNS, K
        assert b"512 <= K <= 4096" in lib.ivl_last_error()
    assert nrm(*n_ok, 1, 16, 520, 0, None) == INV and b"multiple of 32" in lib.ivl_last_error()
    assert nrm(p, None, None, 1e-6, None, p, p, None, p, 1, 16, 512, 1, None) == INV                                   # norm weight
    assert nrm(p, p, p, 1e-6, None, p, p, None, p, 1, 16, 512, 1, None) == INV                                         # residual, no h_out
    assert nrm(p, None, p, 1e-6, None, p, None, None, p, 1, 16, 512, 0, None) == INV                                   # sq
    assert nrm(p, None, p, 1e-6, None, None, p, None, p, 1, 16, 512, 0, None) == INV                                   # wq
    assert nrm(p, None, p, 1e-6, None, odd16, p, None, p, 1, 16, 512, 0, None) == INV
    assert nrm(p, None, p, 1e-6, None, p, odd4, None, p, 1, 16, 512, 0, None) == INV

    def g(H, M=1, K=None, wq=p, sq=p, gate_ld=512):
        return gdn(p, p, gate_ld, p, 1e-5, H, p, 512, 0, 128, p, p, wq, sq, None, p, M, 8, H * 256 if K is None else K, None)
    for H in (0, 1, 17):
        assert g(H) == UNS and b"2 <= H <= 16" in lib.ivl_last_error()
    assert g(2, M=5) == UNS and g(2, M=0) == UNS and g(2, K=544) == UNS
    assert g(2, sq=None) == INV and g(2, wq=None) == INV and g(2, gate_ld=514) == INV
    assert g(2, wq=odd16) == INV and g(2, sq=odd4) == INV and b"aligned" in lib.ivl_last_error()


# ---- PackedWeight and quantize_weights_ -------------------------------------------------------------------------------------------------
def _stack(intermediate=96):
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=intermediate, num_hidden_layers=2,
                               num_attention_heads=4, num_key_value_heads=2, head_dim=16, sliding_window=8,
                               layer_types=["sliding_attention", "linear_attention"], num_linear_heads=4,
                               num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


def test_packed_weight_formats_from_mxfp4_and_stale_detection_through_a_view():
    from infinitevl_amd import ops
    g_ = rw.gen(21)
    fused = (torch.randn(12, 2080, generator=g_) * 0.02).to(BF)
    a, b = fused[:5], fused[5:]                            # "parameters" that are views of the fused weight
    orig = fused.clone()
    codes, e8m0, _ = ops.quantize_rows_mxfp4(orig)
    pw = ops.PackedWeight.from_mxfp4(fused, codes, e8m0, also=(a, b))
    assert pw.fmt == "mxfp4" and pw.shape == (12, 2080) and pw.check(fused) is pw
    assert torch.equal(fused, ops.dequantize_rows_mxfp4(codes, e8m0)) and not torch.equal(fused, orig), "W' in place"
    assert tuple(pw.codes.shape) == (12, 2048) and tuple(pw.scale.shape) == (12, 128) and pw.scale.dtype == torch.uint8
    back = ops.mxfp4_unshuffle(pw.codes, pw.scale, 2080)
    assert torch.equal(back[0], codes) and torch.equal(back[1], e8m0), "the round trip"
    pw2 = ops.PackedWeight.of(orig.clone(), fmt="mxfp4")
    assert torch.equal(pw2.codes, pw.codes) and torch.equal(pw2.scale, pw.scale) and pw2.exp is not None
    pe = ops.PackedWeight.of(orig.clone())
    assert pe.fmt == "e4m3" and pe.shape == (12, 2080) and pe.scale.dtype == torch.float32
    # dispatch on the format: on the CPU both take the library path on W'; neither counter moves, a stale copy raises in both
    x = torch.zeros(1, 1, 2080, dtype=BF)
    n4, n8 = dict(ops.W4_CALLS), dict(ops.W8_CALLS)
    assert torch.equal(ops.linear(x, fused, w8=pw), ops.linear(x, fused))
    assert ops.W4_CALLS == n4 and ops.W8_CALLS == n8 and set(ops.W4_CALLS) == set(ops.W8_CALLS)
    pw.count("linear")
    pe.count("linear")
    assert ops.W4_CALLS["linear"] == n4["linear"] + 1 and ops.W8_CALLS["linear"] == n8["linear"] + 1
    with pytest.raises(RuntimeError, match="does not belong"):
        pw.check(fused[:6])                                # the same pointer and version counter, another logical shape
    b.mul_(2.0)                                            # a write through a view: the fused tensor's own counter moves too
    assert pw.stale(fused)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(x, fused, w8=pw)
    with pytest.raises(ValueError, match="fmt"):
        ops.PackedWeight.of(orig.clone(), fmt="int4")
    with pytest.raises(ValueError, match="from_mxfp4"):
        ops.PackedWeight.from_mxfp4(orig.clone(), codes[:, :-1], e8m0)
    with pytest.raises(ValueError, match="shuffled"):
        ops.PackedWeight(orig, codes, e8m0, fmt="mxfp4")   # plain row-major codes are not the kernel layout (K = 2080: other shapes)


def test_quantize_weights_mxfp4_rounds_in_place_and_keeps_the_fused_views():
    from infinitevl_amd import ops
    m = _stack()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.quantize_weights_(fmt="mxfp4", lm_head=True) is m and m._w8_on and m._w8_fmt == "mxfp4"
    after = m.state_dict()
    proj = [k for k in before if k.endswith("_proj.weight")] + ["embed_tokens.weight"]
    for k, v in before.items():
        if k in proj:
            codes, e8m0, _ = ops.quantize_rows_mxfp4(v)
            assert torch.equal(after[k], ops.dequantize_rows_mxfp4(codes, e8m0)) and not torch.equal(after[k], v), k
        else:
            assert torch.equal(after[k].view(torch.uint8), v.view(torch.uint8)), k
    att, gdn, mlp = m.layers[0].self_attn, m.layers[1].self_attn, m.layers[0].mlp
    for pw, wt in ((att._w8_qkv, att._fused_w), (att._w8_o, att.o_proj.weight), (gdn._w8_in, gdn._fused_w),
                   (gdn._w8_o, gdn.o_proj.weight), (mlp._w8_gu, mlp._fused_w), (mlp._w8_down, mlp.down_proj.weight),
                   (m._w8_lm_head, m.embed_tokens.weight)):
        assert pw.fmt == "mxfp4" and pw.check(wt) is pw and pw.shape == tuple(wt.shape)
        codes, e8m0 = ops.mxfp4_unshuffle(pw.codes, pw.scale, wt.shape[1])
        assert torch.equal(ops.dequantize_rows_mxfp4(codes, e8m0), wt), "the bf16 weight holds W'"
    assert att.q_proj.weight.data_ptr() == att._fused_w.data_ptr()
    m.use_packed_weights(False)
    assert not m._w8_on and att._w8_o is not None
    m.use_packed_weights(True)
    with torch.no_grad():
        mlp.down_proj.weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(torch.zeros(1, 1, 96, dtype=BF), mlp.down_proj.weight, w8=mlp._w8_down)


def test_mxfp4_on_an_e4m3_rounded_model_rerounds_and_a_bad_k_raises_before_anything_is_written():
    from infinitevl_amd import ops
    m = _stack().quantize_weights_()
    assert m._w8_fmt == "e4m3"
    w8_ = m.layers[0].mlp.down_proj.weight.clone()
    m.quantize_weights_(fmt="mxfp4")
    codes, e8m0, _ = ops.quantize_rows_mxfp4(w8_)
    assert torch.equal(m.layers[0].mlp.down_proj.weight, ops.dequantize_rows_mxfp4(codes, e8m0)), "W'(e4m3) re-rounded to 4 bits"
    assert m.layers[0].mlp._w8_down.fmt == "mxfp4" and m._w8_lm_head is None
    bad = _stack(intermediate=80)                          # down_proj K = 80
    before = {k: v.clone() for k, v in bad.state_dict().items()}
    with pytest.raises(ValueError, match="multiple of 32"):
        bad.quantize_weights_(fmt="mxfp4")
    assert all(torch.equal(v, bad.state_dict()[k]) for k, v in before.items()) and bad.layers[0].self_attn._w8_o is None
    with pytest.raises(ValueError, match="fmt"):
        bad.quantize_weights_(fmt="fp4")
    bad.quantize_weights_()                                # e4m3 has no such rule

"""CPU: weight-only e4m3 for the decode step -- the quantiser, the judges of tests/w8.py, the C ABI's refusals and
quantize_weights_ on a small stack.

  * ops.quantize_rows_e4m3 against the independent restatement of tests/w8.py (equal codes and exponents) on gaussian rows, a zero
    row, a row scaled by 1e-3, rows whose amax is exactly 448 2^j and 224 2^j and the next bf16 above each; W' is bf16-exact,
    amax / scale lies in (224, 448], |w - W'| <= 2^-4 |w| from scale 2^-6 up and <= scale 2^-10 below, re-quantising W' with the
    SAME exponents reproduces the codes, no NaN code;
  * the judge bites: the honest fp32 emulation of the stated order passes the exact-integer probe with per-row scales, each of
    four wrong ones is reported;
  * the four entry points are declared and exported, and refuse what their bf16 twins refuse (+ a NULL scale) with the right code
    on a machine without a GPU, i.e. before anything is launched;
  * InfiniteVLTextStack.quantize_weights_: the weights become W', the fused views keep their storage, lm_head=False leaves the
    embedding alone, a PackedWeight goes stale when its weight is written.
"""
import ctypes
import os
import subprocess

import pytest
import torch

import projections as pj
import rowwise as rw
import w8
from conftest import ROOT

BF = torch.bfloat16


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------
def _quantiser_inputs():
    g_ = rw.gen(5)
    K = 72
    rows = [torch.randn(6, K, generator=g_) * 0.02, torch.zeros(1, K), torch.randn(1, K, generator=g_) * 0.02 * 1e-3,
            torch.randn(2, K, generator=g_) * 30.0]
    w = torch.cat(rows).to(BF)
    edge = []
    for j in (-20, -9, -1, 0, 3, 11):
        for top in (448.0, 224.0):
            t = torch.tensor([top * 2.0 ** j], dtype=torch.float64)
            assert float(rw.round_bf16(t)) == float(t)
            for amax in (t, rw.next_bf16(t)):
                r = (torch.randn(K, generator=g_) * float(amax) * 0.3).clamp(-float(amax), float(amax)).to(BF)
                r[int(torch.randint(0, K, (1,), generator=g_))] = float(amax) * (1 if j % 2 else -1)
                edge.append(r)
    return torch.cat([w, torch.stack(edge)])


def test_quantiser_equals_the_restatement_and_keeps_its_promises():
    from infinitevl_amd import ops
    w = _quantiser_inputs()
    codes, exp, scale = ops.quantize_rows_e4m3(w)
    rc, re_, rs = w8.quantize_ref(w)
    assert codes.dtype == torch.uint8 and exp.dtype == torch.int32 and scale.dtype == torch.float32
    assert torch.equal(exp, re_), (exp - re_).nonzero()
    assert torch.equal(scale, rs) and torch.equal(codes, rc), (codes != rc).nonzero()[:5]
    assert int(exp[6]) == 0 and bool((codes[6] == 0).all()), "the zero row"
    assert not bool(((codes & 0x7F) == 0x7F).any()), "no NaN code"
    amax = w.double().abs().amax(1)
    ratio = amax / scale.double()
    nz = amax > 0
    assert bool(((ratio > 224.0) & (ratio <= 448.0))[nz].all()), ratio
    assert {float(r) for r in ratio[10:]} >= {448.0}, "the edge rows sit on the upper end"
    wd = w8.dequantize_ref(codes, exp)
    assert torch.equal(rw.round_bf16(wd), wd), "W' is bf16-exact"
    wq = ops.dequantize_rows_e4m3(codes, scale)
    assert wq.dtype == BF and torch.equal(wq.double(), wd)
    err, a, s = (w.double() - wd).abs(), w.double().abs(), scale.double()[:, None]
    big = a >= s * 2.0 ** -6
    assert bool((err <= a * 2.0 ** -4)[big].all()) and bool((err <= s * 2.0 ** -10)[~big].all())
    # W' again, with the SAME exponents: the codes come back (the exponents need not: an amax that rounds down to 224 2^e)
    again = (wq.float() / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(again, codes) and torch.equal(w8.encode_e4m3fn(wd / s), codes)
    codes2, _, _ = ops.quantize_rows_e4m3(wq)
    assert not bool(((codes2 & 0x7F) == 0x7F).any())


def test_quantiser_refusals_and_the_torch_cast_it_relies_on():
    from infinitevl_amd import ops
    assert torch.tensor([449.0, 464.0, 447.9]).to(torch.float8_e4m3fn).float().tolist() == [448.0, 448.0, 448.0]
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_rows_e4m3(torch.tensor([[1.0, float("inf")]]).to(BF))
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_rows_e4m3(torch.tensor([[1.0, float("nan")]]).to(BF))
    with pytest.raises(ValueError, match="100"):
        ops.quantize_rows_e4m3(torch.full((1, 8), 2.0 ** 120).to(BF))
    with pytest.raises(ValueError, match="100"):
        ops.quantize_rows_e4m3(torch.full((1, 8), 2.0 ** -120).to(BF))
    with pytest.raises(ValueError, match="bf16"):
        ops.quantize_rows_e4m3(torch.zeros(2, 8))
    c = torch.arange(256, dtype=torch.uint8)
    ok = (c & 0x7F) != 0x7F
    assert torch.equal(w8.decode_e4m3fn(c)[ok], c.view(torch.float8_e4m3fn).double()[ok]), "the table is torch's e4m3fn"
    assert torch.equal(w8.encode_e4m3fn(w8.decode_e4m3fn(c[ok])), c[ok])
    assert float(w8.decode_e4m3fn(torch.tensor([0x38], dtype=torch.uint8))) == 1.0
    assert float(w8.decode_e4m3fnuz(torch.tensor([0x38], dtype=torch.uint8))) == 0.5


# ---- the judge -----------------------------------------------------------------------------------------------------------------------
def _modest(glu, N, K):
    return (2 * N if glu else N) * K <= 2.5e6 and (N < 100 or K <= 520)


def _cases():
    for glu, norm, N, K, Ms, variant in pj.SMALL_M:
        if _modest(glu, N, K) and K in (8, 136, 512, 520, 2056, 4096, 4104):
            yield glu, norm, N, K, Ms, variant


def _check(glu, norm, N, K, Ms, variant, wrong=""):
    if norm:
        c = pj.norm_case(N, K, glu, Ms)
        run = lambda *a: w8.emu_w8_norm_linear(*a, wrong=wrong)      # noqa: E731
        return w8.check_norm_linear(run, c, Ms, w8.probe_exponents(c, Ms))
    c = pj.int_case(4, N, K, glu, variant, Ms)
    run = lambda *a: w8.emu_w8_linear(*a, wrong=wrong)               # noqa: E731
    return w8.check_linear(run, c, Ms, w8.probe_exponents(c, Ms))


def test_honest_emulation_of_the_stated_order_passes_the_scaled_probe():
    probed, n = 0, 0
    for case in _cases():
        rep = _check(*case)
        assert rep.ok(), str(rep)
        probed, n = probed + rep.probed, n + 1
    assert n >= 20 and {c[5] for c in _cases()} == {"index", "ties"} and {c[1] for c in _cases()} == {False, True}
    print(f"{n} cases, {probed} elements bit for bit")
    e = w8.probe_exponents(pj.int_case(4, 7, 520, False, "index"), (1, 2, 3, 4))
    assert int(e.min()) >= -3 and int(e.max()) <= 3 and len(e.unique()) > 1


def test_emulated_chain_equals_the_exact_sum_on_integers_and_scales_commute():
    """integer inputs: the chain is exact; gaussian inputs: scaling every weight row by a power of two scales the chain's
    result by it, bit for bit (the reason the w8 kernels can equal the bf16 kernels on W')"""
    c = pj.int_case(4, 7, 520, False, "index")
    assert torch.equal(w8.emu_chain(c["x"], c["w"].float()).double(), c["S"])
    g_ = rw.gen(9)
    x = torch.randn(2, 520, generator=g_).to(BF)
    w = (torch.randn(6, 520, generator=g_) * 0.02).to(BF)
    codes, exp, scale = w8.quantize_ref(w)
    a = w8.emu_chain(x, w8.decode_e4m3fn(codes).float())
    b = w8.emu_chain(x, w8.dequantize_ref(codes, exp).float())
    assert torch.equal(a * scale[None, :], b)


@pytest.mark.parametrize("wrong", w8.WRONG)
def test_wrong_emulation_is_reported(wrong):
    hits = [c for c in _cases() if c[3] <= 520 and not _check(*c, wrong=wrong).ok()]
    print(f"{wrong}: reported in {len(hits)} cases, e.g. {hits[:3]}")
    assert hits, wrong
    assert any(c[1] for c in hits) and any(not c[1] for c in hits), "in a plain / GLU case and in a NORM case"


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NAMES = ("ivl_linear_small_m_w8_fwd", "ivl_linear_swiglu_small_m_w8_fwd", "ivl_norm_linear_small_m_w8_fwd",
         "ivl_gdn_out_linear_small_m_w8_fwd")


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
        twin = _lib.PROTOTYPES[name.replace("_w8", "")][1]
        assert len(_lib.PROTOTYPES[name][1]) == len(twin) + 1, "the twin's argument list + scale"
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12


def test_refusals_come_before_any_launch(lib):
    """never-dereferenced pointers on a machine that may have no GPU: every refusal is decided on the host"""
    from infinitevl_amd import _lib
    p = ctypes.c_void_p(0x1000)
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    lin, glu, nrm, gdn = (getattr(lib, n) for n in NAMES)
    for fn in (lin, glu):
        assert fn(p, p, p, None, p, 5, 16, 64, None) == UNS and fn(p, p, p, None, p, 0, 16, 64, None) == UNS          # M
        assert fn(p, p, p, None, p, 1, 16, 60, None) == INV and fn(p, p, p, None, p, 1, 0, 64, None) == INV           # K % 8, N
        assert fn(p, p, None, None, p, 1, 16, 64, None) == INV and b"NULL" in lib.ivl_last_error()                    # scale
        assert fn(p, None, p, None, p, 1, 16, 64, None) == INV and fn(None, p, p, None, p, 1, 16, 64, None) == INV
        assert fn(p, p, p, None, None, 1, 16, 64, None) == INV
    n_ok = (p, None, p, 1e-6, None, p, p, None, p)
    assert nrm(*n_ok, 5, 16, 512, 0, None) == UNS and nrm(*n_ok, 1, 16, 516, 0, None) == INV
    for K in (8, 256, 504, 4104, 8192):
        assert nrm(*n_ok, 1, 16, K, 0, None) == UNS, K
        assert b"512 <= K <= 4096" in lib.ivl_last_error()
    assert nrm(p, None, None, 1e-6, None, p, p, None, p, 1, 16, 512, 1, None) == INV                                   # norm weight
    assert nrm(p, p, p, 1e-6, None, p, p, None, p, 1, 16, 512, 1, None) == INV                                         # residual, no h_out
    assert nrm(p, None, p, 1e-6, None, p, None, None, p, 1, 16, 512, 0, None) == INV                                   # scale
    assert nrm(p, None, p, 1e-6, None, None, p, None, p, 1, 16, 512, 0, None) == INV                                   # wq

    def g(H, M=1, K=None, wq=p, scale=p, gate_ld=512):
        return gdn(p, p, gate_ld, p, 1e-5, H, p, 512, 0, 128, p, p, wq, scale, None, p, M, 8, H * 256 if K is None else K, None)
    for H in (0, 1, 17):
        assert g(H) == UNS and b"2 <= H <= 16" in lib.ivl_last_error()
    assert g(2, M=5) == UNS and g(2, M=0) == UNS and g(2, K=520) == UNS
    assert g(2, scale=None) == INV and g(2, wq=None) == INV and g(2, gate_ld=514) == INV


# ---- quantize_weights_ on a small stack -----------------------------------------------------------------------------------------------
def _stack():
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
                               num_attention_heads=4, num_key_value_heads=2, head_dim=16, sliding_window=8,
                               layer_types=["sliding_attention", "linear_attention"], num_linear_heads=4,
                               num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


def test_quantize_weights_rounds_in_place_and_keeps_the_fused_views():
    from infinitevl_amd import ops
    m = _stack()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(RuntimeError, match="quantize_weights_"):
        m.use_packed_weights(True)
    assert m.quantize_weights_() is m and m._w8_on and m._w8_lm_head is None
    after = m.state_dict()
    proj = [k for k in before if k.endswith("_proj.weight")]
    assert len(proj) == 4 + 7 + 2 * 3
    for k, v in before.items():
        if k in proj:
            codes, _, scale = ops.quantize_rows_e4m3(v)
            assert torch.equal(after[k], ops.dequantize_rows_e4m3(codes, scale)), k
            assert not torch.equal(after[k], v), k
        else:
            assert torch.equal(after[k].view(torch.uint8), v.view(torch.uint8)), k       # biases, norms, convs, gates, the embedding
    att, gdn, mlp = m.layers[0].self_attn, m.layers[1].self_attn, m.layers[0].mlp
    for mod, names in ((att, ("q_proj", "k_proj", "v_proj")), (gdn, ("q_proj", "k_proj", "v_proj", "g_proj", "a_proj", "b_proj")),
                       (mlp, ("gate_proj", "up_proj"))):
        r = 0
        for n in names:
            wt = getattr(mod, n).weight
            assert wt.untyped_storage().data_ptr() == mod._fused_w.untyped_storage().data_ptr(), n
            assert wt.data_ptr() == mod._fused_w[r:].data_ptr() and torch.equal(wt, mod._fused_w[r:r + wt.shape[0]]), n
            r += wt.shape[0]
    for pw, wt in ((att._w8_qkv, att._fused_w), (att._w8_o, att.o_proj.weight), (gdn._w8_in, gdn._fused_w),
                   (gdn._w8_o, gdn.o_proj.weight), (mlp._w8_gu, mlp._fused_w), (mlp._w8_down, mlp.down_proj.weight)):
        assert isinstance(pw, ops.PackedWeight) and pw.check(wt) is pw
        assert pw.codes.dtype == torch.uint8 and tuple(pw.codes.shape) == tuple(wt.shape) and pw.scale.dtype == torch.float32
        assert torch.equal(ops.dequantize_rows_e4m3(pw.codes, pw.scale), wt), "the bf16 weight holds W'"
        m_, _ = torch.frexp(pw.scale)
        assert bool((m_ == 0.5).all()), "powers of two"
    # the rounded model is a fixed point of the grid: a second pass changes nothing but may pick other exponents
    again = {k: v.clone() for k, v in m.state_dict().items()}
    m.quantize_weights_()
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in again.items())
    m.use_packed_weights(False)
    assert not m._w8_on and not att._w8_on and not mlp._w8_on and att._w8_o is not None
    m.use_packed_weights(True)
    assert gdn._w8_on


def test_lm_head_is_rounded_only_on_request():
    from infinitevl_amd import ops
    m = _stack()
    emb = m.embed_tokens.weight.detach().clone()
    m.quantize_weights_()
    assert torch.equal(m.embed_tokens.weight.view(torch.uint8), emb.view(torch.uint8)) and m._w8_lm_head is None
    m.quantize_weights_(lm_head=True)
    codes, _, scale = ops.quantize_rows_e4m3(emb)
    assert torch.equal(m.embed_tokens.weight, ops.dequantize_rows_e4m3(codes, scale)) and not torch.equal(m.embed_tokens.weight, emb)
    assert m._w8_lm_head.check(m.embed_tokens.weight) is m._w8_lm_head


def test_packed_weight_goes_stale_when_its_weight_is_written():
    from infinitevl_amd import ops
    m = _stack().quantize_weights_()
    mlp, att = m.layers[0].mlp, m.layers[0].self_attn
    x = torch.zeros(1, 1, 96, dtype=BF)
    ops.linear(x, mlp.down_proj.weight, w8=mlp._w8_down)                # fresh: the CPU call takes the library path on W'
    with torch.no_grad():
        mlp.down_proj.weight.mul_(2.0)
    assert mlp._w8_down.stale(mlp.down_proj.weight)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear(x, mlp.down_proj.weight, w8=mlp._w8_down)
    # load_state_dict writes through the parameters, which are views of the fused weights
    assert not att._w8_qkv.stale(att._fused_w) and not mlp._w8_gu.stale(mlp._fused_w)
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    for pw, wt in ((att._w8_qkv, att._fused_w), (mlp._w8_gu, mlp._fused_w), (att._w8_o, att.o_proj.weight)):
        with pytest.raises(RuntimeError, match="stale"):
            pw.check(wt)
    with pytest.raises(RuntimeError, match="stale"):
        ops.linear_swiglu(torch.zeros(1, 1, 64, dtype=BF), mlp._fused_w, w8=mlp._w8_gu)
    other = torch.zeros_like(att.o_proj.weight)
    m.quantize_weights_()
    assert att._w8_o.check(att.o_proj.weight) is att._w8_o and att._w8_o.stale(other), "another tensor: another pointer"

"""GPU (-m gpu): every copy of the rotary formula against an anchor OUTSIDE the library (tests/rotary.py holds builders, references
and judges; tests/test_rotary_cpu.py shows that the judges pass the honest emulations, report every wrong one and that the site list
below reaches every launch form).

  ivl_rope_tables_fwd       per element bit-equal to bf16(cos_float64(fp32(fp32(pos) * inv_freq)) * scaling), either neighbour only
                            within relative D_TRIG = 2^-22 (+ 2^-23 with a scaling) of a bf16 rounding boundary (derived: 2 ulp for
                            cosf / sinf, doubled); positions up to 10^15 + 1, around 2^24 and 2^31, a call beyond the 1024-block cap;
                            InfiniteVLRotaryEmbedding.forward returns the same bits.
  ivl_mrope_fwd / _strided  torch.equal to oracle.swa.apply_mrope on the CPU (bf16 eager chain), adversarial (randn) and real tables,
                            six shapes up to the grid-stride loop; the strided form leaves every column outside q | k untouched.
                            A failure is followed by the read map (which table entry the kernel read, by integer-coded tables).
  every fused SWA site      ops.swa_forward / swa_forward_rows / swa_cache_append with rope=(cos, sin, sections) on un-rotated q / k
                            == the same call with rope=None on q / k rotated on the CPU: o and both rings, torch.equal.
  vision rotation           ops.vision_window_attention(rope=) == the plain call on q, k rotated on the CPU by the fp32 chain, at
                            d = 64 / 80 / 128, in the key loads, the pre-pass, without a workspace and in the 128-row form; randn,
                            real and cancelling tables (the last make a contracted multiply-add visible in bf16: "cancel" in the
                            rotation of q, "cancel_k" in that of k).

pytest -s prints the window share and what the tables imply of the device's cosf / sinf for every call."""
import types

import numpy as np
import pytest
import torch

import rotary as ro
import rowwise as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SEC_IDS = lambda s: "-".join(map(str, s))      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


# ---- 1. tables -----------------------------------------------------------------------------------------------------------------------
def run_tables(pos, inv, scaling):
    from infinitevl_amd import ops
    cos, sin = ops.rope_tables(pos.to(DEV), inv.to(DEV), scaling)
    torch.cuda.synchronize()
    return cos.cpu(), sin.cpu()


def _device_libm_ulps(pos, inv):
    """measured, not asserted: torch's own fp32 cos / sin on the device (the same libm) on the same angles, from float64, in fp32 ulps"""
    f = torch.from_numpy(ro.table_angles(pos, inv))
    worst = 0.0
    for fn in (torch.cos, torch.sin):
        ref = torch.from_numpy(getattr(np, fn.__name__)(f.numpy()))
        got = fn(f.float().to(DEV)).cpu().double()
        _, e = torch.frexp(ref.abs())
        worst = max(worst, float(((got - ref).abs() / torch.pow(2.0, e.double() - 24))[ref != 0].max()))
    return worst


def _tables_pass(half_dim, theta, scaling, pos=None):
    rep = ro.check_tables(run_tables, half_dim, theta, scaling, pos)
    print(rep)
    print(f"   elements that took the other neighbour imply a device cosf / sinf at least {rep.ulps:.3f} fp32 ulps from float64; "
          f"torch's device cos / sin on the same angles: at most {_device_libm_ulps(ro.table_positions() if pos is None else pos, ro.inv_freq(half_dim, theta)):.3f}")
    assert rep.ok(), str(rep)
    assert max(rep.shares) < rw.EXCUSED_MAX, rep.shares


@pytest.mark.parametrize("scaling", ro.SCALINGS)
@pytest.mark.parametrize("half_dim,theta", ro.TABLE_CASES)
def test_rope_tables_against_float64(half_dim, theta, scaling):
    _tables_pass(half_dim, theta, scaling)


def test_rope_tables_beyond_the_block_cap():
    pos = ro.table_positions(ro.WRAP_T)
    assert pos.numel() * 64 > 1024 * 256
    _tables_pass(64, 1e6, 1.0, pos)


@pytest.mark.parametrize("scaling", ro.SCALINGS)
@pytest.mark.parametrize("half_dim,theta", ro.TABLE_CASES)
def test_rotary_module_returns_the_kernel_tables(half_dim, theta, scaling):
    from infinitevl_amd.harness import InfiniteVLTextConfig
    from infinitevl_amd.modules import InfiniteVLRotaryEmbedding
    cfg = InfiniteVLTextConfig() if half_dim == 64 else types.SimpleNamespace(head_dim=2 * half_dim, rope_theta=theta)
    rot = InfiniteVLRotaryEmbedding(cfg)
    assert torch.equal(rot.inv_freq.cpu(), ro.inv_freq(half_dim, theta))
    rot.attention_scaling = scaling
    pos = ro.table_positions()
    cos, sin = rot(torch.zeros(1, dtype=BF, device=DEV), pos.to(DEV))
    ref = run_tables(pos, ro.inv_freq(half_dim, theta), scaling)
    assert torch.equal(cos.cpu(), ref[0]) and torch.equal(sin.cpu(), ref[1])


# ---- 2. M-RoPE -----------------------------------------------------------------------------------------------------------------------
def run_mrope(q, k, cos, sin, sections):
    from infinitevl_amd import ops
    qd, kd = q.to(DEV), k.to(DEV)
    ops.apply_mrope_inplace(qd, kd, cos.to(DEV), sin.to(DEV), sections)
    torch.cuda.synchronize()
    return qd.cpu(), kd.cpu()


def run_mrope_strided(q, k, cos, sin, sections, case=None):
    """through views of one [B * T, ld] buffer (rotary.strided_case's layout) -> (q, k, the whole buffer)"""
    from infinitevl_amd import ops
    B, T, Hq, d = q.shape
    c = dict(case) if case is not None else ro.strided_case((B, T, Hq, k.shape[2], d, tuple(sections)))
    buf = c["buf"].clone()
    vq, vk = ro.strided_views(c, buf)
    vq.copy_(q)
    vk.copy_(k)
    buf = buf.to(DEV)
    vq, vk = ro.strided_views(c, buf)
    assert B * T == 1 or not vq.is_contiguous()
    ops.apply_mrope_strided_inplace(vq, vk, cos.to(DEV), sin.to(DEV), sections)
    torch.cuda.synchronize()
    return vq.cpu().contiguous(), vk.cpu().contiguous(), buf.cpu()


@pytest.mark.parametrize("kind", ro.TABLE_KINDS)
@pytest.mark.parametrize("shape", ro.MROPE_SHAPES, ids=ro.shape_id)
def test_mrope_against_the_eager_arithmetic(shape, kind):
    c = ro.mrope_case(shape, kind, run_tables)
    eq, ek = ro.mrope_expected(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    gq, gk = run_mrope(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    msg = [f"{n}: {m}" for n, m in (("q", ro.rotation_mismatches(gq, eq)), ("k", ro.rotation_mismatches(gk, ek))) if m]
    if msg:
        msg.append(ro.read_map_report(run_mrope, *shape))
    assert not msg, "\n".join(msg)


@pytest.mark.parametrize("kind", ro.TABLE_KINDS)
@pytest.mark.parametrize("shape", ro.STRIDED_SHAPES, ids=ro.shape_id)
def test_mrope_strided_against_the_eager_arithmetic_and_writes_nothing_else(shape, kind):
    c = ro.strided_case(shape, kind, run_tables)
    _, _, after = run_mrope_strided(c["q"], c["k"], c["cos"], c["sin"], c["sections"], case=c)
    msg = ro.strided_report(c, after)
    if msg:
        msg += "\n" + ro.read_map_report(lambda *a: run_mrope_strided(*a)[:2], *shape)
    assert not msg, msg


@pytest.mark.parametrize("shape", [s for s in ro.MROPE_SHAPES if s[1] <= 16], ids=ro.shape_id)
def test_mrope_read_map(shape):
    assert ro.read_map_report(run_mrope, *shape) == ""
    if all(v % 8 == 0 for v in shape[5]):
        assert ro.read_map_report(lambda *a: run_mrope_strided(*a)[:2], *shape) == ""


# ---- 3. every fused site against the CPU rotation ---------------------------------------------------------------------------------------
def _site_call(s, c, with_rope):
    """one call of the site: rope=(cos, sin, sections) on the un-rotated q / k, or rope=None on the CPU-rotated ones"""
    from infinitevl_amd import ops
    dev = lambda t: t.to(DEV)      # noqa: E731
    q, k = (c["q"], c["k"]) if with_rope else (c["q_rot"], c["k_rot"])
    q, k, v, kc, vc = dev(q), dev(k), dev(c["v"]), dev(c["kc"]), dev(c["vc"])          # (the rings are fresh copies: the call appends)
    rope = (dev(c["cos"]), dev(c["sin"]), list(c["sections"])) if with_rope else None
    kw = dict(window=s.W, scaling=128 ** -0.5, k_cache=kc, v_cache=vc, rope=rope)
    o = None
    if s.entry in ("fwd", "append"):
        pos_dev = torch.tensor([s.seens[0]], dtype=torch.int64, device=DEV)
        if s.entry == "append":
            ops.swa_cache_append(k, v, kc, vc, pos_dev=pos_dev, rope=rope)
        else:
            before = ops.SWA_RING256_CALLS
            o = ops.swa_forward(q, k, v, pos_dev=pos_dev, append=True, pos_min=s.seens[0] if s.kernel == "ring256" else 0, **kw)
            assert ops.SWA_RING256_CALLS - before == (s.kernel == "ring256"), s.name
    else:
        pos_rows = torch.tensor(s.seens, dtype=torch.int64, device=DEV)
        mask = torch.tensor(s.mask, dtype=torch.int32, device=DEV) if s.mask else None
        if s.entry == "decode_rows":
            o = ops.swa_forward(q, k, v, pos_rows=pos_rows, append=True, **kw)
        elif s.entry == "hold":
            o = ops.swa_forward(q, k, v, pos_rows=pos_rows, frozen=mask, append=True, **kw)
        else:
            o = ops.swa_forward_rows(q, k, v, pos_rows=pos_rows, append=True, n_rows=mask if s.entry == "rows_n" else None, **kw)
    torch.cuda.synchronize()
    return dict(o=None if o is None else o.cpu(), kc=kc.cpu(), vc=vc.cpu())


@pytest.mark.parametrize("sections", ro.SITE_SECTIONS, ids=SEC_IDS)
@pytest.mark.parametrize("name", sorted(ro.SITES))
def test_fused_site_equals_the_cpu_rotation(name, sections):
    s = ro.SITES[name]
    c = ro.site_inputs(name, sections)
    fused, plain = _site_call(s, c, True), _site_call(s, c, False)
    assert not torch.equal(plain["kc"], c["kc"]), "the call appended nothing"
    if fused["o"] is not None:
        live = [b for b in range(s.B) if not (s.entry == "hold" and s.mask[b]) and not (s.entry == "rows_n" and s.mask[b] == 0)]
        assert all(bool(torch.isfinite(plain["o"][b, :min(s.mask[b], s.T) if s.entry == "rows_n" else s.T].float()).all()) for b in live)
    msg = ro.site_report(s, fused, plain)
    assert not msg, f"{name} sections {sections}: rope= on un-rotated inputs differs from the same call on CPU-rotated inputs\n{msg}"


# ---- 4. the vision rotation -----------------------------------------------------------------------------------------------------------
def _vision_call(x, cu, max_len, rope, workspace=True):
    """x [S, 3, H, d] on the device; workspace=False: the library binding with a NULL workspace (the rotation stays in the tile loads)"""
    from infinitevl_amd import _lib, ops
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    assert not q.is_contiguous()
    if workspace:
        return ops.vision_window_attention(q, k, v, cu, max_len, rope=rope)
    S, H, d = q.shape
    o = torch.zeros(S, H, d, dtype=BF, device=x.device)
    cos, sin = rope
    _lib.check(_lib.load().ivl_vision_attn_fwd(
        ops._p(q), ops._p(k), ops._p(v), ops._p(o), q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
        o.stride(0), o.stride(1), ops._p(cu), cu.numel() - 1, int(max_len), S, H, d, float(d ** -0.5), ops._p(cos), ops._p(sin), None, 0,
        ops._stream(q)))
    return o


@pytest.mark.parametrize("tables", ro.VISION_TABLES)
@pytest.mark.parametrize("form", ro.VISION_FORMS)
@pytest.mark.parametrize("H", ro.VISION_H)
@pytest.mark.parametrize("d", ro.VISION_D)
def test_vision_rotation_equals_the_cpu_arithmetic(d, H, form, tables):
    c = ro.vision_case(d, H, form, tables)
    cu = c["cu"].to(DEV)
    rope = (c["cos"].to(DEV), c["sin"].to(DEV))
    got = _vision_call(c["qkv"].to(DEV), cu, c["max_seqlen"], rope, workspace=form != "prepass_null_ws")
    exp = _vision_call(ro.vision_rotated(c).to(DEV), cu, c["max_seqlen"], None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(exp.float()).all()) and bool((exp != 0).any())
    msg = ro.vision_report(got.cpu(), exp.cpu())
    assert not msg, f"d={d} H={H} {form} {tables} tables, segments {c['lens'][:8]}...: rope= differs from the plain call on CPU-rotated q, k: {msg}"

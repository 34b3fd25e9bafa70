"""GPU (-m gpu): the fused and the single-purpose forms of the row-wise formulas agree BIT FOR BIT where no other test says so
directly.  Each pair below evaluates one helper of infinitevl_amd/csrc/ivl_rowwise.h from two kernels with different load
schedules and element layouts; test_gpu_rowwise.py anchors each kernel to float64, this file pins them to each other:

  conv      ops.ShortConvolution (8 tokens per thread) on the q, k, v column blocks  ==  ops.gdn_prologue (4 tokens per thread,
            clamped loads) -- outputs and the three new conv states; T = 1 (the state shift alone), 5 (crosses the prologue's
            chunk, not the stand-alone kernel's), 11 (crosses both); no carried state / a separate state out / in place
  gates     ops.gdn_gate  ==  the prologue's g and beta, with a + dt_bias on both sides of softplus' threshold 20 and b at +-88
  norm      ops.FusedRMSNormGated on a contiguous gate  ==  ops.rmsnorm_swish_gate_strided reading it from a padded buffer;
            15 rows (not a multiple of the 8 a workgroup takes), gates of +-88, an all-zero x row and an all-zero gate row

Equalities of bit patterns: no tolerance.  Inputs are the edge-value builders of tests/rowwise.py.
"""
import pytest
import torch

import rowwise as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def _same_bits(tag, got, want):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (tag, got.dtype, want.dtype, got.shape, want.shape)
    iv = torch.int16 if got.dtype == BF else torch.int32
    a, b = got.contiguous().cpu().view(iv), want.contiguous().cpu().view(iv)
    bad = (a != b).nonzero()
    assert bad.shape[0] == 0, (tag, f"{bad.shape[0]} of {a.numel()} elements differ; first (index, got, want): "
                               f"{[(tuple(i.tolist()), float(got.cpu()[tuple(i)]), float(want.cpu()[tuple(i)])) for i in bad[:5]]}")


def _prologue(c, si, so):
    from infinitevl_amd import ops
    return ops.gdn_prologue(c["proj"].to(DEV), c["cols"], [w.to(DEV) for w in c["w"]], si, so,
                            c["A_log"].to(DEV), c["dt_bias"].to(DEV), c["H"], *c["D"])


@pytest.mark.parametrize("state", ["none", "separate", "aliased"])
@pytest.mark.parametrize("T", [1, 5, 11])
def test_short_conv_equals_the_prologue_conv(T, state):
    """B = 2, H = 1 (Dq = Dk = 128, Dv = 256), `ld` padded past the last column."""
    from infinitevl_amd import ops
    B = 2
    c = rw.prologue_case(B, T, 1)
    assert c["ld"] > c["cols"][4] + 1 and c["D"] == (128, 128, 256)
    if state == "none":
        si = [None, None, None]
        so = [torch.full((B, D, 4), float("nan"), dtype=BF, device=DEV) for D in c["D"]]
    else:
        si = [s.to(DEV) for s in c["state"]]
        so = si if state == "aliased" else [torch.full_like(s, float("nan")) for s in si]
    q, k, v, _, _ = _prologue(c, si, so)
    for i, (x, D) in enumerate(zip(rw.prologue_slices(c), c["D"])):
        conv = ops.ShortConvolution(D, 4, bias=False, activation="silu", device=DEV, dtype=BF)
        conv.weight.data.copy_(c["w"][i])
        xd = x.contiguous().to(DEV)
        if state == "none":
            y, new = conv(xd, output_final_state=True)
        elif state == "aliased":
            st = c["state"][i].to(DEV)
            y, new = conv(xd, cache=st)
            assert new is st
        else:
            st = c["state"][i].to(DEV)
            y, new = torch.empty_like(xd), torch.full((B, D, 4), float("nan"), dtype=BF, device=DEV)
            conv._launch(xd, y, st, new, B, T, D, 4)
        _same_bits(("qkv"[i], "y"), (q, k, v)[i], y)
        _same_bits(("qkv"[i], "state"), so[i], new)


def test_gdn_gate_equals_the_prologue_gates():
    from infinitevl_amd import ops
    B, T, H = 2, 11, 4
    c = rw.prologue_case(B, T, H)
    ca, cb = c["cols"][3], c["cols"][4]
    n = torch.arange(B * T * H).view(B, T, H)
    c["proj"][..., ca:ca + H] = (17.0 + 0.25 * (n % 25)).to(BF)                       # 17 .. 23 in steps of 1/4, |dt_bias| < 3
    c["proj"][..., cb:cb + H] = torch.tensor(rw.SWEEP)[n % len(rw.SWEEP)].to(BF)
    a, b = c["proj"][..., ca:ca + H], c["proj"][..., cb:cb + H]
    av = a.float() + c["dt_bias"].float()
    assert bool((av > 20.0).any()) and bool((av <= 20.0).any()) and bool((b == 88.0).any()) and bool((b == -88.0).any())
    _, _, _, g, beta = _prologue(c, [None] * 3, [None] * 3)
    g1, beta1 = ops.gdn_gate(a.contiguous().to(DEV), b.contiguous().to(DEV), c["A_log"].to(DEV), c["dt_bias"].to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g1).all())
    _same_bits("g", g, g1)
    _same_bits("beta", beta, beta1)


def test_gated_norm_equals_the_strided_form():
    """B = 1, T = 5, H = 3: 15 rows."""
    from infinitevl_amd import ops
    c = rw.strided_case(3, 5)
    off, H = c["off"], c["H"]
    buf = c["buf"].clone()
    buf[2, off + 256:off + 512] = 0.0                                               # an all-zero gate row (token 2, head 1)
    gate = buf[:, off:off + H * 256].reshape(-1, 256)
    x = c["x"].view(-1, 256)
    assert x.shape[0] == 15 and bool((x == 0).all(-1).any()) and bool((x != 0).any(-1).sum() >= 10)
    assert bool((gate == 88.0).any()) and bool((gate == -88.0).any()) and bool((gate == 0).all(-1).any())
    bd = buf.to(DEV)
    y_strided = ops.rmsnorm_swish_gate_strided(c["x"].to(DEV), bd[:, off:], c["ld"], c["w"].to(DEV), c["eps"])
    norm = ops.FusedRMSNormGated(256, eps=c["eps"], device=DEV, dtype=BF)
    norm.weight.data.copy_(c["w"])
    y = norm(x.to(DEV), gate.contiguous().to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.float()).all())
    _same_bits("y", y_strided.view(-1, 256), y)

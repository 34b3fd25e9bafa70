"""GPU (-m gpu): the 128-row form of the vision attention kernel (`vision_attn_kernel<D, 2>`: two 16-row query groups per
wave) at every head size.  The launcher takes it when n_seg * ceil(max_seqlen / 128) * H >= 512; the parity tests reach that
at d = 80, H = 16 only.  Each case here is the smallest call that gets it (exactly 512), over segment lengths on both sides
of the 64- and 128-row tile borders, checked (a) against the oracle and (b) bit for bit against the 64-row form
(`<D, 1>`): the same call on the first 8 segments alone stays below 512.  Every 16-row group walks the same key tiles in
both forms and a skipped rescale multiplies by exactly 1, so the rows are equal by construction."""
import numpy as np
import pytest
import torch

from conftest import rms_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = [65, 128, 200, 1, 130, 64, 129, 100]           # 817 patches
MAX_SEQLEN = 200


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()          # fails loudly when the HIP extension is missing
    yield


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("d,H,repeats", [(128, 2, 16), (64, 4, 8), (80, 16, 2)])
def test_vision_attention_128_row_form(d, H, repeats, rope):
    from oracle import vision
    from infinitevl_amd import ops
    lens = PATTERN * repeats
    n_small, S = sum(PATTERN), sum(PATTERN) * repeats
    tiles128 = (MAX_SEQLEN + 127) // 128
    assert len(lens) * tiles128 * H == 512 and len(PATTERN) * tiles128 * H < 512       # the launcher's threshold, from both sides
    g_ = torch.Generator().manual_seed(1000 * d + H)
    qkv = torch.randn(S, 3, H, d, generator=g_).to(torch.bfloat16)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    qr, kr = qkv[:, 0], qkv[:, 1]
    tables = None
    if rope:
        cos, sin = vision.vision_rotary_tables(torch.randint(0, 32, (S, 2), generator=g_), d)
        qr, kr = vision.apply_rotary_pos_emb_vision(qr, kr, cos, sin)
        tables = (cos.to(DEV), sin.to(DEV))
    x = qkv.to(DEV)
    big = ops.vision_window_attention(x[:, 0], x[:, 1], x[:, 2], cu.to(DEV), MAX_SEQLEN, rope=tables)
    small = ops.vision_window_attention(x[:n_small, 0], x[:n_small, 1], x[:n_small, 2], cu[:len(PATTERN) + 1].to(DEV), MAX_SEQLEN,
                                        rope=None if tables is None else (tables[0][:n_small], tables[1][:n_small]))
    torch.cuda.synchronize()
    got = big.float().cpu()
    ref = vision.segment_attention(qr, kr, qkv[:, 2], cu.tolist(), p_round_dtype=torch.bfloat16)
    exact = vision.segment_attention(qr, kr, qkv[:, 2], cu.tolist())
    e_ref, e_exact = rms_rel(ref, got), rms_rel(exact, got)
    n_diff = int((big[:n_small] != small).sum())
    print(f"d={d} H={H} rope={rope}: rms_rel vs bf16-probability oracle {e_ref:.3e}, vs exact {e_exact:.3e}; "
          f"elements differing from the 64-row form: {n_diff}")
    assert torch.isfinite(got).all()
    assert e_ref < 3e-3 and e_exact < 5e-3, (d, H, rope, e_ref, e_exact)
    assert torch.equal(big[:n_small], small), (d, H, rope, n_diff)

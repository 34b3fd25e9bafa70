"""Helpers of the ragged frame-step tests (test_ragged_cpu.py, test_gpu_ragged.py): a token count per batch row in the GDN chunk
call (ivl_gdn_chunk_fused_rows_fwd, RAG-1..4) and in sliding-window attention (ivl_swa_rows_n_fwd, RAG-5..10)."""
import contextlib
import ctypes

import torch

FAKE = 4096          # a non-NULL address the argument checks never dereference
BF = torch.bfloat16
K, V = 128, 256
NAN = float("nan")


# ---------------------------------------------------------------------------------------------
# the C entry of the GDN call on fake pointers (CPU: every refusal comes back before anything is launched)
# ---------------------------------------------------------------------------------------------
def gdn_rows_call(lib, **kw):
    """ivl_gdn_chunk_fused_rows_fwd on fake pointers: B = 2, T = 130, H = 2, states in place, a large enough workspace; kw overrides."""
    from infinitevl_amd._lib import IVL_BF16
    H = kw.get("H", 2)
    a = dict(proj=FAKE, ld=2 * H * K + H * V + 2 * H + (-(2 * H) % 8), col_q=0, col_k=H * K, col_v=2 * H * K, col_a=2 * H * K + H * V,
             col_b=2 * H * K + H * V + H, wq=FAKE, wk=FAKE, wv=FAKE, sq_in=FAKE, sk_in=FAKE + 64, sv_in=FAKE + 128, sq_out=FAKE,
             sk_out=FAKE + 64, sv_out=FAKE + 128, A_log=FAKE, dt_bias=FAKE, o=FAKE, h0=FAKE + 256, h0_dtype=IVL_BF16, ht=FAKE + 256,
             ht_dtype=IVL_BF16, B=2, T=130, H=H, K=K, V=V, conv_width=4, scale=1.0, mma_dtype=IVL_BF16, workspace=FAKE,
             workspace_bytes=1 << 40, n_rows=FAKE, stream=None)
    a.update(kw)
    return lib.ivl_gdn_chunk_fused_rows_fwd(*[a[k] for k in (
        "proj", "ld", "col_q", "col_k", "col_v", "col_a", "col_b", "wq", "wk", "wv", "sq_in", "sk_in", "sv_in", "sq_out", "sk_out", "sv_out",
        "A_log", "dt_bias", "o", "h0", "h0_dtype", "ht", "ht_dtype", "B", "T", "H", "K", "V", "conv_width", "scale", "mma_dtype", "workspace",
        "workspace_bytes", "n_rows", "stream")])


def last_error(lib):
    return lib.ivl_last_error().decode()


# ---------------------------------------------------------------------------------------------
# GDN on the GPU
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def two_launch():
    """ops.gdn_chunk_fused without a sync area: the form RAG-1 names (ivl_gdn_chunk_fused_fwd with sync = NULL)"""
    from infinitevl_amd import ops
    ops._GDN_SINGLE_LAUNCH = False
    try:
        yield
    finally:
        ops._GDN_SINGLE_LAUNCH = True


def gdn_inputs(B, T, H, device, seed=0):
    """(proj [B,T,ld], cols, conv taps, conv states, A_log, dt_bias, h0 bf16 [B,H,K,V]) of a fused GDN call"""
    Dq, Dk, Dv = H * K, H * K, H * V
    g = torch.Generator().manual_seed(7000 + 100 * seed + 10 * B + T + H)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(BF).to(device)      # noqa: E731
    cols = (0, Dq, Dq + Dk, Dq + Dk + Dv, Dq + Dk + Dv + H)
    ld = (cols[4] + H + 7) // 8 * 8
    proj = rn(B, T, ld)
    cw = [rn(D_, 1, 4) * 0.5 for D_ in (Dq, Dk, Dv)]
    cs = [rn(B, D_, 4) for D_ in (Dq, Dk, Dv)]
    A32, dt32 = torch.randn(H, generator=g).to(device), torch.randn(H, generator=g).to(device)
    h0 = (torch.randn(B, H, K, V, generator=g) * 0.1).to(BF).to(device)
    return proj, cols, cw, cs, A32, dt32, h0


def gdn_unmasked(inp, H, n):
    """(o [B,n,H,V], conv states, state) of the unmasked two-launch call over the first n tokens of EVERY row, on cloned states"""
    from infinitevl_amd import ops
    proj, cols, cw, cs, A32, dt32, h0 = inp
    so, ht = [c.clone() for c in cs], h0.clone()
    with two_launch():
        o = ops.gdn_chunk_fused(proj[:, :n].contiguous(), cols, cw, so, so, A32, dt32, H, K, V, initial_state=ht, final_state_out=ht)
    return o, so, ht


def gdn_ragged(inp, H, lengths, poison=True):
    """(o, conv states, state, the states as they went in) of ONE ragged call.  poison: tokens t >= n_b of proj and every state of a row
    with n_b = 0 hold NaN."""
    from infinitevl_amd import ops
    proj, cols, cw, cs, A32, dt32, h0 = inp
    proj, so, ht = proj.clone(), [c.clone() for c in cs], h0.clone()
    if poison:
        for b, n in enumerate(lengths):
            proj[b, n:] = NAN
            if n == 0:
                ht[b] = NAN
                for s in so:
                    s[b] = NAN
    before = [s.clone() for s in so] + [ht.clone()]
    n_rows = torch.tensor(lengths, dtype=torch.int32, device=proj.device)
    o = ops.gdn_chunk_fused(proj, cols, cw, so, so, A32, dt32, H, K, V, initial_state=ht, final_state_out=ht, n_rows=n_rows)
    return o, so, ht, before


def words(t):
    """a tensor as raw integer words (NaN compares equal to itself)"""
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_rag1(inp, H, lengths, got, refs, tag=""):
    """RAG-1 / RAG-3 of one ragged result against the unmasked calls in refs = {n: gdn_unmasked(inp, H, n)}"""
    o, so, ht, before = got
    for b, n in enumerate(lengths):
        if n == 0:
            for i, (x, y) in enumerate(zip(so + [ht], before)):
                assert torch.equal(words(x[b]), words(y[b])), (tag, "n = 0: state", i, "of row", b, "changed")
            continue
        ro, rso, rht = refs[n]
        assert torch.isfinite(o[b, :n].float()).all(), (tag, b, n)
        assert torch.equal(words(o[b, :n]), words(ro[b])), (tag, "o", b, n)
        assert torch.equal(words(ht[b]), words(rht[b])), (tag, "recurrent state", b, n)
        for i, (x, y) in enumerate(zip(so, rso)):
            assert torch.equal(words(x[b]), words(y[b])), (tag, "conv state", i, b, n)

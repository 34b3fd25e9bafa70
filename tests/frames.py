"""Helpers of the frame-step tests (test_frames_cpu.py, test_gpu_frames.py): ivl_swa_rows_fwd / ops.swa_forward_rows,
GraphedMultiStreamStep and GraphedMultiStreamDecode.extend_frames."""
import torch

FAKE = 4096          # a non-NULL address the argument checks never dereference
ENTRY = "ivl_swa_rows_fwd"
BF = torch.bfloat16
HQ, HKV, D = 16, 2, 128
SECTIONS = (16, 24, 24)


def swa_args(**kw):
    """A valid ring call of ivl_swa_rows_fwd on fake pointers (B = 3, T = 1, window 96) with NO workspace; fields overridden by kw."""
    from infinitevl_amd._lib import IVL_BF16, SwaArgs
    a = SwaArgs()
    a.q = a.k_new = a.v_new = a.o = a.k_cache = a.v_cache = FAKE
    a.q_sb, a.q_st, a.q_sh = 16 * 128, 16 * 128, 128
    a.kn_sb, a.kn_st, a.kn_sh = 2 * 128, 2 * 128, 128
    a.B, a.T, a.T_new, a.Hq, a.Hkv, a.d = 3, 1, 1, 16, 2, 128
    a.cache_capacity, a.window = 95, 96
    a.scaling = 1.0
    a.mma_dtype = IVL_BF16
    a.append_new = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# name -> (T, C, positions): the shapes of the ROWS-1 test (Hq = 16, Hkv = 2, d = 128; B = len(positions)) and what each covers
CASES = {
    "a": (40, 95, [0, 40, 94, 95, 250, 302]),               # 64-row form, one split, stand-alone rows append, seam and wrap
    "b": (64, 4095, [0, 4090, 4095, 12302]),                # 64-row form, 8 splits
    "c": (256, 4095, [0, 3900, 4112]),                      # prefill form, 3 splits, bf16 partials, pre-pass with rope, crosses the fill point
    "d": (130, 95, [0, 1, 64, 94, 95, 96, 250, 302]),       # prefill, one split, tail tile, T > C (ROWS-4)
    "e": (256, 4095, [0, 517, 1911, 4094, 4095, 6000, 8191, 12285]),    # one split, rope in the kernel
}
# (launch form, KV splits) each case must take, by tests/adversarial.swa_dispatch
PLAN = {"a": ("64row", 1), "b": ("64row", 8), "c": ("prefill", 3), "d": ("prefill", 1), "e": ("prefill", 1)}


def rope_tables(pid):
    """cos / sin bf16 [3,B,T,128] of M-RoPE positions pid int64 [3,B,T] (on pid's device)"""
    from infinitevl_amd import ops
    inv_freq = 1.0 / (1e6 ** (torch.arange(0, 128, 2, device=pid.device, dtype=torch.float32) / 128))
    return ops.rope_tables(pid.contiguous(), inv_freq, 1.0)


def case_tensors(name, device, seed=0, nan_unread=False):
    """(q, k, v, k ring, v ring, pos_rows, rope) of a case.  nan_unread: ring slots at and above a row's position (never written
    for that row: no kernel may read them) hold NaN."""
    T, C, positions = CASES[name]
    B = len(positions)
    g = torch.Generator().manual_seed(1000 * seed + T + C)
    kc = torch.randn(B, HKV, C, D, generator=g).to(BF)
    vc = torch.randn(B, HKV, C, D, generator=g).to(BF)
    q = torch.randn(B, T, HQ, D, generator=g).to(BF)
    k = torch.randn(B, T, HKV, D, generator=g).to(BF)
    v = torch.randn(B, T, HKV, D, generator=g).to(BF)
    if nan_unread:
        for b, p in enumerate(positions):
            kc[b, :, p:] = float("nan")
            vc[b, :, p:] = float("nan")
    pos_rows = torch.tensor(positions, dtype=torch.int64)
    pid = (pos_rows[None, :, None] + torch.arange(T)[None, None, :]).expand(3, B, T) + torch.tensor([0, 3, 11])[:, None, None]
    dev = lambda t: t.to(device)
    cos, sin = rope_tables(dev(pid))
    return dev(q), dev(k), dev(v), dev(kc), dev(vc), dev(pos_rows), (cos, sin, SECTIONS)


def words(t):
    """a bf16 tensor as its raw 16-bit words (NaN compares equal to itself)"""
    return t.contiguous().view(torch.int16)


def chronological(ring, p, C):
    """[Hkv, n, d]: the n = min(p, C) cached tokens of one ring row [Hkv,C,d] at position p, oldest first"""
    n = min(p, C)
    slots = torch.tensor([(p - n + j) % C for j in range(n)], dtype=torch.long, device=ring.device)
    return ring[:, slots]

"""Helpers of the fork tests (tests/test_fork_cpu.py, tests/test_gpu_fork.py): byte buffers with guard bytes around typed views
for the row-copy operator, and the small stack / prompts / state comparisons of the cache and decoder tests."""
import torch

import parity
from oracle import model as omodel

GUARD = 64          # sentinel bytes in front of and behind every payload (a multiple of 16: the payload keeps its alignment)
ROWS = 5
BF = torch.bfloat16

# (name, dtype, shape, byte offset of the view inside its buffer, columns kept of each row or None)
#   row sizes: 8 B, 2 B, 6 B, 16 KB, 16 KB + 2 B starting one bf16 element into the buffer (neither end on a 16-byte line),
#   the same rows at a row stride of 16400 B (every row at the same offset in a 16-byte line: the 16-byte path with a byte head
#   and tail, and a second piece of 2 bytes), 1 MiB + 48 B, and a column slice (row stride 600 B, row 400 B)
SPECS = [("int64_8B", torch.int64, (ROWS,), 0, None),
         ("bf16_2B", BF, (ROWS,), 0, None),
         ("bf16_6B", BF, (ROWS, 3), 0, None),
         ("bf16_16K", BF, (ROWS, 8192), 0, None),
         ("bf16_16K+2_odd", BF, (ROWS, 8193), 2, None),
         ("bf16_16K+2_odd_stride16400", BF, (ROWS, 8200), 2, 8193),
         ("bf16_1M+48", BF, (ROWS, (2 ** 20 + 48) // 2), 0, None),
         ("bf16_colslice", BF, (ROWS, 300), 0, 200)]


def raw_buffers(seed: int, device):
    """One uint8 buffer of random bytes per spec: GUARD + offset + payload + GUARD bytes."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _, dtype, shape, off, _ in SPECS:
        n = torch.empty(0, dtype=dtype).element_size()
        for s in shape:
            n *= s
        out.append(torch.randint(0, 256, (GUARD + off + n + GUARD,), dtype=torch.uint8, generator=g).to(device))
    return out


def typed_views(raws):
    """The typed views of SPECS on a list of raw buffers (they alias the buffers)."""
    out = []
    for raw, (_, dtype, shape, off, cols) in zip(raws, SPECS):
        n = raw.numel() - 2 * GUARD - off
        t = raw[GUARD + off:GUARD + off + n].view(dtype).view(shape)
        out.append(t if cols is None else t[:, :cols])
    return out


def small_stack(device, window=96, seed=3):
    from infinitevl_amd.harness import InfiniteVLTextStack
    hc, oc = parity.small_configs(window)
    params = parity.bf16_params(omodel.random_params(oc, seed=seed, vocab=hc.vocab_size))
    stack = InfiniteVLTextStack(hc)
    parity.load_params(stack, params)
    return stack.to(device, torch.bfloat16).eval().fuse_(), hc


def prompt(hc, T, seed, device):
    """(inputs_embeds bf16 [1,T,hidden] on the device, token ids int64 [T] on the host)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, T, hc.hidden_size, generator=g) * 0.5).to(torch.bfloat16).to(device)
    return x, torch.randint(0, hc.vocab_size, (T,), generator=g)


def assert_rows_equal(cache, a, b, what=""):
    """Slots a and b of a MultiStreamCache hold the same bits in every row tensor, and the same host length."""
    for i, t in enumerate(cache.row_tensors()):
        assert torch.equal(t[a], t[b]), (what, "row tensor", i, a, b)
    assert cache.slot_lengths[a] == cache.slot_lengths[b], (what, cache.slot_lengths)

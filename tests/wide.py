"""The 16-row weight-stream kernel (csrc/linear_m16.hip): its summation PLAN restated in Python, and the case lists that
tests/test_wide_cpu.py and tests/test_gpu_wide.py share.  CPU only, pure torch / Python.

THE PLAN (a function of K alone -- not of M, not of N, not of the weight format).  A chunk is 8 consecutive k; tile t of a
row is the chunks [256 t, 256 t + 256); step s = 16 t + j (j in 0..15) is four MFMAs u = 0..3 whose k-group g (lane >> 4, 8 k each)
holds chunk 256 t + 4 j + g + 64 u.  The steps with a chunk below K / 8 are 0 .. S - 1; they are cut into KSPLIT = 8 contiguous slices
of ceil(S / 8) steps, one per wave; the slices are added in ascending order.  In the shuffled MXFP4 row of ops.mxfp4_shuffle the lane
(row, g) reads ONE 16-byte piece per step at byte 1024 t + 16 (4 j + g), whose dword u is that chunk, and one dword of scales at byte
64 t + 4 j of the scale row, whose byte u is the scale of the chunk's block.  Keep this in step with linear_m16.hip.
"""
from __future__ import annotations

from typing import Iterator, List, Tuple

KS_PLAN = (32, 64, 2016, 2048, 2080, 4128, 11008)           # test_wide_cpu.py: the plan restated
# the kernel-level shapes of test_gpu_wide.py: one chunk group; fewer chunks than waves of the K split; both sides of the 2048-element
# tile the mxfp4 layout pads to -- and N below, at and above one 16-row tile, with a wide tail
KS = (32, 64, 96, 2016, 2048, 2080, 4128)
NS = (1, 15, 16, 17, 100, 4100)
MS = (1, 5, 15, 16)
ROWS = 16


def tiles(K: int) -> int:
    return -(-K // 2048)


def steps(K: int) -> int:
    """S: tile t < T - 1 has all 16 steps, the last one those whose first chunk 256 t + 4 j lies below K / 8"""
    nchunk, T = K // 8, tiles(K)
    last = nchunk - 256 * (T - 1)
    return 16 * (T - 1) + min(16, -(-last // 4))


def chunk(t: int, j: int, g: int, u: int) -> int:
    return 256 * t + 4 * j + g + 64 * u


KSPLIT = 8                                                   # waves that share a range of output columns


def slices(K: int) -> List[range]:
    """the steps of each wave of the K split, in the order the partial sums are added"""
    S = steps(K)
    per = -(-S // KSPLIT)
    return [range(min(S, k * per), min(S, (k + 1) * per)) for k in range(KSPLIT)]


def step_chunks(K: int) -> Iterator[Tuple[int, int, int, int, int]]:
    """(s, j, g, u, chunk) of every operand slot of every step, in the order of issue (s, u ascending; g is the k-group inside one MFMA)"""
    for s in range(steps(K)):
        t, j = divmod(s, 16)
        for u in range(4):
            for g in range(4):
                yield s, j, g, u, chunk(t, j, g, u)


def mxfp4_code_byte(t: int, j: int, g: int, u: int) -> int:
    """byte offset, in a shuffled row of codes, of the 4 bytes of chunk(t, j, g, u)"""
    return 1024 * t + 16 * (4 * j + g) + 4 * u


def mxfp4_scale_byte(t: int, j: int, u: int) -> int:
    """byte offset, in a shuffled row of scales, of the scale of the block of chunk(t, j, ., u)"""
    return 64 * t + 4 * j + u


def kernel_cases() -> List[Tuple[int, int]]:
    return [(K, N) for K in KS for N in NS]

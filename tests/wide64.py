"""The 64-row weight-stream kernel (csrc/linear_m64.hip): the case lists that tests/test_wide64_cpu.py and
tests/test_gpu_wide64.py share.  CPU only, pure Python.

THE PLAN is the 16-row kernel's and is not restated here: tests/wide.py holds it (steps, slices, chunk), and this module takes it
from there.  What is new is the number of x tiles: the 64 rows are XT = ceil(M / 16) B operands, and every (weight tile, x tile) pair
is summed by the plan of tests/wide.py.
"""
from __future__ import annotations

from typing import List, Tuple

from wide import KSPLIT, chunk, slices, steps, tiles  # noqa: F401  (the plan: one statement, in tests/wide.py)

ROWS = 64
# the first row of a second x tile; both sides of each tile boundary; the full operand
MS64 = (17, 31, 32, 33, 48, 49, 64)
# one chunk group; fewer steps than waves of the K split; a full tile of 2048 k; a tile and a step; two tiles and a slice left empty
KS = (32, 96, 2048, 2080, 4128)
# below and above one 16-row weight tile, a tail that is no multiple of 4, a wide tail
NS = (1, 17, 100, 4100)
# plain projections of 8192 weight rows and more: a wave owns two column tiles; 8209: the second tile of the last wave lies past N and
# N % 4 != 0 takes the 2-byte stores
PAIRS = ((96, 8192), (2080, 8209))
# contract C2, row for row: (N, K)
ROW_CASES = ((100, 2080), (17, 4128), (8209, 96))


def xt(M: int) -> int:
    """x tiles of 16 rows of an M-row call"""
    return -(-M // 16)


def kernel_cases() -> List[Tuple[int, int]]:
    return [(K, N) for K in KS for N in NS]


def variants(K: int) -> Tuple[Tuple[bool, str], ...]:
    """(glu, variant) of the exact-integer probe at K: "ties" needs two chunk groups"""
    return ((False, "index"), (True, "index")) + (((False, "ties"),) if K >= 64 else ())

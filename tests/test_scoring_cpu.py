"""CPU (-m "not gpu"): the host side of scoring given tokens -- argument validation of ivl_linear_logprob_m256_fwd and the workspace
formula through ctypes (pointers are never dereferenced), the ABI version, the label shift of harness.score_sequence, and the
float64 reference's own edge conventions (tests/scoring.py)."""
import ctypes
import math
import os

import pytest
import torch

import scoring
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_linear_logprob_argument_validation(lib):
    from infinitevl_amd import _lib
    one = ctypes.c_void_p(0x1000)       # never dereferenced: validation fails first
    f = lib.ivl_linear_logprob_m256_fwd
    big = 1 << 30

    def call(x=one, w=one, bias=None, target=one, logprob=one, top1=None, lse=None, M=256, N=64, K=64, ws=one, ws_bytes=big):
        return f(x, w, bias, target, logprob, top1, lse, M, N, K, ws, ws_bytes, None)
    assert call(target=None) == _lib.IVL_ERR_INVALID_ARG and b"NULL" in lib.ivl_last_error()
    assert call(logprob=None) == _lib.IVL_ERR_INVALID_ARG and b"NULL" in lib.ivl_last_error()
    assert call(ws=None) == _lib.IVL_ERR_INVALID_ARG and b"NULL" in lib.ivl_last_error()
    assert call(x=None) == _lib.IVL_ERR_INVALID_ARG and call(w=None) == _lib.IVL_ERR_INVALID_ARG
    assert call(M=0) == _lib.IVL_ERR_INVALID_ARG and b"M=0" in lib.ivl_last_error()
    assert call(M=257) == _lib.IVL_ERR_UNSUPPORTED and b"M=257" in lib.ivl_last_error()
    assert call(N=100, K=136) == _lib.IVL_ERR_UNSUPPORTED and b"K=136" in lib.ivl_last_error()        # K % 64
    assert call(K=16384 + 64) == _lib.IVL_ERR_UNSUPPORTED                                              # K too large
    assert call(N=102, K=128) == _lib.IVL_ERR_UNSUPPORTED and b"N=102" in lib.ivl_last_error()        # N % 4
    assert call(N=600000, K=4096) == _lib.IVL_ERR_UNSUPPORTED                                          # 32-bit weight offsets
    need = lib.ivl_linear_logprob_workspace_bytes(256, 64)
    assert call(ws_bytes=need - 1) == _lib.IVL_ERR_WORKSPACE
    assert str(need - 1).encode() in lib.ivl_last_error() and str(need).encode() in lib.ivl_last_error()
    assert call(x=ctypes.c_void_p(0x1008)) == _lib.IVL_ERR_INVALID_ARG and b"0x1008" in lib.ivl_last_error()   # x not 16-byte aligned
    with pytest.raises(ValueError):
        _lib.check(call(M=257))
    with pytest.raises(_lib.IvlError):
        _lib.check(call(ws_bytes=16))


def test_linear_logprob_workspace_formula(lib):
    f = lib.ivl_linear_logprob_workspace_bytes
    for M, N in ((256, 151936), (130, 151936), (1, 64), (200, 4100), (256, 1000), (7, 4)):
        exact = -(-N // 64) * M * 16 + M * 4
        assert exact <= f(M, N) < exact + 256 and f(M, N) % 256 == 0, (M, N, f(M, N))
    assert f(256, 151936) < 9.8e6                    # against 77.8 MB for the logits of 256 rows
    assert f(0, 64) == 0 and f(4, 0) == 0


def test_abi_version_is_still_12(lib):
    from infinitevl_amd import _lib
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12


def test_ops_linear_logprob_refuses_what_the_kernel_cannot_take():
    from infinitevl_amd import ops
    x, w, t = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="linear_logprob"):
        ops.linear_logprob(x, w, t)                                      # CPU tensors: there is no other path


# ---- the label shift -------------------------------------------------------------------------
def test_shift_labels_matches_the_hand_loop():
    from infinitevl_amd.harness import IGNORE_INDEX, shift_labels
    assert IGNORE_INDEX == -100
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 512, (600,), generator=g)
    labels[250:262] = -100                            # a run of ignored labels that straddles the chunk boundary at 256
    labels[0] = -100
    for nxt in (None, 7):
        sh = shift_labels(labels, nxt)
        assert sh.dtype == torch.int64 and sh.tolist() == scoring.shifted_by_hand(labels.tolist(), nxt)
        # a chunk takes a slice: the last position of chunk [0, 256) is scored against the FIRST label of the next chunk
        assert sh[255] == labels[256] and sh[511] == labels[512]
        assert sh[599] == (-100 if nxt is None else 7)
        assert sh[248] == labels[249] and sh[249:261].tolist() == [-100] * 12 and sh[261] == labels[262]
    assert torch.equal(labels[250:262], torch.full((12,), -100))          # the input is not modified
    two = torch.stack([labels, labels.flip(0)])
    assert torch.equal(shift_labels(two, 3)[1], shift_labels(labels.flip(0), 3))
    assert shift_labels(torch.tensor([5]), None).tolist() == [-100] and shift_labels(torch.tensor([5]), 9).tolist() == [9]
    with pytest.raises(ValueError):
        shift_labels(labels.to(torch.int32))
    with pytest.raises(ValueError):
        shift_labels(labels, next_label=1.5)
    with pytest.raises(ValueError):
        shift_labels(torch.zeros(0, dtype=torch.int64))


def test_score_sequence_checks_its_arguments_before_any_launch():
    from infinitevl_amd.harness import score_sequence
    ids = torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="exactly one"):
        score_sequence(None, None, labels=ids)
    with pytest.raises(ValueError, match="labels"):
        score_sequence(None, None, input_ids=ids, labels=torch.zeros(1, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match="chunk"):
        score_sequence(None, None, input_ids=ids, labels=ids, chunk=0)
    with pytest.raises(ValueError, match="position_ids"):
        score_sequence(None, None, input_ids=ids, labels=ids, position_ids=torch.zeros(3, 1, 9, dtype=torch.int64))


# ---- the reference's own edges ---------------------------------------------------------------
def test_reference_edge_conventions():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[-inf, -inf, nan, -inf],            # nothing but -inf / NaN: Z = N, every token -log N, top1 = 0
                      [1.0, inf, -inf, inf],              # a +inf tie: Z = 2, lse = +inf, the lowest index wins
                      [nan, 2.0, 2.0, -inf],              # NaN counts as -inf; a finite tie
                      [0.0, 1.0, 2.0, 3.0]], dtype=torch.float64)
    lp, top1, lse = scoring.ref_logprob(x, torch.tensor([2, 3, 0, 3]))
    assert top1.tolist() == [0, 1, 1, 3]
    assert lp[0].item() == -math.log(4.0) and lse[0].item() == -inf
    assert lp[1].item() == -math.log(2.0) and lse[1].item() == inf
    assert lp[2].item() == -inf and lse[2].item() == pytest.approx(2.0 + math.log(2.0), abs=1e-15)
    ref3 = 3.0 - math.log(sum(math.exp(v) for v in (0.0, 1.0, 2.0, 3.0)))
    assert lp[3].item() == pytest.approx(ref3, abs=1e-14)
    lp, top1, _ = scoring.ref_logprob(x, torch.tensor([0, 0, 1, -100]))
    assert lp[0].item() == -math.log(4.0)                 # a target ON a -inf column of the all -inf row
    assert lp[1].item() == -inf                           # a finite logit below a +inf maximum
    assert lp[2].item() == -math.log(2.0)                 # on one of two tied maxima
    assert lp[3].item() == 0.0 and top1[3].item() == 3    # an ignored target: 0.0, top1 still there
    assert scoring.ref_logprob(x, torch.tensor([4, 4, 4, 4]))[0].tolist() == [0.0] * 4     # target == N is not scored
    assert not torch.isnan(torch.stack(scoring.ref_logprob(x, torch.tensor([1, 2, 3, 0]))[::2])).any()


def test_judge_is_exact_on_infinities_and_holds_the_bound():
    r = torch.tensor([-1.0, -float("inf"), 0.0], dtype=torch.float64)
    assert scoring.judge(r.float(), r) == 0.0
    with pytest.raises(AssertionError):
        scoring.judge(torch.tensor([-1.0, -1e30, 0.0]), r)
    with pytest.raises(AssertionError):
        scoring.judge(torch.tensor([-1.0 - 2e-5, -float("inf"), 0.0]), r)
    assert scoring.judge(torch.tensor([-1.0 - 1.5e-5, -float("inf"), 0.0]), r, scale=2.0) > 1.0


@pytest.mark.parametrize("scale", [1.0, 4.0, 12.0])
def test_blocked_arithmetic_stays_inside_the_derived_bound(scale):
    """The blocking of the kernel (64-column fp32 partial sums, a float64 combine, fp32 log) emulated on random bf16 rows of
    the full vocabulary: the error against float64 stays at or under 0.14 of the bound the GPU test holds the kernel to."""
    g = torch.Generator().manual_seed(int(scale))
    x = (torch.randn(4, 151936, generator=g) * scale).to(torch.bfloat16)
    _, _, lse = scoring.ref_logprob(x, torch.zeros(4, dtype=torch.int64))
    got = scoring.blocked_emulation(x)
    ratio = ((got.double() - lse).abs() / scoring.tolerance(lse)).max().item()
    print(f"scale {scale}: max |err| / tolerance = {ratio:.3f}")
    assert ratio <= 0.14

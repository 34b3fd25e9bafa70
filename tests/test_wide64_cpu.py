"""CPU: the opt-in 64-row weight-stream projections -- what can be said without a GPU.

  * the three entry points are declared and exported, with the argument lists of their 16-row counterparts, and refuse, on the host
    and before any launch, what the header says they refuse: the 16-row entries' refusals with the row bound moved to 64;
  * the switch: use_wide_decode(max_rows=) takes an int in 16..64, leaves everything as it was at the default 16, goes down to the
    mixers and the MLP, has no effect on CPU tensors; _stale() turns true when it changes;
  * the case lists of tests/wide64.py: the plan is the one of tests/wide.py (the same objects), the rows cover every tile boundary, and
    the exact-integer probe meets its own conditions on them.
"""
import ctypes
import os
import subprocess

import pytest
import torch

import projections as pj
import rowwise as rw
import wide
import wide64
from conftest import ROOT

BF = torch.bfloat16
NAMES = ("ivl_linear_m64_fwd", "ivl_linear_m64_w8_fwd", "ivl_linear_m64_w4_fwd")
NAMES16 = ("ivl_linear_m16_fwd", "ivl_linear_m16_w8_fwd", "ivl_linear_m16_w4_fwd")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_entry_points_are_declared_and_exported_with_the_m16_argument_lists(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name, name16 in zip(NAMES, NAMES16):
        assert name in _lib.PROTOTYPES and name in exported and hasattr(lib, name), name
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name16], "the argument list of the 16-row counterpart"
    assert len(_lib.PROTOTYPES[NAMES[0]][1]) == 9 and len(_lib.PROTOTYPES[NAMES[1]][1]) == len(_lib.PROTOTYPES[NAMES[2]][1]) == 10
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12, "the change only adds symbols"


def test_refusals_come_before_any_launch(lib):
    """never-dereferenced pointers on a machine that may have no GPU: every refusal is decided on the host"""
    from infinitevl_amd import _lib
    p, odd16, odd4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1002)
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    bf, w8_, w4_ = (getattr(lib, n) for n in NAMES)

    def calls(x=p, w=p, s=p, y=p, M=33, N=16, K=64, glu=0):
        """the same arguments through the three entry points (s: scale / sq)"""
        return [("bf16", lambda: bf(x, w, None, y, M, N, K, glu, None)), ("w8", lambda: w8_(x, w, s, None, y, M, N, K, glu, None)),
                ("w4", lambda: w4_(x, w, s, None, y, M, N, K, glu, None))]

    def refused(code, frag, **kw):
        for (name, fn), who in zip(calls(**kw), NAMES):
            assert fn() == code and frag in lib.ivl_last_error() and who.encode() in lib.ivl_last_error(), (name, kw, lib.ivl_last_error())

    for glu in (0, 1):
        refused(UNS, b"1..64 rows", M=0, glu=glu)
        refused(UNS, b"1..64 rows", M=65, glu=glu)
        refused(UNS, b"1..64 rows", M=-3, glu=glu)
        refused(INV, b"multiple of 32", K=0, glu=glu)
        refused(INV, b"multiple of 32", K=48, glu=glu)
        refused(INV, b"multiple of 32", K=16, glu=glu)
        refused(INV, b"N=0", N=0, glu=glu)
        refused(INV, b"NULL", x=None, glu=glu)
        refused(INV, b"NULL", w=None, glu=glu)
        refused(INV, b"NULL", y=None, glu=glu)
        refused(INV, b"aligned", x=odd16, glu=glu)
        refused(INV, b"aligned", w=odd16, glu=glu)
        refused(INV, b"aligned", y=odd16, glu=glu)
    for fn in (w8_, w4_):                                  # scale / sq
        assert fn(p, p, None, None, p, 33, 16, 64, 0, None) == INV and b"NULL" in lib.ivl_last_error()
        assert fn(p, p, odd4, None, p, 33, 16, 64, 0, None) == INV and b"aligned" in lib.ivl_last_error()
    # a weight past the 32-bit byte offsets: 600000 x 4096 bf16 are 4.9e9 bytes (one bound for the three formats: the plan is theirs in
    # common); 2^20 rows of 2048 are exactly 2^32
    refused(UNS, b"32-bit offsets", N=600000, K=4096)
    refused(UNS, b"32-bit offsets", N=300000, K=4096, glu=1)
    refused(UNS, b"32-bit offsets", N=1 << 20, K=2048)
    assert w4_(p, p, p, None, p, 33, 1 << 22, 32, 0, None) == UNS and b"32-bit offsets" in lib.ivl_last_error(), "padded mxfp4 rows"
    # the 16-row entries keep their own bound and their own words
    assert lib.ivl_linear_m16_fwd(p, p, None, p, 17, 16, 64, 0, None) == UNS and b"1..16 rows" in lib.ivl_last_error()


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def _stack():
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16, sliding_window=8, layer_types=["sliding_attention", "linear_attention"],
                               num_linear_heads=4, num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


def _flags(m):
    mods = [m] + [x for layer in m.layers for x in (layer.self_attn, layer.mlp)]
    return [(x._wide_on, x._wide_lora, x._wide_rows) for x in mods]


@pytest.mark.parametrize("bad", [15, 65, 0, -16, 128, 32.0, "32", None, True])
def test_max_rows_outside_16_to_64_is_refused_and_changes_nothing(bad):
    m = _stack().use_wide_decode(True, max_rows=32)
    was = _flags(m)
    with pytest.raises(ValueError, match="max_rows"):
        m.use_wide_decode(True, max_rows=bad)
    assert _flags(m) == was


def test_the_default_leaves_the_flags_of_the_16_row_switch_as_they_were():
    from infinitevl_amd import ops
    m = _stack()
    n = len(_flags(m))
    assert n == 5 and _flags(m) == [(False, False, 16)] * n
    assert m.use_wide_decode(True) is m and _flags(m) == [(True, False, 16)] * n
    assert m.use_wide_decode(True, adapters=True) is m and _flags(m) == [(True, True, 16)] * n
    assert m.use_wide_decode(True, max_rows=16) is m and _flags(m) == [(True, False, 16)] * n
    # what the modules hand to ops.linear at the default is what the 16-row switch has always handed over: no new key
    assert ops.wide_kwargs(False) == ops.wide_kwargs(False, False, 64) == {}
    assert ops.wide_kwargs(True) == ops.wide_kwargs(True, False, 16) == {"wide": True}
    assert ops.wide_kwargs(True, True) == ops.wide_kwargs(True, True, 16) == {"wide": True, "wide_lora": True}
    assert ops.wide_kwargs(True, False, 64) == {"wide": True, "wide_rows": 64}
    assert ops.wide_kwargs(True, True, 48) == {"wide": True, "wide_lora": True, "wide_rows": 48}
    for R in (17, 48, 64):
        assert m.use_wide_decode(True, max_rows=R) is m and _flags(m) == [(True, False, R)] * n
    assert m.use_wide_decode(True, adapters=True, max_rows=64) is m and _flags(m) == [(True, True, 64)] * n
    m.use_wide_decode(False, max_rows=64)
    assert _flags(m) == [(False, False, 16)] * n, "off is off: nothing of max_rows stays behind"
    assert ops.M64_ROWS == 64 and set(ops.M64_CALLS) == {"bf16", "e4m3", "mxfp4"} and all(isinstance(v, int) for v in ops.M64_CALLS.values())
    assert ops.M16_ROWS == 16 and set(ops.M16_CALLS) == {"bf16", "e4m3", "mxfp4"}


def test_the_switch_leaves_cpu_calls_alone_and_the_direct_entry_needs_the_device():
    from infinitevl_amd import ops
    g_ = rw.gen(6)
    x = (torch.randn(1, 24, 64, generator=g_) * 0.5).to(BF)                # 24 rows: the row count max_rows is about
    w = (torch.randn(96, 64, generator=g_) * 0.1).to(BF)
    b = torch.randn(96, generator=g_).to(BF)
    before = (dict(ops.M64_CALLS), dict(ops.M16_CALLS), dict(ops.W8_CALLS), dict(ops.W4_CALLS))
    want = torch.nn.functional.linear(x, w, b)
    assert torch.equal(ops.linear(x, w, b, wide=True, wide_rows=64), want) and torch.equal(ops.linear(x, w, b, wide=True), want)
    assert (ops.M64_CALLS, ops.M16_CALLS, ops.W8_CALLS, ops.W4_CALLS) == before, "nothing on the CPU reaches a kernel"
    with pytest.raises(RuntimeError):
        ops.linear_m64(x, w, b)                                            # no quiet fall-back


def test_a_graphed_class_is_stale_after_max_rows_changes():
    """_Graphed._stale() on a stub that was 'captured' at one row bound (what _capture records)"""
    from infinitevl_amd.harness import _Graphed

    class Stub(_Graphed):
        def __init__(self, model):
            self.model, self.graph = model, object()
            self._captured_w8, self._captured_fmt = self._w8_on(), self._w8_fmt()
            self._captured_wide, self._captured_wide_lora = self._wide_on(), self._wide_lora_on()
            self._captured_wide_rows, self._captured_lora = self._wide_rows(), self._lora_sig()

    m = _stack().use_wide_decode(True)
    s = Stub(m)
    assert s._captured_wide_rows == 16 and not s._stale()
    m.use_wide_decode(True, max_rows=16)
    assert not s._stale(), "the default spelled out is the default"
    m.use_wide_decode(True, max_rows=64)
    assert s._stale()
    s64 = Stub(m)
    assert s64._captured_wide_rows == 64 and not s64._stale()
    m.use_wide_decode(True, max_rows=48)
    assert s64._stale() and s._stale()
    m.use_wide_decode(True)
    assert s64._stale() and not s._stale()
    m.use_wide_decode(False)
    assert s64._stale() and s._stale()
    assert _Graphed._captured_wide_rows == 16, "a class that never captured has the default"


# ---- the case lists -------------------------------------------------------------------------------------------------------------------
def test_the_plan_is_the_one_of_the_16_row_kernel_and_the_rows_cover_every_tile_boundary():
    assert wide64.steps is wide.steps and wide64.slices is wide.slices and wide64.chunk is wide.chunk and wide64.KSPLIT == 8
    assert wide64.MS64 == (17, 31, 32, 33, 48, 49, 64) and wide64.ROWS == 64
    assert {wide64.xt(M) for M in wide64.MS64} == {2, 3, 4} and all(wide64.xt(M) == 1 for M in wide.MS)
    assert 17 in wide64.MS64 and 64 in wide64.MS64         # (16 rows and fewer are the 16-row kernel's: tests/wide.py)
    for b in (32, 48):                                     # the full tile and the first row of the next
        assert b in wide64.MS64 and b + 1 in wide64.MS64
    # K: a row shorter than one step's four MFMAs, fewer steps than waves, whole slices, a slice left empty
    S = {K: wide.steps(K) for K in wide64.KS}
    assert S == {32: 1, 96: 3, 2048: 16, 2080: 17, 4128: 33}
    assert [sum(1 for r in wide.slices(K) if r) for K in wide64.KS] == [1, 3, 8, 6, 7]
    assert all(N >= 8192 for _, N in wide64.PAIRS) and any(N % 4 for _, N in wide64.PAIRS)


def test_the_kernel_level_cases_meet_the_probes_conditions():
    """the builders assert the conditions while they pick the seed: here for every K at the narrow N (the GPU test builds all)"""
    for K, N in wide64.kernel_cases():
        if N > 100:
            continue
        for glu, variant in wide64.variants(K):
            c = pj.int_case(wide64.ROWS, N, K, glu, variant, Ms=wide64.MS64)
            assert c["x"].shape[0] == 64 and all(pj.conditions(c, M) is None for M in wide64.MS64), (K, N, glu, variant)


def test_the_judge_bites_at_64_rows():
    """the honest fp32 emulation passes check_linear at the rows of MS64; a kernel that swaps two rows, or drops the last piece, does not"""
    lin = lambda wrong: (lambda x, w, bias, glu: pj.emu_linear(x, w, bias, glu, wrong, 0))      # noqa: E731
    c = pj.int_case(wide64.ROWS, 17, 96, False, "index", Ms=wide64.MS64)
    assert pj.check_linear(lin(""), c, wide64.MS64).ok()
    for wrong in ("swap_rows", "drop_last_piece"):
        assert not pj.check_linear(lin(wrong), c, wide64.MS64).ok(), wrong

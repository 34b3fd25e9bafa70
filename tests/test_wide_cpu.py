"""CPU: the opt-in 16-row weight-stream projections -- what can be said without a GPU.

  * the three entry points are declared and exported and refuse, on the host and before any launch, what the header says they refuse;
  * the summation plan restated in tests/wide.py: over (tile, step, k-group, u) the chunks are a permutation of the K / 8 chunks of a
    row plus padding, the steps that exist hold every real chunk, the K split cuts them into contiguous slices, and in a row made by
    ops.mxfp4_shuffle from index-valued codes the byte addresses of the plan hold exactly those chunks and their block scales;
  * the switch: off by default, passed down to the mixers and the MLP, without effect on CPU tensors; _stale() turns true when it flips;
  * the judges bite at 16 rows: the honest fp32 emulation passes check_linear and check_randn in two summation orders, every wrong one
    of projections.WRONG_LINEAR / WRONG_GLU is reported.
"""
import ctypes
import os
import subprocess

import pytest
import torch

import projections as pj
import rowwise as rw
import wide
from conftest import ROOT

BF = torch.bfloat16
NAMES = ("ivl_linear_m16_fwd", "ivl_linear_m16_w8_fwd", "ivl_linear_m16_w4_fwd")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_entry_points_are_declared_and_exported(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in _lib.PROTOTYPES and name in exported and hasattr(lib, name), name
    assert len(_lib.PROTOTYPES[NAMES[0]][1]) == 9 and len(_lib.PROTOTYPES[NAMES[1]][1]) == len(_lib.PROTOTYPES[NAMES[2]][1]) == 10
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12, "the change only adds symbols"


def test_refusals_come_before_any_launch(lib):
    """never-dereferenced pointers on a machine that may have no GPU: every refusal is decided on the host"""
    from infinitevl_amd import _lib
    p, odd16, odd4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0x1002)
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    bf, w8_, w4_ = (getattr(lib, n) for n in NAMES)

    def calls(x=p, w=p, s=p, y=p, M=5, N=16, K=64, glu=0):
        """the same arguments through the three entry points (s: scale / sq)"""
        return [("bf16", lambda: bf(x, w, None, y, M, N, K, glu, None)), ("w8", lambda: w8_(x, w, s, None, y, M, N, K, glu, None)),
                ("w4", lambda: w4_(x, w, s, None, y, M, N, K, glu, None))]

    def refused(code, frag, **kw):
        for name, fn in calls(**kw):
            assert fn() == code and frag in lib.ivl_last_error(), (name, kw, lib.ivl_last_error())

    for glu in (0, 1):
        refused(UNS, b"1..16 rows", M=0, glu=glu)
        refused(UNS, b"1..16 rows", M=17, glu=glu)
        refused(INV, b"multiple of 32", K=0, glu=glu)
        refused(INV, b"multiple of 32", K=40, glu=glu)
        refused(INV, b"N=0", N=0, glu=glu)
        refused(INV, b"NULL", x=None, glu=glu)
        refused(INV, b"NULL", w=None, glu=glu)
        refused(INV, b"NULL", y=None, glu=glu)
        refused(INV, b"aligned", x=odd16, glu=glu)
        refused(INV, b"aligned", w=odd16, glu=glu)
        refused(INV, b"aligned", y=odd16, glu=glu)
    for fn in (w8_, w4_):                                  # scale / sq
        assert fn(p, p, None, None, p, 5, 16, 64, 0, None) == INV and b"NULL" in lib.ivl_last_error()
        assert fn(p, p, odd4, None, p, 5, 16, 64, 0, None) == INV and b"aligned" in lib.ivl_last_error()
    # N K past the 32-bit offsets: 2^20 rows of 2048 bf16 are 2^32 bytes; one row less fits and would be launched, so it is not tried
    refused(UNS, b"32-bit offsets", N=1 << 20, K=2048)
    refused(UNS, b"32-bit offsets", N=1 << 19, K=2048, glu=1)
    assert w4_(p, p, p, None, p, 5, 1 << 22, 32, 0, None) == UNS and b"32-bit offsets" in lib.ivl_last_error(), "padded mxfp4 rows"


def test_a_call_that_breaks_several_rules_is_refused_for_the_first_of_them(lib):
    """the order of the refusals -- NULL, rows, N, K, offsets, alignment -- through all nine entries of the two kernels"""
    from infinitevl_amd import _lib
    p, odd16 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    seen = 0
    for family, max_rows in (("ivl_linear_m16", 16), ("ivl_linear_m64", 64), ("ivl_linear_m16_lora", 16)):
        for suffix, n_weight in (("_fwd", 1), ("_w8_fwd", 2), ("_w4_fwd", 2)):
            name = family + suffix
            fn = getattr(lib, name)
            tail = (None, None) if "lora" in name else (None,)             # (lora,) stream
            assert len(_lib.PROTOTYPES[name][1]) == 1 + n_weight + 6 + len(tail)

            def call(x, M, K):
                return fn(x, *([p] * n_weight), None, p, M, 16, K, 0, *tail)

            assert call(None, 0, 48) == INV and lib.ivl_last_error() == f"{name}: NULL pointer".encode(), name
            assert call(p, 0, 48) == UNS and lib.ivl_last_error() == f"{name}: M=0 (built for 1..{max_rows} rows)".encode(), name
            assert call(odd16, 5, 48) == INV, name
            err = lib.ivl_last_error()
            assert err.startswith(f"{name}: K=48 (".encode()) and b"multiple of 32" in err and b"aligned" not in err, (name, err)
            seen += 1
    assert seen == 9


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", wide.KS_PLAN)
def test_plan_is_a_permutation_of_the_chunks_plus_padding(K):
    nchunk, T, S = K // 8, wide.tiles(K), wide.steps(K)
    every = [wide.chunk(t, j, g, u) for t in range(T) for j in range(16) for g in range(4) for u in range(4)]
    assert sorted(every) == list(range(256 * T)), "over whole tiles: every chunk of the padded row exactly once"
    issued = [c for _, _, _, _, c in wide.step_chunks(K)]
    assert len(issued) == 16 * S == len(set(issued)) and set(range(nchunk)) <= set(issued), "the steps that exist hold every real chunk"
    assert all(c >= nchunk for c in set(every) - set(issued)), "steps that do not exist hold padding only"
    assert S >= 1 and wide.chunk(*divmod(S - 1, 16), 0, 0) < nchunk <= 256 * T, "the last step holds a real chunk"
    assert wide.steps(K) == sum(1 for t in range(T) for j in range(16) if wide.chunk(t, j, 0, 0) < nchunk)
    sl = wide.slices(K)
    assert len(sl) == wide.KSPLIT == 8 and [s for r in sl for s in r] == list(range(S)), "contiguous slices, in order, of all steps"
    assert all(len(r) == -(-S // 8) for r in sl if r and r[-1] != S - 1), "every slice but the last non-empty one is full"
    assert (sum(1 for r in sl if r) < 8) == (K in (32, 64, 2080, 4128)), "fewer steps than waves, and a last wave left without one"


@pytest.mark.parametrize("K", wide.KS_PLAN)
def test_plan_addresses_in_a_shuffled_row_hold_those_chunks_and_their_scales(K):
    from infinitevl_amd import ops
    nchunk, nblock = K // 8, K // 32
    idx = torch.arange(nchunk)
    # chunk c = the 4 bytes (c & 255, c >> 8, 0xA5, 0x5A + row): no chunk is all zero, so padding can be told apart
    codes = torch.stack([torch.stack([idx & 255, idx >> 8, torch.full_like(idx, 0xA5), torch.full_like(idx, 0x5A + r)], 1).reshape(-1)
                         for r in range(2)]).to(torch.uint8)
    e8m0 = torch.stack([(torch.arange(nblock) * 7 + r) % 126 + 1 for r in range(2)]).to(torch.uint8)        # never 127
    wq, sq = ops.mxfp4_shuffle(codes, e8m0)
    seen = 0
    for s, j, g, u, c in wide.step_chunks(K):
        t = s // 16
        a = wide.mxfp4_code_byte(t, j, g, u)
        assert a % 4 == 0 and (a - 4 * u) % 16 == 0, "dword u of one 16-byte piece per (step, lane group)"
        got = wq[:, a:a + 4]
        if c < nchunk:
            assert torch.equal(got, codes[:, 4 * c:4 * c + 4]), (s, g, u, c)
            seen += 1
        else:
            assert not bool(got.any()), "padding: code 0x0"
        b = wide.mxfp4_scale_byte(t, j, u)
        assert (b - u) % 4 == 0, "byte u of one dword per step"
        want = e8m0[:, c // 4] if c // 4 < nblock else torch.full((2,), 127, dtype=torch.uint8)
        assert torch.equal(sq[:, b], want), (s, g, u, c)
    assert seen == nchunk


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def _stack():
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4,
                               num_key_value_heads=2, head_dim=16, sliding_window=8, layer_types=["sliding_attention", "linear_attention"],
                               num_linear_heads=4, num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


def test_switch_is_off_by_default_goes_down_to_the_modules_and_leaves_cpu_calls_alone():
    from infinitevl_amd import ops
    m = _stack()
    mods = [x for layer in m.layers for x in (layer.self_attn, layer.mlp)]
    assert m._wide_on is False and all(x._wide_on is False for x in mods)
    assert ops.wide_kwargs(False) == {} and ops.wide_kwargs(True) == {"wide": True}
    assert set(ops.M16_CALLS) == {"bf16", "e4m3", "mxfp4"} and all(isinstance(v, int) for v in ops.M16_CALLS.values())
    assert set(ops.W8_CALLS) == set(ops.W4_CALLS) == {"linear", "linear_swiglu", "norm_linear", "gdn_out_linear"}
    assert m.use_wide_decode() is m and m._wide_on is True and all(x._wide_on is True for x in mods)
    g_ = rw.gen(5)
    x = (torch.randn(1, 8, 64, generator=g_) * 0.5).to(BF)                 # 8 rows: the row count the switch is about
    w = (torch.randn(96, 64, generator=g_) * 0.1).to(BF)
    b = torch.randn(96, generator=g_).to(BF)
    before = (dict(ops.M16_CALLS), dict(ops.W8_CALLS), dict(ops.W4_CALLS))
    assert torch.equal(ops.linear(x, w, b, wide=True), torch.nn.functional.linear(x, w, b))
    assert torch.equal(ops.linear(x, w, b, wide=True), ops.linear(x, w, b))
    m.use_wide_decode(False)
    assert not m._wide_on and not any(x._wide_on for x in mods)
    assert (ops.M16_CALLS, ops.W8_CALLS, ops.W4_CALLS) == before, "nothing on the CPU reaches a kernel"
    with pytest.raises(RuntimeError):
        ops.linear_m16(x, w, b)                                            # the direct entry needs the device: no quiet fall-back


def test_a_graphed_class_is_stale_after_the_switch_flips():
    """_Graphed._stale() on a stub that was 'captured' with the switch off (what _capture records), as for use_packed_weights"""
    from infinitevl_amd.harness import _Graphed

    class Stub(_Graphed):
        def __init__(self, model):
            self.model, self.graph = model, object()
            self._captured_w8, self._captured_fmt = self._w8_on(), self._w8_fmt()
            self._captured_wide, self._captured_lora = self._wide_on(), self._lora_sig()

    m = _stack()
    s = Stub(m)
    assert s._captured_wide is False and not s._stale()
    m.use_wide_decode(True)
    assert s._stale()
    m.use_wide_decode(False)
    assert not s._stale()
    m.use_wide_decode(True)
    s2 = Stub(m)
    assert s2._captured_wide is True and not s2._stale()
    m.use_wide_decode(False)
    assert s2._stale()
    assert _Graphed._captured_wide is False, "a class that never captured has the default"


# ---- the judges at 16 rows ------------------------------------------------------------------------------------------------------------
JUDGE_CASES = [(False, 17, 96, "index"), (False, 100, 2080, "index"), (False, 15, 64, "ties"), (False, 17, 2016, "ties"),
               (True, 17, 96, "index"), (True, 100, 2080, "index")]


def _lin(wrong="", order=0):
    return lambda x, w, bias, glu: pj.emu_linear(x, w, bias, glu, wrong, order)


def test_honest_emulation_passes_the_judges_at_16_rows_in_two_summation_orders():
    probed = 0
    for glu, N, K, variant in JUDGE_CASES:
        c = pj.int_case(wide.ROWS, N, K, glu, variant, Ms=wide.MS)
        assert c["x"].shape[0] == 16
        for order in (0, 1):
            rep = pj.check_linear(_lin(order=order), c, wide.MS)
            assert rep.ok(), str(rep)
            probed += rep.probed
    for glu, N, K in ((False, 100, 2080), (True, 100, 2080)):
        for order in (0, 1):
            rep = pj.check_randn(_lin(order=order), pj.randn_case(wide.ROWS, N, K, glu), wide.MS)
            assert rep.ok(), str(rep)
    print(f"{probed} elements bit for bit at up to 16 rows")


@pytest.mark.parametrize("wrong", list(pj.WRONG_LINEAR) + list(pj.WRONG_GLU))
def test_wrong_emulation_is_reported_at_16_rows(wrong):
    hits = []
    for glu, N, K, variant in JUDGE_CASES:
        if (wrong in pj.WRONG_GLU and not glu) or (wrong == "truncate" and variant != "ties"):
            continue
        c = pj.int_case(wide.ROWS, N, K, glu, variant, Ms=wide.MS)
        if not pj.check_linear(_lin(wrong), c, (wide.ROWS,)).ok():
            hits.append((glu, N, K, variant))
    print(f"{wrong}: reported at 16 rows in {hits}")
    assert hits, wrong


def test_the_kernel_level_cases_meet_the_probes_conditions():
    """the builders assert the conditions while they pick the seed: here for every K at the narrow N and both N = 4100 cases whose K
    sits at the tile border (the GPU test builds all of them)"""
    for K, N in wide.kernel_cases():
        if N > 100 and K != 2048:
            continue
        for glu in (False, True):
            c = pj.int_case(wide.ROWS, N, K, glu, "index", Ms=wide.MS)
            assert all(pj.conditions(c, M) is None for M in wide.MS), (K, N, glu)
        if K >= 64:
            c = pj.int_case(wide.ROWS, N, K, False, "ties", Ms=wide.MS)
            assert all(pj.conditions(c, M) is None for M in wide.MS), (K, N, "ties")

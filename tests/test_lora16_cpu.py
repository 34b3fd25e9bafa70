"""CPU: per-row LoRA adapters for 5 to 16 decode rows -- the judges of tests/lora16.py, the refusals of the four new
entry points, and the plumbing of use_wide_decode(adapters=True).

  * the 16-row builder's conditions hold for the eight probe shapes (from the float64 reference alone); the honest fp32 emulation
    passes the probe and the randn judge at 16 rows in two summation orders with identical bits; each wrong emulation of lora.WRONG
    is reported;
  * ivl_lora_add_m16_fwd and ivl_linear_m16_lora{,_w8,_w4}_fwd are declared, exported and refuse what the header says they refuse on a
    machine without a GPU, i.e. before anything is launched; the ABI version and the pinned structs are what they were;
  * use_wide_decode(True) leaves the adapters flag off; register allocates t_ws16 next to an unmoved t_ws; a graphed class is stale
    after either half of the pair flips; lora_add(wide=True) on CPU tensors is still peft's computation through torch.
"""
import ctypes
import os
import subprocess

import pytest
import torch

import lora
import lora16
from conftest import ROOT

BF = torch.bfloat16
# the judges' cases: the small shapes of the probe (the two K > 2048 ones and N = 8209 are the GPU's: the straight-order emulation is a
# Python loop over K) and two randn ones
SMALL = [s for s in lora16.SHAPES if s[0] <= 520 and s[1] <= 600]
RANDN = [(520, 600, lora16.SEG6, 16, None, "randn"), (72, 97, (3, 50, 50, 97), 8, 3, "randn")]


def _judge(c, wrong="", order=0, Ms=lora16.MS):
    run = lambda c_, x, res, y0, idx: lora.emu(c_, x, res, y0, idx, wrong=wrong, order=order)          # noqa: E731
    return (lora16.check_randn if c["variant"] == "randn" else lora16.check_probe)(run, c, Ms)


def test_builder_finds_a_seed_for_every_probe_shape_and_its_conditions_hold():
    names = [n for n, _ in lora16.index_patterns(16)]
    assert names == ["none", "last", "same", "different", "mixed", "range"]
    pats = dict(lora16.index_patterns(16))
    assert len(set(pats["different"])) == 16 and pats["mixed"][2::3] == [-1] * 5 and pats["last"] == [-1] * 15 + [3]
    assert {lora16.N_ADAPTERS, -7, 1 << 30} <= set(pats["range"]) and any(0 <= a < lora16.N_ADAPTERS for a in pats["range"])
    for s in lora16.SHAPES:
        c = lora16.shared_case(s)
        K, N, seg, R, rank, variant = s
        assert c["tries"] <= 64 and c["n_adapters"] == 17
        assert tuple(c["x"].shape) == (16, K) and tuple(c["y0"].shape) == (16, N)
        assert tuple(c["A"].shape) == (17, (len(seg) - 1) * R, K) and tuple(c["B"].shape) == (17, N, R)
        assert not bool(c["B"][:, :, c["rank"]:].any()) and not bool(c["B"][:, lora.segment_of(c) < 0].any())
        assert bool((lora.bits(c["y0"]) == -32768).any()), "-0.0 among the zeros of y0"
        want = lora16.INDEX_SCALINGS if variant == "index" else lora16.TIES_SCALINGS
        assert c["s"].tolist() == [want[a % len(want)] for a in range(17)]
        for M in lora16.MS:
            for name, idx in lora16.index_patterns(M):
                assert len(idx) == M
                r_ = lora.chain(c, c["xn"][:M], c["y0"][:M], idx)
                assert lora.conditions(c, r_) is None, (s, M, name)
                assert int(r_["touched"].sum()) == sum(r_["rows"]) * (seg[-1] - seg[0])


def test_honest_emulation_passes_at_16_rows_in_two_orders_with_identical_bits():
    probed = 0
    for s in SMALL + RANDN:
        c = lora16.shared_case(s) if s[5] != "randn" else lora16.case(*s)
        reps = [_judge(c, order=o) for o in (0, 1)]
        for rep in reps:
            assert rep.ok(), str(rep)
        probed += reps[0].probed
        if c["variant"] == "randn":
            assert reps[0].judged > 0 and reps[0].decided <= lora.WINDOW_MAX * reps[0].judged
            continue
        for name, idx in lora16.index_patterns(16):
            a, b = (lora.emu(c, c["x"], None, c["y0"].clone(), idx, order=o) for o in (0, 1))
            assert torch.equal(lora.bits(a[0]), lora.bits(b[0])) and torch.equal(lora.bits(a[1]), lora.bits(b[1])), name
    print(f"{probed} elements bit for bit")
    assert probed > 100000


@pytest.mark.parametrize("wrong", lora.WRONG)
def test_wrong_emulation_is_reported_at_16_rows(wrong):
    hits = []
    for s in SMALL + RANDN[1:]:
        c = lora16.shared_case(s) if s[5] != "randn" else lora16.case(*s)
        if not _judge(c, wrong=wrong, Ms=(5, 16)).ok():
            hits.append(lora16.shape_id(s))
    print(f"{wrong}: reported in {hits}")
    assert hits, wrong


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
ADD = "ivl_lora_add_m16_fwd"
FUSED = ("ivl_linear_m16_lora_fwd", "ivl_linear_m16_lora_w8_fwd", "ivl_linear_m16_lora_w4_fwd")
P = 0x1000                                                        # never dereferenced: every refusal is decided on the host


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def _args(**kw):
    from infinitevl_amd import ops
    a = ops.LoraArgs()
    a.x, a.y = P, 2 * P
    a.adapter_idx = a.A = a.B = a.scaling = a.t_ws = P
    a.M, a.N, a.K, a.R, a.n_adapters, a.n_seg = 8, 600, 512, 16, 3, 2
    cols = kw.pop("cols", (0, 300, 600))
    for k, v in kw.items():
        setattr(a, k, v)
    for i in range(9):
        setattr(a, f"seg_col{i}", cols[min(i, len(cols) - 1)])
    return a


def test_entry_points_are_declared_and_exported_and_the_abi_is_what_it_was(lib):
    from infinitevl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L, V, I = ctypes.POINTER(_lib.LoraArgs), ctypes.c_void_p, ctypes.c_int
    assert _lib.PROTOTYPES[ADD] == (I, [L, V])
    assert _lib.PROTOTYPES[FUSED[0]] == (I, [V, V, V, V, I, I, I, I, L, V])
    assert _lib.PROTOTYPES[FUSED[1]] == _lib.PROTOTYPES[FUSED[2]] == (I, [V, V, V, V, V, I, I, I, I, L, V])
    for name in (ADD,) + FUSED:
        assert name in exported and hasattr(lib, name), name
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12
    assert list(_lib.ARG_STRUCTS) == ["ivl_swa_args", "ivl_lora_args", "ivl_sample_args"] and len(_lib.STRUCTS) == 2


def _common_refusals(lib, call, INV, UNS):
    """the refusals that ivl_lora_add_m16_fwd inherits from the small-M entry; call(**fields of ivl_lora_args)"""
    for f in ("adapter_idx", "A", "B", "scaling", "t_ws"):
        assert call(**{f: None}) == INV and b"NULL" in lib.ivl_last_error(), f
    for R in (0, 4, 12, 24, 48, 128):
        assert call(R=R) == UNS and b"8, 16, 32 or 64" in lib.ivl_last_error(), R
    for n_seg in (0, 9, -1):
        assert call(n_seg=n_seg) == INV and b"n_seg" in lib.ivl_last_error(), n_seg
    for cols in ((0, 700, 600), (-1, 300, 600), (0, 300, 601), (400, 300, 600)):
        assert call(cols=cols) == INV and b"non-decreasing" in lib.ivl_last_error(), cols
    assert call(n_adapters=0) == INV and b"n_adapters" in lib.ivl_last_error()
    assert call(A=P + 8) == INV and b"aligned" in lib.ivl_last_error()
    assert call(adapter_idx=P + 2) == INV and b"aligned" in lib.ivl_last_error()


def test_lora_add_m16_refusals_come_before_any_launch(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    fn = getattr(lib, ADD)
    call = lambda **kw: fn(ctypes.byref(_args(**kw)), None)       # noqa: E731
    assert fn(None, None) == INV
    for f in ("x", "y"):
        assert call(**{f: None}) == INV and b"NULL" in lib.ivl_last_error(), f
    for M in (0, 17, -1):
        assert call(M=M) == UNS and b"1..16 rows" in lib.ivl_last_error(), M
    for K in (4, 12, 516, 0):
        assert call(K=K) == INV, K
    assert call(N=0) == INV
    for K in (512, 2048, 4096):
        assert call(K=K, norm_weight=P) == UNS and b"NORM" in lib.ivl_last_error(), K
    assert call(norm_weight=P, residual=P) == UNS
    assert call(residual=P) == INV and b"residual without norm_weight" in lib.ivl_last_error()
    assert call(x=P + 8) == INV and b"aligned" in lib.ivl_last_error()
    _common_refusals(lib, call, INV, UNS)


@pytest.mark.parametrize("name", FUSED)
def test_fused_entry_refusals_come_before_any_launch(lib, name):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    fn = getattr(lib, name)
    packed = name != FUSED[0]

    def call(x=P, w=P, s=P, y=2 * P, M=8, N=600, K=512, glu=0, lora="default", **kw):
        if lora == "default":
            kw.setdefault("N", 2 * N if glu else N)
            kw.setdefault("cols", (0, 300, kw["N"]))
            lora = ctypes.byref(_args(**{"M": 8, "K": 512, **kw}))
        w_args = (w, s) if packed else (w,)
        return fn(x, *w_args, None, y, M, N, K, glu, lora, None)

    # the m16 entries' own, unchanged
    assert call(x=None) == INV and call(w=None) == INV and call(y=None) == INV
    if packed:
        assert call(s=None) == INV
    for M in (0, 17, -1):
        assert call(M=M) == UNS and b"1..16 rows" in lib.ivl_last_error(), M
    for K in (0, 8, 520, 48):
        assert call(K=K) == INV and b"multiple of 32" in lib.ivl_last_error(), K
    assert call(N=0) == INV
    assert call(x=P + 8) == INV and b"aligned" in lib.ivl_last_error()
    assert call(N=1 << 20, K=4096) == UNS and b"32-bit" in lib.ivl_last_error()
    # what ties `lora` to the call
    assert call(lora=None) == INV and b"NULL lora" in lib.ivl_last_error()
    for f, v in (("x", 3 * P), ("y", 3 * P), ("M", 7), ("K", 544)):
        assert call(**{"lora": ctypes.byref(_args(**{f: v}))}) == INV and b"must be the call's" in lib.ivl_last_error(), f
    assert call(lora=ctypes.byref(_args(N=1200, cols=(0, 300, 1200)))) == INV and b"weight rows" in lib.ivl_last_error()
    assert call(glu=1, N=300, lora=ctypes.byref(_args(N=300, cols=(0, 100, 300)))) == INV and b"weight rows" in lib.ivl_last_error()
    assert call(lora=ctypes.byref(_args(norm_weight=P))) == INV and b"norm fields" in lib.ivl_last_error()
    assert call(lora=ctypes.byref(_args(residual=P))) == INV and b"norm fields" in lib.ivl_last_error()
    # the inherited ones
    _common_refusals(lib, lambda **kw: call(**kw), INV, UNS)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def _stack():
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
                               num_attention_heads=4, num_key_value_heads=2, head_dim=16, sliding_window=8,
                               layer_types=["sliding_attention", "linear_attention"], num_linear_heads=4,
                               num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


def test_the_adapters_flag_is_new_and_off_by_default():
    from infinitevl_amd import ops
    m = _stack()
    mods = [x for layer in m.layers for x in (layer.self_attn, layer.mlp)]
    assert m._wide_lora is False and all(x._wide_lora is False for x in mods)
    assert m.use_wide_decode(True) is m and m._wide_on is True
    assert m._wide_lora is False and not any(x._wide_lora for x in mods), "use_wide_decode(True) leaves the adapters flag off"
    assert m.use_wide_decode(True, adapters=True) is m
    assert m._wide_on is True and m._wide_lora is True and all(x._wide_on and x._wide_lora for x in mods)
    m.use_wide_decode(False, adapters=True)
    assert not m._wide_on and not m._wide_lora and not any(x._wide_lora for x in mods), "no adapters half without the switch"
    assert ops.wide_kwargs(True) == {"wide": True} and ops.wide_kwargs(True, True) == {"wide": True, "wide_lora": True}
    assert ops.wide_kwargs(False, True) == {}
    assert ops._LORA_FUSED in (True, False)
    assert set(ops.LORA_CALLS) == {"small_m", "torch", "m16", "m16_fused"}


def test_register_allocates_t_ws16_and_leaves_t_ws_alone():
    from infinitevl_amd import ops
    t = ops.LoraTable(3, 16, "cpu")
    t.register("p", 600, 520, (0, 300, 600))
    p = t.proj["p"]
    assert tuple(p.t_ws.shape) == (4, ops.LORA_T_LD) and tuple(p.t_ws16.shape) == (16, ops.LORA_T_LD) and p.t_ws16.dtype == BF
    assert p.t_ws16.data_ptr() != p.t_ws.data_ptr()
    ptrs = (p.t_ws.data_ptr(), p.t_ws16.data_ptr(), p.A.data_ptr(), p.B.data_ptr())
    h = t.load({"p": [(torch.ones(4, 520), torch.ones(300, 4)), None]}, 2.0)
    t.unload(h)
    assert ptrs == (p.t_ws.data_ptr(), p.t_ws16.data_ptr(), p.A.data_ptr(), p.B.data_ptr()), "the table's tensors never move"


def test_a_graphed_class_is_stale_after_either_half_of_the_pair_flips():
    from infinitevl_amd.harness import _Graphed

    class Stub(_Graphed):
        def __init__(self, model):
            self.model, self.graph = model, object()
            self._captured_w8, self._captured_fmt = self._w8_on(), self._w8_fmt()
            self._captured_wide, self._captured_wide_lora = self._wide_on(), self._wide_lora_on()
            self._captured_lora = self._lora_sig()

    m = _stack().use_wide_decode(True)
    s = Stub(m)
    assert (s._captured_wide, s._captured_wide_lora) == (True, False) and not s._stale()
    m.use_wide_decode(True, adapters=True)
    assert s._stale(), "the adapters half flipped"
    s2 = Stub(m)
    assert (s2._captured_wide, s2._captured_wide_lora) == (True, True) and not s2._stale()
    m.use_wide_decode(True)
    assert s2._stale() and not s._stale()
    assert _Graphed._captured_wide_lora is False


def test_lora_add_wide_on_cpu_tensors_is_still_the_torch_path():
    from infinitevl_amd import ops
    c = lora16.case(72, 97, (3, 50, 50, 97), 8, 3, "randn")
    t = ops.LoraTable(17, 8, "cpu")
    t.register("p", 97, 72, (3, 50, 50, 97))
    t.proj["p"].A.copy_(c["A"])
    t.proj["p"].B.copy_(c["B"])
    t.scaling.copy_(c["s"])
    idx = dict(lora16.index_patterns(8))["mixed"]
    n0 = dict(ops.LORA_CALLS)
    ya, yb = c["y0"][:8].clone(), c["y0"][:8].clone()
    assert ops.lora_add(ya, c["x"][:8], t, "p", torch.tensor(idx, dtype=torch.int32), wide=True) is ya
    ops.lora_add(yb, c["x"][:8], t, "p", torch.tensor(idx, dtype=torch.int32))
    assert torch.equal(lora.bits(ya), lora.bits(yb)) and not torch.equal(ya, c["y0"][:8])
    assert ops.LORA_CALLS == {**n0, "torch": n0["torch"] + 2}, "nothing on the CPU reaches a kernel"
    # and linear / linear_swiglu with the flag: CPU tensors keep their path
    w = (torch.randn(97, 72, generator=torch.Generator().manual_seed(1)) * 0.1).to(BF)
    kw = dict(lora=(t, "p", torch.tensor(idx, dtype=torch.int32)))
    assert torch.equal(ops.linear(c["x"][:8], w, **kw, **ops.wide_kwargs(True, True)), ops.linear(c["x"][:8], w, **kw))
    assert ops.LORA_CALLS["m16"] == n0["m16"] and ops.LORA_CALLS["m16_fused"] == n0["m16_fused"]

"""CPU: per-row LoRA adapters -- the judges of tests/lora.py, the C ABI's refusals, the adapter table and the model's interface.

  * the builders' conditions hold (asserted from the float64 reference alone) and the honest fp32 emulation of the kernels passes
    the exact-integer probe (index, ties, NORM) and the randn judge in two summation orders, with identical bits on the integers;
  * each of nine wrong emulations is reported by at least one judge;
  * ivl_lora_add_small_m_fwd is declared (the header reader picks its struct up by itself: _lib.ARG_STRUCTS / _lib.LoraArgs, laid out as
    the C compiler lays it out), exported, and refuses what the header says it refuses on a
    machine without a GPU, i.e. before anything is launched;
  * ops.LoraTable: register / load / unload, zero padding, refusals; the torch path of ops.lora_add (CPU tensors, more than 4 rows)
    against the reference chain;
  * InfiniteVLTextStack.enable_adapters / load_adapter (peft key names, prefixes, skipped keys) / merge_adapter_ and
    harness.load_peft_adapter's refusals on a tiny directory.
"""
import ctypes
import json
import os
import subprocess

import pytest
import torch

import lora
import rowwise as rw
from conftest import ROOT

BF = torch.bfloat16

CASES = [dict(K=72, N=257, seg_cols=(3, 100, 250), R=8, rank=3),
         dict(K=8, N=7, seg_cols=(0, 7), R=8),
         dict(K=520, N=600, seg_cols=(5, 101, 203, 301, 399, 501, 595), R=16),
         dict(K=520, N=255, seg_cols=(0, 255), R=64),
         dict(K=512, N=256, seg_cols=(1, 131, 255), R=16, norm=True),
         dict(K=72, N=257, seg_cols=(3, 100, 250), R=8, variant="ties"),
         dict(K=520, N=600, seg_cols=(5, 101, 203, 301, 399, 501, 595), R=16, variant="ties"),
         dict(K=520, N=257, seg_cols=(3, 100, 250), R=16, variant="randn"),
         dict(K=72, N=255, seg_cols=(0, 130, 255), R=8, rank=3, variant="randn")]


@pytest.fixture(scope="module")
def cases():
    return [lora.case(**a) for a in CASES]


def _judge(c, wrong="", order=0):
    run = lambda c_, x, res, y0, idx: lora.emu(c_, x, res, y0, idx, wrong=wrong, order=order)          # noqa: E731
    return (lora.check_randn if c["variant"] == "randn" else lora.check_probe)(run, c)


def test_builder_conditions_hold(cases):
    seen = set()
    for c in cases:
        seen.add((c["variant"], c["norm"]))
        assert tuple(c["A"].shape) == (3, (len(c["seg_cols"]) - 1) * c["R"], c["K"]) and tuple(c["B"].shape) == (3, c["N"], c["R"])
        n_seg, R, r = len(c["seg_cols"]) - 1, c["R"], c["rank"]
        pad = torch.ones(n_seg * R, dtype=torch.bool)
        for i in range(n_seg):
            pad[i * R:i * R + r] = False
        assert not bool(c["A"][:, pad].any()) and not bool(c["B"][:, :, r:].any()), "an adapter of rank r < R is stored zero-padded"
        assert not bool(c["B"][:, lora.segment_of(c) < 0].any())
        if c["variant"] == "randn":
            continue
        assert bool((lora.bits(c["y0"]) == -32768).any()), "-0.0 among the zeros of y0"
        for M in (1, 2, 3, 4):
            for name, idx in lora.index_patterns(M):
                r_ = lora.chain(c, c["xn"][:M], c["y0"][:M], idx)
                assert lora.conditions(c, r_) is None, (c["variant"], M, name)
                assert int(r_["touched"].sum()) == sum(r_["rows"]) * (c["seg_cols"][-1] - c["seg_cols"][0])
    assert seen == {("index", False), ("index", True), ("ties", False), ("randn", False)}
    names = [n for n, _ in lora.index_patterns(4)]
    assert names == ["none", "mixed", "same", "different", "range"]


def test_honest_emulation_passes_in_two_orders_with_identical_bits(cases):
    probed = 0
    for c in cases:
        reps = [_judge(c, order=o) for o in (0, 1)]
        for rep in reps:
            assert rep.ok(), str(rep)
        probed += reps[0].probed
        if c["variant"] != "randn":
            for M in (1, 4):
                for _, idx in lora.index_patterns(M):
                    x, res = (c["x"][:M], c["res"][:M]) if c["norm"] else (c["x"][:M], None)
                    a, b = (lora.emu(c, x, res, c["y0"][:M].clone(), idx, order=o) for o in (0, 1))
                    assert torch.equal(lora.bits(a[0]), lora.bits(b[0])) and torch.equal(lora.bits(a[1]), lora.bits(b[1]))
        else:
            assert reps[0].decided <= lora.WINDOW_MAX * reps[0].judged
    print(f"{len(cases)} cases, {probed} elements bit for bit")
    assert probed > 50000


@pytest.mark.parametrize("wrong", lora.WRONG)
def test_wrong_emulation_is_reported(cases, wrong):
    hits = [(c["variant"], c["K"], c["R"], c["rank"]) for c in cases if not _judge(c, wrong=wrong).ok()]
    print(f"{wrong}: reported in {len(hits)} cases: {hits}")
    assert hits, wrong


def test_rank_padding_equals_the_rank_r_computation_bit_for_bit():
    """zero terms add exactly: the chain on the padded tables is the chain on the rank-3 tables"""
    c = lora.case(K=72, N=255, seg_cols=(0, 130, 255), R=8, rank=3, variant="randn")
    small = dict(c, R=3, A=torch.cat([c["A"][:, :3], c["A"][:, 8:11]], 1), B=c["B"][:, :, :3].contiguous())
    idx = [0, 2, 1, 0]
    a, b = lora.chain(c, c["x"], c["y0"], idx), lora.chain(small, c["x"], c["y0"], idx)
    assert torch.equal(lora.bits(a["y"]), lora.bits(b["y"])) and torch.equal(a["d"], b["d"])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NAME = "ivl_lora_add_small_m_fwd"


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


def test_entry_point_and_struct_are_declared_and_exported(lib, tmp_path):
    import shutil
    from infinitevl_amd import _lib, ops
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NAME in _lib.PROTOTYPES and NAME in exported and hasattr(lib, NAME)
    found = {}
    _lib.parse_header(open(_lib.HEADER_PATH).read(), found)                     # the reader picks the struct up by itself
    assert list(found) == list(_lib.ARG_STRUCTS) == ["ivl_swa_args", "ivl_lora_args", "ivl_sample_args"]
    cls = _lib.ARG_STRUCTS["ivl_lora_args"]
    assert cls is ops.LoraArgs is _lib.LoraArgs and cls.__name__ == "LoraArgs" and found["ivl_lora_args"]._fields_ == cls._fields_
    assert _lib.STRUCTS == {"ivl_swa_args": _lib.SwaArgs, "ivl_sample_args": _lib.SampleArgs}, "the two structs pinned elsewhere"
    assert _lib.PROTOTYPES[NAME] == (ctypes.c_int, [ctypes.POINTER(cls), ctypes.c_void_p])
    names = [n for n, _ in cls._fields_]
    assert names[:6] == ["x", "y", "adapter_idx", "A", "B", "scaling"] and names[-4:] == ["residual", "norm_weight", "eps", "t_ws"]
    offs = [getattr(cls, f"seg_col{i}").offset for i in range(9)]
    assert offs == [offs[0] + 4 * i for i in range(9)], "seg_col0 .. seg_col8 are one int[9]"
    assert lib.ivl_abi_version() == 12 and _lib.IVL_ABI_VERSION == 12
    # sizeof / offsetof against a host C compiler
    hipcc = os.path.realpath(shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(hipcc))
    cc = next(c for c in (shutil.which("cc"), os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"))
              if c and os.path.exists(c))
    lines = ['#include <stdio.h>', '#include "ivl_hip.h"', 'int main(void) {', '  printf("sizeof %zu\\n", sizeof(ivl_lora_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ivl_lora_args, {f}));' for f in names] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER_PATH), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, text=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(cls) == 144 and len(names) == 25
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f


def _args(**kw):
    from infinitevl_amd import ops
    a = ops.LoraArgs()
    p = 0x1000                                                    # never dereferenced: every refusal is decided on the host
    a.x = a.y = a.adapter_idx = a.A = a.B = a.scaling = a.t_ws = p
    a.M, a.N, a.K, a.R, a.n_adapters, a.n_seg = 1, 600, 512, 16, 3, 2
    cols = kw.pop("cols", (0, 300, 600))
    for k, v in kw.items():
        setattr(a, k, v)
    for i in range(9):
        setattr(a, f"seg_col{i}", cols[min(i, len(cols) - 1)])
    return a


def test_refusals_come_before_any_launch(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    fn = getattr(lib, NAME)
    call = lambda **kw: fn(ctypes.byref(_args(**kw)), None)       # noqa: E731
    assert fn(None, None) == INV
    for f in ("x", "y", "adapter_idx", "A", "B", "scaling", "t_ws"):
        assert call(**{f: None}) == INV and b"NULL" in lib.ivl_last_error(), f
    for M in (0, 5, -1):
        assert call(M=M) == UNS and b"1..4 rows" in lib.ivl_last_error()
    for K in (4, 12, 516, 0):
        assert call(K=K) == INV, K
    assert call(N=0) == INV
    for R in (0, 4, 12, 24, 48, 128):
        assert call(R=R) == UNS and b"8, 16, 32 or 64" in lib.ivl_last_error(), R
    for n_seg in (0, 9, -1):
        assert call(n_seg=n_seg) == INV and b"n_seg" in lib.ivl_last_error(), n_seg
    for cols in ((0, 700, 600), (-1, 300, 600), (0, 300, 601), (400, 300, 600)):
        assert call(cols=cols) == INV and b"non-decreasing" in lib.ivl_last_error(), cols
    assert call(n_adapters=0) == INV and b"n_adapters" in lib.ivl_last_error()
    for K in (8, 256, 504, 4104, 8192):
        assert call(K=K, norm_weight=0x1000) == UNS and b"512 <= K <= 4096" in lib.ivl_last_error(), K
    assert call(residual=0x1000) == INV and b"residual without norm_weight" in lib.ivl_last_error()
    assert call(x=0x1008) == INV and b"aligned" in lib.ivl_last_error()


# ---- ops.LoraTable and the torch path of ops.lora_add ------------------------------------------------------------------------------------
def _table(c, through_load=True):
    """the case's three adapters in a LoraTable on the CPU, through load() (the true-rank tensors) or written in place"""
    from infinitevl_amd import ops
    t = ops.LoraTable(c["n_adapters"], c["R"], "cpu")
    t.register("p", c["N"], c["K"], c["seg_cols"])
    n_seg, R, r = len(c["seg_cols"]) - 1, c["R"], c["rank"]
    hs = []
    for a in range(c["n_adapters"]):
        pairs = [(c["A"][a, i * R:i * R + r], c["B"][a, c["seg_cols"][i]:c["seg_cols"][i + 1], :r]) for i in range(n_seg)]
        hs.append(t.load({"p": pairs}, float(c["s"][a])))
    return t, hs


def test_table_load_unload_and_refusals(cases):
    from infinitevl_amd import ops
    c = cases[0]
    t, hs = _table(c)
    assert [h.index for h in hs] == [0, 1, 2] and all(h.rank == 3 for h in hs) and t.handles() == hs
    p = t.proj["p"]
    assert torch.equal(p.A, c["A"]) and torch.equal(p.B, c["B"]) and torch.equal(t.scaling, c["s"]), "zero-padded to R"
    assert tuple(p.t_ws.shape) == (4, ops.LORA_T_LD) and p.t_ws.dtype == BF
    ptrs = (p.A.data_ptr(), p.B.data_ptr(), t.scaling.data_ptr(), p.t_ws.data_ptr())
    with pytest.raises(ValueError, match="taken"):
        t.load({"p": [None, None]}, 1.0)
    t.unload(hs[1])
    assert not bool(p.A[1].any()) and not bool(p.B[1].any()) and float(t.scaling[1]) == 0.0 and t.handles() == [hs[0], hs[2]]
    with pytest.raises(ValueError, match="not loaded"):
        t.unload(hs[1])
    with pytest.raises(ValueError, match="not an adapter loaded"):
        t.index_of(hs[1])
    h = t.load({"p": [(c["A"][1, :3], c["B"][1, 3:100, :3]), None]}, 0.25)          # segment 1 not targeted: zeros
    assert h.index == 1 and not bool(p.B[1, 100:].any()) and torch.equal(p.A[1, :3], c["A"][1, :3])
    assert ptrs == (p.A.data_ptr(), p.B.data_ptr(), t.scaling.data_ptr(), p.t_ws.data_ptr()), "the tensors never move"
    assert t.index_of(None) == -1 and t.index_of(h) == 1
    t.unload(h)
    with pytest.raises(ValueError, match="rank"):
        t.load({"p": [(torch.zeros(9, 72), torch.zeros(97, 9)), None]}, 1.0)
    with pytest.raises(ValueError, match="expected"):
        t.load({"p": [(torch.zeros(3, 72), torch.zeros(96, 3)), None]}, 1.0)
    with pytest.raises(ValueError, match="not registered"):
        t.load({"q": [None]}, 1.0)
    with pytest.raises(ValueError, match="registered already"):
        t.register("p", 8, 8, (0, 8))
    for bad in (dict(n_adapters=0, R=8), dict(n_adapters=2, R=12)):
        with pytest.raises(ValueError):
            ops.LoraTable(device="cpu", **bad)
    t2 = ops.LoraTable(2, 8, "cpu")
    for N, K, cols in ((8, 12, (0, 8)), (8, 8, (0, 9)), (8, 8, (4, 2)), (8, 8, tuple(range(11)))):
        with pytest.raises(ValueError):
            t2.register("x", N, K, cols)
    assert ops.lora_kwargs(None, "p") == {} and ops.lora_kwargs(t, "p") == {"lora": (t, "p", None)}


def test_torch_path_of_lora_add_follows_the_chain(cases):
    """CPU tensors take peft's computation through torch: bf16 GEMMs, so t and d are judged as the randn judge judges them --
    through the reference chain from float64 t within the bound, here simply: close to the float64 chain, untouched bits kept"""
    from infinitevl_amd import ops
    c = next(c_ for c_ in cases if c_["variant"] == "randn")
    t, hs = _table(c)
    n0 = dict(ops.LORA_CALLS)
    for idx in ([0, 2, -1, 1], [-1, -1, -1, -1], [1, 1, 1, 1]):
        y = c["y0"].clone()
        out = ops.lora_add(y, c["x"], t, "p", torch.tensor(idx, dtype=torch.int32))
        assert out is y
        r = lora.chain(c, c["x"], c["y0"], idx)
        assert torch.equal(lora.bits(y)[~r["touched"]], lora.bits(c["y0"])[~r["touched"]])
        ref = c["y0"].double() + torch.where(r["touched"], r["D"] * torch.tensor([float(c["s"][a]) if lora.valid(c, a) else 0.0 for a in idx],
                                                                                dtype=torch.float64)[:, None], torch.zeros(()).double())
        assert bool(((y.double() - ref).abs() <= 2.0 ** -6 * (ref.abs() + r["D"].abs() * 3 + 1.0)).all())
    y = c["y0"].clone()
    ops.lora_add(y, c["x"], t, "p", hs[2])                              # a handle: that adapter for every row
    y2 = c["y0"].clone()
    ops.lora_add(y2, c["x"], t, "p", torch.full((4,), 2, dtype=torch.int32))
    assert torch.equal(lora.bits(y), lora.bits(y2)) and not torch.equal(y, c["y0"])
    x8, y8 = torch.cat([c["x"], c["x"]]), torch.cat([c["y0"], c["y0"]])
    ops.lora_add(y8, x8, t, "p", hs[2])                                 # more than 4 rows
    assert torch.equal(lora.bits(y8[:4]), lora.bits(y8[4:]))
    assert ops.LORA_CALLS["torch"] == n0["torch"] + 6 and ops.LORA_CALLS["small_m"] == n0["small_m"]
    with pytest.raises(ValueError, match="not registered"):
        ops.lora_add(y, c["x"], t, "nope", hs[2])
    with pytest.raises(ValueError, match="got x"):
        ops.lora_add(y[:, :5].contiguous(), c["x"], t, "p", hs[2])


# ---- the model's interface -----------------------------------------------------------------------------------------------------------------
def _stack():
    from infinitevl_amd.harness import InfiniteVLTextConfig, InfiniteVLTextStack
    cfg = InfiniteVLTextConfig(vocab_size=97, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
                               num_attention_heads=4, num_key_value_heads=2, head_dim=16, sliding_window=8,
                               layer_types=["sliding_attention", "linear_attention"], num_linear_heads=4,
                               num_linear_key_value_heads=4, linear_head_dim=16, rope_scaling={"mrope_section": [2, 3, 3]})
    return InfiniteVLTextStack(cfg).to(BF).eval().init_weights_(seed=1).fuse_()


TARGETS = {0: ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"),
           1: ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.g_proj", "self_attn.a_proj", "self_attn.b_proj",
               "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}


def _peft_state(m, r, prefix="base_model.model.model.language_model.", name="", seed=3, skip=()):
    g_ = rw.gen(seed)
    sd = {}
    for i, mods in TARGETS.items():
        for mod in mods:
            if (i, mod) in skip:
                continue
            w = m.get_submodule(f"layers.{i}.{mod}").weight
            sd[f"{prefix}layers.{i}.{mod}.lora_A{name}.weight"] = (torch.randn(r, w.shape[1], generator=g_) * 0.1).to(BF)
            sd[f"{prefix}layers.{i}.{mod}.lora_B{name}.weight"] = (torch.randn(w.shape[0], r, generator=g_) * 0.1).to(BF)
    return sd


def test_enable_and_load_adapter_map_peft_names_onto_the_fused_projections():
    from infinitevl_amd import ops
    m = _stack()
    with pytest.raises(RuntimeError, match="enable_adapters"):
        m.load_adapter({}, alpha=8, rank=4)
    assert m.enable_adapters(2, 8) is m and isinstance(m._lora, ops.LoraTable)
    t = m._lora
    assert set(t.proj) == {(0, "qkv"), (0, "o"), (0, "gu"), (0, "down"), (1, "in"), (1, "o"), (1, "gu"), (1, "down")}
    assert t.proj[(0, "qkv")].seg_cols == (0, 64, 96, 128) and t.proj[(0, "gu")].seg_cols == (0, 96, 192)
    gdn = m.layers[1].self_attn
    assert t.proj[(1, "in")].seg_cols == tuple(gdn._fused_cols) + (gdn._fused_cols[-1] + 4,) and t.proj[(1, "in")].N == gdn._fused_w.shape[0]
    assert all(mod._lora is t for layer in m.layers for mod in (layer.self_attn, layer.mlp))
    sd = _peft_state(m, 4, skip={(0, "self_attn.k_proj")})
    sd["base_model.model.model.visual.blocks.0.attn.qkv.lora_A.weight"] = torch.zeros(4, 8)
    sd["base_model.model.lm_head.lora_B.weight"] = torch.zeros(97, 4)
    h = m.load_adapter(sd, alpha=8, rank=4)
    assert (h.index, h.rank, h.scaling) == (0, 4, 2.0)
    assert sorted(h.skipped) == sorted(["base_model.model.model.visual.blocks.0.attn.qkv.lora_A.weight", "base_model.model.lm_head.lora_B.weight"])
    pre = "base_model.model.model.language_model.layers."
    p = t.proj[(0, "qkv")]
    assert torch.equal(p.A[0, 0:4], sd[pre + "0.self_attn.q_proj.lora_A.weight"]) and not bool(p.A[0, 4:16].any()), "k_proj: zeros"
    assert torch.equal(p.A[0, 16:20], sd[pre + "0.self_attn.v_proj.lora_A.weight"])
    assert torch.equal(p.B[0, 96:128, :4], sd[pre + "0.self_attn.v_proj.lora_B.weight"]) and not bool(p.B[0, 64:96].any())
    p = t.proj[(1, "in")]
    cb = gdn._fused_cols[5]
    assert torch.equal(p.B[0, cb:cb + 4, :4], sd[pre + "1.self_attn.b_proj.lora_B.weight"]) and not bool(p.B[0, cb + 4:].any())
    assert torch.equal(t.proj[(1, "down")].A[0, :4], sd[pre + "1.mlp.down_proj.lora_A.weight"])
    # the legacy prefix, an adapter name in the key, rslora
    h2 = m.load_adapter(_peft_state(m, 8, prefix="base_model.model.model.", name=".default", seed=5), alpha=16, rank=8, use_rslora=True)
    assert (h2.index, h2.rank) == (1, 8) and abs(h2.scaling - 16 / 8 ** 0.5) < 1e-12 and h2.skipped == ()
    with pytest.raises(ValueError, match="taken"):
        m.load_adapter(sd, alpha=8, rank=4)
    m.unload_adapter(h)
    with pytest.raises(ValueError, match="rank"):
        m.load_adapter(sd, alpha=8, rank=16)
    with pytest.raises(ValueError, match="not of rank"):
        m.load_adapter(sd, alpha=8, rank=8)
    with pytest.raises(KeyError, match="only"):
        m.load_adapter({k: v for k, v in sd.items() if "lora_B" not in k or "o_proj" not in k}, alpha=8, rank=4)
    with pytest.raises(KeyError, match="no lora_A"):
        m.load_adapter({"base_model.model.lm_head.lora_A.weight": torch.zeros(4, 64)}, alpha=8, rank=4)
    m.enable_adapters(0)
    assert m._lora is None and all(mod._lora is None for layer in m.layers for mod in (layer.self_attn, layer.mlp))


def test_merge_adapter_is_pefts_merge_and_makes_packed_copies_stale():
    m = _stack().quantize_weights_()
    m.enable_adapters(1, 8)
    sd = _peft_state(m, 4)
    h = m.load_adapter(sd, alpha=8, rank=4)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.merge_adapter_(h) is m
    pre = "base_model.model.model.language_model."
    for i, mods in TARGETS.items():
        for mod in mods:
            A, B = sd[f"{pre}layers.{i}.{mod}.lora_A.weight"], sd[f"{pre}layers.{i}.{mod}.lora_B.weight"]
            want = before[f"layers.{i}.{mod}.weight"] + (B @ A) * 2.0
            assert torch.equal(m.state_dict()[f"layers.{i}.{mod}.weight"], want), (i, mod)
    assert torch.equal(m.state_dict()["embed_tokens.weight"], before["embed_tokens.weight"])
    mlp = m.layers[0].mlp
    with pytest.raises(RuntimeError, match="stale"):
        mlp._w8_down.check(mlp.down_proj.weight)


def test_load_peft_adapter_reads_a_directory_and_refuses_what_is_out_of_scope(tmp_path):
    from safetensors.torch import save_file
    from infinitevl_amd.harness import load_peft_adapter
    m = _stack().enable_adapters(2, 8)
    sd = _peft_state(m, 4)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "adapter_model.safetensors"))
    cfg = dict(peft_type="LORA", r=4, lora_alpha=8, use_rslora=False, use_dora=False, bias="none", modules_to_save=None,
               rank_pattern={}, alpha_pattern={}, target_modules=["q_proj", "v_proj"])

    def write(**kw):
        (tmp_path / "adapter_config.json").write_text(json.dumps({**cfg, **kw}))
    write()
    h = load_peft_adapter(m, str(tmp_path))
    assert (h.index, h.rank, h.scaling, h.skipped) == (0, 4, 2.0, ())
    assert torch.equal(m._lora.proj[(0, "o")].A[0, :4], sd["base_model.model.model.language_model.layers.0.self_attn.o_proj.lora_A.weight"])
    write(use_rslora=True)
    assert load_peft_adapter(m, str(tmp_path)).scaling == 4.0
    for bad, word in ((dict(use_dora=True), "use_dora"), (dict(bias="all"), "bias"), (dict(modules_to_save=["lm_head"]), "modules_to_save"),
                      (dict(rank_pattern={"q_proj": 8}), "rank_pattern"), (dict(alpha_pattern={"q_proj": 8}), "alpha_pattern"),
                      (dict(r=16), "rank capacity"), (dict(peft_type="IA3"), "peft_type")):
        write(**bad)
        with pytest.raises(ValueError, match=word):
            load_peft_adapter(m, str(tmp_path))
    assert len(m._lora.handles()) == 2

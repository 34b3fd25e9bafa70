"""CPU (-m "not gpu"): the host side of the adjustment group -- ivl_sample_adj_args and ivl_sample_rows_adj_fwd as the header
reader finds them, the struct's layout against the host C compiler, the unchanged ABI version and pinned structs, the dynamic
symbol table against the header, every refusal of the entry point on pointers that are never dereferenced; the builders of
tests/adjust.py (both margins, from the reference alone), adjust() on special values; ops.BiasTables, ops.sample_tokens' and
Sampler's new arguments, and what the graphed classes refuse before any device work."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import adjust
import fork as fk
import generation
import sampling
from conftest import ROOT

INF = float("inf")
NAME = adjust.NAME


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_header_yields_the_prototype_and_the_struct(lib, tmp_path):
    from infinitevl_amd import _lib
    found, groups = {}, {}
    _lib.parse_header(open(_lib.HEADER_PATH).read(), found, groups)
    assert list(groups) == list(_lib.GROUP_STRUCTS) == ["ivl_sample_adj_args"], "the reader picks the group up by itself"
    cls = _lib.GROUP_STRUCTS["ivl_sample_adj_args"]
    assert cls is _lib.SampleAdjArgs and cls.__name__ == "SampleAdjArgs" and groups["ivl_sample_adj_args"]._fields_ == cls._fields_
    assert [n for n, _ in cls._fields_] == adjust.ADJ_FIELDS
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert [t for _, t in cls._fields_] == [P, P, P, P, I64, P, P, I64, P, I64, I]
    assert _lib.PROTOTYPES[NAME] == (I, [ctypes.POINTER(_lib.SampleArgs), ctypes.POINTER(cls), P])
    # the change only adds symbols: the version, the pinned structs and the structs an entry point takes first are what they were
    assert lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12
    assert _lib.STRUCTS == {"ivl_swa_args": _lib.SwaArgs, "ivl_sample_args": _lib.SampleArgs}
    assert ctypes.sizeof(_lib.SampleArgs) == 312
    assert list(found) == list(_lib.ARG_STRUCTS) == ["ivl_swa_args", "ivl_lora_args", "ivl_sample_args"]
    # nm -D equals the header
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    declared = re.findall(r"^IVL_API [^\n(]*?\b(ivl_[a-z0-9_]+)\s*\(", open(_lib.HEADER_PATH).read(), flags=re.M)
    assert NAME in declared and exported == set(declared) == set(_lib.EXPORTED_SYMBOLS) and hasattr(lib, NAME)
    # sizeof / offsetof against a host C compiler
    hipcc = os.path.realpath(shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(hipcc))
    cc = next(c for c in (shutil.which("cc"), os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"))
              if c and os.path.exists(c))
    lines = ['#include <stdio.h>', '#include "ivl_hip.h"', 'int main(void) {', '  printf("sizeof %zu\\n", sizeof(ivl_sample_adj_args));']
    lines += [f'  printf("{f} %zu\\n", offsetof(ivl_sample_adj_args, {f}));' for f in adjust.ADJ_FIELDS] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER_PATH), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, text=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(cls) == 88
    for f in adjust.ADJ_FIELDS:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_entry_point_refuses_before_any_launch(lib):
    from infinitevl_amd import _lib
    one, INV = adjust.ONE, _lib.IVL_ERR_INVALID_ARG
    ctl = {"seen": one, "seen_ld": 2}                                  # V = 64: two words
    pen = {"count": one, "count_ld": 64, "freq_penalty": one, "pres_penalty": one, "min_p": one}
    bias = {"bias_idx": one, "bias_mask": one, "bias_mask_ld": 2, "bias_val": one, "bias_ld": 64, "n_bias": 1}

    def refused(word, adj, **kw):
        return adjust.c_refused(lib, INV, word, adj, **kw)

    # count without seen, or with count_ld < V
    assert refused(b"count needs seen", pen)
    assert refused(b"count needs seen", {"count": one, "count_ld": 64})
    assert refused(b"count_ld", {**pen, "count_ld": 63}, **ctl) and refused(b"count_ld", {**pen, "count_ld": 0}, **ctl)
    assert refused(b"count_ld", {**pen, "count_ld": -64}, **ctl)
    # a penalty pointer without count
    assert refused(b"need count", {"freq_penalty": one}, **ctl) and refused(b"need count", {"pres_penalty": one}, **ctl)
    assert refused(b"need count", {"freq_penalty": one, "pres_penalty": one, "count_ld": 64})
    # bias_idx with a table field missing or too small
    assert refused(b"bias_mask", {**bias, "bias_mask": None}) and refused(b"bias_val", {**bias, "bias_val": None})
    assert refused(b"n_bias", {**bias, "n_bias": 0}) and refused(b"n_bias", {**bias, "n_bias": -1})
    assert refused(b"bias_mask_ld", {**bias, "bias_mask_ld": 1}) and refused(b"bias_mask_ld", {**bias, "bias_mask_ld": 0})
    assert refused(b"bias_ld", {**bias, "bias_ld": 63}) and refused(b"bias_ld", {**bias, "bias_ld": -1})
    # score_only with the group, even an empty one
    score = dict(temperature=None, top_k=None, top_p=None, seed=None, counter=None, token=None, token_stride=0, n_top=3,
                 top_ids=one, top_logprobs=one, score_only=1)
    assert refused(b"score_only", {}, **score) and refused(b"score_only", {"min_p": one}, **score)
    assert refused(b"score_only", {**pen, **bias}, **{**ctl, **score})
    # after the existing checks: what ivl_sample_rows_fwd refuses is refused first, under this entry's name
    assert lib.ivl_sample_rows_adj_fwd(None, None, None) == INV and NAME.encode() in lib.ivl_last_error()
    for name in ("logits", "temperature", "top_k", "top_p", "seed", "counter", "token"):
        assert refused(b"NULL", {**pen, **bias}, **{**ctl, name: None}), name
    assert refused(b"rep_penalty needs seen", {**pen, "count_ld": 1}, rep_penalty=one)
    assert refused(b"seen_ld", {**pen, "count_ld": 1}, seen=one, seen_ld=1)
    assert refused(b"n_top", {**bias, "n_bias": 0}, n_top=21, top_ids=one, top_logprobs=one)
    assert refused(b"fsm_state needs fsm_mask", {**bias, "n_bias": 0}, fsm_state=one)
    assert adjust.c_refused(lib, _lib.IVL_ERR_UNSUPPORTED, b"2^23", {**bias, "n_bias": 0}, V=1 << 23, ld=1 << 24)
    # with a NULL group the entry is ivl_sample_rows_fwd under its own name in the message
    assert refused(b"rep_penalty needs seen", None, rep_penalty=one)
    # the group's scalars alone select nothing and are not looked at
    assert refused(b"n_top", {"count_ld": -5, "bias_ld": -5, "bias_mask_ld": -5, "n_bias": -5}, n_top=21, top_ids=one, top_logprobs=one)


# ---------------------------------------------------------------------------------------------
# the helper: adjust() and the builders
# ---------------------------------------------------------------------------------------------
def _bf(vals):
    return torch.tensor(vals, dtype=torch.float32).to(torch.bfloat16)


def test_adjust_special_values_and_operation_order():
    nan = float("nan")
    # the row:           0    1     2    3     4    5     6     7    8     9
    x = _bf([nan, INF, INF, -INF, -INF, 0.0, -0.0, -0.0, 1.0, 1.0])
    seen = np.array([1, 1, 0, 1, 0, 1, 1, 0, 1, 0], dtype=bool)
    count = np.array([1, 1, 7, 1, 7, 1, 1, 7, 1, 7], dtype=np.int32)   # (the 7s sit under clear seen bits)
    got = adjust.adjust(x, seen, count, 0.5, 0.25)
    want = _bf([nan, INF, INF, -INF, -INF, -0.75, -0.75, -0.0, 0.25, 1.0])
    assert adjust.bits(got)[1:].tolist() == adjust.bits(want)[1:].tolist() and torch.isnan(got[0])
    assert adjust.bits(got)[7] == 0x8000, "an untouched -0 keeps its bits"
    # the penalty that sums to zero touches the element all the same: -0 - 0 = -0, +0 - 0 = +0 (IEEE), both the class of zero
    z = adjust.adjust(_bf([-0.0, 0.0]), [True, True], [1, 1], 1.0, -1.0)
    assert adjust.bits(z).tolist() == [0x8000, 0x0000]
    # bias: -inf bans, +inf forces, +inf - inf is a NaN (= -inf), -0 + 0 = +0, a bias on a NaN stays a NaN
    bm = np.ones(6, dtype=bool)
    b = adjust.adjust(_bf([1.0, 1.0, INF, -0.0, nan, -INF]), np.zeros(6, dtype=bool), np.zeros(6, dtype=np.int32), 0.0, 0.0, bm,
                      np.array([-INF, INF, -INF, 0.0, 5.0, INF], dtype=np.float32))
    assert adjust.bits(b)[[0, 1, 3]].tolist() == [0xFF80, 0x7F80, 0x0000] and torch.isnan(b[[2, 4, 5]]).all()
    # (f, p) == (0, 0): the counts are not looked at; a zero count is not penalised; a negative count neither
    same = adjust.adjust(_bf([2.0, 3.0]), [True, True], [5, 5], 0.0, 0.0)
    assert adjust.bits(same).tolist() == adjust.bits(_bf([2.0, 3.0])).tolist()
    assert adjust.adjust(_bf([2.0, 3.0]), [True, True], [0, -3], 1.0, 1.0).tolist() == [2.0, 3.0]
    # c = 2^24 and beyond: (float)c rounds to nearest even, then f * c rounds once, then + p rounds once
    c24 = adjust.adjust(_bf([0.0, 0.0]), [True] * 2, [2 ** 24, 2 ** 24 + 1], 1.0, 0.0)
    assert c24.float().tolist() == [-2.0 ** 24, -2.0 ** 24]
    f = float(np.float32(1e-3))
    for c in (2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 12345):   # RN(RN(f c) + p), not an fma and not float64
        a = np.float32(np.float32(f) * np.float32(c))
        want = np.float32(np.float32(8.0) - np.float32(a + np.float32(0.1)))
        got = adjust.adjust(_bf([8.0]), [True], [c], f, 0.1)
        assert adjust.bits(got)[0] == adjust.bits(torch.tensor([want]).to(torch.bfloat16))[0]
    # negative penalties raise a repeated token
    up = adjust.adjust(_bf([1.0, -2.0]), [True, True], [2, 1], -0.5, -0.25)
    assert up.float().tolist() == [2.25, -1.25]
    # the order: the penalty first, then the bias, one rounding to bf16 at the end (257/256 is not a bf16 value)
    both = adjust.adjust(_bf([1.0]), [True], [1], 0.0, -2.0 ** -8, np.array([True]), np.array([2.0 ** -8], dtype=np.float32))
    assert both.float().tolist() == [1.0078125], "t = 1 + 2^-8 survives in fp32 and the bias lifts it to 1 + 2^-7, a bf16 value"


def test_reference_min_p_and_margins():
    x = _bf([4.0, 3.0, 2.0, 1.0, 4.0, -INF])
    r0 = adjust.reference(x, 1.0, 0, 1.0, 0.0)
    assert r0.n_kept == 6 and r0.minp_margin == INF
    r = adjust.reference(x, 1.0, 0, 1.0, 0.2)                          # e^-1 = 0.37 stays, e^-2 = 0.135 goes
    assert r.P.tolist() == [True, True, False, False, True, False] and r.n_kept == 3
    assert abs(r.Z - (2 + np.exp(-1))) < 1e-12 and r.C[-1] == r.Z
    assert abs(r.minp_margin - (0.2 - np.exp(-2)) / float(np.float32(0.2))) < 1e-6
    one = adjust.reference(x, 1.0, 0, 1.0, 1.0)                        # the top class alone, whatever sits next to it
    assert one.P.tolist() == [True, False, False, False, True, False] and one.minp_margin > 0.5
    g = adjust.reference(x, 0.0, 0, 1.0, 0.5)
    assert g.greedy and g.n_kept == 1 and g.minp_margin == INF         # a greedy row ignores it
    k2 = adjust.reference(x, 1.0, 3, 1.0, 0.5)                         # behind top-k: the classes of P only
    assert k2.P.tolist() == [True, False, False, False, True, False]
    assert not adjust.has_margins(adjust.reference(_bf([0.0, -1.0]), 1.0, 0, 1.0, float(np.exp(-1.0))))


@pytest.mark.parametrize("V", adjust.FIXED_VS)
def test_every_builder_case_has_both_margins(V):
    ops_, mps = adjust.operator_cases(V), adjust.minp_cases(V)
    assert len(mps) == len(sampling.TAUS) * len(adjust.MIN_PS) * len(adjust.KPS) and len(ops_) >= 12
    for c in ops_ + mps + [adjust.special_row()]:
        ref = adjust.reference(adjust.adjusted_row(c), c["tau"], c["k"], c["p"], c["min_p"])
        assert ref.greedy or (ref.margin >= sampling.MARGIN and ref.minp_margin >= adjust.MINP_MARGIN), c["name"]
        assert c["count"].dtype == np.int32 and not (c["count"][~c["seen"]] != 0).any(), c["name"]
    assert {(c["f"] != 0, c["pp"] != 0, c["bias_mask"] is not None) for c in ops_} >= {(True, True, False), (True, False, True),
                                                                                      (False, True, True), (False, False, True)}
    if V > 1:                                                           # the adjustments move the outcome (else the tests show nothing)
        moved = [c for c in ops_ if adjust.bits(adjust.adjusted_row(c)).tolist() != adjust.bits(generation.penalise(c["x"], c["seen"], c["r"])).tolist()]
        assert len(moved) == len(ops_)
        cut = [c for c in mps if adjust.reference(c["x"], c["tau"], c["k"], c["p"], c["min_p"]).n_kept
               < sampling.reference(c["x"], c["tau"], c["k"], c["p"]).n_kept]
        assert len(cut) >= len(mps) // 2


def test_frequency_chain_moves_on():
    x = sampling.random_row(97, 3)
    chain = adjust.frequency_chain(x, 0.5, 0.0, 64)
    assert len(chain) == 64 and len(set(chain)) > 8 and max(chain.count(t) for t in set(chain)) > 1
    assert adjust.frequency_chain(x, 0.0, 0.0, 4) == [chain[0]] * 4


# ---------------------------------------------------------------------------------------------
# ops and Sampler
# ---------------------------------------------------------------------------------------------
def test_bias_tables_load_unload_and_full():
    from infinitevl_amd import ops
    V = 97
    tab = ops.BiasTables("cpu", V, 2)
    assert (tab.n_bias, tab.mask_ld, tab.ld) == (2, 4, V) and tab.mask.dtype == torch.int32 and tuple(tab.mask.shape) == (2, 4)
    assert tab.val.dtype == torch.float32 and tuple(tab.val.shape) == (2, V)
    ptrs = [tab.mask.data_ptr(), tab.val.data_ptr()]
    a = tab.load({0: -INF, 31: 1.5, 32: -2, 96: INF})
    assert a.index == 0 and a.ids == (0, 31, 32, 96) and tab.handles() == [a]
    bits_ = generation.unpack(tab.mask[0].numpy().view(np.uint32))
    assert np.nonzero(bits_)[0].tolist() == [0, 31, 32, 96]
    assert tab.val[0, [0, 31, 32, 96]].tolist() == [-INF, 1.5, -2.0, INF] and tab.val[0].nonzero().numel() == 4
    b = tab.load({5: 1e39})                                            # beyond fp32: +inf, as the cast says
    assert b.index == 1 and tab.val[1, 5].item() == INF and not tab.mask[1, 1:].any()
    with pytest.raises(ValueError, match="taken"):
        tab.load({1: 1.0})
    tab.unload(a)
    assert not tab.mask[0].any() and not tab.val[0].any() and tab.handles() == [b]
    with pytest.raises(ValueError, match="not loaded"):
        tab.unload(a)
    again = tab.load({0: 1.0, 31: 1.0, 32: 1.0, 96: 1.0})              # the same ids in the same place: not the handle that was
    assert again.index == a.index and again.ids == a.ids and again != a
    with pytest.raises(ValueError, match="not loaded"):
        tab.unload(a)
    tab.unload(again)
    c = tab.load({})                                                   # an empty table biases nothing
    assert c.index == 0 and not tab.mask[0].any()
    tab.unload(c)
    for bad in ({V: 1.0}, {-1: 1.0}, {True: 1.0}, {"3": 1.0}, {3: float("nan")}, {3: "x"}, {3: True}, [(3, 1.0)]):
        with pytest.raises(ValueError):
            tab.load(bad)
    assert tab.handles() == [b] and [tab.mask.data_ptr(), tab.val.data_ptr()] == ptrs
    for bad in (dict(vocab_size=0), dict(n_tables=0), dict(n_tables=True)):
        with pytest.raises(ValueError):
            ops.BiasTables("cpu", **{"vocab_size": V, "n_tables": 2, **bad})


def test_ops_check_the_adjustment_arguments():
    from infinitevl_amd import ops
    S, V = 2, 40
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    tab = (torch.zeros(S), torch.zeros(S, dtype=torch.int32), torch.ones(S), torch.zeros(S, dtype=torch.int64),
           torch.zeros(S, dtype=torch.int64))
    seen, count = torch.zeros(S, 2, dtype=torch.int32), torch.zeros(S, V, dtype=torch.int32)
    z, idx = torch.zeros(S), torch.zeros(S, dtype=torch.int32)
    bias = ops.BiasTables("cpu", V, 2)
    assert ops.SAMPLE_ADJ_CALLS == {"adj": 0}
    for name in ("min_p", "freq_penalty", "pres_penalty"):
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, *tab, seen=seen, count=count, **{name: z.double()})
        with pytest.raises(ValueError, match=name):
            ops.sample_tokens(lg, *tab, seen=seen, count=count, **{name: torch.zeros(S + 1)})
    with pytest.raises(ValueError, match="count needs the seen"):
        ops.sample_tokens(lg, *tab, count=count)
    with pytest.raises(ValueError, match="count must be"):
        ops.sample_tokens(lg, *tab, seen=seen, count=count.long())
    with pytest.raises(ValueError, match="count must be"):
        ops.sample_tokens(lg, *tab, seen=seen, count=[[0] * V] * S)
    with pytest.raises(ValueError, match="entries per row"):
        ops.sample_tokens(lg, *tab, seen=seen, count=count[:, :V - 1])
    with pytest.raises(ValueError, match="need count"):
        ops.sample_tokens(lg, *tab, seen=seen, freq_penalty=z)
    with pytest.raises(ValueError, match="need count"):
        ops.sample_tokens(lg, *tab, seen=seen, pres_penalty=z)
    with pytest.raises(ValueError, match="come together"):
        ops.sample_tokens(lg, *tab, bias_idx=idx)
    with pytest.raises(ValueError, match="come together"):
        ops.sample_tokens(lg, *tab, bias=bias)
    with pytest.raises(ValueError, match="bias_idx"):
        ops.sample_tokens(lg, *tab, bias_idx=idx.long(), bias=bias)
    with pytest.raises(ValueError, match="words and"):
        ops.sample_tokens(lg, *tab, bias_idx=idx, bias=ops.BiasTables("cpu", 32, 2))
    holder = types.SimpleNamespace(mask=bias.mask, val=bias.val.double(), n_bias=2, mask_ld=2, ld=V)
    with pytest.raises(ValueError, match="bias.val"):
        ops.sample_tokens(lg, *tab, bias_idx=idx, bias=holder)
    holder = types.SimpleNamespace(mask=bias.mask, val=bias.val, n_bias=3, mask_ld=2, ld=V)
    with pytest.raises(ValueError, match="n_bias"):
        ops.sample_tokens(lg, *tab, bias_idx=idx, bias=holder)
    with pytest.raises(RuntimeError, match="MI355X"):                 # everything checks out: only the device is missing
        ops.sample_tokens(lg, *tab, seen=seen, count=count, min_p=z, freq_penalty=z, pres_penalty=z, bias_idx=idx, bias=bias)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.sample_tokens(lg, *tab, min_p=z)
    assert ops.SAMPLE_ADJ_CALLS == {"adj": 0}, "only a call that reaches the library is counted"


def test_sampler_tensor_counts_validation_and_state():
    from infinitevl_amd.harness import Sampler
    V = 97
    # a sampler built without the two keywords holds exactly the tensors it held
    assert len(Sampler(4, "cpu").row_tensors()) == 11 and len(Sampler(4, "cpu", max_stop=0).row_tensors()) == 10
    plain = Sampler(4, "cpu", vocab_size=V, history=4, logprobs=2)
    assert len(plain.row_tensors()) == 20 and not plain.penalties and plain.biases is None
    assert all(getattr(plain, n) is None for n in ("min_p", "freq_penalty", "pres_penalty", "count", "bias_idx"))
    assert "count" not in plain.state()
    pen = Sampler(4, "cpu", vocab_size=V, penalties=True)
    assert len(pen.row_tensors()) == len(Sampler(4, "cpu", vocab_size=V).row_tensors()) + 4 and pen.bias_idx is None and pen.controlled
    assert [(t.dtype, tuple(t.shape)) for t in (pen.min_p, pen.freq_penalty, pen.pres_penalty, pen.count)] == \
        [(torch.float32, (4,))] * 3 + [(torch.int32, (4, V))]
    assert "count" in pen.state() and "min_p" not in pen.state()
    both = Sampler(4, "cpu", vocab_size=V, history=4, logprobs=2, grammar_states=8, penalties=True, bias_tables=2)
    assert len(both.row_tensors()) == 21 + 5 and both.bias_idx.tolist() == [-1] * 4 and both.bias_idx.dtype == torch.int32
    assert "bias_idx" not in both.state(), "a parameter"
    assert (both.biases.n_bias, both.biases.mask_ld, both.biases.ld) == (2, 4, V)
    only_bias = Sampler(4, "cpu", vocab_size=V, bias_tables=1)
    assert only_bias.count is None and only_bias.min_p is None and only_bias.bias_idx is not None
    for bad in (dict(penalties=True), dict(bias_tables=2), dict(vocab_size=V, penalties=1), dict(vocab_size=V, bias_tables=-1),
                dict(vocab_size=V, bias_tables=True)):
        with pytest.raises(ValueError, match="penalties|bias_tables"):
            Sampler(4, "cpu", **bad)
    # set(): validation
    both.set(1, temperature=0.7, min_p=0.1, frequency_penalty=0.5, presence_penalty=-0.25)
    assert both.min_p.tolist() == [0, float(np.float32(0.1)), 0, 0] and both.freq_penalty.tolist() == [0, 0.5, 0, 0]
    assert both.pres_penalty.tolist() == [0, -0.25, 0, 0]
    both.set(2, min_p=1, frequency_penalty=2)                          # ints are numbers
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(frequency_penalty=INF),
                dict(presence_penalty=float("nan")), dict(min_p="0.1"), dict(frequency_penalty=True), dict(presence_penalty=None)):
        with pytest.raises(ValueError, match="min_p|frequency_penalty|presence_penalty"):
            both.set(0, **bad)
    for bad in (dict(min_p=0.1), dict(frequency_penalty=0.5), dict(presence_penalty=-1.0)):
        with pytest.raises(ValueError, match="penalties=True"):
            plain.set(0, **bad)
        with pytest.raises(ValueError, match="penalties=True"):
            only_bias.set(0, **bad)
    plain.set(0, min_p=0.0, frequency_penalty=0.0, presence_penalty=0)  # the defaults are fine anywhere
    with pytest.raises(TypeError):
        both.set(0, min_q=0.1)
    # the logit bias of a row, and what set() clears
    for who in (plain.load_logit_bias, plain.unload_logit_bias, lambda h: plain.set_logit_bias(0, h), pen.load_logit_bias):
        with pytest.raises(ValueError, match="bias_tables"):
            who(None)
    a, b = both.load_logit_bias({3: -INF}), both.load_logit_bias({5: 2.0, 96: -1.0})
    both.set_logit_bias(1, b)
    both.set_logit_bias(3, a)
    assert both.bias_idx.tolist() == [-1, 1, -1, 0]
    both.count[1, 7] = 3
    both.count[2, 8] = 1
    both.seen[1, 0] = 1 << 7
    st = both.state()
    both.set(1, temperature=0.7)                                       # clears the row's counts and its bias, not its neighbours'
    assert both.bias_idx.tolist() == [-1, -1, -1, 0] and not both.count[1].any() and both.count[2, 8] == 1 and not both.seen[1].any()
    assert both.min_p[1] == 0 and both.freq_penalty[1] == 0 and both.pres_penalty[1] == 0, "parameters go back to their defaults"
    both.load_state(st)
    assert both.count[1, 7] == 3 and both.bias_idx.tolist() == [-1, -1, -1, 0], "state() holds the counts; bias_idx is a parameter"
    both.set_logit_bias(3, None)
    assert both.bias_idx.tolist() == [-1] * 4
    both.unload_logit_bias(a)
    with pytest.raises(ValueError, match="not loaded"):
        both.set_logit_bias(0, a)
    with pytest.raises(ValueError, match="not loaded"):
        both.set_logit_bias(0, "b")
    with pytest.raises(ValueError, match="taken"):
        both.load_logit_bias({1: 1.0})
        both.load_logit_bias({1: 1.0})
    # fork follows the table: the plan copies counts and bias_idx with every other row tensor
    names = [f.name for f in both._fields]
    assert names[-5:] == ["min_p", "freq_penalty", "pres_penalty", "count", "bias_idx"]
    assert [id(t) for t in both.row_tensors()[-5:]] == [id(both.min_p), id(both.freq_penalty), id(both.pres_penalty), id(both.count),
                                                        id(both.bias_idx)]


def test_graphed_classes_refuse_on_the_host():
    from infinitevl_amd.cache import MultiStreamCache
    from infinitevl_amd.harness import GraphedBeamDecode, GraphedMultiStreamDecode, Sampler
    stack, hc = fk.small_stack("cpu")
    V = hc.vocab_size

    def cache():
        return MultiStreamCache(config=hc, n_slots=4, device="cpu", dtype=torch.bfloat16)

    for kw in (dict(penalties=True), dict(bias_tables=1)):
        with pytest.raises(ValueError, match="penalties or bias_tables"):
            GraphedBeamDecode(stack, cache(), 2, V, 16, sampler=Sampler(4, "cpu", vocab_size=V, max_stop=0, history=16, logprobs=4,
                                                                         score_rings=False, **kw))
    x = fk.prompt(hc, 5, 1, "cpu")[0]
    smp = Sampler(4, "cpu", vocab_size=V, penalties=True, bias_tables=2)
    h = smp.load_logit_bias({3: -INF})
    dec = GraphedMultiStreamDecode(stack, cache(), sampler=Sampler(4, "cpu", vocab_size=V, penalties=True))
    for call in (lambda: dec.admit(0, x, logit_bias=h), lambda: dec.admit_n([0, 1], x, logit_bias=h),
                 lambda: dec.load([0], None, logit_bias=h)):
        with pytest.raises(ValueError, match="bias_tables"):
            call()
    dec = GraphedMultiStreamDecode(stack, cache(), sampler=smp)
    with pytest.raises(ValueError, match="penalties=True"):
        GraphedMultiStreamDecode(stack, cache(), sampler=Sampler(4, "cpu", vocab_size=V)).admit(0, x, sampling=dict(min_p=0.2))
    with pytest.raises(ValueError, match="min_p"):
        dec.admit_n([0, 1], x, sampling=[dict(min_p=0.2), dict(min_p=2.0)])
    smp.unload_logit_bias(h)
    with pytest.raises(ValueError, match="not loaded"):
        dec.admit(0, x, logit_bias=h)

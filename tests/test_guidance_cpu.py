"""CPU: guidance on paired rows (ivl_logit_guide_fwd / ivl_rows_follow_fwd, ops.guide_logits / ops.rows_follow,
Sampler(guidance=True)).

  1 the host reference of tests/guidance.py against transformers' ClassifierFreeGuidanceLogitsProcessor in float64, against the
    formula of visual contrastive decoding (up to a constant per row, the cut included), and by hand at the infinities; the
    builders' margin condition and the judge itself;
  2 the header: both prototypes, the ABI version and the struct registries, which this change leaves alone; every refusal code
    through the loaded library, with no GPU;
  3 ops: refusals before the device; Sampler on "cpu": which fields exist when, set_guidance's refusals, fork."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import guidance as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "infinitevl_amd", "libivl_hip.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    import infinitevl_amd
    return infinitevl_amd.load_library()


# ---------------------------------------------------------------------------------------------
# 1. the reference, the builders, the judge
# ---------------------------------------------------------------------------------------------
def _pairs():
    for i, (V, s, beta, un, cn) in enumerate(((1, 1.5, 0.0, 0.0, 0.0), (7, 0.0, 0.0, 0.0, 0.0), (33, 1.0, 0.0, 0.0, 0.0),
                                              (257, 3.0, 0.1, 0.0, 0.0), (1025, 8.0, 0.5, 0.0, 0.0), (513, -2.0, 0.0, 0.0, 0.0),
                                              (300, 1.5, 0.1, 0.0, 0.3), (64, 2.5, 0.999, 0.0, 0.0))):
        yield (V, s, beta) + G.pair_rows(V, 900 + i, s, beta, u_ninf=un, c_ninf=cn)


class _Stub(dict):
    """what UnbatchedClassifierFreeGuidanceLogitsProcessor asks of a model: a call that returns the negative prompt's logits"""

    def __init__(self, logits):
        super().__init__(logits=logits)
        self.logits = logits

    def __call__(self, *a, **kw):
        return self


def test_reference_equals_transformers_cfg_processor_in_float64():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (ClassifierFreeGuidanceLogitsProcessor,
                                                        UnbatchedClassifierFreeGuidanceLogitsProcessor)
    n = 0
    for V, s, beta, c, u, s32, cut in _pairs():
        if beta != 0.0:
            continue                                                     # (HF has no plausibility rule: the VCD test has it)
        both = torch.from_numpy(np.stack([G.bf16_value(c), G.bf16_value(u)]).astype(np.float64))
        ids = torch.zeros(1, 1, dtype=torch.int64)
        # the batched processor is the bare formula on what it is given: HF's generate hands it rows it does not normalise, the
        # unbatched one (guidance_scale with negative_prompt_ids) normalises both rows first -- which is GUIDE-2
        proc = ClassifierFreeGuidanceLogitsProcessor(1.5)
        proc.guidance_scale = float(s32)                                 # (its constructor wants a scale above 1; its formula does not)
        want = proc(ids, torch.log_softmax(both, dim=-1))[0].numpy()
        neg = UnbatchedClassifierFreeGuidanceLogitsProcessor(float(s32), _Stub(both[1:2, None, :]), unconditional_ids=ids)
        want_u = neg(ids, both[0:1])[0].numpy()
        got = G.ref_row(c, u, s32, cut)
        fin = np.isfinite(got)
        for w in (want, want_u):
            assert fin.sum() > 0 and np.abs(got[fin] - w[fin]).max() <= 1e-12 * (1 + np.abs(w[fin]).max()), (V, s)
        assert np.isneginf(got[~fin]).all() and np.isneginf(G.bf16_value(c)[~fin]).all(), "only where the leader is -inf"
        n += 1
    assert n >= 4


def test_reference_is_visual_contrastive_decoding_up_to_a_constant_per_row():
    n_cut = 0
    for V, s, beta, c, u, s32, cut in _pairs():
        alpha = float(s32) - 1.0
        cv, uv = G.bf16_value(c).astype(np.float64), G.bf16_value(u).astype(np.float64)
        with np.errstate(invalid="ignore"):
            cd = (1.0 + alpha) * cv - alpha * uv                         # VCD: cd_logits = (1 + cd_alpha) logits - cd_alpha logits_cd
            cutoff = float(cut) + cv.max()                               #      cutoff = log(cd_beta) + max logits
            cd = np.where(cv < cutoff, -np.inf, cd)                      #      cd_logits.masked_fill(logits < cutoff, -inf)
        got = G.ref_row(c, u, s32, cut)
        assert G.margin_ok(c, cut)
        assert (np.isneginf(got) == (np.isneginf(cd) | np.isneginf(cv))).all(), (V, s, beta)
        fin = np.isfinite(got) & np.isfinite(cd)
        if alpha != 0.0:
            fin &= np.isfinite(uv)
        k = got[fin] - cd[fin]
        assert k.size > 0 and np.ptp(k) <= 1e-9 * (1 + np.abs(cd[fin]).max()), (V, s, beta, np.ptp(k))
        n_cut += bool(beta > 0 and np.isneginf(got).sum() > np.isneginf(cv).sum())
    assert n_cut >= 3, "the cut removed something"


def test_reference_by_hand_at_the_infinities():
    ninf = -np.inf
    bits = lambda *x: G.to_bf16(np.array(x, dtype=np.float64))
    c, u = bits(0.0, 1.0, ninf, 2.0), bits(1.0, ninf, 0.0, 1.0)
    lc = np.array([0.0, 1.0, ninf, 2.0]) - np.log(np.exp([0.0, 1.0, 2.0]).sum())
    lu = np.array([1.0, ninf, 0.0, 1.0]) - np.log(np.exp([1.0, 0.0, 1.0]).sum())
    got = G.ref_row(c, u, 3.0, ninf)
    assert got[2] == ninf, "c(v) = -inf gives -inf"
    assert abs(got[1] - lc[1]) < 1e-14, "u(v) = -inf with c(v) finite gives lc (HF has a NaN there)"
    assert np.allclose(got[[0, 3]], lu[[0, 3]] + 3.0 * (lc - lu)[[0, 3]], rtol=0, atol=1e-14)
    assert np.allclose(G.ref_row(c, u, 0.0, ninf)[[0, 3]], lu[[0, 3]], rtol=0, atol=1e-14) and np.allclose(G.ref_row(c, u, 1.0, ninf)[[0, 3]], lc[[0, 3]])
    # the cut: ln(0.5) = -0.69: 1.0 is 1 below the maximum and goes, the maximum stays even under a cut above 0
    assert np.isneginf(G.ref_row(c, u, 3.0, np.log(0.5))).tolist() == [True, True, True, False]
    assert np.isneginf(G.ref_row(c, u, 3.0, 0.25)).tolist() == [True, True, True, False]
    # all -inf rows
    allninf = bits(ninf, ninf, ninf, ninf)
    assert np.isneginf(G.ref_row(allninf, u, 2.0, ninf)).all() and np.isneginf(G.ref_row(allninf, allninf, 2.0, ninf)).all()
    assert np.allclose(G.ref_row(c, allninf, 2.0, ninf)[[0, 1, 3]], lc[[0, 1, 3]], rtol=0, atol=1e-14)
    # a NaN reads as -inf, in either row
    cn = c.copy()
    cn[0] = np.int16(0x7FC1)
    assert G.ref_row(cn, u, 2.0, ninf)[0] == ninf and np.isfinite(G.ref_row(cn, u, 2.0, ninf)[3])
    # GUIDE-0
    P = np.array([1, -1, 5, 0, 4, 9], dtype=np.int32)
    s = np.array([1, 1, np.inf, 1, 1, 1], dtype=np.float32)
    assert [G.guided(P, s, None, r) for r in range(6)] == [True, False, False, False, False, False]
    assert not G.guided(P, s, np.array([2, 0, 0, 0, 0, 0]), 0)
    assert G.followers(P) == {1: 0, 5: 2} and G.followers(np.array([2, 2, -1, 2], dtype=np.int32)) == {2: 0}
    assert G.followers(np.array([1, 1, -1], dtype=np.int32)) == {1: 0}, "a row that names itself is nobody's leader, and may be a partner"


def test_builders_keep_the_margin_the_span_and_the_scale():
    cases = G.all_cases()
    assert len(cases) == 6 * 6
    n_guided = n_cut = 0
    for k in cases:
        S, V = 6, k["V"]
        want = sorted(k["leaders"])
        assert [r for r in range(S) if G.guided(k["partner"], k["scale"], k["done"], r)] == want
        assert any(G.guided(k["partner"], k["scale"], None, r) for r in range(S) if k["done"][r]), "a row only `done` switches off"
        for r in want:
            c, u = k["bits"][r, :V], k["bits"][k["partner"][r], :V]
            assert abs(float(k["scale"][r])) <= G.MAX_SCALE
            assert G.margin_ok(c, k["cut"][r]), "no element within 2^-16 |cut| below the cut"
            for row in (c, u):
                v = G.bf16_value(row).astype(np.float64)
                fin = np.isfinite(v)
                assert not np.isnan(v).any() and (not fin.any() or v[fin].max() - v[fin].min() <= G.SPAN)   # (a row of V = 1 may be -inf)
            ref = G.ref_row(c, u, k["scale"][r], k["cut"][r])
            n_cut += bool(np.isneginf(ref).sum() > np.isneginf(G.bf16_value(c)).sum())
            n_guided += 1
    assert n_guided == 72 and n_cut >= 20
    # margin_ok does see an element just below the cut
    cut = np.float32(np.log(0.1))
    c = G.to_bf16(np.array([0.0, -3.0]))
    assert G.margin_ok(c, cut) and G.margin_ok(c, np.float32(-np.inf))
    assert not G.margin_ok(G.to_bf16(np.array([0.0, -3.0])), np.float32(-3.0 + 2.0 ** -17))


def test_judge_takes_the_rounded_value_and_its_neighbour_only_at_a_boundary():
    ref = np.array([-1.0, -1.00390625 + 1e-6, -5.5, -np.inf, -2.0])      # -1.00390625 = -1 - 2^-8: a bf16 rounding boundary
    exact = G.to_bf16(ref)
    assert G.judge(exact, ref, 1.0)[0].size == 0
    up = exact.copy()
    up[1] += 1                                                           # the neighbour across the boundary: within E of it
    assert G.judge(up, ref, 1.0)[0].size == 0 and G.judge(up, ref, 1.0)[1] == 1
    off = exact.copy()
    off[2] += 1                                                          # a whole bf16 step at a value far from a boundary
    assert G.judge(off, ref, 1.0)[0].tolist() == [2]
    inf = exact.copy()
    inf[3] = G.to_bf16(np.array([-300.0]))[0]
    assert G.judge(inf, ref, 1.0)[0].tolist() == [3], "an infinity must be an infinity"
    nan = exact.copy()
    nan[4] = np.int16(0x7FC0)
    assert G.judge(nan, ref, 1.0)[0].tolist() == [4]
    fin = exact.copy()
    fin[0] = G.NINF_BITS
    assert G.judge(fin, ref, 1.0)[0].tolist() == [0]
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 ** -130), 0.3])
    assert G.bf16_rne(x).tolist()[:2] == [1.0, 1.0 + 2.0 ** -6] and G.bf16_rne(x)[3] == float(torch.tensor(0.3).bfloat16())


# ---------------------------------------------------------------------------------------------
# 2. the header and the C entry points
# ---------------------------------------------------------------------------------------------
def test_header_declares_both_prototypes_and_leaves_the_structs_and_the_version_alone():
    from infinitevl_amd import _lib
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.PROTOTYPES["ivl_logit_guide_fwd"] == (i, [p, l, i, i, p, p, p, p, p])
    assert _lib.PROTOTYPES["ivl_rows_follow_fwd"] == (i, [p, l, p, p, i, p])
    assert len(_lib.PROTOTYPES["ivl_logit_guide_fwd"][1]) == 9 and len(_lib.PROTOTYPES["ivl_rows_follow_fwd"][1]) == 6
    assert _lib.IVL_ABI_VERSION == 12
    assert sorted(_lib.ARG_STRUCTS) == ["ivl_lora_args", "ivl_sample_args", "ivl_swa_args"]
    assert list(_lib.GROUP_STRUCTS) == ["ivl_sample_adj_args"] and list(_lib.EDIT_STRUCTS) == ["ivl_ban_args"]
    assert _lib.STRUCTS == {"ivl_swa_args": _lib.SwaArgs, "ivl_sample_args": _lib.SampleArgs}
    hdr = open(os.path.join(ROOT, "include", "ivl_hip.h")).read()
    assert all(f"GUIDE-{k}" in hdr for k in range(6)) and "ivl_guide_args" not in hdr


def test_entry_point_refusals_and_export(lib):
    from infinitevl_amd import _lib
    INV, UNS = _lib.IVL_ERR_INVALID_ARG, _lib.IVL_ERR_UNSUPPORTED
    one = 0x1000                                                          # a pointer that is never followed: every call is refused

    def guide(logits=one, ld=64, S=2, V=64, partner=one, scale=one, cut=one, done=None):
        return lib.ivl_logit_guide_fwd(logits, ld, S, V, partner, scale, cut, done, None)

    def follow(token=one, stride=1, done=None, partner=one, S=2):
        return lib.ivl_rows_follow_fwd(token, stride, done, partner, S, None)

    for kw in (dict(logits=None), dict(partner=None), dict(scale=None), dict(cut=None), dict(S=0), dict(V=0), dict(ld=63)):
        assert guide(**kw) == INV and b"ivl_logit_guide_fwd" in lib.ivl_last_error(), kw
    assert guide(V=1 << 23, ld=1 << 23) == UNS and b"2^23" in lib.ivl_last_error()
    assert guide(S=64) == UNS and b"64" in lib.ivl_last_error()
    for kw in (dict(token=None), dict(partner=None), dict(S=0), dict(stride=0)):
        assert follow(**kw) == INV and b"ivl_rows_follow_fwd" in lib.ivl_last_error(), kw
    assert follow(S=64) == UNS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"ivl_logit_guide_fwd", "ivl_rows_follow_fwd"} <= names & set(_lib.EXPORTED_SYMBOLS)
    assert lib.ivl_abi_version() == _lib.IVL_ABI_VERSION == 12


# ---------------------------------------------------------------------------------------------
# 3. ops and the Sampler
# ---------------------------------------------------------------------------------------------
def test_ops_refuse_before_the_device():
    from infinitevl_amd import ops
    S, V = 3, 40
    lg = torch.zeros(S, V, dtype=torch.bfloat16)
    i32, f32 = (lambda n=S: torch.full((n,), -1, dtype=torch.int32)), (lambda n=S: torch.zeros(n, dtype=torch.float32))
    ok = dict(partner=i32(), scale=f32(), cut=f32())
    assert ops.GUIDE_CALLS == {"guide": 0, "follow": 0}
    for kw, word in (({**ok, "partner": i32().long()}, "partner"), ({**ok, "scale": f32().double()}, "scale"),
                     ({**ok, "cut": f32(S + 1)}, "cut"), ({**ok, "done": f32()}, "done"), ({**ok, "partner": None}, "needed"),
                     ({**ok, "scale": torch.zeros(2 * S)[::2]}, "contiguous")):
        with pytest.raises(ValueError, match=word):
            ops.guide_logits(lg, **kw)
    with pytest.raises(ValueError, match="bf16"):
        ops.guide_logits(lg.float(), **ok)
    with pytest.raises(ValueError, match="strides"):
        ops.guide_logits(torch.zeros(S, 2 * V, dtype=torch.bfloat16)[:, ::2], **ok)
    with pytest.raises(ValueError, match="at most 63"):
        ops.guide_logits(torch.zeros(64, 8, dtype=torch.bfloat16), partner=i32(64), scale=f32(64), cut=f32(64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.guide_logits(lg, **ok, done=i32())
    tok = torch.zeros(S, 1, dtype=torch.int64)
    for args, word in (((tok.int(), i32()), "int64"), ((torch.zeros(S, 2, dtype=torch.int64), i32()), "int64"),
                       ((tok, i32(S + 1)), "partner"), ((tok, None), "needed"), ((tok, i32(), f32()), "done")):
        with pytest.raises(ValueError, match=word):
            ops.rows_follow(*args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_follow(tok, i32(), i32())
    assert ops.GUIDE_CALLS == {"guide": 0, "follow": 0}


NEW = ("guide_partner", "guide_scale", "guide_cut")


def test_sampler_fields_exist_exactly_with_guidance():
    from infinitevl_amd.harness import Sampler
    V = 40
    plain = Sampler(4, "cpu", vocab_size=V, history=8, logprobs=2)
    assert len(plain.row_tensors()) == 20 and not plain.guidance and all(getattr(plain, k) is None for k in NEW)
    assert len(Sampler(4, "cpu").row_tensors()) == 11
    smp = Sampler(4, "cpu", vocab_size=V, history=8, logprobs=2, guidance=True)
    assert smp.guidance and len(smp.row_tensors()) == 23 and set(smp.state()) == set(plain.state())
    assert [f.name for f in smp._fields][-3:] == list(NEW) and [f.name for f in Sampler._TABLE][-3:] == list(NEW)
    assert all(f.kw is None for f in smp._fields[-3:]), "none of them is a keyword of ops.sample_tokens"
    assert [(getattr(smp, k).dtype, tuple(getattr(smp, k).shape)) for k in NEW] == [
        (torch.int32, (4,)), (torch.float32, (4,)), (torch.float32, (4,))]
    assert smp.guide_partner.tolist() == [-1] * 4 and smp.guide_scale.tolist() == [1.0] * 4 and torch.isneginf(smp.guide_cut).all()
    assert len(Sampler(2, "cpu", guidance=True).row_tensors()) == 14, "guidance needs no other group"
    with pytest.raises(ValueError, match="bool"):
        Sampler(2, "cpu", guidance=1)
    with pytest.raises(ValueError, match="at most 63"):
        Sampler(64, "cpu", guidance=True)
    with pytest.raises(ValueError, match="guidance=True"):
        plain.set_guidance(0, 1, 1.5)
    with pytest.raises(ValueError, match="guidance=True"):
        plain.clear_guidance(0)


def test_set_guidance_writes_the_row_and_refuses_what_the_kernel_would_switch_off():
    from infinitevl_amd.harness import Sampler
    smp = Sampler(6, "cpu", history=4, guidance=True)
    smp.set_guidance(0, 1, 1.5, plausibility=0.1)
    smp.set_guidance(2, 5, 3, 0.0)
    assert smp.guide_partner.tolist() == [1, -1, 5, -1, -1, -1] and smp.guide_scale.tolist() == [1.5, 1, 3, 1, 1, 1]
    assert smp.guide_cut[0].item() == np.float32(math.log(0.1)) and torch.isneginf(smp.guide_cut[1:]).all()
    assert [smp.guided_role(r) for r in range(6)] == ["leader", "partner", "leader", None, None, "partner"]
    assert smp.leader_of(5) == 2 and smp.leader_of(0) is None
    for args, word in (((3, 4, math.inf), "finite"), ((3, 4, math.nan), "finite"), ((3, 4, 1e39), "finite"),
                       ((3, 4, "2"), "number"), ((3, 4, True), "number"),
                       ((3, 4, 1.5, 1.0), r"\[0, 1\)"), ((3, 4, 1.5, -0.1), r"\[0, 1\)"), ((3, 4, 1.5, math.nan), r"\[0, 1\)"),
                       ((3, 6, 1.5), "partner must be"), ((3, -1, 1.5), "partner must be"), ((3, 3, 1.5), "partner must be"),
                       ((3, 1.0, 1.5), "partner must be"),
                       ((3, 0, 1.5), "leads a pair itself"), ((3, 1, 1.5), "already the partner of row 0"),
                       ((1, 4, 1.5), "is the partner of row 0"), ((6, 4, 1.5), "row must be")):
        with pytest.raises(ValueError, match=word):
            smp.set_guidance(*args)
    assert smp.guide_partner.tolist() == [1, -1, 5, -1, -1, -1] and smp.guide_scale.tolist() == [1.5, 1, 3, 1, 1, 1], "nothing was written"
    smp.set_guidance(0, 1, 2.0)                                           # the same pair again: new numbers
    assert smp.guide_scale[0].item() == 2.0 and torch.isneginf(smp.guide_cut[0]) and smp._partner == {0: 1, 2: 5}
    for src, dsts in ((0, [3]), (1, [3]), (3, [5]), (3, [4, 2])):
        with pytest.raises(ValueError, match="guided pair"):
            smp.fork(src, dsts)
    smp.clear_guidance(2)
    assert smp.guide_partner.tolist() == [1, -1, -1, -1, -1, -1] and smp.guided_role(5) is None
    smp.set_guidance(5, 2, 1.0)                                           # the former partner may lead, the former leader follow
    smp.set(0, temperature=0.7)                                           # a fresh stream in the row: it leads no pair
    assert smp.guide_partner.tolist() == [-1, -1, -1, -1, -1, 2] and smp.guided_role(1) is None and smp._partner == {5: 2}
    saved = smp.state()
    assert not set(saved) & set(NEW), "parameters, not state"
    smp.load_state(saved)

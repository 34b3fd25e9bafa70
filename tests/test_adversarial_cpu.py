"""CPU: the adversarial probes of tests/adversarial.py must BITE.

Each probe's expectation holds for the oracle itself, and each probe reports a deliberately wrong oracle (a band one key too
wide or too narrow, on every row or only on one row in 64; a segment boundary shifted by one; a GDN rule that lets something
pass a wipe token).  The reference-model distances the GPU bounds of probes C and D are derived from are computed and printed
here (pytest -s), so the figures quoted in tests/test_gpu_adversarial.py can be re-derived without a GPU.
"""
import numpy as np
import pytest
import torch

import adversarial as adv
from conftest import rms_rel
from oracle import gdn as ogdn
from oracle import swa as oswa
from oracle import vision as ovis

BF = torch.bfloat16
_TRUE_BOUNDS = oswa.window_bounds


def _lo_minus_1(n_prev, T, W):
    lo, hi = _TRUE_BOUNDS(n_prev, T, W)
    return lo - 1, hi


def _hi_plus_1(n_prev, T, W):
    lo, hi = _TRUE_BOUNDS(n_prev, T, W)
    return lo, hi + 1


def _lo_minus_1_every_64th_row(n_prev, T, W):
    lo, hi = _TRUE_BOUNDS(n_prev, T, W)
    return lo - (np.arange(T) % 64 == 0), hi


def _lo_plus_1(n_prev, T, W):
    lo, hi = _TRUE_BOUNDS(n_prev, T, W)
    return np.minimum(lo + 1, hi), hi


MUTANTS = {"lo-1": _lo_minus_1, "hi+1": _hi_plus_1, "lo-1 on rows i%64==0": _lo_minus_1_every_64th_row}


def _oracle_out(case, **kw):
    """the oracle on the whole call -> [B, T, Hq, d] fp32"""
    out = torch.empty(case.B, case.T, case.Hq, case.d)
    for b in range(case.B):
        for h in range(case.Hq):
            out[b, :, h] = adv.swa_oracle(case, b, h, 0, case.T, **kw)
    return out


# small shapes of every kind of band: growing from an empty ring, partly filled, full with the seam inside, T > C, W = 2, rows
SMALL = [(5, 4, 2, 8, (0,)), (19, 2, 1, 8, (0, 3)), (70, 4, 2, 96, (250,)), (3, 16, 2, 96, (40,)), (130, 2, 1, 64, (40,)),
         (1, 16, 2, 2, (5, 0, 1)), (200, 2, 1, 1024, (3000,)), (2, 4, 2, 96, (0, 94, 95, 96, 302))]


@pytest.mark.parametrize("T,Hq,Hkv,W,seens", SMALL)
def test_band_probe_is_exact_on_the_oracle(T, Hq, Hkv, W, seens):
    for enc in adv.BAND_ENCODINGS:
        case = adv.band_probe(T, Hq, Hkv, W, seens, enc)
        assert adv.band_mismatches(case, _oracle_out(case)) == []
        assert adv.band_mismatches(case, _oracle_out(case).to(BF)) == [], "the bf16 rounding of the output must not move an integer"


def test_band_probe_survives_bf16_at_the_full_window():
    """W = 4096, full ring: 32 .. 33 keys per class; the histogram read from a bf16 output is still exact"""
    for enc in adv.BAND_ENCODINGS:
        case = adv.band_probe(64, 1, 1, 4096, (9000,), enc)
        assert max(c.max() for c in case.extra["counts"]) <= 34
        assert adv.band_mismatches(case, _oracle_out(case).to(BF), heads=[0]) == []


@pytest.mark.parametrize("name", list(MUTANTS))
def test_band_and_needle_probes_report_a_band_one_key_too_wide(name, monkeypatch):
    """T = 130 rows over a full ring of W = 96 (every row has a key in front of its band and, but the last, one behind it)"""
    T, Hq, Hkv, W, seens = 130, 4, 2, 96, (250,)
    probes_a = [adv.band_probe(T, Hq, Hkv, W, seens, enc) for enc in adv.BAND_ENCODINGS]
    outside = adv.needle_probe(T, Hq, Hkv, W, seens, "outside", seed=1)
    refs = [adv.swa_f64(outside, 0, h, 0, T) for h in range(Hq)]
    _, bound = adv.swa_peaked_bound(T, Hq, Hkv, W, seens)
    good = _oracle_out(outside, p_round_dtype=BF).to(BF)
    assert max(float(adv.row_err(refs[h], good[0, :, h]).max()) for h in range(Hq)) < bound
    monkeypatch.setattr(oswa, "window_bounds", MUTANTS[name])
    for case in probes_a:
        bad = adv.band_mismatches(case, _oracle_out(case).to(BF), heads=range(Hq), limit=1000)
        assert bad, (name, case.extra["enc"])
        if "i%64" in name:
            assert all(" row=64 " in m or " row=128 " in m for m in bad), bad[:3]      # row 0 of this call has no key in front
    leak = _oracle_out(outside, p_round_dtype=BF).to(BF)
    worst = max(float(adv.row_err(refs[h], leak[0, :, h]).max()) for h in range(Hq))
    print(f"mutant {name}: needle outside, worst row {worst:.3f} against the bound {bound:.2e}")
    assert worst > 0.5 > bound, (name, worst)


@pytest.mark.parametrize("T,Hq,Hkv,W,seens", [(130, 4, 2, 96, (250,)), (130, 2, 1, 4096, (9000,))])
@pytest.mark.parametrize("name", list(MUTANTS))
def test_outside_needle_reports_a_leak_with_e4m3_operands_too(name, T, Hq, Hkv, W, seens, monkeypatch):
    """The fp8 decode step is judged against the e4m3-operand oracle under adv.fp8_outside_bound (from the outside inputs
    themselves).  A band one key too wide must exceed it -- also at W = 4096, where the key at the other end of the band shares
    the target's code and a leak only halves the row (error about 0.7)."""
    e4m3 = torch.float8_e4m3fn
    outside = adv.needle_probe(T, Hq, Hkv, W, seens, "outside", seed=1)
    m, bound = adv.fp8_outside_bound(outside)
    refs = [adv.swa_oracle(outside, 0, h, 0, T, mma_rounding=e4m3) for h in range(Hq)]
    monkeypatch.setattr(oswa, "window_bounds", MUTANTS[name])
    leak = _oracle_out(outside, mma_rounding=e4m3).to(BF)
    per_row = torch.stack([adv.row_err(refs[h], leak[0, :, h]) for h in range(Hq)], 1)          # [T, Hq]
    print(f"e4m3 mutant {name} W={W}: model {m:.2e} -> bound {bound:.2e}; leaking rows at least {float(per_row[per_row > bound].min()):.2f}")
    assert 0 < bound < 0.2
    hit = per_row > 0.5
    assert int(hit.sum()) >= (2 if "i%64" in name else T // 2), (name, int(hit.sum()))


def test_inside_needle_sweep_aims_at_every_tile_and_split_edge():
    """decode-sized forms: the sweeps of adv.needle_probe aim every row at every one of its candidates (both ends of the band, the seam,
    the first and last key of all 64-key tiles in the four alignments) and stay exact on the oracle"""
    for name in ("packed_T1_W4096_wide", "rows_T4_W4096", "packed_T5_W300", "packed_T1_W2"):
        f = adv.SWA_FORMS[name]
        n = adv.inside_sweeps(f.T, f.Hq, f.W, f.seens)
        hit = [[set() for _ in range(f.T)] for _ in f.seens]
        for s_ in range(n):
            case = adv.needle_probe(f.T, f.Hq, f.Hkv, f.W, f.seens, "inside", seed=2, sweep=s_)
            for b in range(case.B):
                for i in range(f.T):
                    hit[b][i] |= set(case.extra["target"][b, i].tolist())
            if s_ in (0, n - 1) and f.W <= 300:
                assert adv.needle_mismatches(case, _oracle_out(case, p_round_dtype=BF).to(BF), adv.needle_expected(case)) == []
        for b in range(case.B):
            lo, hi = case.bounds_abs(b)
            for i in range(f.T):
                cand, seam = adv._inside_candidates(int(lo[i]), int(hi[i]), case.seens[b], case.first(b), case.C)
                assert set(cand) | set(seam) == hit[b][i], (name, b, i)
                if f.W == 4096 and case.seens[b] >= 4095:
                    tiles = {p for p in range(int(lo[i]), int(hi[i]) + 1) if (p - case.first(b)) % 64 in (0, 63)}
                    assert len(tiles) >= 127 and tiles <= hit[b][i]


def test_needle_probe_is_bit_exact_on_the_oracle_and_reports_a_band_one_key_too_narrow(monkeypatch):
    for T, Hq, Hkv, W, seens in SMALL:
        case = adv.needle_probe(T, Hq, Hkv, W, seens, "inside", seed=2)
        exp = adv.needle_expected(case)
        assert adv.needle_mismatches(case, _oracle_out(case, p_round_dtype=BF).to(BF), exp) == []
        assert adv.needle_mismatches(case, _oracle_out(case), exp) == []
        # e4m3 operands: the needle still wins and the row is v[target] rounded to e4m3
        exp8 = adv.needle_expected(case, torch.float8_e4m3fn)
        assert adv.needle_mismatches(case, _oracle_out(case, mma_rounding=torch.float8_e4m3fn).to(BF), exp8) == []
    case = adv.needle_probe(130, 4, 2, 96, (250,), "inside", seed=3)
    exp = adv.needle_expected(case)
    monkeypatch.setattr(oswa, "window_bounds", _lo_plus_1)
    assert adv.needle_mismatches(case, _oracle_out(case, p_round_dtype=BF).to(BF), exp)


def test_needle_margin_at_the_full_window():
    """W = 4096 over a full ring: the target scores 90.5, nothing else above 45.25 + noise -- measured on the probe itself"""
    case = adv.needle_probe(64, 2, 1, 4096, (9000,), "inside", seed=4)
    q, k, v, n_prev = adv._swa_slab(case, 0, 1, 0, 64)
    s = (q[0, 0].double() @ k[0, 0].double().T) * 128 ** -0.5
    s = s.masked_fill(~torch.from_numpy(oswa.band_mask(n_prev, 64, 4096)), float("-inf"))
    top2 = s.topk(2, dim=-1).values
    print(f"needle at W=4096: best {float(top2[:, 0].min()):.2f}, runner-up at most {float(top2[:, 1].max()):.2f}")
    assert float(top2[:, 0].min()) == pytest.approx(90.51, abs=0.01) and float(top2[:, 1].max()) < 49.0
    exp = adv.needle_expected(case)
    assert adv.needle_mismatches(case, _oracle_out(case, p_round_dtype=BF).to(BF), exp) == []


def test_present_style_of_check_does_not_notice_one_extra_key_on_one_row_in_64(monkeypatch):
    """The record of why the probes were needed: randn inputs at W = 4096 over a full ring, T = 256, the band one key too wide on
    the rows i % 64 == 0 only.  Tensor rms_rel < 5e-3 and per-row < 4e-2 (the suite's bounds) both pass on the WRONG result:
    measured rms_rel 8.1e-4 and worst row 1.7e-2 (printed below); the band probe reports rows 64, 128 and 192 of the same call."""
    T, Hq, Hkv, W, seens = 256, 2, 1, 4096, (9000,)
    case = adv.peaked_probe(T, Hq, Hkv, W, seens, seed=0, q_scale=1.0)            # q_scale 1: the suite's plain randn data
    good = _oracle_out(case)
    probe = adv.band_probe(T, Hq, Hkv, W, seens, "fine")
    monkeypatch.setattr(oswa, "window_bounds", _lo_minus_1_every_64th_row)
    wrong = _oracle_out(case)
    e_rms = rms_rel(good, wrong)
    e_row = float(adv.row_err(good, wrong).max())
    print(f"one extra key on rows i%64==0 at W=4096, randn data: tensor rms_rel {e_rms:.2e} (bound 5e-3), worst row {e_row:.2e} (bound 4e-2)")
    assert 0 < e_rms < 5e-3 and 0 < e_row < 4e-2, (e_rms, e_row)
    bad = adv.band_mismatches(probe, _oracle_out(probe).to(BF), heads=[0], limit=10)
    assert len(bad) == 3 and all(f" row={i} " in m for i, m in zip((64, 128, 192), bad)), bad


def test_launch_form_table_follows_the_dispatch_rules():
    for f in adv.SWA_FORMS.values():
        assert adv.swa_dispatch(f.B, f.T, f.Hq, f.Hkv, f.W, f.kernel == "ring256", f.kernel == "fp8", f.rows) == (f.kernel, f.nsplit), f.name
        if f.kernel == "ring256":
            assert min(f.seens) >= f.W - 1 and f.T % 256 == 0 and f.B * f.Hq * f.T // 256 >= 256, f.name
    kinds = {(f.kernel, f.nsplit > 16, min(f.nsplit, 16) if f.kernel in ("prefill", "64row") else 0) for f in adv.SWA_FORMS.values()}
    for want in [("packed", True, 0), ("packed", False, 0), ("fp8", True, 0), ("fp8", False, 0), ("rows", True, 0), ("rows", False, 0),
                 ("64row", False, 1), ("64row", False, 4), ("64row", False, 8), ("64row", False, 16), ("prefill", False, 1),
                 ("prefill", False, 4), ("prefill", False, 8), ("prefill", False, 16), ("ring256", False, 0)]:
        assert want in kinds, want


@pytest.mark.parametrize("name", ["packed_T3_W96_partly", "64row_T40_W96_seam", "prefill_T256_s1", "rows_T2_W96"])
def test_ring_layout_matches_the_cache_oracle(name):
    """SwaCase.ring / ring_after against oracle.cache's ring append (slot p % C, the last C tokens survive)"""
    f = adv.SWA_FORMS[name]
    case = adv.peaked_probe(f.T, f.Hq, f.Hkv, f.W, f.seens, seed=5)
    before, after = case.ring("k", 7.0), case.ring_after("k", 7.0)
    for b in range(case.B):
        seen, C = case.seens[b], case.C
        for p in range(case.first(b), seen):
            assert torch.equal(before[b, :, p % C], case.k_loc[b][p - case.first(b)])
        for p in range(max(case.first(b), seen + f.T - C), seen + f.T):
            assert torch.equal(after[b, :, p % C], case.k_loc[b][p - case.first(b)]), (b, p)
        untouched = [s for s in range(C) if s not in {(seen + t) % C for t in range(f.T)}]
        assert torch.equal(after[b][:, untouched], before[b][:, untouched])


# ---- vision -----------------------------------------------------------------------------------------------------------------
V_SMALL = (0, 1, 63, 64, 65, 0, 129, 200)


@pytest.mark.parametrize("d,H", [(64, 2), (80, 3), (128, 2)])
def test_vision_probes_hold_on_the_oracle_and_report_a_shifted_segment_boundary(d, H):
    cu = adv._cu(V_SMALL)
    shifted = list(cu)
    shifted[4] += 1                                     # the boundary between the 64- and the 65-patch segment
    for enc in adv.BAND_ENCODINGS:
        case = adv.vision_band_probe(V_SMALL, H, d, enc)
        out = ovis.segment_attention(case.q, case.k, case.v, cu, p_round_dtype=BF).to(BF)
        assert adv.vision_band_mismatches(case, out) == []
        bad = adv.vision_band_mismatches(case, ovis.segment_attention(case.q, case.k, case.v, shifted, p_round_dtype=BF).to(BF), limit=10 ** 6)
        # every patch of the two segments on every head (patch 128 can tie in ONE encoding: 64..128 and 128..192 share a fine histogram at d = 64)
        assert len(bad) >= (64 + 64) * H, (enc, len(bad))
    inside = adv.vision_needle_probe(V_SMALL, H, d, "inside", seed=d)
    exp = adv.vision_needle_expected(inside)
    assert adv.vision_needle_mismatches(inside, ovis.segment_attention(inside.q, inside.k, inside.v, cu, p_round_dtype=BF).to(BF), exp) == []
    assert adv.vision_needle_mismatches(inside, ovis.segment_attention(inside.q, inside.k, inside.v, shifted, p_round_dtype=BF).to(BF), exp)
    outside = adv.vision_needle_probe(V_SMALL, H, d, "outside", seed=d)
    _, bound = adv.vision_peaked_bound(V_SMALL, H, d)
    good = adv.vision_row_report(outside, ovis.segment_attention(outside.q, outside.k, outside.v, cu, p_round_dtype=BF).to(BF))
    rep = adv.vision_row_report(outside, ovis.segment_attention(outside.q, outside.k, outside.v, shifted, p_round_dtype=BF).to(BF))
    print(f"vision d={d}: needle outside, bound {bound:.2e}; oracle {good['kernel']:.2e}; shifted boundary: worst row {rep['kernel']:.3f}")
    assert good["kernel"] < bound and rep["kernel"] > 0.5 > bound


# ---- probes C and D: the reference model's own distances (the figures behind the GPU bounds) -------------------------------------
def test_peaked_softmax_model_distances_are_printed_and_usable():
    """Per launch form: the largest per-row distance of the oracle's bf16 model (fp8 forms: of its e4m3-operand model) from the
    float64 result on the probe C inputs of that form, and the bound the kernel gets from it."""
    worst = 0.0
    for f in adv.SWA_FORMS.values():
        if f.T > 1100:
            continue                                    # the two longest forms: same rule, computed in the GPU test (seconds there)
        m, bound = adv.swa_peaked_bound(f.T, f.Hq, f.Hkv, f.W, f.seens, fp8=f.kernel == "fp8")
        print(f"probe C {f.name}: model vs float64, worst row {m:.2e} -> kernel bound {bound:.2e}")
        assert m > 0
        if f.kernel != "fp8":
            worst = max(worst, m)
    assert worst < adv.ROW_BOUND_CAP / 2, "twice the bf16 model's distance stays under the suite's per-row bound"
    for d, H in ((64, 2), (80, 3), (128, 2)):
        m, bound = adv.vision_peaked_bound(V_SMALL, H, d)
        print(f"probe C vision d={d}: model vs float64, worst row {m:.2e} -> kernel bound {bound:.2e}")
        assert 0 < m < adv.ROW_BOUND_CAP / 2


@pytest.mark.parametrize("c", adv.GDN_CASES, ids=adv.gdn_case_id)
def test_gdn_case_model_distances_and_share_of_absolutely_judged_slices(c):
    """From the reference alone: per (batch, head, chunk) distance of the oracle's rounding model from the float64 rule, and how
    many slices have a reference RMS so small that they are judged absolutely (must stay under 10 %)."""
    x = adv.gdn_case_inputs(c)
    ref_o, ref_s = adv.gdn_f64(x["q"], x["k"], x["v"], x["g"], x["beta"], x["h0"])
    mo, ms = adv.gdn_model(x, c[7], fp8=c[6] == "fp8")
    r = adv.gdn_slice_verdict(ref_o, ref_s, mo, ms)
    print(f"probe D {adv.gdn_case_id(c)}: model vs float64 worst slice {r['model_max']:.2e}; {r['absolute']} of {r['slices']} slices absolute")
    assert r["absolute"] < 0.1 * r["slices"], r
    assert torch.isfinite(mo).all() and torch.isfinite(ms).all()
    # the verdict bites: an error of 3 % (e4m3 operands, whose own model sits 4e-2 off: 20 %) in one chunk of one head -- invisible
    # in the whole-tensor RMS of a long call -- fails it
    wrong = mo.clone()
    wrong[0, -40:, 1] *= 1.2 if c[6] == "fp8" else 1.03
    assert adv.gdn_slice_verdict(ref_o, ref_s, mo, ms, wrong, ms)["worst"] > 1.0
    assert adv.gdn_slice_verdict(ref_o, ref_s, mo, ms, mo, ms)["worst"] < 1.0


def test_gdn_repeated_key_closed_form():
    """one key, beta = 1, g = 0, h0 = 0: S_t = k_hat v_t^T and o_t = scale (q_hat_t . k_hat) v_t, in float64"""
    x = adv.gdn_case("repeat", 1, 130, 2, seed=3)
    o, s = adv.gdn_f64(x["q"], x["k"], x["v"], x["g"], x["beta"], None)
    qh = x["q"].double() / torch.sqrt((x["q"].double() ** 2).sum(-1, keepdim=True) + 1e-6)
    kh = x["k"].double() / torch.sqrt((x["k"].double() ** 2).sum(-1, keepdim=True) + 1e-6)
    closed = 128 ** -0.5 * (qh * kh).sum(-1, keepdim=True) * x["v"].double()
    assert rms_rel(closed, o) < 1e-5                    # |k_hat|^2 = 1 - eps / |k|^2
    assert rms_rel(torch.einsum("bhk,bhv->bhkv", kh[:, -1], x["v"][:, -1].double()), s) < 1e-5
    o32, _ = ogdn.gdn_recurrent(x["q"], x["k"], x["v"], x["g"], x["beta"])
    oc, _ = ogdn.gdn_chunk(x["q"], x["k"], x["v"], x["g"], x["beta"])
    assert rms_rel(closed, o32) < 1e-4 and rms_rel(closed, oc) < 1e-3


@pytest.mark.parametrize("wipe_at", [64, 65, 95, 127, 195])
def test_gdn_wipe_token_property_holds_on_the_oracle_and_catches_a_leak(wipe_at):
    """T = 200 (ragged last chunk of 8): chunk offsets 0, 1, 31, 63 and inside the ragged chunk.  Outputs from the wipe token on
    and the final state are bit-identical for two h0 and two prefixes, in the recurrent rule and in the chunk rule with the
    reference's bf16 rounding points and with e4m3 operands; a rule whose decay underflows later (g = -80 instead of -200:
    e^-80 is still a number) is caught."""
    a, b = adv.gdn_wipe_pair(1, 200, 2, wipe_at, seed=wipe_at)
    assert not torch.equal(a["q"][:, :wipe_at], b["q"][:, :wipe_at]) and torch.equal(a["q"][:, wipe_at:], b["q"][:, wipe_at:])
    for mode, fp8 in (("recurrent", False), ("chunk", False), ("chunk", True)):
        (oa, sa), (ob, sb) = adv.gdn_model(a, mode, fp8), adv.gdn_model(b, mode, fp8)
        assert torch.isfinite(oa).all() and torch.isfinite(sa).all()
        assert torch.equal(oa[:, wipe_at:], ob[:, wipe_at:]) and torch.equal(sa, sb), (mode, fp8)
        assert not torch.equal(oa[:, :wipe_at], ob[:, :wipe_at])
    for x in (a, b):
        x["g"][:, wipe_at] = -8.0
    (oa, sa), (ob, sb) = adv.gdn_model(a, "chunk"), adv.gdn_model(b, "chunk")
    assert not torch.equal(oa[:, wipe_at:], ob[:, wipe_at:])


def test_gdn_still_state_comes_back_bit_equal_on_the_oracle():
    x = adv.gdn_case("still", 1, 130, 2, seed=5)
    for mode in ("recurrent", "chunk"):
        _, s = adv.gdn_model(x, mode)
        assert torch.equal(s, x["h0"]), mode

"""CPU: the probes and judges of tests/projections.py must BITE, and must not bite an honest kernel.

  * the case list reaches every one of the 60 linear_small_m_kernel instantiations, every tail N and every K the kernels branch at;
  * every builder's conditions hold for every listed case and every M it is run at: at most 1 % of the exact sums above 256 (index
    variant), at least 10 % exact bf16 ties and nothing from 2^11 (ties variant), the silu window share (GLU), every |logit| <= 256
    (SCORE), and the +-w[k] identity of the NORM probe in float64;
  * an honest fp32 emulation passes every judge, summing in two different orders -- and the two orders agree BIT FOR BIT, which is
    the whole point of the probe: integer sums below 2^24 do not depend on the order;
  * each of eleven deliberately wrong emulations is reported in at least one listed case.
"""
import pytest
import torch

import projections as pj
import rowwise as rw

BF = torch.bfloat16


def _build(glu, norm, N, K, Ms, variant):
    return pj.norm_case(N, K, glu, Ms) if norm else pj.int_case(4, N, K, glu, variant, Ms)


def _lin(wrong="", order=0):
    return lambda x, w, bias, glu: pj.emu_linear(x, w, bias, glu, wrong, order)


def _norm(wrong="", order=0):
    return lambda x, res, nw, eps, w, bias, glu: pj.emu_norm_linear(x, res, nw, eps, w, bias, glu, wrong, order)


def _score(wrong="", order=0):
    return lambda x, w, bias, target: pj.emu_score(x, w, bias, target, wrong, order)


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)
    return rep


# ---- the lists -------------------------------------------------------------------------------------------------------------------
def test_case_list_reaches_all_60_instantiations_and_every_listed_shape():
    assert len(pj.ALL_INSTANTIATIONS) == 60 and sum(1 for i in pj.ALL_INSTANTIATIONS if i[3]) == 40
    reached = {pj.instantiation(M, N, K, glu, norm) for glu, norm, N, K, Ms, _ in pj.SMALL_M for M in Ms}
    assert reached == pj.ALL_INSTANTIATIONS, sorted(pj.ALL_INSTANTIATIONS - reached)
    for norm, Ks in ((False, pj.K_PLAIN), (True, pj.K_NORM)):
        for glu, N in pj.TAILS:
            mine = [(K, Ms) for g, n, N_, K, Ms, v in pj.SMALL_M if (g, n, N_, v) == (glu, norm, N, "index")]
            assert all(1 in Ms and 4 in Ms for _, Ms in mine), "every tail at M = 1 and M = 4"
            assert {K for K, _ in mine} >= {K for K in Ks if K <= 2048}, (glu, norm, N)
        for K in Ks:                                        # a K above 2048 meets every rows-per-wave
            rpw = {pj.instantiation(1, N, K, g, n)[1] for g, n, N, K_, _, v in pj.SMALL_M if K_ == K and n == norm and v == "index"}
            assert rpw == {1, 2, 4}, (norm, K, rpw)
    assert all(K >= 64 for g, n, N, K, Ms, v in pj.SMALL_M if v == "ties")
    assert max((2 * N if glu else N) * K * 2 for glu, _, N, K, _, _ in pj.SMALL_M if K <= 520) < 9.5e6
    for lst, Ns in ((pj.M256_PLAIN, (4, 60, 64, 68, 100)), (pj.M256_GLU, (4, 44, 48, 52, 100))):
        assert {K for _, _, K in lst} == {64, 128, 192, 256, 2048}
        assert all(sum(1 for M_, _, _ in lst if M_ == M) >= 2 for M in (1, 31, 33, 255, 256))
        assert all({(N, 192), (N, 2048)} <= {(N_, K) for _, N_, K in lst} for N in Ns)
    assert {M for M, _, _ in pj.SCORE} == {1, 33, 256} and {N for _, N, _ in pj.SCORE} == {4, 64, 68, 4100}
    assert pj.instantiation(3, 8192, 2048, False, True) == (3, 4, False, True, 1)
    assert pj.instantiation(1, 4095, 2056, True, True) == (1, 1, True, True, 2)


def test_helpers():
    v = torch.tensor([255.0, 256.0, 257.0, 258.0, 511.0, 513.0, 514.0, 516.0, -1026.0, 1028.0, 1032.0, 0.0, 0.5], dtype=torch.float64)
    assert pj.is_tie(v).tolist() == [False, False, True, False, True, False, True, False, False, True, False, False, False]
    assert [float(rw.round_bf16(torch.tensor([s], dtype=torch.float64))) for s in (257.0, 259.0, 514.0, 518.0)] == [256.0, 260.0, 512.0, 520.0]
    x, w = torch.randn(3, 40).to(BF), torch.randn(5000, 40).to(BF)
    assert torch.equal(pj.exact_sum(x, w), x.double() @ w.double().T)
    t = pj.ternary(64, 4096, 0.25, rw.gen(1))
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and abs(float((t != 0).float().mean()) - 0.25) < 0.01
    st, new = torch.arange(24.0).view(2, 3, 4), -torch.ones(2, 3)
    assert pj.conv_shift_ref(st, new)[1, 2].tolist() == [21.0, 22.0, 23.0, -1.0]


# ---- the builders' conditions, for every listed case -------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
def test_small_m_cases_meet_the_probes_conditions(norm):
    """(the builders assert them while they pick the seed; here they are evaluated once more, per M of every case, and printed)"""
    worst_big, least_ties, most_window = 0.0, 1.0, 0.0
    for glu, n, N, K, Ms, variant in pj.SMALL_M:
        if n != norm:
            continue
        c = _build(glu, n, N, K, Ms, variant)
        assert c["x"].abs().max() <= (200 if variant == "ties" else 3) and bool(((c["w"] == 0) | (c["w"].abs() == 1)).all())
        assert bool(torch.isfinite(c["S"]).all()) and bool((c["S"] == c["S"].round()).all())
        for M in Ms:
            assert pj.conditions(c, M) is None, (glu, n, N, K, M, variant, pj.conditions(c, M))
            v = c["S"][:M] + c["bias"].double()
            if variant == "ties":
                least_ties = min(least_ties, float(pj.is_tie(v).double().mean()))
            else:
                worst_big = max(worst_big, float((v.abs() > 256).double().mean()))
            if glu:
                most_window = max(most_window, rw.silu_ref(rw.round_bf16(v).to(BF))["share"])
                assert 3.0 < float(c["S"][:, :N].std()) < 9.0, "the gate rows stay in silu's curved range"
        if norm:
            assert set(c["h"].unique().tolist()) == {-1.0, 1.0} and float(c["nw"].abs().max()) == 4.0
            assert torch.equal((c["x"].float() + c["res"].float()).to(BF), c["h"])
    print(f"norm={norm}: largest share above 256: {worst_big:.5f}; least tie share {least_ties:.3f}; largest silu window share {most_window:.5f}")


def test_m256_and_score_cases_meet_the_probes_conditions():
    for glu, lst in ((False, pj.M256_PLAIN), (True, pj.M256_GLU)):
        for M, N, K in lst:
            for variant in ("index",) if glu else ("index", "ties"):
                assert pj.conditions(pj.int_case(M, N, K, glu, variant), M) is None
    tied = 0
    for M, N, K in pj.SCORE:
        c = pj.score_case(M, N, K)
        assert pj.conditions(c, M) is None and float((c["S"] + c["bias"].double()).abs().max()) <= 256.0
        t = c["target"]
        assert bool(((t >= 0) & (t < N) | (t == -100)).all())
        if M >= 5:
            assert {0, N - 1, (N - 1) // 64 * 64, -100} <= set(t.tolist())
        tied += int(((c["S"] == c["S"].max(1, keepdim=True).values).sum(1) > 1).sum())
    assert tied > 100, "ties for the row maximum must be common"
    print(f"rows whose maximum is attained more than once: {tied}")


# ---- an honest emulation passes, in either summation order, with the same bits ---------------------------------------------------------
def _modest(glu, N, K):
    return (2 * N if glu else N) * K <= 2.5e6


def test_honest_emulation_passes_every_judge_in_two_summation_orders():
    probed = 0
    for glu, norm, N, K, Ms, variant in pj.SMALL_M:
        if not _modest(glu, N, K):
            continue
        c = _build(glu, norm, N, K, Ms, variant)
        for order in (0, 1):
            rep = pj.check_norm_linear(_norm(order=order), c, Ms) if norm else pj.check_linear(_lin(order=order), c, Ms)
            assert rep.ok(), str(rep)
            probed += rep.probed
        xx = c["xn"] if norm else c["x"]
        assert torch.equal(pj._fp32_sums(xx, c["w"], 0), pj._fp32_sums(xx, c["w"], 1)), "integer sums do not depend on the order"
        assert torch.equal(pj._fp32_sums(xx, c["w"], 0).double(), c["S"])
    for glu, lst in ((False, pj.M256_PLAIN), (True, pj.M256_GLU)):
        for M, N, K in lst:
            for variant in ("index",) if glu else ("index", "ties"):
                c = pj.int_case(M, N, K, glu, variant)
                for order in (0, 1):
                    rep = pj.check_linear(_lin(order=order), c, (M,))
                    assert rep.ok(), str(rep)
                    probed += rep.probed
    worst = 0.0
    for M, N, K in pj.SCORE:
        c = pj.score_case(M, N, K)
        for order in (0, 1):
            rep = pj.check_score(_score(order=order), c)
            assert rep.ok(), str(rep)
            worst = max(worst, rep.worst)
    print(f"{probed} elements bit for bit; largest scoring.judge ratio of the emulation {worst:.3f}")


def test_honest_emulation_passes_the_randn_judge():
    for glu, N, K in ((False, 7, 520), (True, 5, 2056), (False, 4099, 136), (True, 4097, 136)):
        _passes(pj.check_randn(_lin(), pj.randn_case(4, N, K, glu), (1, 4)))


# ---- the wrong emulations are reported --------------------------------------------------------------------------------------------
def _reported(wrong, variant=None):
    """the listed cases (modest sizes) in which the wrong emulation is reported"""
    hits = []
    if wrong in pj.WRONG_NORM:
        for glu, norm, N, K, Ms, v in pj.SMALL_M:
            if norm and _modest(glu, N, K) and K <= 520:
                if not pj.check_norm_linear(_norm(wrong), _build(glu, norm, N, K, Ms, v), Ms).ok():
                    hits.append((glu, N, K))
        return hits
    if wrong == "top1_highest":
        return [s for s in pj.SCORE if not pj.check_score(_score(wrong), pj.score_case(*s)).ok()]
    for glu, norm, N, K, Ms, v in pj.SMALL_M:
        if norm or not _modest(glu, N, K) or (variant and v != variant) or (wrong in pj.WRONG_GLU and not glu):
            continue
        if v == "index" and K not in (8, 520, 4104):      # (three K per tail are plenty here; the ties cases all run)
            continue
        if not pj.check_linear(_lin(wrong), _build(glu, norm, N, K, Ms, v), Ms).ok():
            hits.append((glu, N, K, v))
    for glu, lst in ((False, pj.M256_PLAIN), (True, pj.M256_GLU)):
        for M, N, K in lst:
            v = variant or "index"
            if (glu and (v == "ties")) or (wrong in pj.WRONG_GLU and not glu):
                continue
            if not pj.check_linear(_lin(wrong), pj.int_case(M, N, K, glu, v), (M,)).ok():
                hits.append((glu, M, N, K, v))
    return hits


@pytest.mark.parametrize("wrong", [w for w in pj.WRONG_LINEAR if w != "truncate"] + list(pj.WRONG_GLU) + list(pj.WRONG_NORM) + ["top1_highest"])
def test_wrong_emulation_is_reported(wrong):
    hits = _reported(wrong)
    print(f"{wrong}: reported in {len(hits)} cases, e.g. {hits[:3]}")
    assert hits, wrong
    if wrong in ("drop_last_piece", "double_last_piece", "bias_prev", "swap_rows", "tail_clamped"):
        assert any(len(h) == 4 for h in hits) and any(len(h) == 5 for h in hits), "in a small-M case and in a 256-row case"


def test_truncation_is_seen_by_the_ties_variant_only():
    """below 256 every integer is a bf16 value: the index variant cannot tell one rounding rule from another; the ties variant must,
    in EVERY one of its cases"""
    assert _reported("truncate", "index") == []
    ties = [c for c in pj.SMALL_M if c[5] == "ties"]
    hits = _reported("truncate", "ties")
    assert len([h for h in hits if len(h) == 4]) == len(ties) and len([h for h in hits if len(h) == 5]) == len(pj.M256_PLAIN), hits

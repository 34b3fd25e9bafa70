"""CPU-only: the judges of tests/rotary.py pass the honest emulations -- numpy fp32 cos / sin of the fp32 product for the tables, the
bf16 eager chain for M-RoPE and the fused sites, the fp32 chain for the vision rotation -- for every case tests/test_gpu_rotary.py
runs, the excuse-window share of every table call is under 1 % (from the float64 reference alone), every wrong emulation is reported
by the judge that should catch it, and the GPU file's site list reaches every launch form a rotation is inlined into (the plan read
from the library, as test_swa_plan_cpu.py does, not guessed)."""
import ctypes

import numpy as np
import pytest
import torch

import rotary as ro
from oracle import vision as ovis
import rowwise as rw
import test_swa_plan_cpu as plan

BF = torch.bfloat16


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)


# ---- 1. tables -----------------------------------------------------------------------------------------------------------------------
def test_int64_to_fp32_is_to_nearest_even_at_2_pow_24():
    p = torch.tensor([2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 10 ** 15 + 1], dtype=torch.int64)
    assert ro.pos_to_f32(p).astype(np.float64).tolist() == [2 ** 24 - 1, 2 ** 24, 2 ** 24, 2 ** 24 + 4, 2 ** 31, 999999986991104.0]
    assert ro.pos_to_f32(p, "truncate").astype(np.float64).tolist() == [2 ** 24 - 1, 2 ** 24, 2 ** 24, 2 ** 24 + 2, 2 ** 31 - 128, 999999986991104.0]
    pos = ro.table_positions()
    assert pos.shape == (3, 1, len(ro.NAMED_POSITIONS) + ro.N_RANDOM) and set(ro.NAMED_POSITIONS) <= set(pos[0, 0].tolist())
    assert not torch.equal(pos[0], pos[1]) and not torch.equal(pos[0], pos[2]) and not torch.equal(pos[1], pos[2])
    assert 3 * ro.WRAP_T * 64 > 1024 * 256 and ro.table_positions(ro.WRAP_T).shape == (3, 1, ro.WRAP_T)


@pytest.mark.parametrize("scaling", ro.SCALINGS)
@pytest.mark.parametrize("half_dim,theta", ro.TABLE_CASES)
def test_honest_table_emulation_passes_and_the_window_is_small(half_dim, theta, scaling):
    rep = ro.check_tables(ro.emu_tables, half_dim, theta, scaling)
    _passes(rep)
    assert len(rep.shares) == 2 and max(rep.shares) < rw.EXCUSED_MAX, rep.shares


def test_honest_table_emulation_passes_on_the_grid_stride_call():
    rep = ro.check_tables(ro.emu_tables, 64, 1e6, 1.0, ro.table_positions(ro.WRAP_T))
    _passes(rep)
    assert max(rep.shares) < rw.EXCUSED_MAX, rep.shares


def _bad_positions(wrong, half_dim=64, theta=1e6, scaling=1.0):
    """positions of the elements neither the model nor an excused neighbour"""
    pos, inv = ro.table_positions(), ro.inv_freq(half_dim, theta)
    ref = ro.tables_ref(pos, inv, scaling)
    bad = set()
    for t, name in zip(ro.emu_tables(pos, inv, scaling, wrong), ("cos", "sin")):
        g, m = t[..., :half_dim].double(), ref[name]
        ok = (g == m["model"]) | (m["window"] & (g == m["alt"]))
        bad |= set(pos[(~ok).any(-1)].tolist())
    return bad


def test_wrong_table_emulations_are_reported_where_they_should_be():
    for wrong in ("float64", "fast", "truncate"):
        assert not ro.check_tables(lambda p, i, s: ro.emu_tables(p, i, s, wrong), 64, 1e6, 1.0).ok(), wrong
    big = {p for p in ro.NAMED_POSITIONS if p >= 2 ** 24}
    bad = _bad_positions("float64")                       # the product kept in float64: wrong only where fp32(pos) * inv_freq rounds
    assert {2 ** 24 + 1, 2 ** 24 + 3, 10 ** 8 + 7, 2 ** 31 - 1, 2 ** 40 + 12345, 10 ** 15 + 1} <= bad, sorted(big - bad)
    assert not bad & {0, 1, 2, 64, 4096, 2 ** 24, 2 ** 31}, bad     # (a power of two times inv_freq[j] is exact either way)
    bad = _bad_positions("truncate")                      # only where the nearest fp32 lies above the position
    assert (bad & big) <= {2 ** 24 + 3, 10 ** 8 + 7, 2 ** 31 - 1, 2 ** 40 + 12345}, bad & big
    assert 2 ** 24 + 3 in bad and 2 ** 24 + 1 not in bad
    assert {2 ** 31 - 1, 2 ** 31, 2 ** 40 + 12345, 10 ** 15 + 1} <= _bad_positions("fast")
    assert not ro.check_tables(lambda p, i, s: tuple(t.roll(1, -1) for t in ro.emu_tables(p, i, s)), 8, 1e4, 0.75).ok()


# ---- 2. M-RoPE -----------------------------------------------------------------------------------------------------------------------
def _emu_run(wrong=""):
    return lambda q, k, cos, sin, sec: ro.emu_mrope(q, k, cos, sin, sec, wrong)


@pytest.mark.parametrize("kind", ro.TABLE_KINDS)
@pytest.mark.parametrize("shape", ro.MROPE_SHAPES, ids=ro.shape_id)
def test_bf16_eager_chain_is_the_oracle(shape, kind):
    c = ro.mrope_case(shape, kind)
    eq, ek = ro.mrope_expected(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    gq, gk = ro.emu_mrope(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    assert ro.rotation_mismatches(gq, eq) == "" and ro.rotation_mismatches(gk, ek) == ""
    assert not torch.equal(eq, c["q"]) and not torch.equal(ek, c["k"])
    if kind == "randn":                                   # halves differ, axes unrelated, every row different
        h = shape[4] // 2
        assert not torch.equal(c["cos"][..., :h], c["cos"][..., h:]) and not torch.equal(c["cos"][0], c["cos"][1])
    if shape[1] <= 16:
        assert ro.read_map_report(_emu_run(), *shape) == ""


@pytest.mark.parametrize("shape", [ro.MROPE_SHAPES[1], ro.MROPE_SHAPES[2]], ids=ro.shape_id)
def test_wrong_mrope_emulations_are_reported(shape):
    c = ro.mrope_case(shape, "randn")
    exp = ro.mrope_expected(c["q"], c["k"], c["cos"], c["sin"], c["sections"])
    named = dict(half="channel pass", boundary="axis pass", axes="axis pass", batch="batch pass", fused="")
    for wrong in ro.MROPE_WRONG:
        got = ro.emu_mrope(c["q"], c["k"], c["cos"], c["sin"], c["sections"], wrong)
        for g, e in zip(got, exp):
            assert ro.rotation_mismatches(g, e) != "", (wrong, "passes")
        rm = ro.read_map_report(_emu_run(wrong), *shape)
        print(wrong, "->", rm.splitlines()[:1])
        assert (named[wrong] in rm) if named[wrong] else rm == "", (wrong, rm)      # (a rounding is no read: the map cannot see it)
    # why the tables must be adversarial: real tables repeat their halves, and the wrong half passes
    r = ro.mrope_case(shape, "real")
    assert torch.equal(ro.emu_mrope(r["q"], r["k"], r["cos"], r["sin"], r["sections"], "half")[0],
                       ro.mrope_expected(r["q"], r["k"], r["cos"], r["sin"], r["sections"])[0])


@pytest.mark.parametrize("shape", ro.STRIDED_SHAPES[:4], ids=ro.shape_id)
def test_strided_report(shape):
    c = ro.strided_case(shape)
    after = c["buf"].clone()
    vq, vk = ro.strided_views(c, after)
    assert vq.data_ptr() != vk.data_ptr() and vq.stride(-1) == 1 and vq.stride(2) == shape[4]
    rq, rk = ro.emu_mrope(vq, vk, c["cos"], c["sin"], c["sections"])
    vq.copy_(rq)
    vk.copy_(rk)
    assert ro.strided_report(c, after) == ""
    for col in (0, c["q_off"] - 1, c["k_off"] - 1, c["ld"] - 1):
        junk = after.clone()
        junk[-1, col] += 1.0
        assert "outside" in ro.strided_report(c, junk), col
    bad = after.clone()
    bad[0, c["k_off"]] += 1.0
    assert ro.strided_report(c, bad).startswith("k:")


# ---- 3. the fused sites ----------------------------------------------------------------------------------------------------------------
def test_site_list_reaches_every_form_with_the_plan_the_library_states():
    from infinitevl_amd import _lib
    lib = _lib.load()
    assert {(s.entry, s.kernel, s.prepass) for s in ro.SITES.values()} == ro.SITE_FORMS
    for s in ro.SITES.values():
        C, G = s.W - 1, s.Hq // s.Hkv
        scalar = s.entry in ("fwd", "append")
        assert (len(set(s.seens)) == 1) == scalar and (scalar or s.B == 3), s.name
        cross = [(p % C) + s.T > C for p in s.seens]
        assert (all(cross) if s.wraps else not any(cross)) if scalar else (any(cross) and not all(cross)), (s.name, cross)
        if s.entry == "append":
            continue
        assert ro.stated_plan(s) == (s.kernel, s.nsplit, s.prepass), (s.name, ro.stated_plan(s))
        assert (s.T * G <= 64) == (s.kernel in ("packed", "rows")), s.name
        if s.kernel == "ring256":                        # the caller's bound holds, the shape qualifies
            assert min(s.seens) >= C and s.T >= 256 and lib.ivl_swa_ring256_workspace_bytes(s.B, s.T, s.Hq, s.Hkv, 128, C) > 0, s.name
            continue
        if s.nsplit == 1 and not s.prepass:
            continue                                     # the call would launch: nothing to refuse (test_swa_plan_cpu.py)
        a = plan._args(s.B, s.T, s.Hq, s.Hkv, s.W, True)
        if s.entry == "fwd":
            rc = lib.ivl_swa_fwd(ctypes.byref(a), None)
        elif s.entry in ("decode_rows", "hold"):
            rc = lib.ivl_swa_decode_rows_fwd(ctypes.byref(a), plan.FAKE, None)
        else:
            rc = lib.ivl_swa_rows_fwd(ctypes.byref(a), plan.FAKE, None)
        msg = lib.ivl_last_error().decode()
        assert rc == _lib.IVL_ERR_WORKSPACE, (s.name, rc, msg)
        want = f"required {plan._partials_bytes(s.B, s.nsplit, s.T, s.Hq)} (nsplit={s.nsplit})" if s.nsplit > 1 else "(rope pre-pass)"
        assert want in msg, (s.name, msg)
    for sec in ro.SITE_SECTIONS:
        assert all(v % 8 == 0 for v in sec) and sum(sec) == 64


@pytest.mark.parametrize("sections", ro.SITE_SECTIONS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(ro.SITES))
def test_site_inputs_tell_every_wrong_rotation(name, sections):
    c = ro.site_inputs(name, sections)
    gq, gk = ro.emu_mrope(c["q"], c["k"], c["cos"], c["sin"], sections)
    assert torch.equal(gq, c["q_rot"]) and torch.equal(gk, c["k_rot"])
    n = min(ro.SITES[name].T, 8)                            # the wrong forms on the first tokens (every row of the tables is adversarial)
    cut = lambda x, dim: x.narrow(dim, 0, n)                # noqa: E731
    for wrong in ro.MROPE_WRONG:
        if wrong == "batch" and ro.SITES[name].B == 1:
            continue                                        # (one batch row: no other row to read)
        wq, wk = ro.emu_mrope(cut(c["q"], 1), cut(c["k"], 1), cut(c["cos"], 2), cut(c["sin"], 2), sections, wrong)
        assert ro.rotation_mismatches(wq, cut(c["q_rot"], 1)) != "" and ro.rotation_mismatches(wk, cut(c["k_rot"], 1)) != "", (name, wrong)


def test_site_report():
    s = ro.SITES["rows_n_64row"]
    o = torch.randn(3, 40, 16, 128).to(BF)
    ring = torch.randn(3, 2, 95, 128).to(BF)
    a = dict(o=o, kc=ring, vc=ring)
    other = o.clone()
    other[1, 17:] += 1.0                                  # beyond n_rows[1] = 17 and the idle row: unspecified
    other[2] += 1.0
    assert ro.site_report(s, a, dict(o=other, kc=ring, vc=ring)) == ""
    other[1, 16, 3, 5] += 1.0
    assert "o[b=1]" in ro.site_report(s, a, dict(o=other, kc=ring, vc=ring)) and "t=16, head=3, channel=5" in ro.site_report(s, a, dict(o=other, kc=ring, vc=ring))
    r2 = ring.clone()
    r2[2, 1, 94, 127] += 1.0
    assert "vc ring" in ro.site_report(s, a, dict(o=o, kc=ring, vc=r2))
    h = ro.SITES["hold"]
    o = torch.randn(3, 2, 16, 128).to(BF)
    other = o.clone()
    other[1] += 1.0                                       # the frozen row
    assert ro.site_report(h, dict(o=o, kc=ring, vc=ring), dict(o=other, kc=ring, vc=ring)) == ""
    other[0, 0, 0, 0] += 1.0
    assert ro.site_report(h, dict(o=o, kc=ring, vc=ring), dict(o=other, kc=ring, vc=ring)) != ""


# ---- 4. the vision rotation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", ro.VISION_H)
@pytest.mark.parametrize("d", ro.VISION_D)
def test_vision_fp32_chain_is_the_oracle_and_contraction_is_reported(d, H):
    from infinitevl_amd import _lib
    lib = _lib.load()
    for form in ro.VISION_FORMS:
        lens, max_len = ro.vision_segments(form, H), ro.VISION_MAX_SEQLEN[form]
        S = sum(lens)
        assert max(lens) <= max_len and (form != "inload" or max_len <= 64)
        assert (len(lens) * ((max_len + 127) // 128) * H >= 512) == (form == "rows128"), (form, len(lens))      # the launcher's threshold
        assert (lib.ivl_vision_attn_workspace_bytes(S, H, d, max_len) > 0) == (form != "inload")              # key pre-pass or in the loads
        for tables in ro.VISION_TABLES:
            c = ro.vision_case(d, H, form, tables)
            assert c["cos"].dtype == torch.float32 and tuple(c["cos"].shape) == (S, d) and bool(torch.isfinite(c["sin"]).all())
            exp = ro.vision_rotated(c)
            assert torch.equal(ro.vision_rotated(c, ro.emu_vision), exp) and torch.equal(exp[:, 2], c["qkv"][:, 2])
            for wrong in ro.VISION_WRONG:
                got = ro.vision_rotated(c, lambda q, k, cs, sn: ro.emu_vision(q, k, cs, sn, wrong))
                n = int((got != exp).sum())
                if tables.startswith("cancel") and wrong != "half" or tables == "randn" and wrong == "half":
                    assert ro.vision_report(got[:, int(tables == "cancel_k")], exp[:, int(tables == "cancel_k")]) != "", (form, tables, wrong)
                    assert n >= (S * d // 64 if wrong != "half" else S * d), (form, tables, wrong, n)         # not one lucky element
                if tables.startswith("cancel") and wrong != "half":   # ... and the attention output, all the GPU test sees of q, shows it
                    cu = c["cu"].tolist()
                    o = [ovis.segment_attention(x[:, 0], x[:, 1], x[:, 2], cu, p_round_dtype=BF).to(BF) for x in (exp, got)]
                    assert bool(torch.isfinite(o[0].float()).all()) and int((o[0] != o[1]).sum()) >= S * d // 64, (form, wrong)
                if form == "prepass" and wrong == "fma":
                    print(f"d={d} H={H} {tables} tables: a contracted multiply-add moves {n} of {2 * S * H * d} rotated elements")

"""CPU: the judges of tests/rowwise.py must BITE, and must not bite an honest kernel.

For each row-wise kernel an fp32 torch emulation with the kernel's rounding points goes through the very checks the GPU test
runs (rowwise.check_*), on every input set of the GPU test: it must pass each of them; its largest error relative to the bound
and the share of elements inside the excuse window of the double-rounding judges are printed (pytest -s) and the share -- a
property of the float64 model alone -- is asserted to stay under 1 % per case.  Then each of thirteen wrong emulations must be
reported by at least one case.
"""
import pytest
import torch

import rowwise as rw

BF = torch.bfloat16


# ---- the emulations as `run` callables ----------------------------------------------------------------------------------------
def run_add(wrong=""):
    return lambda x, res, w, eps: rw.emu_add_rmsnorm(x, res, w, eps, wrong)


def _neighbour_rows(y):
    """one row in 1000 taken from its neighbour"""
    y = y.clone()
    idx = torch.arange(0, y.shape[0] - 1, 1000)
    y[idx] = y[idx + 1]
    return y


def run_gated(wrong=""):
    def run(x, gate, w, eps, res, variant):
        y, row = rw.emu_gated_norm(x, gate, w, eps, res, wrong)
        if wrong == "neighbour_row":
            y = _neighbour_rows(y)
        return y, {"res_bf16": row.to(BF), "res_fp32": row, "res_out_fp32": row}.get(variant)
    return run


def run_strided(wrong=""):
    def run(c):
        n = c["x"].numel()
        dense_ld = c["buf"].flatten()[c["off"]:c["off"] + n].view(-1, 256)           # the gate as read with gate_ld = H * 256
        return rw.emu_gated_norm(c["x"].view(-1, 256), c["gate"], c["w"], c["eps"], None, wrong, dense_ld)[0]
    return run


def run_silu(wrong=""):
    return lambda gu: rw.emu_silu_mul(gu, wrong)


def run_conv(wrong=""):
    def run(x, w, bias, state_in, out, silu):
        y, new = rw.emu_conv(x, w, bias, state_in, silu, wrong)
        return y, (new if out is not None else None)
    return run


def run_prologue(c, aliased):
    H, cols = c["H"], c["cols"]
    outs, states = [], []
    for i, x in enumerate(rw.prologue_slices(c)):
        y, new = rw.emu_conv(x, c["w"][i], None, c["state"][i], True)
        outs.append(y)
        states.append(new)
    g, beta = rw.emu_gate(c["proj"][..., cols[3]:cols[3] + H], c["proj"][..., cols[4]:cols[4] + H], c["A_log"], c["dt_bias"])
    return outs + [g, beta, states]


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)
    return rep


# ---- the grid helpers -----------------------------------------------------------------------------------------------------------
def test_bf16_grid_helpers_agree_with_torch():
    g_ = rw.gen(0)
    v = torch.randn(200000, generator=g_).double() * torch.exp2(torch.randint(-130, 120, (200000,), generator=g_).double())
    assert torch.equal(rw.round_bf16(v.float().double()), v.float().to(BF).double())          # one rounding from an fp32 value
    r = rw.round_bf16(v)
    o = rw.other_neighbour(v, r)
    assert bool(((v - r).abs() <= (v - o).abs()).all()) and bool((torch.minimum(r, o) <= v).all()) and bool((v <= torch.maximum(r, o)).all())
    assert torch.equal(o.float().to(BF).double(), o) and bool((o != r).all())
    # a value a hair above a tie: the cast through fp32 rounds twice (to the tie, then to even), round_bf16 once
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(rw.round_bf16(x)) == 1.0 + 2.0 ** -7 and float(x.float().to(BF)) == 1.0
    assert float(rw.bf_spacing(torch.tensor([0.999], dtype=torch.float64), widen=True)) == 2.0 ** -7


# ---- honest emulations pass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rw.ADD_N)
def test_add_rmsnorm_emulation_passes(N):
    _passes(rw.check_add_rmsnorm(run_add(), N))
    _passes(rw.check_add_rmsnorm_onehot(run_add(), N))


@pytest.mark.parametrize("variant", rw.GATED_VARIANTS)
@pytest.mark.parametrize("rows", rw.GATED_ROWS)
def test_gated_norm_emulation_passes(rows, variant):
    _passes(rw.check_gated(run_gated(), rows, variant))


def test_gated_norm_one_hot_and_strided_emulation_pass():
    for variant in ("gated", "plain"):
        _passes(rw.check_gated_onehot(run_gated(), variant))
    for H, tokens in rw.STRIDED:
        _passes(rw.check_strided(run_strided(), H, tokens))


@pytest.mark.parametrize("rows,I", rw.SILU_SHAPES)
def test_silu_mul_emulation_passes(rows, I):
    _passes(rw.check_silu(run_silu(), rows, I))


def test_silu_mul_where_the_sigmoid_is_an_fp32_subnormal():
    """the honest emulation passes; one that returns 0 once 1 / (1 + e^-a) is an fp32 subnormal (a < -87.3) is reported"""
    _passes(rw.check_silu_deep(run_silu()))

    def flushed(gu):
        y = rw.emu_silu_mul(gu)
        y[gu[..., :64].float() < -87.4] = 0.0
        return y
    _reported([rw.check_silu_deep(flushed)], "silu_mul with the subnormal sigmoid flushed")


@pytest.mark.parametrize("T", rw.CONV_T)
def test_short_conv_emulation_passes(T):
    _passes(rw.check_conv(run_conv(), T))


def test_short_conv_wrap_emulation_passes():
    _passes(rw.check_conv_wrap(run_conv()))


@pytest.mark.parametrize("B,T,H", rw.PROLOGUE_SHAPES)
def test_prologue_emulation_passes(B, T, H):
    _passes(rw.check_prologue(run_prologue, B, T, H))


# ---- wrong emulations are reported -------------------------------------------------------------------------------------------------
def _reported(reps, what):
    bad = [r for r in reps if not r.ok()]
    print(f"{what}: reported by {len(bad)} of {len(reps)} cases; first: {bad[0] if bad else None}")
    assert bad, what


def test_last_vector_left_out_of_the_mean_square_at_8192_is_reported():
    _reported([rw.check_add_rmsnorm(run_add("drop_last_vector"), 8192)], "statistics over N - 8 elements (mixed rows)")
    _reported([rw.check_add_rmsnorm_onehot(run_add("drop_last_vector"), 8192)], "statistics over N - 8 elements (one-hot)")


@pytest.mark.parametrize("wrong", ["eps", "no_inner_round", "scale"])
def test_wrong_add_rmsnorm_is_reported(wrong):
    _reported([rw.check_add_rmsnorm(run_add(wrong), N) for N in (8, 2048, 8192)], f"add_rmsnorm {wrong}")


@pytest.mark.parametrize("wrong", ["eps", "extra_round", "scale", "sigmoid_of_x"])
def test_wrong_gated_norm_is_reported(wrong):
    _reported([rw.check_gated(run_gated(wrong), rows, "gated") for rows in (7, 9)], f"gated norm {wrong}")
    if wrong != "sigmoid_of_x":
        _reported([rw.check_gated(run_gated(wrong), 7, v) for v in ("plain", "res_fp32")], f"plain / res norm {wrong}")


@pytest.mark.parametrize("wrong", ["eps", "extra_round", "scale", "sigmoid_of_x"])
def test_wrong_norm_is_reported_by_the_single_row_cases(wrong):
    """rows = 1 and (H, tokens) = (1, 1) -- the decode shape -- must bite on their own: they run once per magnitude class"""
    _reported([rw.check_gated(run_gated(wrong), 1, "gated")], f"gated norm, one row, {wrong}")
    _reported([rw.check_strided(run_strided(wrong), 1, 1)], f"strided gated norm, one row, {wrong}")
    if wrong != "sigmoid_of_x":
        _reported([rw.check_gated(run_gated(wrong), 1, "plain")], f"plain norm, one row, {wrong}")
        _reported([rw.check_gated(run_gated(wrong), 1, "res_bf16")], f"res norm, one row, {wrong}")


def test_no_case_of_the_norms_is_vacuous():
    """every gated / strided case holds rows that are not all zero, gates that reach the sweep's ends, and a non-trivial result"""
    for rows in rw.GATED_ROWS:
        for variant in rw.GATED_VARIANTS:
            cs = [rw.gated_case(rows, variant, f) for f in rw.first_classes(rows)]
            assert sum(int((c["x"] != 0).any(-1).sum()) for c in cs) >= max(1, len(cs) - 1), (rows, variant)
            if variant != "plain":
                assert all(float(c["gate"].float().min()) == -100.0 and float(c["gate"].float().max()) == 100.0 for c in cs)
    for H, tokens in rw.STRIDED:
        cs = [rw.strided_case(H, tokens, f) for f in rw.first_classes(tokens * H)]
        assert sum(int((c["x"] != 0).any(-1).sum()) for c in cs) >= max(1, len(cs) - 1), (H, tokens)


def test_gate_read_with_a_dense_row_stride_is_reported():
    for H, tokens in rw.STRIDED:
        if tokens > 1:                       # a single token has no second row to misplace
            _reported([rw.check_strided(run_strided("gate_ld"), H, tokens)], f"gate_ld = H * 256, H={H} tokens={tokens}")


def test_a_row_in_1000_taken_from_its_neighbour_is_reported():
    _reported([rw.check_gated(run_gated("neighbour_row"), 16389, v) for v in ("gated", "plain")], "neighbour row")


@pytest.mark.parametrize("wrong", ["taps_reversed", "state_slot", "state_not_carried", "bias_after_silu"])
def test_wrong_short_conv_is_reported(wrong):
    _reported([rw.check_conv(run_conv(wrong), T) for T in (1, 3, 9)], f"short_conv {wrong}")


@pytest.mark.parametrize("wrong", ["halves_swapped", "no_inner_round"])
def test_wrong_silu_mul_is_reported(wrong):
    _reported([rw.check_silu(run_silu(wrong), rows, I) for rows, I in rw.SILU_SHAPES[:3]], f"silu_mul {wrong}")

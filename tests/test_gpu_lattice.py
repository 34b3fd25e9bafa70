"""GPU (-m gpu): the Gated DeltaNet operators on the EXACT LATTICE (tests/lattice.py; tests/test_lattice_cpu.py shows that the
oracle's rounding models are exact on every case used here and that no case is degenerate).

use_qk_l2norm_in_kernel=False, power-of-two scale, signed one-hot keys, small-integer q / v / h0, beta in {0, 1} ({0, 0.5, 1} in
"half"), g in {0, -200}: every intermediate of the rule is exactly representable in bf16 (in e4m3 too, "half" excepted), so
every assertion below is torch.equal against the token-by-token rule in float64 -- for o and for the final state, no tolerance
anywhere.  A failure names the first differing (batch, token, chunk, row in chunk, head, column).

What the lattice reaches: ops.chunk_gated_delta_rule -- the two-launch form of gdn_chunk_launch (pre-pass + scan) with 32- and
64-column scan workgroups, one and several workspace segments, bf16 and e4m3 operands, fp32 / bf16 state in and out, in place
or not, no state out, variable-length input -- and ops.fused_recurrent_gated_delta_rule with bf16 and fp16 activations; both with
the l2norm OFF and a scale other than 128^-0.5, which no other GPU test passes.

What it cannot reach: the fused-front-end forms (ops.gdn_chunk_fused*: the single and the overlapped launch, the ragged rows
form) and the decode step apply SiLU to q and k and fix the l2norm on, so no input puts them on the lattice.  They remain pinned
bit for bit to the two-launch form by test_gpu_parity.py, test_gpu_adversarial.py, test_gpu_frames.py and test_gpu_ragged.py.
"""
import functools

import pytest
import torch

import lattice as lat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FP8 = "fp8_e4m3"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


@functools.lru_cache(maxsize=None)
def _case(kind, B, T, H, with_h0=True):
    """(inputs, (o, state) float64 at scale 1): computed once per case and shared, never written to"""
    case = lat.make(kind, B, T, H)
    if not with_h0:
        case["h0"] = None
    return case, lat.lattice_expected(case, 1.0)


def _scaled(exp, scale):
    return exp[0] * scale, exp[1]


def _run(op, case, scale, *, l2norm=False, act=BF, mma=None, state_dtype=F32, inplace=False, state_out=True, out_dtype=None,
         h0="case", cu=None):
    """One operator call -> (o in the activation dtype, final state or None), on the CPU.  inplace: final_state_out IS the
    initial state; out_dtype: final_state_out is a fresh tensor of that dtype."""
    from infinitevl_amd import ops
    fn = ops.chunk_gated_delta_rule if op == "chunk" else ops.fused_recurrent_gated_delta_rule
    q, k, v, beta = (case[n].to(DEV, act) for n in ("q", "k", "v", "beta"))
    h0 = case["h0"] if isinstance(h0, str) else h0
    h0 = None if h0 is None else h0.to(DEV, state_dtype)
    kw = dict(scale=scale, initial_state=h0, use_qk_l2norm_in_kernel=l2norm)
    if mma is not None:
        kw["mma_dtype"] = mma
    if cu is not None:
        kw["cu_seqlens"] = torch.tensor(cu, dtype=torch.int32, device=DEV)
    if inplace:
        assert h0 is not None
        kw["final_state_out"] = h0
    elif out_dtype is not None:
        kw["final_state_out"] = torch.full_like(h0, float("nan"), dtype=out_dtype) if h0 is not None else \
            torch.full((len(cu) - 1 if cu else q.shape[0], q.shape[2], lat.GDN_K, lat.GDN_V), float("nan"), dtype=out_dtype, device=DEV)
    else:
        kw["output_final_state"] = state_out
    o, ht = fn(q, k, v, case["g"].to(DEV), beta, **kw)
    torch.cuda.synchronize()
    assert o.dtype == act and tuple(o.shape) == tuple(case["v"].shape)
    if inplace:
        assert ht.data_ptr() == h0.data_ptr()
    return o.cpu(), None if ht is None else ht.cpu()


def _check(exp, got, what):
    """bit equality of o and (where there is one) of the final state with the float64 expectation"""
    o, ht = got
    ok = torch.equal(o.double(), exp[0]) and (ht is None or torch.equal(ht.double(), exp[1]))
    assert ok, f"{what}: " + "\n  ".join(lat.lattice_mismatches(exp[0], exp[1], o, ht))


def _check_same(a, b, what):
    """two kernel results bit-equal to each other, reported the same way"""
    ok = torch.equal(a[0].double(), b[0].double()) and torch.equal(a[1].double(), b[1].double())
    assert ok, f"{what}: " + "\n  ".join(lat.lattice_mismatches(a[0], a[1], b[0], b[1]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the chunk kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", lat.CHUNK_T)
@pytest.mark.parametrize("kind", ["memory", "half", "still"])
def test_chunk_bf16_is_exact_at_every_length_and_scale(kind, T):
    """B = 2, H = 3 (32-column scan workgroups; batch and head strides), one chunk, a ragged chunk, several; every scale"""
    case, exp = _case(kind, 2, T, 3)
    for scale in lat.SCALES:
        _check(_scaled(exp, scale), _run("chunk", case, scale), f"chunk bf16 {kind} T={T} scale={scale}")


@pytest.mark.parametrize("T", lat.CHUNK_T_FP8)
@pytest.mark.parametrize("kind", ["memory", "still"])
def test_chunk_fp8_is_exact_at_every_length(kind, T):
    """e4m3 operands in the serial pass: every operand and intermediate of these kinds is at or below 16"""
    case, exp = _case(kind, 2, T, 3)
    for scale in (1.0, 0.125):
        _check(_scaled(exp, scale), _run("chunk", case, scale, mma=FP8), f"chunk e4m3 {kind} T={T} scale={scale}")


@pytest.mark.parametrize("kind,mma", [("memory", None), ("half", None), ("still", None), ("memory", FP8), ("still", FP8)])
def test_chunk_wide_scan_workgroups_are_exact(kind, mma):
    """B * H = 48 > 32: the scan runs 64-column workgroups; T = 70 has a ragged second chunk"""
    B, T, H = lat.WIDE
    case, exp = _case(kind, B, T, H)
    _check(_scaled(exp, 0.5), _run("chunk", case, 0.5, mma=mma), f"chunk {mma or 'bf16'} {kind} B={B} T={T} H={H}")


@pytest.mark.parametrize("mma", [None, FP8])
def test_chunk_long_call_carries_the_state_exactly_between_workspace_segments(mma):
    """T = 4096 + 65: two segments of the 64-chunk workspace, the fp32 state carried between their launches"""
    case, exp = _case("memory", 1, lat.LONG_T, 1)
    _check(_scaled(exp, 0.5), _run("chunk", case, 0.5, mma=mma), f"chunk {mma or 'bf16'} T={lat.LONG_T}")


@pytest.mark.parametrize("T", [65, 200])
def test_chunk_default_scale_rounds_once(T):
    """scale=None is 128^-0.5, which takes the output off the lattice: the epilogue's one multiplication of the exact integer
    accumulator, bf16(float32(o_int) * float32(128^-0.5)); the state does not see the scale"""
    case, exp = _case("memory", 2, T, 3)
    want = lat.default_scale_expected(exp[0]).double()
    for mma in (None, FP8):
        _check((want, exp[1]), _run("chunk", case, None, mma=mma), f"chunk {mma or 'bf16'} T={T} default scale")


STATE_FORMS = [
    # with_h0, state dtype in, inplace, fresh final_state_out dtype, output_final_state
    (True, F32, False, None, True), (False, F32, False, None, True), (True, BF, False, None, True),
    (True, F32, True, None, True), (True, BF, True, None, True),
    (True, F32, False, BF, True), (False, F32, False, BF, True), (True, BF, False, F32, True),
    (True, F32, False, None, False), (False, F32, False, None, False),
]


@pytest.mark.parametrize("op,mma", [("chunk", None), ("chunk", FP8), ("recurrent", None)])
@pytest.mark.parametrize("with_h0,sd,inplace,out_dtype,state_out", STATE_FORMS)
def test_state_in_and_out_forms_are_exact(op, mma, with_h0, sd, inplace, out_dtype, state_out):
    """h0 given or None, fp32 or bf16 state (every lattice state is exact in bf16), the final state written over the initial
    one, into a fresh tensor of the other dtype, or not asked for -- o stays exact"""
    T = 129 if op == "chunk" else 70
    case, exp = _case("memory", 2, T, 3, with_h0)
    o, ht = _run(op, case, 0.5, mma=mma, state_dtype=sd, inplace=inplace, out_dtype=out_dtype, state_out=state_out)
    if state_out:
        assert ht is not None and ht.dtype == (sd if inplace else out_dtype or F32)
    else:
        assert ht is None
    _check(_scaled(exp, 0.5), (o, ht), f"{op} {mma or 'bf16'} h0={with_h0} {sd} inplace={inplace} out={out_dtype} state_out={state_out}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the recurrent kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", lat.RECURRENT_T)
@pytest.mark.parametrize("act", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["memory", "half", "still"])
def test_recurrent_is_exact(kind, act, T):
    """bf16 and fp16 activations; fp16 also through chunk_gated_delta_rule, which routes such calls to the recurrent kernel"""
    case, exp = _case(kind, 2, T, 3)
    for scale in lat.SCALES:
        _check(_scaled(exp, scale), _run("recurrent", case, scale, act=act), f"recurrent {act} {kind} T={T} scale={scale}")
    if act == F16:
        _check(_scaled(exp, 0.5), _run("chunk", case, 0.5, act=act), f"chunk entry, fp16 {kind} T={T}")


# ---------------------------------------------------------------------------------------------------------------------------------
# across the two kernels, the flag, call boundaries
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(set(lat.RECURRENT_T) | {65, 129}))
def test_l2norm_flag_is_a_no_op_on_unit_rows(T):
    """"onehot_q": q and k are unit rows, 1 / sqrt(1 + 1e-6) rounds to 1 in bf16 and fp16 -- each operator with the flag on
    equals its own result with the flag off bit for bit, and both equal the expectation"""
    case, exp = _case("onehot_q", 2, T, 3)
    e = _scaled(exp, 0.5)
    for op, act, mma in (("chunk", BF, None), ("chunk", BF, FP8), ("recurrent", BF, None), ("recurrent", F16, None)):
        off = _run(op, case, 0.5, act=act, mma=mma, l2norm=False)
        on = _run(op, case, 0.5, act=act, mma=mma, l2norm=True)
        _check(e, off, f"{op} {act} {mma or ''} T={T} l2norm off")
        _check_same(off, on, f"{op} {act} {mma or ''} T={T} l2norm on against off")


@pytest.mark.parametrize("T", sorted(set(lat.RECURRENT_T) | {65, 129, 200}))
@pytest.mark.parametrize("kind", ["memory", "half"])
def test_chunk_equals_recurrent_bit_for_bit(kind, T):
    """the one GDN cross-kernel comparison with no tolerance"""
    case, exp = _case(kind, 2, T, 3)
    a, b = _run("chunk", case, 0.5), _run("recurrent", case, 0.5)
    _check_same(a, b, f"chunk against recurrent {kind} T={T}")
    _check(_scaled(exp, 0.5), a, f"chunk {kind} T={T}")


@pytest.mark.parametrize("op,mma", [("chunk", None), ("chunk", FP8), ("recurrent", None)])
def test_split_at_an_odd_token_equals_one_call(op, mma):
    """37 | 93 tokens, neither a multiple of 64, the fp32 state carried by the caller: o and the final state equal the one-call
    result (and the expectation)"""
    T, cut = lat.SPLIT
    case, exp = _case("memory", 2, T, 2)
    whole = _run(op, case, 0.5, mma=mma)
    parts = [{n: (x[:, a:b] if n in ("q", "k", "v", "g", "beta") else x) for n, x in case.items()} for a, b in ((0, cut), (cut, T))]
    o1, s1 = _run(op, parts[0], 0.5, mma=mma)
    o2, s2 = _run(op, parts[1], 0.5, mma=mma, h0=s1)
    both = (torch.cat([o1, o2], 1), s2)
    _check(_scaled(exp, 0.5), whole, f"{op} {mma or 'bf16'} one call")
    _check_same(whole, both, f"{op} {mma or 'bf16'} split at {cut} against one call")


@pytest.mark.parametrize("op,mma", [("chunk", None), ("chunk", FP8), ("recurrent", None)])
def test_varlen_sequences_each_equal_their_own_expectation(op, mma):
    """cu_seqlens over lengths (70, 1, 0, 64, 65) of one flattened case: every sequence starts its chunks at its own first
    token and from its own initial state; the empty one passes its state through"""
    flat = lat.varlen_case()
    cu = [0]
    for n in lat.VARLEN_LENGTHS:
        cu.append(cu[-1] + n)
    o, ht = _run(op, flat, 0.5, mma=mma, h0=flat["h0_seq"], cu=cu)
    for i, seq in enumerate(lat.varlen_sequences(flat, lat.VARLEN_LENGTHS)):
        if seq is None:
            assert torch.equal(ht[i], flat["h0_seq"][i]), f"sequence {i} is empty: its state passes through"
            continue
        exp = lat.lattice_expected(seq, 0.5)
        _check(exp, (o[:, cu[i]:cu[i + 1]], ht[i:i + 1]), f"{op} {mma or 'bf16'} sequence {i} (tokens {cu[i]}..{cu[i + 1] - 1})")

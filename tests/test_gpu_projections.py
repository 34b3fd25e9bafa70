"""GPU (-m gpu): the projection kernels -- linear_small_m_kernel in all 60 instantiations (plain / GLU / NORM, M = 1 .. 4, 1 / 2 / 4
rows per wave, NIT 1 / 2), linear_gdn_out_kernel, linear_m256_kernel (plain, GLU, SCORE) -- against the EXACT-INTEGER probe of
tests/projections.py: integer-valued bf16 inputs whose fp32 sums are exact in any order, so the output must be
bf16_RNE(exact float64 sum + bias) BIT FOR BIT, with column tails under every rows-per-wave, K around every step of the weight
loop and of the norm prologue, the bias of the GLU form through the C entry point, and sums that sit on exact bf16 ties
(tests/test_projections_cpu.py shows that the judges pass an honest fp32 emulation and report eleven wrong ones).  Every output
buffer is followed by a guard area that must come back untouched.

What an MI355X gave (pytest -s prints it per case):

  small-M plain          80 listed cases (with NORM and GLU below) that reach all 60 instantiations; index variant and ties variant,
                         with the bias and without: 0 mismatches -- every element EQUALS bf16_RNE(exact sum + bias), the ties
                         (10 % and more of every ties call) all rounded to even, every guard area untouched.
  small-M GLU            integer g (standard deviation about 6) and u, the gate bias and the up bias through the C entry point:
                         every element equals rowwise.silu_ref's model; 0 % took the other neighbour (no listed call has an
                         element inside the window at all: the integer gates keep clear of it).  randn data at I = 5 and 4097,
                         judged on the kernel's own plain output: at most 0.007 % of a call took the other neighbour, all inside
                         the window (up to 0.39 % of a call).
  small-M NORM           plain and GLU, NIT 1 and 2, with a residual and without: 0 mismatches, h_out bit for bit; the same through
                         ops.PreNorm.
  small-M randn          at the tail shapes against float64 with |ref| 2^-8 + 1e-5: worst error / bound 0.995 (a value next to a
                         bf16 tie: half a spacing is owed to any correct rounding).
  gdn_out                H = 2, 3, 5, 16 x M = 1 .. 4 x N = 7, 2048 x bias: bit-equal to the gated norm + ivl_linear_small_m_fwd, conv
                         states bit-equal to the CPU shift.  FOUND by reading the kernel, before any launch: H = 1 (K = 256) left
                         lanes 32 .. 63 of every wave outside the weight loop whose first trip holds the gated norm (half a wave
                         in wave_sum, columns 128 .. 255 of the staged row never written, both read by the dot product) -- a wrong
                         answer, not a fault.  Fixed by refusing H < 2 on the host (test_gdn_out_refuses_a_single_head); nothing
                         here launches H = 1.
  m256 plain / GLU       the MFMA with its fp32 accumulator IS exact on these integers: 0 mismatches in the index and the ties
                         variant (1 .. 32 K-tiles, M = 1 .. 256, N = 4 .. 100); GLU 0 % excused.
  SCORE                  integer logits: top1 = the lowest index of the maximum in every row (254 of the listed rows attain it
                         more than once); largest scoring.judge ratio 0.186 (logprob and lse together).

Nothing else was found: no kernel change beyond the H < 2 refusal, no instantiation or form left out.

That the probe bites the REAL kernels was measured once with two deliberately wrong (memory-safe) developer builds of the two
source files: (A) the K-tail clamp without its zeroing in linear_small_m_kernel + truncation in linear_m256's plain store: all 64
small-M probe cases with K % 2048 != 0 failed and none of the 16 at K = 2048 / 4096, all 13 m256 ties cases and none of the index
ones; (B) truncation in the small-M plain store, the gate bias used for the up half, m256's up row off by one: all 9 small-M ties
cases and no plain index case, all 26 small-M GLU cases, all 13 m256 GLU cases.
"""
import pytest
import torch

import projections as pj
import rowwise as rw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 64                      # elements behind every output that must keep this value
SENTINEL = 24576.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


_ON_DEV = {}


@pytest.fixture(autouse=True)
def _fresh_uploads():
    _ON_DEV.clear()
    yield
    _ON_DEV.clear()


def _dev(t):
    """the device copy of a CPU tensor of the current case (a 67 MB weight is uploaded once, not once per launch)"""
    if t is None:
        return None
    key = (t.data_ptr(), tuple(t.shape), t.dtype)
    if key not in _ON_DEV:
        _ON_DEV[key] = (t, t.to(DEV))
    return _ON_DEV[key][1]


def _out(rows, cols, dtype=BF):
    """(the [rows, cols] output, NaN-filled; the whole buffer with its guard area)"""
    buf = torch.full((rows * cols + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    buf[:rows * cols] = float("nan")
    return buf[:rows * cols].view(rows, cols), buf


def _guard_ok(buf):
    assert bool((buf[-GUARD:] == SENTINEL).all()), "a store went past the end of the output"


def _passes(rep):
    print(rep)
    assert rep.ok(), str(rep)
    return rep


# ---- the kernels as `run` callables (CPU tensors in, CPU tensors out) ----------------------------------------------------------------
def run_small_m(x, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    y, buf = _out(M, N)
    fn = _lib.load().ivl_linear_swiglu_small_m_fwd if glu else _lib.load().ivl_linear_small_m_fwd
    _lib.check(fn(ops._p(xd), ops._p(wd), ops._p(bd), ops._p(y), M, N, K, ops._stream(xd)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    return y.cpu()


def run_norm_small_m(x, res, nw, eps, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    xd, rd, nwd, wd, bd = _dev(x), _dev(res), _dev(nw), _dev(w), _dev(bias)
    y, buf = _out(M, N)
    h, hbuf = _out(M, K) if res is not None else (None, None)
    _lib.check(_lib.load().ivl_norm_linear_small_m_fwd(ops._p(xd), ops._p(rd), ops._p(nwd), float(eps), ops._p(h), ops._p(wd), ops._p(bd),
                                                       ops._p(y), M, N, K, 1 if glu else 0, ops._stream(xd)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    if hbuf is not None:
        _guard_ok(hbuf)
    return y.cpu(), (None if h is None else h.cpu())


def run_ops(x, w, bias, glu):
    """the same kernels as the package reaches them (ops.linear / ops.linear_swiglu; the latter never passes a bias)"""
    from infinitevl_amd import ops
    if not glu:
        y = ops.linear(_dev(x)[None], _dev(w), _dev(bias))[0]
    elif bias is None:
        y = ops.linear_swiglu(_dev(x)[None], _dev(w))[0]
    else:
        return run_small_m(x, w, bias, glu)
    torch.cuda.synchronize()
    return y.cpu()


def run_m256(x, w, bias, glu):
    from infinitevl_amd import _lib, ops
    M, K = x.shape
    N = w.shape[0] // 2 if glu else w.shape[0]
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    y, buf = _out(M, N)
    _lib.check(_lib.load().ivl_linear_m256_fwd(ops._p(xd), ops._p(wd), ops._p(bd), ops._p(y), M, N, K, 1 if glu else 0, ops._stream(xd)))
    torch.cuda.synchronize()
    _guard_ok(buf)
    return y.cpu()


def run_score(x, w, bias, target):
    from infinitevl_amd import ops
    lp, top1, lse = ops.linear_logprob(_dev(x), _dev(w), _dev(target), _dev(bias), top1=True, lse=True)
    torch.cuda.synchronize()
    return lp.cpu(), top1.cpu(), lse.cpu()


def _id(c):
    return "-".join(str(v) if not isinstance(v, tuple) else "M" + "".join(map(str, v)) for v in c)


# ---- linear_small_m_kernel: all 60 instantiations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("glu,norm,N,K,Ms,variant", pj.SMALL_M, ids=[_id(c) for c in pj.SMALL_M])
def test_small_m_exact_integer_probe(glu, norm, N, K, Ms, variant):
    """plain / GLU / NORM x every rows-per-wave with a column tail (N = 7, 4099, 8195; I = 5, 4097) x K around the 2048-element
    trips of the weight loop and the NIT step of the norm prologue x M (1 and 4 everywhere, 1 .. 4 where the list says so), with
    the bias and without (GLU too: the C entry point), NORM with a residual and without (h_out bit for bit).  Plain outputs bit
    for bit; GLU outputs through rowwise.silu_ref on the exact [g | u]."""
    if norm:
        _passes(pj.check_norm_linear(run_norm_small_m, pj.norm_case(N, K, glu, Ms), Ms))
    else:
        _passes(pj.check_linear(run_small_m, pj.int_case(4, N, K, glu, variant, Ms), Ms))


@pytest.mark.parametrize("glu,N", pj.TAILS, ids=[_id(c) for c in pj.TAILS])
def test_small_m_randn_at_the_tail_shapes_vs_float64(glu, N):
    """randn data at the tail shapes through ops.linear / ops.linear_swiglu (the GLU bias through the C entry point):
    |y - float64| <= |ref| 2^-8 + 1e-5 per element; GLU (odd I) = rowwise.silu_ref of the kernel's own plain output, per element."""
    for K in (136, 520) if N > 100 else (8, 520, 2056, 4104):
        _passes(pj.check_randn(run_ops, pj.randn_case(4, N, K, glu), (1, 4) if N > 100 else (1, 2, 3, 4)))


def test_prenorm_through_ops_reaches_the_norm_form_and_equals_the_probe():
    """ops.linear / ops.linear_swiglu on an ops.PreNorm (what the decoder stack does in a decode step): the probe's answer, and the
    residual stream in PreNorm.h"""
    from infinitevl_amd import ops

    def run(x, res, nw, eps, w, bias, glu):
        pn = ops.PreNorm(_dev(x)[None], None if res is None else _dev(res)[None], _dev(nw), eps)
        y = ops.linear_swiglu(pn, _dev(w)) if glu else ops.linear(pn, _dev(w), _dev(bias))
        torch.cuda.synchronize()
        assert pn.done and pn._y is None, "the fused launch must have run the norm"
        return y[0].cpu(), (None if res is None else pn.h[0].cpu())
    for glu, N, K in ((False, 7, 520), (True, 5, 2056), (False, 4099, 512)):
        c = pj.norm_case(N, K, glu)
        if glu:
            c["bias"] = torch.zeros_like(c["bias"])                 # (no bias on this path)
        _passes(pj.check_norm_linear(run, c, (1, 3)))


# ---- linear_gdn_out_kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,N", pj.GDN_OUT)
def test_gdn_out_equals_gated_norm_plus_linear_small_m_and_shifts_the_conv_states(H, N):
    """H = 2, 3 (fewer heads than waves), 5, 16; M = 1 .. 4; N = 7 (a partial workgroup) and 2048; bias on / off; the gate read in
    place at a row stride of 4 mod 8 elements, 8 bytes into a 16-byte line.  y bit-equal to ops.rmsnorm_swish_gate_strided (on a
    copy of the gate: that kernel wants 16-byte rows) + ivl_linear_small_m_fwd; the conv states of q and k bit-equal to the shift
    computed in plain torch on the CPU."""
    from infinitevl_amd import ops
    c = pj.gdn_out_case(H, N)
    Dv = H * 256
    w, nw = _dev(c["w"]), _dev(c["nw"])
    for M in (1, 2, 3, 4):
        for wb in (False, True):
            proj = c["proj"][:M].to(DEV).view(M, 1, c["ld"])
            o_raw = c["o_raw"][:M].to(DEV).view(M, 1, Dv)
            cq, ck = c["cq"][:M].to(DEV), c["ck"][:M].to(DEV)
            bias = _dev(c["bias"]) if wb else None
            y = ops.gdn_out_linear(o_raw, proj, c["col_g"], c["col_q"], c["col_k"], nw, c["eps"], cq, ck, w, bias, H)
            gate = torch.empty(M, Dv, dtype=BF, device=DEV).copy_(proj.view(M, c["ld"])[:, c["col_g"]:c["col_g"] + Dv])
            xn = ops.rmsnorm_swish_gate_strided(o_raw.view(M, 1, H, 256), gate, Dv, nw, c["eps"])
            y_ref = ops.linear(xn.view(M, 1, Dv), w, bias)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y.float()).all()) and torch.equal(y, y_ref), (M, wb)
            p = c["proj"][:M]
            assert torch.equal(cq.cpu(), pj.conv_shift_ref(c["cq"][:M], p[:, c["col_q"]:c["col_q"] + H * 128])), (M, wb, "q")
            assert torch.equal(ck.cpu(), pj.conv_shift_ref(c["ck"][:M], p[:, c["col_k"]:c["col_k"] + H * 128])), (M, wb, "k")
        rep = rw.Report(f"gdn_out H={H} N={N}: the gated norm it equals")                # ... which is itself anchored to float64
        r = rw.gated_norm_ref(c["o_raw"][:M].view(-1, 256), c["proj"][:M, c["col_g"]:c["col_g"] + Dv].reshape(-1, 256), c["nw"], c["eps"])
        rep.single("xn", xn.cpu().view(-1, 256), r["ref"], r["noise"], r["floor"])
        assert rep.ok(), str(rep)


def test_gdn_out_refuses_a_single_head():
    """H = 1 (K = 256) would leave lanes 32 .. 63 of every wave outside the weight loop whose first trip holds the gated norm: the
    entry point refuses it on the host (nothing is launched), and so does H = 17"""
    from infinitevl_amd import _lib, ops
    lib = _lib.load()
    z = torch.zeros(4 * 4352, dtype=BF, device=DEV)
    y = torch.full((8,), SENTINEL, dtype=BF, device=DEV)
    p, st = ops._p(z), ops._stream(z)
    for H in (1, 17, 0):
        rc = lib.ivl_gdn_out_linear_small_m_fwd(p, p, 512, p, 1e-5, H, p, 512, 0, 128, p, p, p, None, ops._p(y), 1, 8, H * 256, st)
        assert rc == _lib.IVL_ERR_UNSUPPORTED, (H, rc)
        msg = lib.ivl_last_error().decode()
        assert "2 <= H <= 16" in msg and "every lane must enter the weight loop" in msg, msg
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ---- linear_m256_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["index", "ties"])
@pytest.mark.parametrize("M,N,K", pj.M256_PLAIN)
def test_m256_plain_exact_integer_probe(M, N, K, variant):
    """the MFMA with its fp32 accumulator on integer sums: bit for bit, ties included; 1 .. 32 K-tiles against the 3-stage ring,
    M around a wave's 32 rows and the call's 256, N around the 64 columns of a workgroup; bias on / off"""
    _passes(pj.check_linear(run_m256, pj.int_case(M, N, K, False, variant), (M,)))


@pytest.mark.parametrize("M,I,K", pj.M256_GLU)
def test_m256_glu_exact_integer_probe(M, I, K):
    """I around the 48 output columns of a GLU workgroup; the gate bias and the up bias"""
    _passes(pj.check_linear(run_m256, pj.int_case(M, I, K, True), (M,)))


@pytest.mark.parametrize("N", [4, 64, 68, 4100])
def test_score_exact_integer_logits(N):
    """M = 1, 33, 256 x K = 64, 192: integer logits, so ties for the maximum are common -- top1 must be the lowest index; targets in
    the first column, the last, the first of the tail column block, anywhere, and not scored"""
    worst = 0.0
    for M, N_, K in pj.SCORE:
        if N_ == N:
            worst = max(worst, _passes(pj.check_score(run_score, pj.score_case(M, N, K))).worst)
    print(f"N={N}: largest scoring.judge ratio {worst:.3f}")

"""GPU (-m gpu): ivl_linear_m256_fwd, the 256-row projection kernel of a prefill chunk (plain, and SwiGLU-gated on the fused
gate|up weight) -- against a float64 reference, against its own plain form + silu_mul bit for bit, deterministic, graph-safe,
reached by ops.linear_swiglu at 256 rows only (plain projections stay on the library GEMM), and inside a streamed 4-layer stack against the oracle."""
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import infinitevl_amd
    infinitevl_amd.load_library()
    yield


def bf(x):
    return x.to(torch.bfloat16)


def m256(x, w, bias, N, glu, M=None):
    from infinitevl_amd import _lib, ops
    K = w.shape[-1]
    M = x.numel() // K if M is None else M
    y = torch.empty(*x.shape[:-1], N, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().ivl_linear_m256_fwd(ops._p(x), ops._p(w), ops._p(bias), ops._p(y), M, N, K, 1 if glu else 0,
                                               ops._stream(x)))
    return y


def _inputs(M, N, K, seed, with_bias=False, glu=False):
    g = torch.Generator().manual_seed(seed)
    x = bf(torch.randn(1, M, K, generator=g)).to(DEV)
    w = bf(torch.randn((2 * N if glu else N), K, generator=g) * K ** -0.5).to(DEV)
    b = bf(torch.randn((2 * N if glu else N), generator=g)).to(DEV) if with_bias else None
    return x, w, b


@pytest.mark.parametrize("M,N,K,with_bias", [(256, 12320, 2048, False), (256, 2560, 2048, True), (256, 100, 128, True),
                                             (200, 1000, 4096, False), (1, 64, 64, False)])
def test_linear_m256_vs_float64(M, N, K, with_bias):
    """Tolerance of test_linear_small_m_vs_fp32: half a bf16 ulp of the output plus fp32 summation-order noise."""
    x, w, b = _inputs(M, N, K, M * 7 + N + K, with_bias)
    y = m256(x, w, b, N, False)
    ref = x.double() @ w.double().T + (b.double() if with_bias else 0.0)
    err = (y.double() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 1e-5
    assert bool((err <= tol).all()), float((err / (ref.abs() + 1e-3)).max())


@pytest.mark.parametrize("M,I,K,with_bias", [(256, 11008, 2048, False), (256, 1000, 1024, True), (130, 8192, 640, False)])
def test_linear_m256_glu_equals_plain_plus_silu_mul(M, I, K, with_bias):
    """The gate in the epilogue == the plain kernel on the fused gate|up weight followed by ivl_silu_mul_fwd, bit for bit."""
    from infinitevl_amd import ops
    x, w, b = _inputs(M, I, K, M + I + K, with_bias, glu=True)
    act = m256(x, w, b, I, True)
    gu = m256(x, w, b, 2 * I, False)
    assert torch.equal(act, ops.silu_mul(gu))


def test_linear_m256_deterministic_and_graph_replay():
    """No K split and no cross-workgroup reduction: two runs and a captured-graph replay give the same bits."""
    x, w, _ = _inputs(256, 11008, 2048, 3, glu=True)
    xp, wp, _ = _inputs(256, 12320, 2048, 4)
    a1, p1 = m256(x, w, None, 11008, True), m256(xp, wp, None, 12320, False)
    a2, p2 = m256(x, w, None, 11008, True), m256(xp, wp, None, 12320, False)
    assert torch.equal(a1, a2) and torch.equal(p1, p2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a3, p3 = m256(x, w, None, 11008, True), m256(xp, wp, None, 12320, False)
    a3.zero_()
    p3.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a1, a3) and torch.equal(p1, p3)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()]


@pytest.mark.parametrize("rows,hit", [(256, True), (4, False), (4096, False)])
def test_ops_dispatch_reaches_m256_at_256_rows_only(rows, hit):
    """ops.linear_swiglu takes the fused kernel for a 256-row chunk only, and computes what the path it replaces (library GEMM +
    silu_mul) computes."""
    from infinitevl_amd import ops
    x = bf(torch.randn(1, rows, 2048)).to(DEV)
    w_gu = bf(torch.randn(2 * 11008, 2048) * 2048 ** -0.5).to(DEV)
    names = _kernel_names(lambda: ops.linear_swiglu(x, w_gu))
    assert any("linear_m256_kernel" in n for n in names) == hit, (rows, [n for n in names if "kernel" in n.lower()][:8])
    if hit:
        y_new = ops.linear_swiglu(x, w_gu)
        y_old = ops.silu_mul(ops.linear(x, w_gu))            # the path it replaces: library GEMM (plain N = 22016) + silu_mul
        d = (y_new.float() - y_old.float())
        assert float(d.pow(2).mean().sqrt() / y_old.float().pow(2).mean().sqrt()) < 4e-3


def test_plain_and_unaligned_projections_stay_on_the_library():
    """Plain projections (the GDN in-projection, down / o_proj, SWA qkv) and a non-contiguous gate|up input keep today's path."""
    from infinitevl_amd import ops
    x = bf(torch.randn(1, 256, 2048)).to(DEV)
    for N in (2048, 2560, 12320):
        w = bf(torch.randn(N, 2048) * 2048 ** -0.5).to(DEV)
        assert not any("linear_m256_kernel" in n for n in _kernel_names(lambda: ops.linear(x, w)))
    xt = bf(torch.randn(2048, 256)).to(DEV).T[None]
    w = bf(torch.randn(2 * 11008, 2048) * 2048 ** -0.5).to(DEV)
    assert not any("linear_m256_kernel" in n for n in _kernel_names(lambda: ops.linear_swiglu(xt, w)))


def test_stack_streamed_in_256_token_chunks_with_m256_vs_oracle(monkeypatch):
    """4-layer stack at the model's width (hidden 2048, 16 heads) with the model's MLP width (I = 11008: the fused gate|up
    kernel in every layer), 4 graphed 256-token steps over a 1024-key window, against the oracle's
    reference-rounding model and its exact fp32 run, with the bounds of the real-width long-horizon test."""
    import test_gpu_longhorizon as lh
    small = parity.small_configs

    def wide(window, n_layers=4, heads=2):
        hc, oc = small(window, n_layers=n_layers, heads=heads)
        hc.intermediate_size = 11008
        oc.intermediate_size = 11008
        return hc, oc
    monkeypatch.setattr(parity, "small_configs", wide)
    from infinitevl_amd import ops
    launched = []
    fused = ops._linear_swiglu_m256

    def counting(*a):
        launched.append(a[0].shape)
        return fused(*a)
    monkeypatch.setattr(ops, "_linear_swiglu_m256", counting)       # the captured step must take the fused kernel
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(nthr, 16))
    try:
        at, per_step = lh._stream_stack(4, 256, 1024, checkpoints={1, 4}, heads=16)
    finally:
        torch.set_num_threads(nthr)
    assert len(launched) >= 4 and all(sh[-2:] == (256, 2048) for sh in launched), launched   # one per layer at least
    for step, r in sorted(at.items()):
        print(f"  step {step}: hidden hip-model {r['h_vs_model']:.2e} hip-exact {r['h_vs_exact']:.2e} model-exact {r['model_vs_exact']:.2e}")
        assert r["finite"] and r["pos_dev"] == step * 256, (step, r)
        assert r["h_vs_model"] < 2.5e-2 and r["h_vs_exact"] < 1.25 * r["model_vs_exact"] + 1e-3, (step, r)
        assert r["state_vs_exact"] < 1.5 * r["state_model_vs_exact"] + 1e-3 and r["state_vs_model"] < 4e-2, (step, r)

"""Float64 reference and judge of the scoring path (tests/test_scoring_cpu.py, tests/test_gpu_scoring.py): the log-probability of
given tokens under bf16 logits, with the edge conventions of ivl_linear_logprob_m256_fwd (include/ivl_hip.h, S1-S5):
  a NaN logit counts as -inf; m = the row maximum; w_c = exp(x_c - m), exactly 1 where x_c == m (also at m = +-inf), 0 where
  x_c = -inf < m; Z = sum w_c (= N in a row of nothing but -inf / NaN); lse = m + log Z (= m when m is infinite);
  logprob = (x_target - m) - log Z (= -log Z on the maximum, -inf on a -inf below it); a target outside [0, N) gives 0.0;
  top1 = the lowest index with x == m (0 in the all -inf row)."""
import torch

NEG_INF = float("-inf")


def tolerance(ref: torch.Tensor) -> torch.Tensor:
    """|err| <= 1e-5 + 2^-22 |ref|: <= 2 ulp per expf, 64-term fp32 partial sums (<= 64 * 2^-24 relative), a float64 combine,
    1 ulp of logf, one rounding of the difference.  Derived, not measured."""
    return 1e-5 + 2.0 ** -22 * ref.abs()


def ref_logprob(logits: torch.Tensor, target: torch.Tensor):
    """(logprob, top1, lse) in float64 / int64 on the CPU from logits [M,N] (any float dtype; used as they are) and target [M]."""
    x = logits.detach().cpu().double()
    t = target.detach().cpu().to(torch.int64)
    M, N = x.shape
    x = torch.where(torch.isnan(x), torch.full_like(x, NEG_INF), x)
    m = x.max(dim=1).values
    at_max = x == m[:, None]
    # exp(x - m) with the conventions: exactly 1 on the maximum (the only place where x - m can be inf - inf: discarded there);
    # below it x - m is finite or -inf (x = -inf, or m = +inf), and exp gives the 0 the convention asks for
    w = torch.where(at_max, torch.ones_like(x), torch.exp(x - m[:, None]))
    Z = w.sum(dim=1)
    logZ = torch.log(Z)
    lse = torch.where(torch.isinf(m), m, m + logZ)
    top1 = at_max.to(torch.int64).argmax(dim=1)                          # the first True of each row
    scored = (t >= 0) & (t < N)
    xt = x.gather(1, t.clamp(0, N - 1)[:, None])[:, 0]
    on_max = xt == m
    diff = torch.where(on_max, torch.zeros_like(xt), xt - m)
    lp = torch.where(scored, diff - logZ, torch.zeros_like(xt))
    return lp, top1, lse


def judge(got: torch.Tensor, ref: torch.Tensor, what: str = "", scale: float = 1.0) -> float:
    """Assert |got - ref| <= scale * tolerance(ref) element-wise, infinities and exact zeros matching exactly; returns the
    largest observed ratio err / tolerance over the finite elements."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert not bool(torch.isnan(g).any()), (what, "NaN in the result")
    inf = torch.isinf(r)
    assert torch.equal(g[inf], r[inf]), (what, "infinite entries differ", g[inf][:8], r[inf][:8])
    assert not bool(torch.isinf(g[~inf]).any()), (what, "infinite where the reference is finite")
    if not bool((~inf).any()):
        return 0.0
    ratio = ((g[~inf] - r[~inf]).abs() / tolerance(r[~inf])).max().item()
    assert ratio <= scale, (what, f"max |err| / tolerance = {ratio:.3f} (allowed {scale})")
    return ratio


def blocked_emulation(logits_bf16: torch.Tensor) -> torch.Tensor:
    """The kernel's arithmetic on the CPU for rows of bf16 logits [M,N]: per 64-column block the maximum and an fp32 sum of
    fp32 exp(x - m_j), then a float64 combine, fp32 log.  Returns lse fp32 [M] (finite rows only)."""
    x = logits_bf16.float()
    M, N = x.shape
    pad = (-N) % 64
    if pad:
        x = torch.cat([x, torch.full((M, pad), NEG_INF)], dim=1)
    xb = x.view(M, -1, 64)
    mj = xb.max(dim=2).values
    zj = torch.zeros_like(mj)
    e = torch.exp(xb - mj[:, :, None])                                   # fp32
    for c in range(64):                                                 # a sequential fp32 sum: the worst order
        zj = zj + e[:, :, c]
    m = mj.max(dim=1).values
    Z = (zj.double() * torch.exp(mj.double() - m.double()[:, None])).sum(dim=1)
    return m + torch.log(Z.float())


def shifted_by_hand(labels, next_label=None):
    """The label shift as a plain Python loop over a list: position t takes labels[t + 1], the last one next_label or -100."""
    labels = [int(v) for v in labels]
    return [labels[t + 1] for t in range(len(labels) - 1)] + [-100 if next_label is None else int(next_label)]


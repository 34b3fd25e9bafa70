// Online softmax of the 64-key attention tile, part 2 (part 1: tile64_probs, attn_tile64.h): the row's running state takes the
// tile's probabilities `t`.  Included inside the per-query-group loop of the tile loops of swa_fwd_kernel and vision_attn_kernel.
// A text fragment and not a function: as a __forceinline__ template that holds oacc[qg] by reference the branch is inlined late
// and vision_attn_kernel<128, 2> goes from 253 to 256 VGPRs with scratch (so did the whole phase as one function).
// Expects in scope: qg, t (Tile64Probs), m_run[QG], l_run[QG], oacc[QG][NDT], pf[QG][2].
  if (__any(t.m_new > m_run[qg])) {                                  // some row's running maximum moved: rescale (exact)
    const float alpha = __builtin_amdgcn_exp2f(m_run[qg] - t.m_use);   // m_run = -inf -> 0
    l_run[qg] = l_run[qg] * alpha + t.rsum;
    for (f32x4& o : oacc[qg]) o *= alpha;
  } else {
    l_run[qg] += t.rsum;
  }
  m_run[qg] = t.m_new;
  pf[qg][0] = t.pf0;
  pf[qg][1] = t.pf1;

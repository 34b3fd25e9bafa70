// Body of the one-launch GDN decode step (gdn_decode.hip), included inside the two kernel functions that share it:
// gdn_decode_step_kernel (GDN_HOLD 0) and gdn_decode_step_rows_kernel (GDN_HOLD 1: `frozen`, int32[B], in scope -- the workgroup of a
// frozen batch row leaves before its first state load).  Textual inclusion keeps the generated code of gdn_decode_step_kernel exactly
// what it was when the body was written inside it (a __forceinline__ device function is inlined later in the optimisation pipeline
// and changes its register allocation).  Expects: the DEC_HEAD_PARAMS and p (DecParams) in scope, GDN_HOLD defined.
  DEC_HEAD_APPLY(p);
#if GDN_HOLD
  if (frozen[blockIdx.x / hd_H] != 0) return;        // workgroup-uniform, ahead of every load and barrier (HOLD-1)
#endif
  __shared__ __attribute__((aligned(16))) float s_k[DK], s_q[DK], s_v[DV];
  __shared__ __attribute__((aligned(16))) float s_red[DNW][2][DV];
  __shared__ float s_part[4][2];
  __shared__ float s_sc[4];          // decay, beta, k.q

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const bf16_t* xrow = p.proj + (long long)b * p.ld;

  // ---- state rows of this wave: issue every load up front --------------------------------------------
  float S[DRW][4];
  const size_t sbase = ((size_t)bh * DK + DRW * wave) * DV + 4 * lane;
  if (p.state_dtype == IVL_F32) {
    const float* sp = (const float*)p.state + sbase;
#pragma unroll
    for (int r = 0; r < DRW; ++r) {
      const f32x4 v4 = *(const f32x4*)(sp + (size_t)r * DV);
      S[r][0] = v4[0]; S[r][1] = v4[1]; S[r][2] = v4[2]; S[r][3] = v4[3];
    }
  } else {
    const bf16_t* sp = (const bf16_t*)p.state + sbase;
    u32x2 raw[DRW];
#pragma unroll
    for (int r = 0; r < DRW; ++r) raw[r] = *(const u32x2*)(sp + (size_t)r * DV);
#pragma unroll
    for (int r = 0; r < DRW; ++r) {
      S[r][0] = bflo(raw[r].x); S[r][1] = bfhi(raw[r].x); S[r][2] = bflo(raw[r].y); S[r][3] = bfhi(raw[r].y);
    }
  }

  // ---- convs: thread t -> q channel t (t < 128) or k channel t-128, and v channel t -------------------
  const int Dq = p.H * DK, Dv = p.H * DV;
  float qk = 0.f;
  if (tid >= 2 * DK) {
    // waves 4..7 only hold state rows; the 256 conv / l2norm lanes are waves 0..3
  } else if (tid < DK) qk = conv1(xrow, p.col_q + h * DK + tid, p.wq, h * DK + tid, p.cq, (size_t)b * Dq + h * DK + tid);
  else qk = conv1(xrow, p.col_k + h * DK + (tid - DK), p.wk, h * DK + tid - DK, p.ck, (size_t)b * Dq + h * DK + (tid - DK));
  if (tid < DV) s_v[tid] = conv1(xrow, p.col_v + h * DV + tid, p.wv, h * DV + tid, p.cv, (size_t)b * Dv + h * DV + tid);
  // l2norm: q in waves 0,1 ; k in waves 2,3
  if (wave < 4) {
    const float ss = wave_sum(qk * qk);
    if (lane == 0) s_part[wave][0] = ss;
  }
  if (tid == 0) {
    float g, beta;
    gdn_gate_(bf2f(xrow[p.col_a + h]), p.dt_bias[h], bf2f(xrow[p.col_b + h]), p.A_log + h, g, beta);
    s_sc[0] = __expf(g);
    s_sc[1] = bf_round(beta);                                           // the prologue stores beta in bf16
  }
  __syncthreads();
  if (tid < 2 * DK) {
    const float tot = tid < DK ? s_part[0][0] + s_part[1][0] : s_part[2][0] + s_part[3][0];
    const float nrm = bf_round(qk * (1.0f / sqrtf(tot + 1e-6f)));       // fla l2norm_fwd writes bf16
    if (tid < DK) s_q[tid] = nrm * p.scale;
    else s_k[tid - DK] = nrm;
  }
  __syncthreads();
  // k . (q*scale): every wave computes it redundantly (2 elements per lane)
  const float kq = wave_sum(s_k[2 * lane] * s_q[2 * lane] + s_k[2 * lane + 1] * s_q[2 * lane + 1]);

  // ---- decay + the two column reductions over the rows of this wave --------------------------------------
  const float decay = s_sc[0], beta = s_sc[1];
  float pk[4] = {0.f, 0.f, 0.f, 0.f}, pq[4] = {0.f, 0.f, 0.f, 0.f};
  float kk[DRW];
#pragma unroll
  for (int r4 = 0; r4 < DRW / 4; ++r4) {
    const f32x4 k4 = *(const f32x4*)&s_k[DRW * wave + 4 * r4];
    const f32x4 q4 = *(const f32x4*)&s_q[DRW * wave + 4 * r4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * r4 + i;
      kk[r] = k4[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        S[r][c] *= decay;
        pk[c] = fmaf(S[r][c], k4[i], pk[c]);
        pq[c] = fmaf(S[r][c], q4[i], pq[c]);
      }
    }
  }
  *(f32x4*)&s_red[wave][0][4 * lane] = f32x4{pk[0], pk[1], pk[2], pk[3]};
  *(f32x4*)&s_red[wave][1][4 * lane] = f32x4{pq[0], pq[1], pq[2], pq[3]};
  __syncthreads();
  float o4[4], delta[4];
  {
    f32x4 kv = *(const f32x4*)&s_red[0][0][4 * lane], oq = *(const f32x4*)&s_red[0][1][4 * lane];
#pragma unroll
    for (int w = 1; w < DNW; ++w) {
      kv += *(const f32x4*)&s_red[w][0][4 * lane];
      oq += *(const f32x4*)&s_red[w][1][4 * lane];
    }
    const f32x4 v4 = *(const f32x4*)&s_v[4 * lane];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      delta[c] = beta * (v4[c] - kv[c]);
      o4[c] = bf_round(fmaf(delta[c], kq, oq[c]));            // the recurrent kernel stores o in bf16
    }
  }
  // ---- state update + write-back -------------------------------------------------------------------
#pragma unroll
  for (int r = 0; r < DRW; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) S[r][c] = fmaf(kk[r], delta[c], S[r][c]);
  if (p.state_dtype == IVL_F32) {
    float* sp = (float*)p.state + sbase;
#pragma unroll
    for (int r = 0; r < DRW; ++r) *(f32x4*)(sp + (size_t)r * DV) = f32x4{S[r][0], S[r][1], S[r][2], S[r][3]};
  } else {
    bf16_t* sp = (bf16_t*)p.state + sbase;
#pragma unroll
    for (int r = 0; r < DRW; ++r) *(u32x2*)(sp + (size_t)r * DV) = u32x2{pack2bf(S[r][0], S[r][1]), pack2bf(S[r][2], S[r][3])};
  }
  // ---- gated RMSNorm over the head's 256 outputs (every wave holds all of them, 4 per lane) -----------
  if (wave == 0) {
    const float ss = wave_sum(o4[0] * o4[0] + o4[1] * o4[1] + o4[2] * o4[2] + o4[3] * o4[3]);
    const float rstd = rms256_rstd_(ss, p.eps);
    const u32x2 wv = *(const u32x2*)(p.norm_w + 4 * lane);
    const u32x2 gv = *(const u32x2*)(xrow + p.col_g + h * DV + 4 * lane);
    const float wf[4] = {bflo(wv.x), bfhi(wv.x), bflo(wv.y), bfhi(wv.y)};
    const float gf[4] = {bflo(gv.x), bfhi(gv.x), bflo(gv.y), bfhi(gv.y)};
    float y4[4];
    gated_norm_n_(o4, rstd, wf, gf, y4);
    *(u32x2*)(p.y + ((size_t)b * p.H + h) * DV + 4 * lane) = u32x2{pack2bf(y4[0], y4[1]), pack2bf(y4[2], y4[3])};
  }

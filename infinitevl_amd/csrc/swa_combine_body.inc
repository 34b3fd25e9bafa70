// Bodies of the split-KV combine kernels (swa.hip), included inside the kernel functions that share them: SWA_WIDE 0 the
// templated combine (NS, BF16P in scope), SWA_WIDE 1 the wide one; SWA_ROWS 1 (ivl_swa_decode_rows_fwd, ivl_swa_rows_fwd) appends every batch
// row at its own position (ring_append<1>); SWA_ROWS 2 (ivl_swa_decode_rows_hold_fwd, `frozen` in scope) also skips the merge, the o
// store and the ring slots of a frozen batch row.  Textual inclusion keeps the generated code of the pre-existing combine kernels
// exactly what it was when the bodies were written inside them.
// Expects: part_o, part_ml, o, B, rows_per_b, nsplit, ap in scope, SWA_WIDE and SWA_ROWS defined.
#if SWA_WIDE
  if (ap.first_block >= 0 && (int)blockIdx.x >= ap.first_block) {
#if SWA_ROWS == 2
    ring_append<2>(ap, (long long)blockIdx.x - ap.first_block, (long long)gridDim.x - ap.first_block, frozen);
#else
    ring_append<SWA_ROWS>(ap, (long long)blockIdx.x - ap.first_block, (long long)gridDim.x - ap.first_block);
#endif
    return;
  }
  // one WORKGROUP per row: wave w merges the splits 16w .. 16w + 15 (all 16 partial rows requested at once: one memory
  // round trip instead of nsplit / 8), the four partial sums meet in LDS
  __shared__ float2 red[4][64];
  const int ncb = ap.first_block >= 0 ? ap.first_block : (int)gridDim.x;       // combine blocks
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = blockIdx.x; r < (long long)B * rows_per_b; r += ncb) {
    int rr_;
    const long long b = divmod_idx(r, rows_per_b, rr_), rr = rr_;
#if SWA_ROWS == 2
    if (frozen[b] != 0) continue;        // uniform over the row's workgroup / wavefront: its partials were never written
#endif
    const bool on = lane < nsplit;
    const float2 ml = *(const float2*)(part_ml + ((b * nsplit + (on ? lane : 0)) * rows_per_b + rr) * 2);
    float2 ov[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s2 = min(16 * wave + j, nsplit - 1);
      ov[j] = *(const float2*)(part_o + ((b * nsplit + s2) * rows_per_b + rr) * SWA_D + 2 * lane);
    }
    const float ms = on ? ml.x : -INFINITY;
    float m = ms;
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) m = fmaxf(m, __shfl_xor(m, ofs, 64));
    const float w = ms == -INFINITY ? 0.f : exp2f(ms - m);
    const float l = wave_sum(w * (on ? ml.y : 0.f));
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s2 = 16 * wave + j;
      const float ws = s2 < nsplit ? __shfl(w, s2, 64) : 0.f;
      a0 = fmaf(ws, ov[j].x, a0);
      a1 = fmaf(ws, ov[j].y, a1);
    }
    red[wave][lane] = float2{a0, a1};
    __syncthreads();
    if (wave == 0) {
      const float2 p1 = red[1][lane], p2 = red[2][lane], p3 = red[3][lane];
      const float inv = l > 0.f ? 1.0f / l : 0.f;
      *(unsigned int*)(o + r * SWA_D + 2 * lane) = pack2bf((a0 + p1.x + p2.x + p3.x) * inv, (a1 + p1.y + p2.y + p3.y) * inv);
    }
    __syncthreads();
  }
#else
  if (ap.first_block >= 0 && (int)blockIdx.x >= ap.first_block) {
#if SWA_ROWS == 2
    ring_append<2>(ap, (long long)blockIdx.x - ap.first_block, (long long)gridDim.x - ap.first_block, frozen);
#else
    ring_append<SWA_ROWS>(ap, (long long)blockIdx.x - ap.first_block, (long long)gridDim.x - ap.first_block);
#endif
    return;
  }
  const int ncb = ap.first_block >= 0 ? ap.first_block : (int)gridDim.x;       // combine blocks
  const int lane = threadIdx.x & 63;
  const long long wid = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)ncb * blockDim.x) >> 6;
  for (long long r = wid; r < (long long)B * rows_per_b; r += nw) {
    int rr_;
    const long long b = divmod_idx(r, rows_per_b, rr_), rr = rr_;
#if SWA_ROWS == 2
    if (frozen[b] != 0) continue;        // uniform over the row's workgroup / wavefront: its partials were never written
#endif
    float ms[NS], ls[NS];
    float2 ov[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bool on = s < nsplit;
      const long long pr = (b * nsplit + (on ? s : 0)) * rows_per_b + rr;
      const float2 ml = *(const float2*)(part_ml + pr * 2);
      ms[s] = on ? ml.x : -INFINITY;
      ls[s] = on ? ml.y : 0.f;
      if (BF16P) {
        const unsigned int w2 = *(const unsigned int*)((const bf16_t*)part_o + pr * SWA_D + 2 * lane);
        ov[s] = float2{bflo(w2), bfhi(w2)};
      } else {
        ov[s] = *(const float2*)(part_o + pr * SWA_D + 2 * lane);
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < NS; ++s) m = fmaxf(m, ms[s]);
    float l = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float w = ms[s] == -INFINITY ? 0.f : exp2f(ms[s] - m);
      if (BF16P) w *= ls[s];
      l = BF16P ? l + w : fmaf(w, ls[s], l);
      a0 = fmaf(w, ov[s].x, a0);
      a1 = fmaf(w, ov[s].y, a1);
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    *(unsigned int*)(o + r * SWA_D + 2 * lane) = pack2bf(a0 * inv, a1 * inv);
  }
#endif

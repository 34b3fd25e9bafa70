// Body of the 64-row attention kernel (swa.hip), included inside the kernel functions that share it: swa_fwd_kernel<PACK, QG>
// (SWA_ROWS 0: pos_dev is a scalar position, or NULL for p.pos), swa_rows_decode_kernel and swa_rows_fwd_kernel (SWA_ROWS 1: pos_dev
// is an int64[B], one ring position per batch row; PACK = true resp. false; SWA_ROWS 2, swa_rows_hold_decode_kernel: the same with `frozen` (int32[B]) in scope -- the
// workgroups of a frozen batch row leave before their first load, ahead of every barrier).  Textual inclusion keeps the generated code of swa_fwd_kernel exactly what it was when the
// body was written inside it (a __forceinline__ device function is inlined later in the optimisation pipeline and changes it).
// Expects: PACK, QG (compile-time), pos_dev, p (SwaParams) in scope, SWA_ROWS defined.  The tile phases are attn_tile64.h's.
  __shared__ __attribute__((aligned(16))) unsigned char smem[SWA_LDS_BYTES];
  constexpr int QT = SWA_QT * QG;      // query rows per workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int G = p.Hq / p.Hkv;
  // 1-D grid with an XCD-aware (bijective) remap: hardware block id i runs on XCD i % 8; logical ids are
  // ordered (b, split, kv-head, head-in-group, q-tile) so the workgroups that read the SAME K/V range are
  // consecutive and therefore land on the same XCD / L2 (they re-read each K/V tile up to 8 x n_qtiles times).
  const int heads_y = PACK ? p.Hkv : p.Hq;
  int bx, rest;                      // q-tile, and (b * nsplit + split) * heads_y + head
  {
    const int nwg = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int qn = nwg >> 3, rn = nwg & 7;
    if (rn == 0 && qn % p.n_qtiles == 0) {
      // every XCD owns whole (batch, split, head) rows.  Inside an XCD the workgroups are issued heaviest first
      // (the work of a q-tile grows with its index: causal / window not yet full), so the long workgroups no
      // longer form the tail.  When all of them are co-resident (<= 2 per CU) the upper half goes first in
      // descending order and the lower half follows in ascending order: a heavy one shares its CU with a light one.
      const int hx = qn / p.n_qtiles;                       // rows per XCD
      const int r = slot / hx, half = (p.n_qtiles + 1) >> 1;
      bx = qn > 64 ? p.n_qtiles - 1 - r : (r < half ? p.n_qtiles - 1 - r : r - half);
      rest = xcd * hx + slot % hx;
    } else {
      const int lid = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
      bx = lid % p.n_qtiles;
      rest = lid / p.n_qtiles;
    }
  }
  const int by = rest % heads_y;                         // q head (or kv head when PACK); heads of one group adjacent
  const int bz = rest / heads_y;                         // b * nsplit + split
  const int b = bz / p.nsplit, split = bz % p.nsplit;
  const int hk = PACK ? by : by / G;
#if SWA_ROWS == 2
  if (frozen[b] != 0) return;          // workgroup-uniform (HOLD-1): no q / ring read, no partial written
#endif
  IVL_T(tr_start);
#ifdef IVL_TRACE
  const long long rt_start = (long long)__builtin_amdgcn_s_memrealtime();
#endif
  IVL_TVAR(tr_b1); IVL_TVAR(tr_st); IVL_TVAR(tr_qk); IVL_TVAR(tr_sm); IVL_TVAR(tr_pv);

  const long long pos = SWA_ROWS ? pos_dev[b] : (pos_dev ? *pos_dev : p.pos);
  const int n_ring = p.C > 0 ? (int)(pos < (long long)p.C ? pos : (long long)p.C) : 0;
  const int n_extra = p.T_new - p.T;
  const int n_prev = n_ring + n_extra;
  const int S = n_prev + p.T;
  const int s0 = p.C > 0 ? mod_pos(pos - n_ring, p.C) : 0;      // ring slot of call-local key 0

  // ---- rows of this workgroup / wave / lane ----------------------------------------------------
  const int total_rows = PACK ? p.T * G : p.T;
  const int tile_row0 = bx * QT;
  int t_row[QG], hq[QG], hi[QG], lo[QG];
  bool row_ok[QG];
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    const int row = tile_row0 + (wave * QG + qg) * 16 + l15;
    row_ok[qg] = row < total_rows;
    t_row[qg] = PACK ? row / G : row;
    hq[qg] = PACK ? hk * G + row % G : by;
    hi[qg] = n_prev + t_row[qg];
    lo[qg] = p.W > 0 ? max(0, n_prev + t_row[qg] - p.W + 1) : 0;
  }

  // band extremes over the rows of THIS wave (rows are consecutive; lo/hi are monotone in the row index)
  int w_lo_max, w_hi_min;
  {
    const int wr0 = tile_row0 + wave * 16 * QG;
    const int wr1 = min(wr0 + 16 * QG - 1, total_rows - 1);
    const int t_first = PACK ? wr0 / G : wr0;
    const int t_last = PACK ? max(wr1, wr0) / G : max(wr1, wr0);
    w_hi_min = n_prev + t_first;
    w_lo_max = p.W > 0 ? max(0, n_prev + t_last - p.W + 1) : 0;
  }

  // workgroup key-tile range
  const int last_row = min(tile_row0 + QT, total_rows) - 1;
  const int t_min = PACK ? tile_row0 / G : tile_row0;
  const int t_max = PACK ? last_row / G : last_row;
  const int lo_min = p.W > 0 ? max(0, n_prev + t_min - p.W + 1) : 0;
  const int kt0 = lo_min / SWA_KT, kt1 = (n_prev + t_max) / SWA_KT + 1;
  const int per = (kt1 - kt0 + p.nsplit - 1) / p.nsplit;
  const int kt_begin = kt0 + split * per;
  const int kt_end = min(kt1, kt_begin + per);

  // ---- Q fragments (B operand of S^T = K Q^T): lane = query row, k-slots 8g..8g+7 of each 32-chunk ----
  u32x4 qf[QG][4];
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    const bf16_t* qp = p.q + (long long)b * p.q_sb + (long long)t_row[qg] * p.q_st + (long long)hq[qg] * p.q_sh;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (row_ok[qg]) qf[qg][ks] = *(const u32x4*)(qp + 32 * ks + 8 * g);
      else qf[qg][ks] = u32x4{0u, 0u, 0u, 0u};
    }
  }

  const long long rplane = (long long)p.B * p.T * SWA_D;
  if (p.rcos != nullptr) {
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      const long long row_off = ((long long)b * p.T + min(t_row[qg], p.T - 1)) * SWA_D;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) rope_pair(qf[qg][ks], qf[qg][ks + 2], p.rcos, p.rsin, rplane, row_off, 32 * ks + 8 * g, p.rs0, p.rs1);
    }
  }
  float m_run[QG], l_run[QG];
  f32x4 oacc[QG][8];
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    m_run[qg] = -INFINITY;
    l_run[qg] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) oacc[qg][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging: thread -> rows (tid>>4) + 16 i, 16-byte chunk tid&15 ------------------------------
  const int srow = tid >> 4, schunk = tid & 15;
  u32x4 kreg[4], vreg[4];
  // per-(batch, kv-head) base pointers; rows are addressed with 32-bit element offsets from them
  const bf16_t* kb_ring = p.C > 0 ? p.k_cache + (((long long)b * p.Hkv + hk) * p.C) * SWA_D + schunk * 8 : p.k_new;
  const bf16_t* vb_ring = p.C > 0 ? p.v_cache + (((long long)b * p.Hkv + hk) * p.C) * SWA_D + schunk * 8 : p.v_new;
  const bf16_t* kb_new = p.k_new + (long long)b * p.kn_sb + (long long)hk * p.kn_sh + schunk * 8;
  const bf16_t* vb_new = p.v_new + (long long)b * p.kn_sb + (long long)hk * p.kn_sh + schunk * 8;
  const unsigned int kn_st32 = (unsigned int)p.kn_st;
  // the call's new keys arrive un-rotated when the rope is fused: thread (row, 16-byte chunk) fetches the partner chunk
  // (channels +-64) and the row's cos / sin and rotates its chunk in place (only the few tiles that hold new keys pay this)
  auto rope_new_key = [&](u32x4& kv, int jn /* index among the new keys */) {
    const int lo_ch = (schunk & 7) * 8;                    // channel block of the "lo" half of the pair
    const u32x4 part = *(const u32x4*)(kb_new - schunk * 8 + (unsigned int)jn * kn_st32 + (schunk ^ 8) * 8);
    u32x4 lo = schunk < 8 ? kv : part, hi = schunk < 8 ? part : kv;
    rope_pair(lo, hi, p.rcos, p.rsin, rplane, ((long long)b * p.T + jn) * SWA_D, lo_ch, p.rs0, p.rs1);
    kv = schunk < 8 ? lo : hi;
  };
  auto load_tile = [&](int kt) {
    const int j0 = kt * SWA_KT;
    const int slot0 = s0 + j0;
    if (j0 + SWA_KT <= n_ring && (slot0 + SWA_KT <= p.C || slot0 >= p.C)) {
      // wave-uniform fast path (almost every tile of a full window): 64 consecutive ring slots, no wrap inside
      const unsigned int off = (unsigned int)((slot0 >= p.C ? slot0 - p.C : slot0) + srow) * SWA_D;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        kreg[i] = *(const u32x4*)(kb_ring + off + 16 * i * SWA_D);
        vreg[i] = *(const u32x4*)(vb_ring + off + 16 * i * SWA_D);
      }
      return;
    }
    if (j0 >= n_ring && j0 + SWA_KT <= S) {
      // wave-uniform fast path: 64 keys of this call
      const unsigned int off = (unsigned int)(j0 - n_ring + srow) * kn_st32;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        kreg[i] = *(const u32x4*)(kb_new + off + 16 * i * kn_st32);
        vreg[i] = *(const u32x4*)(vb_new + off + 16 * i * kn_st32);
      }
      if (p.rcos != nullptr) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rope_new_key(kreg[i], j0 - n_ring + srow + 16 * i);
      }
      return;
    }
    // generic tile (ring wrap, ring/new seam or tail).  Branch-free per row: every row issues its two 16-byte
    // loads (clamped address); a conditional load per row would serialise one memory round trip per row.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + srow + 16 * i;
      const int jc = min(j, S - 1);
      const bool in_ring = jc < n_ring;
      int slot = s0 + jc;
      slot = slot >= p.C ? slot - p.C : slot;
      const unsigned int off = in_ring ? (unsigned int)slot * SWA_D : (unsigned int)(jc - n_ring) * kn_st32;
      const bf16_t* kp = (in_ring ? kb_ring : kb_new) + off;
      const bf16_t* vp = (in_ring ? vb_ring : vb_new) + off;
      kreg[i] = *(const u32x4*)kp;
      vreg[i] = *(const u32x4*)vp;
      if (p.rcos != nullptr && !in_ring) rope_new_key(kreg[i], jc - n_ring);
    }
    if (j0 + SWA_KT > S) {          // wave-uniform: tail tile, rows >= S are zeroed
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (j0 + srow + 16 * i >= S) {
          kreg[i] = u32x4{0u, 0u, 0u, 0u};
          vreg[i] = u32x4{0u, 0u, 0u, 0u};
        }
    }
  };
  if (kt_begin < kt_end) load_tile(kt_begin);
  const float sc = p.scaling * LOG2E;
  IVL_T(tr_loop);

  for (int kt = kt_begin; kt < kt_end; ++kt) {
    IVL_T(tr0);
    __syncthreads();
    IVL_T(tr1);
    tile64_stage<SWA_VSTRIDE>(smem, srow, schunk, kreg, vreg);
    __syncthreads();
    IVL_T(tr2);

    f32x4 sacc[QG][4];
    tile64_qk<4, QG>(smem, l15, g, qf, sacc);
    // next tile's global loads are issued behind the first MFMA batch (their address arithmetic no longer
    // delays it); they have the softmax + PV phases to land before the stage store of the next iteration
    if (kt + 1 < kt_end) load_tile(kt + 1);
    IVL_T(tr3);
    // ---- band mask + online softmax (lane-local rows) -----------------------------------------
    // Interior tiles (every key visible to every row of this wave) skip the per-element band test.
    const int jbase = kt * SWA_KT + 4 * g;
    const bool interior = kt * SWA_KT >= w_lo_max && kt * SWA_KT + SWA_KT - 1 <= w_hi_min;
    u32x4 pf[QG][2];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
      if (!interior) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jbase + 16 * mt + r;
            const bool vis = row_ok[qg] && j >= lo[qg] && j <= hi[qg];
            sacc[qg][mt][r] = vis ? sacc[qg][mt][r] : -INFINITY;
          }
      }
      const Tile64Probs t = tile64_probs<true>(sacc[qg][0], sacc[qg][1], sacc[qg][2], sacc[qg][3], sc, m_run[qg]);
#include "attn_tile64_rescale.inc"
    }
    IVL_T(tr4);
    tile64_pv<8, QG, SWA_VSTRIDE>(smem, l15, g, pf, oacc);
    IVL_T(tr5);
    IVL_TACC(tr_b1, tr1, tr0); IVL_TACC(tr_st, tr2, tr1); IVL_TACC(tr_qk, tr3, tr2); IVL_TACC(tr_sm, tr4, tr3); IVL_TACC(tr_pv, tr5, tr4);
  }
  IVL_T(tr_end);

  // ---- epilogue: lane owns its rows, d = 16 mt2 + 4g + r ----------------------------------------
#pragma unroll
  for (int qg = 0; qg < QG; ++qg) {
    if (!row_ok[qg]) continue;
    if (p.nsplit == 1) {
      tile64_store_row<8, true>(p.o + (((long long)b * p.T + t_row[qg]) * p.Hq + hq[qg]) * SWA_D + 4 * g, oacc[qg], l_run[qg]);
    } else {
      const long long prow = (((long long)b * p.nsplit + split) * p.T + t_row[qg]) * p.Hq + hq[qg];
      tile64_store_partial(p.part_o + prow * SWA_D + 4 * g, p.part_ml + prow * 2, g, oacc[qg], m_run[qg], l_run[qg]);
    }
  }
  IVL_T(tr_fin);
  IVL_TOUT(32, tr_loop - tr_start); IVL_TOUT(33, tr_b1); IVL_TOUT(34, tr_st); IVL_TOUT(35, tr_qk); IVL_TOUT(36, tr_sm);
#ifdef IVL_TRACE
  IVL_TOUT(41, (long long)__builtin_amdgcn_s_memrealtime() - rt_start);
#endif
  IVL_TOUT(37, tr_pv); IVL_TOUT(38, tr_fin - tr_end); IVL_TOUT(39, tr_fin - tr_start); IVL_TOUT(40, kt_end - kt_begin);

// y[M,N] = x[M,K] W[N,K]^T (+ bias), bf16 in / fp32 accumulate / bf16 out, for M <= 256 rows: the wide projections of a
// 256-token prefill chunk.  The package dispatches the GLU form -- the fused MLP gate|up with the SwiGLU gate in the epilogue,
// 32.5 us against 39.7 for library GEMM + silu_mul at 256 x 22016 x 2048 (tools/ab_linear_m256.py, same box).  The plain
// form on the GDN in-projection (256 x 12320 x 2048) loses to the library (22.6 against 20.7 us) and is not dispatched.
//
// Decomposition: ONE workgroup per column range with ALL (up to 256) rows -- no K split, no reduction across workgroups, no
// workspace, no inter-workgroup signalling; the same bits on every run.  The column range is chosen so that the grid is one
// wave of workgroups over the 256 CUs: the plain form takes 64 weight rows (N = 12320: 193 workgroups), the GLU form 48 output
// columns = 48 gate rows + the 48 matching up rows (I = 11008: 230 workgroups; the fused [2I, K] weight is not re-packed).
//
// Every workgroup re-reads all of x (1 MB at K = 2048, served by L2) beside its own 0.39 MB of weights.  Both operands are
// k-contiguous and are staged the same way: per K-tile of 64, 1 KB LDS-DMA pieces (global_load_lds_dwordx4: 8 rows x one full
// 128-byte line, no VGPR round trip) into a [rows][128 B] image whose 16-byte chunks are XOR-swizzled on the SOURCE side (chunk c of
// row r stored at c ^ ((r >> 1) & 7): the ds_read_b128 fragment reads of 16 consecutive rows hit 16 distinct bank slots).  A ring of
// L256_STAGES stages; one barrier per tile, behind a counted vmcnt that leaves the later tiles' pieces in flight.  The DMA is inline asm
// the compiler does not track, and the loop holds no other vector-memory load, so no compiler-inserted vmcnt(0) drains the ring.
// Counters: HBM 0.46, MFMA 0.27, TA ~0.42 busy -- no unit saturated; latency-bound with two tiles in flight.
// L256_WG_ROWS / L256_STAGES / L256_W_NT select the variants measured there (developer A/B builds; the defaults are what ships).
//
// ROWS / 32 waves: wave w owns x rows 32w .. 32w + 31 (the B operand, two 16-row fragments) and every weight row of the workgroup (the A
// operand), v_mfma_f32_16x16x32_bf16.  With the weight rows on the MFMA's row axis a lane ends up holding 4 CONSECUTIVE output
// columns of one x row: one 8-byte store per lane and fragment, written through (store_out8: the consumer is the next kernel).
//
// GLU epilogue: act = bf16( bf16(silu(g)) * u ) with g, u the accumulators rounded to bf16 -- the arithmetic of silu_mul_kernel
// (and of linear_small_m_kernel's GLU form), so the fused output is bit-equal to the plain output followed by ivl_silu_mul_fwd.
//
// SCORE epilogue (ivl_linear_logprob_m256_fwd: the log-probability of a GIVEN token under lm_head, the logits never written): the
// plain form's configuration; the accumulators are rounded to the bf16 logits the plain form would store, and the 64 columns of a
// row -- 16 in each of the lanes l, l + 16, l + 32, l + 48 -- are reduced in registers and by two xor-shuffles to one partial
// {max, sum exp(x - max), lowest index of the max} per (column block, row), one 16-byte store; the lane that owns column
// target[row] stores that logit.  logprob_combine_kernel (one workgroup per row) merges the ceil(N / 64) partials in float64 in a
// fixed order.  No atomics, no LDS beyond the ring; the plain and GLU
// instantiations are untouched by it.
#include "ivl_common.h"

namespace ivl {

constexpr int L256_ROWS = 256;                 // x rows of a call (at most)
constexpr int L256_BK = 64;                    // K-tile: one 128-byte line per row
constexpr int L256_KMAX = 16384;
#ifndef L256_WG_ROWS
#define L256_WG_ROWS 256                       // x rows per workgroup: 256 (all) or 128 (two workgroups per column range, one XCD)
#endif
#ifndef L256_STAGES
#define L256_STAGES 3                          // ring stages (tiles requested STAGES - 1 ahead)
#endif
#ifndef L256_W_NT
#define L256_W_NT 1                            // the GLU form requests its weight pieces non-temporal (each weight byte is read once):
#endif                                         // 33.9 -> 32.5 us; the plain form keeps the default policy (nt: 22.6 -> 25.3 us)

template <bool GLU, int ROWS, int NST>
struct L256Cfg {
  static constexpr int NCOL = GLU ? 48 : 64;                   // output columns per workgroup
  static constexpr int NW = GLU ? 2 * NCOL : NCOL;             // weight rows per workgroup
  static constexpr int NT = NW / 16;                           // 16-row weight fragments
  static constexpr int WAVES = ROWS / 32;                      // a wave owns 32 x rows
  static constexpr int PIECES = (ROWS + NW) / 8;               // 1 KB DMA pieces per K-tile (x image first, then the weight rows)
  static constexpr int PW_MAX = (PIECES + WAVES - 1) / WAVES;  // pieces per wave: waves < PIECES % WAVES take one more
  static constexpr int STAGE = (ROWS + NW) * 128;              // bytes per ring stage
  static constexpr int LDS = NST * STAGE;
};

template <int N>
__device__ __forceinline__ void l256_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most `ahead` (< 3) tiles of this wave's pieces are still in flight; PW: this wave's pieces per tile
template <int PW>
__device__ __forceinline__ void l256_wait_tiles(int ahead) {
  if (ahead <= 0) l256_vmcnt<0>();
  else if (ahead == 1) l256_vmcnt<PW>();
  else l256_vmcnt<2 * PW>();
}

__device__ __forceinline__ const bf16_t* l256_uniform(const bf16_t* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v), hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
  return (const bf16_t*)(((unsigned long long)hi << 32) | lo);
}

// TARGET: empty (y = the bf16 output [M,N]), or one `const long long*` = the SCORE form: `target`, and y is the workspace
// (ceil(N/64) x M partials of 16 bytes, then M target logits).  The plain and GLU instantiations have the signature they always had.
template <bool GLU, int ROWS, int NST, bool WNT, typename... TARGET>
__global__ __launch_bounds__(ROWS * 2) void linear_m256_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                               const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int M, int N, int K,
                                                               TARGET... target_arg) {
  constexpr bool SCORE = sizeof...(TARGET) != 0;
  static_assert(!(SCORE && GLU) && sizeof...(TARGET) <= 1, "the SCORE epilogue is a plain-form epilogue");
  using C = L256Cfg<GLU, ROWS, NST>;
  static_assert(NST >= 2 && NST <= 3, "ring of 2 or 3 stages");
  constexpr int AHEAD = NST - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroup -> (column range, row block).  ROWS < 256: the row blocks of a column range are workgroups b and b + 8 of a group of
  // 16 -- the same XCD under round-robin placement (a speed choice only), so the second reads the weight rows from that XCD's L2
  int colblk = (int)blockIdx.x, r0 = 0;
  if constexpr (ROWS < L256_ROWS) {
    const int b = (int)blockIdx.x;
    colblk = (b >> 4) * 8 + (b & 7);
    r0 = ((b >> 3) & 1) * ROWS;
    if (colblk * C::NCOL >= N || r0 >= M) return;    // (whole workgroup, before any barrier)
  }
  const int n0 = colblk * C::NCOL;
  const int nkt = K / L256_BK;
  const unsigned int lds_base = (unsigned int)(size_t)smem;

  // ---- DMA pieces of this wave: p = wave + WAVES i.  Lane l moves the 16-byte chunk (l & 7) of row 8p + (l >> 3) of the stage
  // image; the chunk it stores there is logical chunk (l & 7) ^ swz(row).  Source offsets are relative to the K-tile's first
  // column and are the same for every tile (the tile advances the uniform base pointer).
  const bool pw_full = wave < C::PIECES % C::WAVES || C::PIECES % C::WAVES == 0;
  unsigned int src_off[C::PW_MAX];
#pragma unroll
  for (int i = 0; i < C::PW_MAX; ++i) {
    const int p = min(wave + C::WAVES * i, C::PIECES - 1);
    const int r = 8 * p + (lane >> 3);                           // row of the stage image
    const int c = (lane & 7) ^ ((r >> 1) & 7);                   // logical chunk stored at (lane & 7)
    long long grow;                                              // row of x / of w
    if (r < ROWS) {
      grow = min(r0 + r, M - 1);
    } else {
      const int j = r - ROWS;                                    // weight row of the workgroup
      if (GLU) grow = j < C::NCOL ? min(n0 + j, N - 1) : (long long)N + min(n0 + j - C::NCOL, N - 1);
      else grow = min(n0 + j, N - 1);
    }
    src_off[i] = (unsigned int)(grow * K * 2 + c * 16);
  }
  auto dma_tile = [&](int t) __attribute__((always_inline)) {
    const unsigned int dst0 = lds_base + (unsigned int)(t % NST) * C::STAGE;
    const bf16_t* xb = l256_uniform(x + (size_t)t * L256_BK);
    const bf16_t* wb = l256_uniform(w + (size_t)t * L256_BK);
#pragma unroll
    for (int i = 0; i < C::PW_MAX; ++i) {
      const int p = wave + C::WAVES * i;
      if (i == C::PW_MAX - 1 && p >= C::PIECES) break;            // (wave-uniform)
      const unsigned int dst = __builtin_amdgcn_readfirstlane(dst0 + 1024u * p);
      unsigned int keep;
      if (p < ROWS / 8 || !WNT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src_off[i]), "s"(dst), "s"(p < ROWS / 8 ? xb : wb) : "memory");
      else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3 nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src_off[i]), "s"(dst), "s"(wb) : "memory");
    }
  };

  // ---- fragment reads: lane l reads row (l & 15) of a 16-row fragment, chunk 4 s + (l >> 4) of k32-step s
  unsigned int frag_off[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) frag_off[s] = (unsigned int)((lane & 15) * 128 + (((4 * s + (lane >> 4)) ^ ((lane >> 1) & 7)) << 4));

  f32x4 acc[C::NT][2];
#pragma unroll
  for (int j = 0; j < C::NT; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int t = 0; t < AHEAD; ++t)
    if (t < nkt) dma_tile(t);
  for (int t = 0; t < nkt; ++t) {
    // tile t has landed for this wave's pieces; the barrier makes every wave's pieces visible and retires every wave's reads of
    // tile t - 1, whose stage tile t + AHEAD then reuses
    const int ahead = min(AHEAD - 1, nkt - 1 - t);
    if (pw_full) l256_wait_tiles<C::PW_MAX>(ahead);
    else l256_wait_tiles<C::PW_MAX - 1>(ahead);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + AHEAD < nkt) dma_tile(t + AHEAD);
    const unsigned char* st = smem + (t % NST) * C::STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 xf[2], wf[C::NT];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = *(const bf16x8*)(st + (32 * wave + 16 * i) * 128 + frag_off[s]);
#pragma unroll
      for (int j = 0; j < C::NT; ++j) wf[j] = *(const bf16x8*)(st + (ROWS + 16 * j) * 128 + frag_off[s]);
#pragma unroll
      for (int j = 0; j < C::NT; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[j][i], 0, 0, 0);
    }
  }

  // ---- epilogue: acc[j][i][r] = y[row r0 + 32 wave + 16 i + (l & 15)][col n0 + 16 j + 4 (l >> 4) + r]
  const int cq = 4 * (lane >> 4);
  if constexpr (GLU) {
#pragma unroll
    for (int j = 0; j < C::NT / 2; ++j) {
      const int col = n0 + 16 * j + cq;
      float bg[4] = {0.f, 0.f, 0.f, 0.f}, bu[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr && col < N)
#pragma unroll
        for (int r = 0; r < 4; ++r) { bg[r] = bf2f(bias[col + r]); bu[r] = bf2f(bias[N + col + r]); }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = r0 + 32 * wave + 16 * i + (lane & 15);
        float g[4], o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) g[r] = bf_round(acc[j][i][r] + bg[r]);
        siluf_n_(g, o);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = bf_round(o[r]) * bf_round(acc[j + C::NT / 2][i][r] + bu[r]);
        if (row < M && col < N) store_out8(y + (size_t)row * N + col, u32x2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])});
      }
    }
  } else if constexpr (SCORE) {
    const long long* __restrict__ target = (target_arg, ...);
    // xl = the bf16 logit the plain form stores (NaN = -inf; columns >= N are absent).  Per row: m = the maximum over the
    // workgroup's 64 columns, z = sum of exp(xl - m) (exactly 1 where xl == m, also at m = +-inf), idx = the lowest column with xl == m
    constexpr float NEG_INF = -__builtin_huge_valf();
    u32x4* part = (u32x4*)y;
    float* tlogit = (float*)(part + (size_t)((N + C::NCOL - 1) / C::NCOL) * M);
    float bb[C::NT][4];
#pragma unroll
    for (int j = 0; j < C::NT; ++j) {
      const int col = n0 + 16 * j + cq;
#pragma unroll
      for (int r = 0; r < 4; ++r) bb[j][r] = bias != nullptr && col < N ? bf2f(bias[col + r]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = r0 + 32 * wave + 16 * i + (lane & 15);
      const long long t = row < M ? target[row] : -1ll;
      const int tc = t >= 0 && t < (long long)N ? (int)t : -1;       // the scored column (any workgroup's), -1: none
      float xl[C::NT][4], m = NEG_INF;
#pragma unroll
      for (int j = 0; j < C::NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = bf_round(acc[j][i][r] + bb[j][r]);
          xl[j][r] = (n0 + 16 * j + cq < N && v == v) ? v : NEG_INF;
          m = fmaxf(m, xl[j][r]);
        }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      float z = 0.f, tv = 0.f;
      int idx = 0x7fffffff;
      bool hit = false;
#pragma unroll
      for (int j = 0; j < C::NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = n0 + 16 * j + cq + r;
          const bool top = xl[j][r] == m;
          if (n0 + 16 * j + cq < N) {
            z += top ? 1.f : expf(xl[j][r] - m);
            if (top) idx = min(idx, col);
            if (col == tc) { tv = xl[j][r]; hit = true; }
          }
        }
      z += __shfl_xor(z, 16, 64);
      z += __shfl_xor(z, 32, 64);
      idx = min(idx, __shfl_xor(idx, 16, 64));
      idx = min(idx, __shfl_xor(idx, 32, 64));
      if (row < M) {
        if (lane < 16) part[(size_t)colblk * M + row] = u32x4{__float_as_uint(m), __float_as_uint(z), (unsigned int)idx, 0u};
        if (hit) tlogit[row] = tv;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < C::NT; ++j) {
      const int col = n0 + 16 * j + cq;
      float bb[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr && col < N)
#pragma unroll
        for (int r = 0; r < 4; ++r) bb[r] = bf2f(bias[col + r]);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = r0 + 32 * wave + 16 * i + (lane & 15);
        if (row < M && col < N)
          store_out8(y + (size_t)row * N + col,
                     u32x2{pack2bf(acc[j][i][0] + bb[0], acc[j][i][1] + bb[1]), pack2bf(acc[j][i][2] + bb[2], acc[j][i][3] + bb[3])});
      }
    }
  }
}

// Launch 2 of ivl_linear_logprob_m256_fwd: one workgroup per row merges the row's nblk partials {m_j, z_j, idx_j}.
//   M_r = max m_j;  top1 = the smallest idx_j among m_j == M_r;  Z = sum_j z_j exp(m_j - M_r) in float64 (unscaled where m_j == M_r,
//   nothing from a block at -inf below M_r).  Thread t adds blocks t, t + 256, ... in that order, then a fixed xor tree over the wave and
//   the four wave sums in wave order: the same bits for any M and whichever row of a call the logits sit in.
constexpr int LPC_THREADS = 256;
__global__ __launch_bounds__(LPC_THREADS) void logprob_combine_kernel(const u32x4* __restrict__ part, const float* __restrict__ tlogit,
                                                                      const long long* __restrict__ target, float* __restrict__ logprob,
                                                                      long long* __restrict__ top1, float* __restrict__ lse, int M,
                                                                      int N, int nblk) {
  __shared__ float s_m[LPC_THREADS / 64];
  __shared__ int s_i[LPC_THREADS / 64];
  __shared__ double s_z[LPC_THREADS / 64];
  const int row = (int)blockIdx.x, tid = threadIdx.x;
  const float NEG_INF = -__builtin_huge_valf();
  float m = NEG_INF;
  int idx = 0x7fffffff;
  for (int j = tid; j < nblk; j += LPC_THREADS) {
    const u32x4 p = part[(size_t)j * M + row];
    const float mj = __uint_as_float(p.x);
    const int ij = (int)p.z;
    if (mj > m || (mj == m && ij < idx)) { m = mj; idx = ij; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float mo = __shfl_xor(m, o, 64);
    const int io = __shfl_xor(idx, o, 64);
    if (mo > m || (mo == m && io < idx)) { m = mo; idx = io; }
  }
  if ((tid & 63) == 0) { s_m[tid >> 6] = m; s_i[tid >> 6] = idx; }
  __syncthreads();
  m = s_m[0];
  idx = s_i[0];
#pragma unroll
  for (int v = 1; v < LPC_THREADS / 64; ++v)
    if (s_m[v] > m || (s_m[v] == m && s_i[v] < idx)) { m = s_m[v]; idx = s_i[v]; }
  double z = 0.0;
  for (int j = tid; j < nblk; j += LPC_THREADS) {
    const u32x4 p = part[(size_t)j * M + row];
    const float mj = __uint_as_float(p.x), zj = __uint_as_float(p.y);
    if (mj == m) z += (double)zj;
    else if (mj > NEG_INF) z += (double)zj * exp((double)mj - (double)m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
  if ((tid & 63) == 0) s_z[tid >> 6] = z;
  __syncthreads();
  if (tid == 0) {
    z = s_z[0];
#pragma unroll
    for (int v = 1; v < LPC_THREADS / 64; ++v) z += s_z[v];
    const float lz = logf((float)z);
    const long long t = target[row];
    float lp = 0.f;                                            // a target outside [0, N) is not scored
    if (t >= 0 && t < (long long)N) {
      const float xt = tlogit[row];
      lp = (xt == m ? 0.f : xt - m) - lz;
    }
    logprob[row] = lp;
    if (top1 != nullptr) top1[row] = (long long)idx;
    if (lse != nullptr) lse[row] = (m == NEG_INF || m == -NEG_INF) ? m : m + lz;
  }
}

static size_t logprob_workspace_bytes(int M, int N) {
  const size_t nblk = ((size_t)N + 63) / 64;
  return (nblk * (size_t)M * 16 + (size_t)M * 4 + 255) & ~(size_t)255;
}

static int launch_l256_score(const void* x, const void* w, const void* bias, const int64_t* target, float* logprob, int64_t* top1,
                             float* lse, int M, int N, int K, void* ws, hipStream_t st) {
  constexpr int ROWS = L256_WG_ROWS, NST = L256_STAGES;
  using C = L256Cfg<false, ROWS, NST>;
  static_assert(C::NCOL == 64, "the workspace formula and the combine count 64-column blocks");
  const void* fn = (const void*)linear_m256_kernel<false, ROWS, NST, false, const long long*>;
  static bool attr_set[64];                        // per device, as in launch_l256
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!__atomic_load_n(&attr_set[dev & 63], __ATOMIC_ACQUIRE)) {
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
    __atomic_store_n(&attr_set[dev & 63], true, __ATOMIC_RELEASE);
  }
  const int ncol = (N + C::NCOL - 1) / C::NCOL;
  const dim3 grid(ROWS < L256_ROWS ? (ncol + 7) / 8 * 16 : ncol);
  hipLaunchKernelGGL((linear_m256_kernel<false, ROWS, NST, false, const long long*>), grid, dim3(ROWS * 2), C::LDS, st,
                     (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)ws, M, N, K, (const long long*)target);
  const int rc = check_launch("ivl_linear_logprob_m256_fwd");
  if (rc != IVL_OK) return rc;
  const u32x4* part = (const u32x4*)ws;
  hipLaunchKernelGGL(logprob_combine_kernel, dim3(M), dim3(LPC_THREADS), 0, st, part, (const float*)(part + (size_t)ncol * M),
                     (const long long*)target, logprob, (long long*)top1, lse, M, N, ncol);
  return check_launch("ivl_linear_logprob_m256_fwd (combine)");
}

template <bool GLU>
static int launch_l256(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
  constexpr int ROWS = L256_WG_ROWS, NST = L256_STAGES;
  using C = L256Cfg<GLU, ROWS, NST>;
  constexpr bool WNT = GLU && L256_W_NT != 0;
  const void* fn = (const void*)linear_m256_kernel<GLU, ROWS, NST, WNT>;
  static bool attr_set[64];                        // per device: a function attribute belongs to the device's copy of the code object
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!__atomic_load_n(&attr_set[dev & 63], __ATOMIC_ACQUIRE)) {
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS);
    __atomic_store_n(&attr_set[dev & 63], true, __ATOMIC_RELEASE);
  }
  const int ncol = (N + C::NCOL - 1) / C::NCOL;
  const dim3 grid(ROWS < L256_ROWS ? (ncol + 7) / 8 * 16 : ncol);
  hipLaunchKernelGGL((linear_m256_kernel<GLU, ROWS, NST, WNT>), grid, dim3(ROWS * 2), C::LDS, st, (const bf16_t*)x,
                     (const bf16_t*)w, (const bf16_t*)bias, (bf16_t*)y, M, N, K);
  return check_launch("ivl_linear_m256_fwd");
}

}  // namespace ivl

using namespace ivl;

extern "C" int ivl_linear_m256_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream) {
  IVL_REQUIRE(x && w && y, IVL_ERR_INVALID_ARG, "ivl_linear_m256_fwd: NULL pointer");
  IVL_REQUIRE(M > 0 && N > 0 && K > 0, IVL_ERR_INVALID_ARG, "ivl_linear_m256_fwd: M=%d N=%d K=%d", M, N, K);
  IVL_REQUIRE(M <= L256_ROWS, IVL_ERR_UNSUPPORTED, "ivl_linear_m256_fwd: M=%d (built for at most %d rows)", M, L256_ROWS);
  IVL_REQUIRE(K % L256_BK == 0 && K <= L256_KMAX, IVL_ERR_UNSUPPORTED,
              "ivl_linear_m256_fwd: K=%d (a multiple of %d, at most %d)", K, L256_BK, L256_KMAX);
  IVL_REQUIRE(N % 4 == 0, IVL_ERR_UNSUPPORTED, "ivl_linear_m256_fwd: N=%d (a multiple of 4: 8-byte output pieces)", N);
  // every source offset of the DMA is a 32-bit byte offset from the weight (x) base
  IVL_REQUIRE((long long)(glu ? 2 : 1) * N * K * 2 < (1ll << 32), IVL_ERR_UNSUPPORTED,
              "ivl_linear_m256_fwd: weight of %d x %d rows does not fit 32-bit offsets", glu ? 2 * N : N, K);
  IVL_REQUIRE((((size_t)x | (size_t)w) & 15) == 0 && ((size_t)y & 7) == 0 && ((size_t)bias & 1) == 0, IVL_ERR_INVALID_ARG,
              "ivl_linear_m256_fwd: x / w must be 16-byte aligned, y 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return glu ? launch_l256<true>(x, w, bias, y, M, N, K, st) : launch_l256<false>(x, w, bias, y, M, N, K, st);
}

extern "C" size_t ivl_linear_logprob_workspace_bytes(int M, int N) {
  if (M < 1 || N < 1) return 0;
  return logprob_workspace_bytes(M, N);
}

extern "C" int ivl_linear_logprob_m256_fwd(const void* x, const void* w, const void* bias, const int64_t* target, float* logprob,
                                           int64_t* top1, float* lse, int M, int N, int K, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  IVL_REQUIRE(x && w, IVL_ERR_INVALID_ARG, "ivl_linear_logprob_m256_fwd: NULL pointer (x / w)");
  IVL_REQUIRE(target && logprob, IVL_ERR_INVALID_ARG, "ivl_linear_logprob_m256_fwd: NULL pointer (target / logprob)");
  IVL_REQUIRE(workspace, IVL_ERR_INVALID_ARG, "ivl_linear_logprob_m256_fwd: NULL workspace");
  IVL_REQUIRE(M > 0 && N > 0 && K > 0, IVL_ERR_INVALID_ARG, "ivl_linear_logprob_m256_fwd: M=%d N=%d K=%d", M, N, K);
  IVL_REQUIRE(M <= L256_ROWS, IVL_ERR_UNSUPPORTED, "ivl_linear_logprob_m256_fwd: M=%d (built for at most %d rows)", M, L256_ROWS);
  IVL_REQUIRE(K % L256_BK == 0 && K <= L256_KMAX, IVL_ERR_UNSUPPORTED,
              "ivl_linear_logprob_m256_fwd: K=%d (a multiple of %d, at most %d)", K, L256_BK, L256_KMAX);
  IVL_REQUIRE(N % 4 == 0, IVL_ERR_UNSUPPORTED, "ivl_linear_logprob_m256_fwd: N=%d (a multiple of 4, as the plain form)", N);
  IVL_REQUIRE((long long)N * K * 2 < (1ll << 32), IVL_ERR_UNSUPPORTED,
              "ivl_linear_logprob_m256_fwd: weight of %d x %d rows does not fit 32-bit offsets", N, K);
  IVL_REQUIRE((((size_t)x | (size_t)w | (size_t)workspace) & 15) == 0 && ((size_t)bias & 1) == 0 && ((size_t)target & 7) == 0 &&
                  ((size_t)top1 & 7) == 0 && (((size_t)logprob | (size_t)lse) & 3) == 0,
              IVL_ERR_INVALID_ARG, "ivl_linear_logprob_m256_fwd: x / w / workspace must be 16-byte aligned (x=%p w=%p workspace=%p)", x,
              w, workspace);
  const size_t need = logprob_workspace_bytes(M, N);
  IVL_REQUIRE(workspace_bytes >= need, IVL_ERR_WORKSPACE, "ivl_linear_logprob_m256_fwd: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  return launch_l256_score(x, w, bias, target, logprob, top1, lse, M, N, K, workspace, (hipStream_t)stream);
}

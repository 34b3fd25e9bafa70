// y[M,N] = x[M,K] W[N,K]^T (+ bias), bf16 in / fp32 accumulate / bf16 out, for 1 <= M <= 16 rows: the projections of a decode step
// that advances 5 to 16 slots.  Still a weight stream -- 2 M FLOP per weight element -- but no longer one for fmaf
// chains: sixteen x rows are exactly one B operand of v_mfma_f32_16x16x32_bf16, so a wave owns a TILE of 16 weight rows (the A operand),
// streams their K elements once, non-temporally, straight into VGPRs, and one MFMA per 32 k serves all rows of x.
//
// THE PLAN is a function of K alone -- not of M, not of N, not of the weight format:
//   a CHUNK is 8 consecutive k; TILE t of a row is the chunks [256t, 256t + 256); STEP s = 16t + j (j in 0..15) issues four MFMAs
//   u = 0..3 whose k-group g (the 8 k that lane group g = lane >> 4 feeds) holds chunk 256t + 4j + g + 64u -- of weight row
//   lane & 15 in the A operand, of x row lane & 15 in the B operand.  That is the order in which the shuffled MXFP4 layout hands a lane
//   its pieces (position p = 4j + g of tile t: ONE 16-byte load holds the four chunks p + 64u, one dword their four block scales); the
//   bf16 and e4m3 policies load the same chunks from their row-major rows.  Steps past the row end do not exist (S = the number of
//   steps with a chunk below K/8); chunks past the row end inside a step are zeros on both operands.
//   K SPLIT: the S steps are cut into 8 contiguous slices of ceil(S / 8) steps, one per wave of the workgroup that owns the columns;
//   a wave adds its steps in ascending order, u ascending, from 0, and the partial accumulators meet in LDS in ascending slice order
//   (fp32), then the bias, then the ONE rounding.  A slice without steps adds zeros.  No split across workgroups, no atomics, no
//   second launch: the same bits on every run.  (A split by the number of rows -- 1, 2, 4 waves for the wide projections -- was
//   measured and lost at every one of the model's seven shapes: DESIGN 4.16.)
//
// WEIGHT ELEMENT POLICIES (W16Bf16 / W16E4m3 / W16Mxfp4): a policy says where a lane's pieces of a step are and how a piece becomes
// the bf16 bit pattern of W' (exact for both packed formats); everything behind that -- operands, MFMA sequence, reduction, epilogue
// -- is the kernel's, so the packed forms equal the bf16 form on W' bit for bit.
//
// D = A B^T has the x row on the lane (col = lane & 15) and weight rows 4 (lane >> 4) + reg in its four registers: a lane stores four
// consecutive output columns of one x row.  Rows M .. 15 of B are zeros: never read from x, never written to y; weight rows past the
// last are neither read (the row index is clamped) nor stored.  Every output element is its own fp32 sum over k in the plan's order:
// row m of y depends on row m of x only.
//
// x comes straight from L2 in fragment shape (16 rows x 64 B per load instruction): it is at most 16 x 11008 bf16 = 352 KB and is
// re-read by every tile -- at M = 16 as many bytes as the bf16 weights themselves; a wave of a wide plain projection therefore owns
// two tiles per x fragment (M16_PAIR), as the GLU form does by construction.  Staging x in LDS was not built.
#include "ivl_lora.h"
#include "linear_m16.h"

namespace ivl {

constexpr int M16_PF = 2;         // steps in flight per wave: 8 weight pieces + 8 x pieces per lane and accumulator

// PAIR from 512 tiles on (measured, DESIGN 4.16: the GDN in-projection and lm_head gain 20 %, the N <= 2560 projections lose 25 %)
static bool m16_pair(int R) { return R >= 8192; }

// N = number of OUTPUT columns (GLU: I; the weight then has 2N rows); per = steps per slice
// MODE: what a wave owns -- M16_ONE: one tile of 16 weight rows; M16_GLU: the gate tile and the up tile of the same 16 columns;
// M16_PAIR: two adjacent tiles (32 columns) of a plain projection, which halves the x fragments read per weight byte.  ONE or PAIR is a
// choice of speed: every output element is the same sum in the same order in both.
enum { M16_ONE = 0, M16_GLU = 1, M16_PAIR = 2 };

// LORA: the per-row adapter's expand-add in the epilogue -- after the LDS combine and the bias, the slice-0 lane that owns
// x row r16 forms y0 = bf16(acc + bias) of each of its columns and, where adapter_idx[r16] is valid and the column's WEIGHT ROW (GLU:
// c and I + c of the fused gate|up rows) lies in a segment, replaces it by lora_expand_ on that row of B and t_ws[r16] (written by the
// shrink launch in front); the gate then runs on the adapted gate and up values.  The tables travel as ONE trailing by-value argument
// that the LORA = false instantiations do not have: their signature, and their code, are what they were.
struct M16Lora {
  const int* idx; const bf16_t* B; const float* scaling; const bf16_t* t_ws;
  int n_adapters, n_seg, R, rows;                  // rows: weight rows = the N of the adapter tables
  LoraSegs segs;
};
template <class T> __device__ __forceinline__ const T& m16_first(const T& t) { return t; }

template <class WT, int MODE, bool LORA = false, class... LP>
__global__ __launch_bounds__(64 * M16_KS) void linear_m16_kernel(const bf16_t* __restrict__ x, typename WT::arg w,
                                                                   const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int M, int N,
                                                                   int K, int per, LP... lp) {
  static_assert(sizeof...(LP) == (LORA ? 1 : 0), "the LoRA tables are the one trailing argument of the LORA form");
  constexpr bool GLU = MODE == M16_GLU;
  constexpr int NA = MODE == M16_ONE ? 1 : 2;      // accumulators (tiles) per wave
  constexpr int COLS = MODE == M16_PAIR ? 32 : 16; // output columns per wave
  __shared__ f32x4 s_part[M16_KS][NA][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int tile = (int)blockIdx.x, slice = wave;
  const int nchunk = K >> 3;
  const int n0 = tile * COLS;
  typename WT::row wr[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a)                     // (GLU: a = 1 is the "up" row; PAIR: the row 16 further on)
    wr[a] = WT::open(w, GLU ? min(n0 + r16, N - 1) + a * N : min(n0 + 16 * a + r16, N - 1), K);
  const u32x4* xrow = (const u32x4*)(x + (size_t)min(r16, M - 1) * K);
  const bool mlive = r16 < M;
  f32x4 acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};

  const int S = m16_steps(K);
  const int s_end = min(S, (slice + 1) * per);
  for (int s = slice * per; s < s_end; s += M16_PF) {
    typename WT::raw wv[M16_PF][NA];
    u32x4 xv[M16_PF][4];
#pragma unroll
    for (int i = 0; i < M16_PF; ++i) {             // (a step past the slice repeats the last one and is masked below)
      const int ss = min(s + i, s_end - 1), t = ss >> 4, j = ss & 15;
#pragma unroll
      for (int a = 0; a < NA; ++a) WT::load(w, wr[a], t, j, g, nchunk, wv[i][a]);
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[i][u] = xrow[min(256 * t + 4 * j + g + 64 * u, nchunk - 1)];
    }
#pragma unroll
    for (int i = 0; i < M16_PF; ++i) {
      const int ss = min(s + i, s_end - 1), t = ss >> 4, j = ss & 15;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = s + i < s_end && 256 * t + 4 * j + g + 64 * u < nchunk;
        const bf16x8 b = m16_frag(ok && mlive ? xv[i][u] : zero);
#pragma unroll
        for (int a = 0; a < NA; ++a)
          acc[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(m16_frag(ok ? WT::bits(wv[i][a], wr[a], u) : zero), b, acc[a], 0, 0, 0);
      }
    }
  }

  if (slice != 0) {                                // slices 1 .. 7 hand over, slice 0 adds them in ascending order
#pragma unroll
    for (int a = 0; a < NA; ++a) s_part[slice][a][lane] = acc[a];
  }
  __syncthreads();
  if (slice != 0) return;
#pragma unroll
  for (int k = 1; k < M16_KS; ++k)
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] += s_part[k][a][lane];

  if (!mlive) return;
  // LORA: v = acc + bias of weight row `row` -> bf16(v), or the adapted value where the row of x has an adapter and `row` a segment
  [[maybe_unused]] auto adapt = [&](float v, int row) -> float {
    if constexpr (LORA) {
      const M16Lora& L = m16_first(lp...);
      v = bf_round(v);
      const int ad = L.idx[r16];
      if ((unsigned int)ad >= (unsigned int)L.n_adapters) return v;               // a row without an adapter: the base bits
      const int seg = lora_seg_of_(row, L.n_seg, L.segs);
      if (seg < 0) return v;                                                      // a column in no segment
      return lora_expand_(v, (const u32x4*)(L.B + ((size_t)ad * L.rows + row) * L.R),
                          (const u32x4*)(L.t_ws + r16 * LORA_T_LD + seg * L.R), L.R >> 3, L.scaling[ad]);
    } else {
      return v;
    }
  };
#pragma unroll
  for (int a = 0; a < (GLU ? 1 : NA); ++a) {
  const int n = n0 + 16 * a + 4 * g;               // this lane: x row r16, output columns n .. n + 3
  if (n >= N) return;
  float o[4];
  if constexpr (GLU) {
    float gt[4], sg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = min(n + r, N - 1);
      if constexpr (LORA) {
        gt[r] = adapt(acc[0][r] + (bias != nullptr ? bf2f(bias[col]) : 0.f), col);
        o[r] = adapt(acc[1][r] + (bias != nullptr ? bf2f(bias[N + col]) : 0.f), N + col);
      } else {
      gt[r] = bf_round(acc[0][r] + (bias != nullptr ? bf2f(bias[col]) : 0.f));                    // gate_proj output
      o[r] = bf_round(acc[1][r] + (bias != nullptr ? bf2f(bias[N + col]) : 0.f));                 // up_proj output
      }
    }
    siluf_n_(gt, sg);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = bf_round(sg[r]) * o[r];                                     // = silu_mul_kernel
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = acc[a][r] + (bias != nullptr ? bf2f(bias[min(n + r, N - 1)]) : 0.f);
    if constexpr (LORA) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = adapt(o[r], min(n + r, N - 1));
    }
  }
  bf16_t* yp = y + (size_t)r16 * N + n;
  if ((N & 3) == 0) {                              // (n is a multiple of 4: the four columns exist and the piece is 8-byte aligned)
    *(u32x2*)yp = u32x2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < N) yp[r] = f2bf(o[r]);
  }
  }
}

// LP: nothing, or the M16Lora of the LORA form
template <class WT, class... LP>
static int m16_launch(const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N, int K, int glu, void* stream,
                      const char* who, LP... lp) {
  constexpr bool LORA = sizeof...(LP) != 0;
  const int R = glu ? 2 * N : N;
  const int per = (m16_steps(K) + M16_KS - 1) / M16_KS;
  const bool pair = !glu && m16_pair(R);
  const dim3 grid((N + (pair ? 31 : 15)) / (pair ? 32 : 16)), block(64 * M16_KS);       // one range of output columns per workgroup
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *xp = (const bf16_t*)x, *bp = (const bf16_t*)bias;
  if (glu) hipLaunchKernelGGL((linear_m16_kernel<WT, M16_GLU, LORA, LP...>), grid, block, 0, st, xp, wp, bp, (bf16_t*)y, M, N, K, per, lp...);
  else if (pair) hipLaunchKernelGGL((linear_m16_kernel<WT, M16_PAIR, LORA, LP...>), grid, block, 0, st, xp, wp, bp, (bf16_t*)y, M, N, K, per, lp...);
  else hipLaunchKernelGGL((linear_m16_kernel<WT, M16_ONE, LORA, LP...>), grid, block, 0, st, xp, wp, bp, (bf16_t*)y, M, N, K, per, lp...);
  return check_launch(who);
}

// The LORA form of an entry: the refusals that tie `lora` to the base call (after the base entry's own), those of the LoRA entries,
// then the shrink of the x rows into lora->t_ws and the m16 kernel with the LoRA epilogue.
static int m16_lora_check(const char* who, const ivl_lora_args* lora, const void* x, const void* y, int M, int N, int K, int glu,
                          M16Lora& L) {
  IVL_REQUIRE(lora != nullptr, IVL_ERR_INVALID_ARG, "%s: NULL lora", who);
  IVL_REQUIRE(lora->adapter_idx && lora->A && lora->B && lora->scaling && lora->t_ws, IVL_ERR_INVALID_ARG,
              "%s: NULL pointer in lora (adapter_idx, A, B, scaling and t_ws are all required)", who);
  IVL_REQUIRE(lora->x == x && lora->y == y && lora->M == M && lora->K == K, IVL_ERR_INVALID_ARG,
              "%s: lora->x, y, M=%d and K=%d must be the call's (M=%d, K=%d)", who, lora->M, lora->K, M, K);
  IVL_REQUIRE(lora->N == (glu ? 2 * N : N), IVL_ERR_INVALID_ARG, "%s: lora->N=%d must be the number of weight rows, %d", who, lora->N,
              glu ? 2 * N : N);
  IVL_REQUIRE(lora->norm_weight == nullptr && lora->residual == nullptr, IVL_ERR_INVALID_ARG,
              "%s: the norm fields of lora must be NULL (no NORM group)", who);
  const int rc = lora_check(who, lora, 16, false, L.segs);
  if (rc != IVL_OK) return rc;
  L.idx = (const int*)lora->adapter_idx; L.B = (const bf16_t*)lora->B; L.scaling = lora->scaling; L.t_ws = (const bf16_t*)lora->t_ws;
  L.n_adapters = lora->n_adapters; L.n_seg = lora->n_seg; L.R = lora->R; L.rows = lora->N;
  return IVL_OK;
}

static int m16_lora_shrink(const char* who, const ivl_lora_args* lora, void* stream) {
  lora_launch_shrink((const bf16_t*)lora->x, (const int*)lora->adapter_idx, (const bf16_t*)lora->A, (bf16_t*)lora->t_ws, lora->M, lora->K,
                     lora->n_seg * lora->R, lora->n_adapters, (hipStream_t)stream);
  return check_launch(who);
}

// the entries of a format: name, policy, weight argument; the LORA forms also name their shrink launch
template <class WT>
static int m16_fwd(const char* who, const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N, int K, int glu,
                   void* stream) {
  return m16_entry<WT>(who, x, wp, bias, y, M, N, K, glu, 16, [&] { return m16_launch<WT>(x, wp, bias, y, M, N, K, glu, stream, who); });
}

template <class WT>
static int m16_lora_fwd(const char* who, const char* shrink, const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N,
                        int K, int glu, const ivl_lora_args* lora, void* stream) {
  return m16_entry<WT>(who, x, wp, bias, y, M, N, K, glu, 16, [&] {
    M16Lora L;
    int rc = m16_lora_check(who, lora, x, y, M, N, K, glu, L);
    if (rc == IVL_OK) rc = m16_lora_shrink(shrink, lora, stream);
    return rc != IVL_OK ? rc : m16_launch<WT>(x, wp, bias, y, M, N, K, glu, stream, who, L);
  });
}

}  // namespace ivl

using namespace ivl;

extern "C" int ivl_linear_m16_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream) {
  return m16_fwd<W16Bf16>("ivl_linear_m16_fwd", x, (const bf16_t*)w, bias, y, M, N, K, glu, stream);
}

extern "C" int ivl_linear_m16_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K,
                                     int glu, void* stream) {
  return m16_fwd<W16E4m3>("ivl_linear_m16_w8_fwd", x, {(const unsigned char*)wq, scale}, bias, y, M, N, K, glu, stream);
}

extern "C" int ivl_linear_m16_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                     int glu, void* stream) {
  return m16_fwd<W16Mxfp4>("ivl_linear_m16_w4_fwd", x, {(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, N, K, glu, stream);
}

// ---- the LORA forms: the argument lists above plus the adapter tables; two launches (shrink, then the kernel with the LoRA epilogue)
extern "C" int ivl_linear_m16_lora_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu,
                                       const ivl_lora_args* lora, void* stream) {
  return m16_lora_fwd<W16Bf16>("ivl_linear_m16_lora_fwd", "ivl_linear_m16_lora_fwd (shrink)", x, (const bf16_t*)w, bias, y, M, N, K, glu,
                               lora, stream);
}

extern "C" int ivl_linear_m16_lora_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N,
                                          int K, int glu, const ivl_lora_args* lora, void* stream) {
  return m16_lora_fwd<W16E4m3>("ivl_linear_m16_lora_w8_fwd", "ivl_linear_m16_lora_w8_fwd (shrink)", x, {(const unsigned char*)wq, scale},
                               bias, y, M, N, K, glu, lora, stream);
}

extern "C" int ivl_linear_m16_lora_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                          int glu, const ivl_lora_args* lora, void* stream) {
  return m16_lora_fwd<W16Mxfp4>("ivl_linear_m16_lora_w4_fwd", "ivl_linear_m16_lora_w4_fwd (shrink)", x,
                                {(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, N, K, glu, lora, stream);
}

// Device code and argument checks shared by the per-row LoRA entry points: lora_small_m.hip (M <= 4, with the
// NORM group), lora_m16.hip (M <= 16) and the LoRA epilogue of linear_m16.hip.  ONE helper owns the expand formula and ONE the segment
// lookup, so the three callers cannot drift apart: a row of y is the same bits whichever of them wrote it.
#pragma once
#include "ivl_rowwise.h"

namespace ivl {

namespace {

__device__ __forceinline__ float lora_dot8(u32x4 a, u32x4 b, float acc) {          // = dot8 of linear_small_m.hip
  acc = fmaf(bflo(a.x), bflo(b.x), acc); acc = fmaf(bfhi(a.x), bfhi(b.x), acc);
  acc = fmaf(bflo(a.y), bflo(b.y), acc); acc = fmaf(bfhi(a.y), bfhi(b.y), acc);
  acc = fmaf(bflo(a.z), bflo(b.z), acc); acc = fmaf(bfhi(a.z), bfhi(b.z), acc);
  acc = fmaf(bflo(a.w), bflo(b.w), acc); acc = fmaf(bfhi(a.w), bfhi(b.w), acc);
  return acc;
}

constexpr int LORA_T_LD = 512;            // row pitch of t_ws: 8 segments x R = 64
constexpr int LORA_JPW = 2;               // rows of A per wave
constexpr int LORA_NORM_KMAX = 4096;      // = LSM_NORM_KMAX
constexpr int LORA_MAX_SEG = 8;

struct LoraSegs { int col[LORA_MAX_SEG + 1]; };

// the segment that owns output column n, -1 = none (a column in no segment is not touched)
__device__ __forceinline__ int lora_seg_of_(int n, int n_seg, const LoraSegs& segs) {
  int seg = -1;
#pragma unroll
  for (int i = 0; i < LORA_MAX_SEG; ++i)
    if (i < n_seg && n >= segs.col[i] && n < segs.col[i + 1]) seg = i;
  return seg;
}

// THE expand formula on one output element: d = sum_j B[j] t[j] (one fmaf per j, ascending from 0), e = bf16(s bf16(d)),
// the value of bf16(y0 + e).  bp: the column's B row, tp: the t of its segment, both R bf16 = `pieces` = R / 8 16-byte pieces (a
// constant at the call site of the expand-add kernels, whose loop then unrolls; the m16 epilogue passes the table's at run time).
__device__ __forceinline__ float lora_expand_(float y0, const u32x4* __restrict__ bp, const u32x4* __restrict__ tp, int pieces,
                                              float s) {
  float d = 0.f;
#pragma unroll
  for (int p = 0; p < pieces; ++p) d = lora_dot8(bp[p], tp[p], d);
  const float e = bf_round(s * bf_round(d));
  return bf_round(y0 + e);
}

// NIT: 16-byte pieces of the row per thread in the norm prologue (1: K <= 2048, 2: K <= 4096), as in linear_small_m_kernel
template <bool NORM, int NIT>
__global__ __launch_bounds__(256) void lora_shrink_kernel(const bf16_t* __restrict__ x, const int* __restrict__ adapter_idx,
                                                          const bf16_t* __restrict__ A, bf16_t* __restrict__ t_ws, int K, int nrank,
                                                          int n_adapters, const bf16_t* __restrict__ residual,
                                                          const bf16_t* __restrict__ norm_weight, float eps) {
  __shared__ __attribute__((aligned(16))) u32x4 s_x[NORM ? LORA_NORM_KMAX / 8 : 1];
  __shared__ float s_part[4];
  const int m = blockIdx.y;
  const int a = adapter_idx[m];
  if ((unsigned int)a >= (unsigned int)n_adapters) return;          // a row without an adapter (workgroup-uniform: before any barrier)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = K >> 3;
  const bf16_t* xrow = x + (size_t)m * K;
  if constexpr (NORM) {
    u32x4 xraw[NIT], rraw[NIT], wraw[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int v = min(tid + it * 256, nchunk - 1);
      wraw[it] = *(const u32x4*)(norm_weight + v * 8);
      xraw[it] = *(const u32x4*)(xrow + v * 8);
      rraw[it] = residual != nullptr ? *(const u32x4*)(residual + (size_t)m * K + v * 8) : u32x4{0u, 0u, 0u, 0u};
    }
    float hv[NIT][8];
    float ss = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int v = tid + it * 256;
      if (v < nchunk) {
        unpack8(xraw[it], hv[it]);
        if (residual != nullptr) {
          float rv[8];
          unpack8(rraw[it], rv);
#pragma unroll
          for (int i = 0; i < 8; ++i) hv[it][i] = add_round_(hv[it][i], rv[i]);
        }
        ss = sumsq8_(hv[it], ss);
      }
    }
    ss = wave_sum(ss);
    if (lane == 0) s_part[wave] = ss;
    __syncthreads();
    const float tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    const float rstd = qwen_rstd_(tot, K, eps);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int v = tid + it * 256;
      if (v < nchunk) {
        float wv8[8], o8[8];
        unpack8(wraw[it], wv8);
#pragma unroll
        for (int i = 0; i < 8; ++i) o8[i] = qwen_norm_(hv[it][i], rstd, wv8[i]);
        s_x[v] = pack8(o8);
      }
    }
    __syncthreads();
  }
  const int j0 = (blockIdx.x * 4 + wave) * LORA_JPW;
  if (j0 >= nrank) return;                                          // (behind the barriers)
  const u32x4* arow[LORA_JPW];
  float acc[LORA_JPW];
#pragma unroll
  for (int r = 0; r < LORA_JPW; ++r) {
    arow[r] = (const u32x4*)(A + ((size_t)a * nrank + min(j0 + r, nrank - 1)) * K);
    acc[r] = 0.f;
  }
#pragma unroll 4
  for (int c = lane; c < nchunk; c += 64) {
    u32x4 xl;
    if constexpr (NORM) xl = s_x[c];
    else xl = *((const u32x4*)xrow + c);
#pragma unroll
    for (int r = 0; r < LORA_JPW; ++r) acc[r] = lora_dot8(arow[r][c], xl, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < LORA_JPW; ++r) {
    const float s = wave_sum(acc[r]);
    if (lane == 0 && j0 + r < nrank) t_ws[m * LORA_T_LD + j0 + r] = f2bf(s);
  }
}

template <int R>
__global__ __launch_bounds__(256) void lora_expand_add_kernel(bf16_t* __restrict__ y, const int* __restrict__ adapter_idx,
                                                              const bf16_t* __restrict__ B, const float* __restrict__ scaling,
                                                              const bf16_t* __restrict__ t_ws, int N, int n_adapters, int n_seg,
                                                              LoraSegs segs) {
  const int m = blockIdx.y;
  const int a = adapter_idx[m];
  if ((unsigned int)a >= (unsigned int)n_adapters) return;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int seg = lora_seg_of_(n, n_seg, segs);
  if (seg < 0) return;                                              // a column in no segment
  bf16_t* yp = y + (size_t)m * N + n;
  *yp = f2bf(lora_expand_(bf2f(*yp), (const u32x4*)(B + ((size_t)a * N + n) * R), (const u32x4*)(t_ws + m * LORA_T_LD + seg * R), R / 8,
                          scaling[a]));
}

// the non-NORM shrink of M rows (grid (ceil(n_seg R / 8), M)): rows without an adapter exit at once
inline void lora_launch_shrink(const bf16_t* x, const int* idx, const bf16_t* A, bf16_t* t_ws, int M, int K, int nrank, int n_adapters,
                               hipStream_t st) {
  const dim3 sgrid((nrank + 4 * LORA_JPW - 1) / (4 * LORA_JPW), M);
  hipLaunchKernelGGL((lora_shrink_kernel<false, 1>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, K, nrank, n_adapters,
                     (const bf16_t*)nullptr, (const bf16_t*)nullptr, 0.f);
}

template <int R>
void lora_launch_expand_r(bf16_t* y, const int* idx, const bf16_t* B, const float* scaling, const bf16_t* t_ws, int M, int N,
                          int n_adapters, int n_seg, const LoraSegs& segs, hipStream_t st) {
  hipLaunchKernelGGL((lora_expand_add_kernel<R>), dim3((N + 255) / 256, M), dim3(256), 0, st, y, idx, B, scaling, t_ws, N, n_adapters,
                     n_seg, segs);
}

inline void lora_launch_expand(const ivl_lora_args* a, const LoraSegs& segs, hipStream_t st) {
  bf16_t* y = (bf16_t*)a->y;
  const bf16_t *B = (const bf16_t*)a->B, *t_ws = (const bf16_t*)a->t_ws;
  const int* idx = (const int*)a->adapter_idx;
  switch (a->R) {
    case 8: lora_launch_expand_r<8>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    case 16: lora_launch_expand_r<16>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    case 32: lora_launch_expand_r<32>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    default: lora_launch_expand_r<64>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
  }
}

// Every refusal of a LoRA entry point, before anything is launched.  max_m: 4 (small-M) or 16; norm_ok: whether the entry has the
// NORM group.  Fills `segs` (entries past n_seg repeat the last border).
inline int lora_check(const char* who, const ivl_lora_args* a, int max_m, bool norm_ok, LoraSegs& segs) {
  IVL_REQUIRE(a != nullptr, IVL_ERR_INVALID_ARG, "%s: NULL args", who);
  IVL_REQUIRE(a->x && a->y && a->adapter_idx && a->A && a->B && a->scaling && a->t_ws, IVL_ERR_INVALID_ARG,
              "%s: NULL pointer (x, y, adapter_idx, A, B, scaling and t_ws are all required)", who);
  if (max_m == 4)
    IVL_REQUIRE(a->M >= 1 && a->M <= 4, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..4 rows; larger calls are library GEMMs)", who, a->M);
  else
    IVL_REQUIRE(a->M >= 1 && a->M <= max_m, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..%d rows)", who, a->M, max_m);
  IVL_REQUIRE(a->N > 0 && a->K >= 8 && a->K % 8 == 0, IVL_ERR_INVALID_ARG, "%s: N=%d K=%d (K must be a multiple of 8)", who, a->N, a->K);
  IVL_REQUIRE(a->R == 8 || a->R == 16 || a->R == 32 || a->R == 64, IVL_ERR_UNSUPPORTED, "%s: R=%d (rank capacity 8, 16, 32 or 64)", who, a->R);
  IVL_REQUIRE(a->n_adapters >= 1, IVL_ERR_INVALID_ARG, "%s: n_adapters=%d", who, a->n_adapters);
  IVL_REQUIRE(a->n_seg >= 1 && a->n_seg <= LORA_MAX_SEG, IVL_ERR_INVALID_ARG, "%s: n_seg=%d (1..%d segments)", who, a->n_seg, LORA_MAX_SEG);
  const int cols[LORA_MAX_SEG + 1] = {a->seg_col0, a->seg_col1, a->seg_col2, a->seg_col3, a->seg_col4,
                                      a->seg_col5, a->seg_col6, a->seg_col7, a->seg_col8};
  for (int i = 0; i <= LORA_MAX_SEG; ++i) segs.col[i] = i <= a->n_seg ? cols[i] : cols[a->n_seg];
  for (int i = 0; i <= a->n_seg; ++i)
    IVL_REQUIRE(cols[i] >= 0 && cols[i] <= a->N && (i == 0 || cols[i] >= cols[i - 1]), IVL_ERR_INVALID_ARG,
                "%s: seg_col[%d]=%d (the segment borders must be non-decreasing within [0, N=%d])", who, i, cols[i], a->N);
  const bool norm = a->norm_weight != nullptr;
  IVL_REQUIRE(norm || a->residual == nullptr, IVL_ERR_INVALID_ARG, "%s: residual without norm_weight", who);
  if (norm) {
    IVL_REQUIRE(norm_ok, IVL_ERR_UNSUPPORTED, "%s: no NORM group (norm_weight must be NULL: the caller materialises the norm)", who);
    IVL_REQUIRE(a->K >= 512 && a->K <= LORA_NORM_KMAX, IVL_ERR_UNSUPPORTED,
                "%s: K=%d (the normalised row is staged in LDS by the whole workgroup: 512 <= K <= %d)", who, a->K, LORA_NORM_KMAX);
  }
  IVL_REQUIRE((((size_t)a->x | (size_t)a->y | (size_t)a->A | (size_t)a->B | (size_t)a->t_ws | (size_t)a->residual |
                (size_t)a->norm_weight) & 15) == 0 && ((size_t)a->adapter_idx & 3) == 0 && ((size_t)a->scaling & 3) == 0,
              IVL_ERR_INVALID_ARG, "%s: x, y, A, B, t_ws, residual and norm_weight must be 16-byte aligned", who);
  return IVL_OK;
}

}  // namespace

}  // namespace ivl

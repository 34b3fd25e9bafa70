// Per-row LoRA adapters on the output of a decode projection, unmerged (ivl_lora_add_small_m_fwd):
//   y[m] += s_a B_a (A_a x[m]),  a = adapter_idx[m] read on the device,  M <= 4 rows,
// at the rounding points of peft's bf16 lora.Linear.forward (include/ivl_hip.h states the chain).  The base projection is a weight
// stream of linear_small_m.hip, bf16 or packed; this is the second, small weight stream next to it: A_a [n_seg R, K] and
// B_a [N, R] of ONE adapter per row -- at R = 16 and the q|k|v projection of the 3B model 3 x 16 x 2048 + 2560 x 16 elements,
// 180 KB against 10.5 MB of base weight.  No MFMA (M <= 4), no atomics, a fixed order.
//
//   shrink      grid (ceil(n_seg R / 8), M), 256 threads: workgroup = (8 rows of A, x row m), a wave = two rows of A.  Lane l adds the
//               16-byte chunks l + 64 i of a row, i ascending, with dot8's fmaf chain, then wave_sum; lane 0 stores bf16 t to t_ws.
//               A workgroup whose row has no adapter exits at once (the index is workgroup-uniform).
//               NORM: the workgroup first forms the normalised row in LDS -- the prologue of linear_small_m_kernel's NORM form at
//               M = 1: the thread -> element mapping and summation order of add_rmsnorm_kernel through add_round_ / sumsq8_ /
//               qwen_rstd_ / qwen_norm_, so the row is the materialised norm's bit for bit -- and reads x from there.  (8 KB of
//               L2-resident input per workgroup; h_out is the base launch's to write.)
//   expand-add  grid (ceil(N / 256), M): one thread per output column n; its B row is R bf16 = R / 8 16-byte pieces, the t of its
//               segment comes from t_ws (L2); d, e and the add are rounded as stated; a column in no segment and a row without an
//               adapter are left alone (no read-modify-write).
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
  int seg = -1;
#pragma unroll
  for (int i = 0; i < LORA_MAX_SEG; ++i)
    if (i < n_seg && n >= segs.col[i] && n < segs.col[i + 1]) seg = i;
  if (seg < 0) return;                                              // a column in no segment
  const u32x4* bp = (const u32x4*)(B + ((size_t)a * N + n) * R);
  const u32x4* tp = (const u32x4*)(t_ws + m * LORA_T_LD + seg * R);
  u32x4 bv[R / 8];
#pragma unroll
  for (int p = 0; p < R / 8; ++p) bv[p] = bp[p];
  float d = 0.f;
#pragma unroll
  for (int p = 0; p < R / 8; ++p) d = lora_dot8(bv[p], tp[p], d);
  const float e = bf_round(scaling[a] * bf_round(d));
  bf16_t* yp = y + (size_t)m * N + n;
  *yp = f2bf(bf2f(*yp) + e);
}

template <int R>
void launch_expand(bf16_t* y, const int* idx, const bf16_t* B, const float* scaling, const bf16_t* t_ws, int M, int N, int n_adapters,
                   int n_seg, const LoraSegs& segs, hipStream_t st) {
  hipLaunchKernelGGL((lora_expand_add_kernel<R>), dim3((N + 255) / 256, M), dim3(256), 0, st, y, idx, B, scaling, t_ws, N, n_adapters,
                     n_seg, segs);
}

}  // namespace

}  // namespace ivl

using namespace ivl;

extern "C" int ivl_lora_add_small_m_fwd(const ivl_lora_args* a, void* stream) {
  const char* who = "ivl_lora_add_small_m_fwd";
  IVL_REQUIRE(a != nullptr, IVL_ERR_INVALID_ARG, "%s: NULL args", who);
  IVL_REQUIRE(a->x && a->y && a->adapter_idx && a->A && a->B && a->scaling && a->t_ws, IVL_ERR_INVALID_ARG,
              "%s: NULL pointer (x, y, adapter_idx, A, B, scaling and t_ws are all required)", who);
  IVL_REQUIRE(a->M >= 1 && a->M <= 4, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..4 rows; larger calls are library GEMMs)", who, a->M);
  IVL_REQUIRE(a->N > 0 && a->K >= 8 && a->K % 8 == 0, IVL_ERR_INVALID_ARG, "%s: N=%d K=%d (K must be a multiple of 8)", who, a->N, a->K);
  IVL_REQUIRE(a->R == 8 || a->R == 16 || a->R == 32 || a->R == 64, IVL_ERR_UNSUPPORTED, "%s: R=%d (rank capacity 8, 16, 32 or 64)", who, a->R);
  IVL_REQUIRE(a->n_adapters >= 1, IVL_ERR_INVALID_ARG, "%s: n_adapters=%d", who, a->n_adapters);
  IVL_REQUIRE(a->n_seg >= 1 && a->n_seg <= LORA_MAX_SEG, IVL_ERR_INVALID_ARG, "%s: n_seg=%d (1..%d segments)", who, a->n_seg, LORA_MAX_SEG);
  const int cols[LORA_MAX_SEG + 1] = {a->seg_col0, a->seg_col1, a->seg_col2, a->seg_col3, a->seg_col4,
                                      a->seg_col5, a->seg_col6, a->seg_col7, a->seg_col8};
  LoraSegs segs;
  for (int i = 0; i <= LORA_MAX_SEG; ++i) segs.col[i] = i <= a->n_seg ? cols[i] : cols[a->n_seg];
  for (int i = 0; i <= a->n_seg; ++i)
    IVL_REQUIRE(cols[i] >= 0 && cols[i] <= a->N && (i == 0 || cols[i] >= cols[i - 1]), IVL_ERR_INVALID_ARG,
                "%s: seg_col[%d]=%d (the segment borders must be non-decreasing within [0, N=%d])", who, i, cols[i], a->N);
  const bool norm = a->norm_weight != nullptr;
  IVL_REQUIRE(norm || a->residual == nullptr, IVL_ERR_INVALID_ARG, "%s: residual without norm_weight", who);
  if (norm)
    IVL_REQUIRE(a->K >= 512 && a->K <= LORA_NORM_KMAX, IVL_ERR_UNSUPPORTED,
                "%s: K=%d (the normalised row is staged in LDS by the whole workgroup: 512 <= K <= %d)", who, a->K, LORA_NORM_KMAX);
  IVL_REQUIRE((((size_t)a->x | (size_t)a->y | (size_t)a->A | (size_t)a->B | (size_t)a->t_ws | (size_t)a->residual |
                (size_t)a->norm_weight) & 15) == 0 && ((size_t)a->adapter_idx & 3) == 0 && ((size_t)a->scaling & 3) == 0,
              IVL_ERR_INVALID_ARG, "%s: x, y, A, B, t_ws, residual and norm_weight must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *x = (const bf16_t*)a->x, *A = (const bf16_t*)a->A, *B = (const bf16_t*)a->B;
  const bf16_t *res = (const bf16_t*)a->residual, *nw = (const bf16_t*)a->norm_weight;
  bf16_t *y = (bf16_t*)a->y, *t_ws = (bf16_t*)a->t_ws;
  const int* idx = (const int*)a->adapter_idx;
  const int nrank = a->n_seg * a->R;
  const dim3 sgrid((nrank + 4 * LORA_JPW - 1) / (4 * LORA_JPW), a->M);
  if (!norm)
    hipLaunchKernelGGL((lora_shrink_kernel<false, 1>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, a->K, nrank, a->n_adapters, res, nw, a->eps);
  else if (a->K <= 2048)
    hipLaunchKernelGGL((lora_shrink_kernel<true, 1>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, a->K, nrank, a->n_adapters, res, nw, a->eps);
  else
    hipLaunchKernelGGL((lora_shrink_kernel<true, 2>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, a->K, nrank, a->n_adapters, res, nw, a->eps);
  const int rc = check_launch("ivl_lora_add_small_m_fwd (shrink)");
  if (rc != IVL_OK) return rc;
  switch (a->R) {
    case 8: launch_expand<8>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    case 16: launch_expand<16>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    case 32: launch_expand<32>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
    default: launch_expand<64>(y, idx, B, a->scaling, t_ws, a->M, a->N, a->n_adapters, a->n_seg, segs, st); break;
  }
  return check_launch("ivl_lora_add_small_m_fwd (expand-add)");
}

// y[M,N] = x[M,K] W[N,K]^T (+ bias), bf16 in / fp32 accumulate / bf16 out, for M <= 4 rows: the projections of a
// single-token decode step (InfiniteVLSelfAttention / GatedDeltaNet / MLP / lm_head at T = 1, demo:399-422 loop).
// At M = 1 a GEMM is a pure weight stream (2 FLOP per weight byte): the bound is HBM, so the kernel is a
// bandwidth kernel, not an MFMA kernel -- every wave owns RPW weight rows, every lane streams 16-byte pieces of
// them (whole 1 KB wavefront loads, non-temporal: each weight byte is used once per step) with 4*RPW loads in
// flight, multiplies in fp32 (bf16 -> fp32 is a shift; v_dot2c_f32_bf16 did not reproduce the fp32 reference on
// gfx950 and is not used) and the 64 partial sums of a row meet in one wave reduction.
//
// GLU variant (the SwiGLU MLP, std:945): W is the fused gate|up weight [2I,K]; a wave owns rows n and I+n and writes
// act[n] = bf16(bf16(silu(bf16(gate_n))) * bf16(up_n)) -- the gate costs one exp per OUTPUT element.  (Forming the
// gate on the input side of down_proj instead repeats it in every wave: measured 2.49 -> 2.88 ms per decode token.)
//
// NORM variant (round 3): the RMSNorm in front of the projection -- (residual add +) Qwen2RMSNorm, 73 one-row launches of
// ivl_add_rmsnorm_fwd per decode token, each ~4.2 us inside the token's graph: 15 % of the token -- runs in the prologue of
// the weight stream.  Every workgroup forms the normalised rows itself (M x K <= 4 x 4096 elements: 8 KB of L2-resident
// input per row, the same thread -> element mapping and summation order as add_rmsnorm_kernel, through the same
// add_round_ / sumsq8_ / qwen_norm_: the rows are bit-identical to that kernel's) into LDS while its first weight pieces are in
// flight, and reads x from there;
// workgroup 0 also writes the new residual stream h = bf16(x + residual).
//
// WEIGHT-ONLY E4M3 (the *_w8 entry points): the same kernels instantiated on 1-byte OCP e4m3fn codes with one fp32 scale
// per weight row -- half the bytes of the stream, the x side untouched, and with power-of-two scales the bf16 kernels' output on the
// dequantised weight bit for bit.
//
// WEIGHT-ONLY MXFP4 (the *_w4 entry points): the same kernels on OCP e2m1 codes, two per byte, with one e8m0 power-of-two
// scale per 32 weights, in a pre-shuffled layout (include/ivl_hip.h) that hands a lane the four pieces of a loop trip in one 16-byte
// load -- a quarter of the bytes, and again the bf16 kernels' output on the dequantised weight bit for bit.
#include "ivl_rowwise.h"

namespace ivl {

__device__ __forceinline__ float dot8(u32x4 a, u32x4 b, float acc) {
  acc = fmaf(bflo(a.x), bflo(b.x), acc); acc = fmaf(bfhi(a.x), bfhi(b.x), acc);
  acc = fmaf(bflo(a.y), bflo(b.y), acc); acc = fmaf(bfhi(a.y), bfhi(b.y), acc);
  acc = fmaf(bflo(a.z), bflo(b.z), acc); acc = fmaf(bfhi(a.z), bfhi(b.z), acc);
  acc = fmaf(bflo(a.w), bflo(b.w), acc); acc = fmaf(bfhi(a.w), bfhi(b.w), acc);
  return acc;
}

constexpr int LSM_U = 4;          // 16-byte pieces per lane per row in flight

// e4m3 (OCP e4m3fn, the gfx950 encoding) piece of 8 weights = 8 bytes: v_cvt_pk_f32_fp8 decodes two bytes per instruction, exactly;
// the products and their order are dot8's
__device__ __forceinline__ float dot8_e4m3(u32x2 a, u32x4 b, float acc) {
  const auto w01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.x, false), w23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.x, true);
  const auto w45 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.y, false), w67 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.y, true);
  acc = fmaf(w01[0], bflo(b.x), acc); acc = fmaf(w01[1], bfhi(b.x), acc);
  acc = fmaf(w23[0], bflo(b.y), acc); acc = fmaf(w23[1], bfhi(b.y), acc);
  acc = fmaf(w45[0], bflo(b.z), acc); acc = fmaf(w45[1], bfhi(b.z), acc);
  acc = fmaf(w67[0], bflo(b.w), acc); acc = fmaf(w67[1], bfhi(b.w), acc);
  return acc;
}

// WEIGHT-ELEMENT POLICIES.  The kernels below are written once; a policy says what a lane's piece of 8 weights is, how a row is
// found and how a piece meets its 8 x values.  The lane -> chunk mapping, the fmaf chain and wave_sum -- the summation ORDER -- are
// the kernels', so the e4m3 stream has the bf16 stream's order by construction.  Both keep LSM_U pieces per row in flight: an e4m3
// piece is half the bytes, but 8 (and 16) of them per row measured SLOWER at M = 1 than 4 (lm_head 73 and 123 us against 47, gate|up
// 14.5 against 12.3: DESIGN 4.13) -- the registers they take cost more occupancy than the bytes in flight buy.
//
// WMxfp4 (the *_w4 entry points) replaces the LSM_U piece loads of a trip by ONE 16-byte load of codes and one 4-byte load
// of block scales per weight row (PACKED: the shuffled layout of include/ivl_hip.h puts a lane's four pieces of a trip side by side);
// the block scale is part of the weight, so there is no scaled epilogue.
struct WBf16 {                                     // bf16 [N,K]: 16-byte pieces
  using piece = u32x4;
  using arg = const bf16_t* __restrict__;
  static constexpr bool SCALED = false, PACKED = false;
  static bool null(arg w) { return w == nullptr; }
  static __device__ __forceinline__ const piece* row(arg w, size_t r, int K) { return (const piece*)(w + r * K); }
  static __device__ __forceinline__ float scale(arg, int) { return 1.f; }
  static __device__ __forceinline__ float dot(piece a, u32x4 b, float acc) { return dot8(a, b, acc); }
};
struct W8Arg { const unsigned char* q; const float* scale; };
struct WE4m3 {                                     // e4m3 codes [N,K] + one fp32 scale per row: 8-byte pieces
  using piece = u32x2;
  using arg = W8Arg;
  static constexpr bool SCALED = true, PACKED = false;
  static bool null(arg w) { return w.q == nullptr || w.scale == nullptr; }
  static __device__ __forceinline__ const piece* row(arg w, size_t r, int K) { return (const piece*)(w.q + r * K); }
  static __device__ __forceinline__ float scale(arg w, int r) { return w.scale[r]; }
  static __device__ __forceinline__ float dot(piece a, u32x4 b, float acc) { return dot8_e4m3(a, b, acc); }
};
struct W4Arg { const unsigned char* q; const unsigned char* s; };
struct WMxfp4 {                                    // e2m1 codes, two per byte, + one e8m0 scale per 32 weights, shuffled: 4-byte pieces
  using piece = unsigned int;
  using arg = W4Arg;
  static constexpr bool SCALED = false, PACKED = true;
  static bool null(arg w) { return w.q == nullptr || w.s == nullptr; }
  static __host__ __device__ __forceinline__ int kp(int K) { return (K + 2047) & ~2047; }      // a row is whole tiles of 2048 weights
  static __device__ __forceinline__ const piece* row(arg w, size_t r, int K) { return (const piece*)(w.q + r * (size_t)(kp(K) >> 1)); }
  static __device__ __forceinline__ const unsigned int* srow(arg w, size_t r, int K) {
    return (const unsigned int*)(w.s + r * (size_t)(kp(K) >> 5));
  }
  static __device__ __forceinline__ float scale(arg, int) { return 1.f; }
  // trip t of a row (chunks 256t + lane + 64u): the lane's four pieces are dwords 4 (64t + lane) .. + 3 of the row, their four scale
  // bytes dword 16t + (lane >> 2) of the scale row
  static __device__ __forceinline__ u32x4 load_codes(const piece* row, int t, int lane) {
    return __builtin_nontemporal_load((const u32x4*)row + t * 64 + lane);
  }
  static __device__ __forceinline__ unsigned int load_scales(const unsigned int* srow, int t, int lane) {
    return __builtin_nontemporal_load(srow + t * 16 + (lane >> 2));
  }
  // piece a (element 2j in the low nibble of byte j) with the e8m0 byte sb: v_cvt_scalef32_pk_f32_fp4 decodes two codes and multiplies
  // by 2^(sb - 127), exactly; the products and their order are dot8's
  static __device__ __forceinline__ void decode(piece a, unsigned int sb, float (&w)[8]) {
    const float s = __builtin_bit_cast(float, sb << 23);
    const auto w01 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 0), w23 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 1);
    const auto w45 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 2), w67 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 3);
    w[0] = w01[0]; w[1] = w01[1]; w[2] = w23[0]; w[3] = w23[1]; w[4] = w45[0]; w[5] = w45[1]; w[6] = w67[0]; w[7] = w67[1];
  }
  static __device__ __forceinline__ float dot(const float (&w)[8], u32x4 b, float acc) {
    acc = fmaf(w[0], bflo(b.x), acc); acc = fmaf(w[1], bfhi(b.x), acc);
    acc = fmaf(w[2], bflo(b.y), acc); acc = fmaf(w[3], bfhi(b.y), acc);
    acc = fmaf(w[4], bflo(b.z), acc); acc = fmaf(w[5], bfhi(b.z), acc);
    acc = fmaf(w[6], bflo(b.w), acc); acc = fmaf(w[7], bfhi(b.w), acc);
    return acc;
  }
};

struct NormArgs {
  const bf16_t* residual;          // NULL: plain norm of x
  const bf16_t* weight;            // RMSNorm weight [K]
  bf16_t* h_out;                   // new residual stream (written by workgroup 0 when residual != NULL)
  float eps;
};
constexpr int LSM_NORM_KMAX = 4096;

// N = number of OUTPUT columns (GLU: I; the weight then has 2N rows)
// NIT: 16-byte pieces of a row per thread in the norm prologue (1: K <= 2048 -- the hidden size of the model; 2: K <= 4096);
// the prologue's registers are live while the first weight batch is in flight, and 218 VGPRs meant 2 workgroups per CU: the M = 1
// instances (the decode token) are capped at 168 (three workgroups per CU); M >= 2 would spill there and keeps the default
template <class WT, int RPW, int M, bool GLU, bool NORM, int NIT = 2>
__global__ __launch_bounds__(256, (NORM && M == 1) ? 3 : 1) void linear_small_m_kernel(const bf16_t* __restrict__ x, typename WT::arg w,
                                                            const bf16_t* __restrict__ bias, bf16_t* __restrict__ y,
                                                            int N, int K, NormArgs na) {
  constexpr int NR = GLU ? 2 * RPW : RPW;          // weight rows per wave
  using piece_t = typename WT::piece;
  __shared__ __attribute__((aligned(16))) u32x4 s_x[NORM ? M * (LSM_NORM_KMAX / 8) : 1];
  __shared__ float s_part[NORM ? M : 1][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = K >> 3;
  const int row0 = (blockIdx.x * 4 + wave) * RPW;
  if (!NORM && row0 >= N) return;                  // (NORM: every wave takes part in the barriers; its rows are clamped, its stores guarded)
  const piece_t* wrow[NR];
  float wscale[WT::SCALED ? NR : 1];               // (e4m3: the rows' scales, requested ahead of the stream -- the epilogue would wait for them)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int rr = min(row0 + (r % RPW), N - 1) + (r >= RPW ? N : 0);      // GLU: rows [RPW, 2RPW) are the "up" rows
    wrow[r] = WT::row(w, (size_t)rr, K);
    if constexpr (WT::SCALED) wscale[r] = WT::scale(w, __builtin_amdgcn_readfirstlane(rr));      // (wave-uniform: SGPRs)
  }
  const unsigned int* wsrow[WT::PACKED ? NR : 1];  // (mxfp4: the rows' block scales)
  if constexpr (WT::PACKED) {
#pragma unroll
    for (int r = 0; r < NR; ++r) wsrow[r] = WT::srow(w, (size_t)(min(row0 + (r % RPW), N - 1) + (r >= RPW ? N : 0)), K);
  }
  float acc[NR][M];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[r][m] = 0.f;

  // NORM: the rows' pieces (x, residual, norm weight) are requested FIRST -- vector-memory results return in issue order, so
  // requested behind the weight pieces they would only arrive behind the whole weight stream of the wave -- then the weight
  // pieces; norm_rows (every wave: workgroup barriers inside) then runs while the weights are in flight.
  const int tid = threadIdx.x;
  u32x4 xraw[NORM ? M : 1][NIT], rraw[NORM ? M : 1][NIT], wraw[NIT];
  if constexpr (NORM) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int v = min(tid + it * 256, nchunk - 1);
      wraw[it] = *(const u32x4*)(na.weight + v * 8);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        xraw[m][it] = *(const u32x4*)(x + (size_t)m * K + v * 8);
        rraw[m][it] = na.residual != nullptr ? *(const u32x4*)(na.residual + (size_t)m * K + v * 8) : u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
  auto norm_rows = [&]() {
    float hv[M][NIT][8];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float ss = 0.f;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int v = tid + it * 256;
        if (v < nchunk) {
          unpack8(xraw[m][it], hv[m][it]);
          if (na.residual != nullptr) {
            float rv[8];
            unpack8(rraw[m][it], rv);
#pragma unroll
            for (int i = 0; i < 8; ++i) hv[m][it][i] = add_round_(hv[m][it][i], rv[i]);
            if (blockIdx.x == 0) *(u32x4*)(na.h_out + (size_t)m * K + v * 8) = pack8(hv[m][it]);
          }
          ss = sumsq8_(hv[m][it], ss);
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) s_part[m][wave] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float tot = s_part[m][0] + s_part[m][1] + s_part[m][2] + s_part[m][3];
      const float rstd = qwen_rstd_(tot, K, na.eps);
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int v = tid + it * 256;
        if (v < nchunk) {
          float wv8[8], o8[8];
          unpack8(wraw[it], wv8);
#pragma unroll
          for (int i = 0; i < 8; ++i) o8[i] = qwen_norm_(hv[m][it][i], rstd, wv8[i]);
          s_x[m * (LSM_NORM_KMAX / 8) + v] = pack8(o8);
        }
      }
    }
    __syncthreads();
  };
  bool first = true;
  // mxfp4: a trip is 20 bytes per lane and row, so the plain and GLU forms of M >= 2 keep TWO trips in flight -- the next trip's codes
  // and scales are requested before this trip's are used.  Measured: at M = 4 down K = 11008 19.6 -> 14.7 us, GDN o_proj
  // 7.6 -> 6.3, lm_head 93 -> 84 (its one trip is requested ahead of the x rows); at M = 1 nothing gains and the 4-rows-per-wave
  // instance goes from 71 to 131 VGPRs (lm_head 38 -> 44 us).  Not the NORM form: its K <= 4096 is two trips at most, and its
  // M = 1 instances (capped at 168 VGPRs) would spill.
  constexpr bool AHEAD = WT::PACKED && !NORM && M > 1;
  u32x4 qnext[WT::PACKED ? NR : 1];
  unsigned int snext[WT::PACKED ? NR : 1];
  auto load_trip = [&](int t) {                    // (a padded row holds whole trips: no clamp)
    if constexpr (WT::PACKED) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        qnext[r] = WT::load_codes(wrow[r], t, lane);
        snext[r] = WT::load_scales(wsrow[r], t, lane);
      }
    }
  };
  if constexpr (AHEAD) {
    if (lane < nchunk) load_trip(0);
  }
  for (int c0 = lane; c0 < nchunk; c0 += 64 * LSM_U) {
    piece_t wv[LSM_U][NR];
    u32x4 xv[LSM_U][M];
    unsigned int wsb[WT::PACKED ? NR : 1];         // (mxfp4: byte u = the block scale of piece u)
    if constexpr (WT::PACKED) {
      static_assert(LSM_U == 4, "a 16-byte load holds the four pieces of a trip");
      if constexpr (!AHEAD) load_trip(c0 >> 8);    // (c0 = lane + 256 t)
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        wv[0][r] = qnext[r].x; wv[1][r] = qnext[r].y; wv[2][r] = qnext[r].z; wv[3][r] = qnext[r].w;
        wsb[r] = snext[r];
      }
      if constexpr (AHEAD) {
        if (c0 + 64 * LSM_U < nchunk) load_trip((c0 >> 8) + 1);
      }
    } else {
#pragma unroll
      for (int u = 0; u < LSM_U; ++u) {
        const int cc = min(c0 + 64 * u, nchunk - 1);
#pragma unroll
        for (int r = 0; r < NR; ++r) wv[u][r] = __builtin_nontemporal_load(wrow[r] + cc);
      }
    }
    if constexpr (NORM) {
      if (first) norm_rows();                      // (the loop trip count is workgroup-uniform)
      first = false;
    }
#pragma unroll
    for (int u = 0; u < LSM_U; ++u) {
      const int c = c0 + 64 * u;
      const int cc = min(c, nchunk - 1);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        u32x4 xl;
        if constexpr (NORM) xl = s_x[m * (LSM_NORM_KMAX / 8) + cc];
        else xl = *((const u32x4*)(x + (size_t)m * K) + cc);
        xv[u][m] = c < nchunk ? xl : u32x4{0u, 0u, 0u, 0u};      // pieces past the row end contribute nothing
      }
    }
    if constexpr (WT::PACKED) {
#pragma unroll
      for (int u = 0; u < LSM_U; ++u)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float wf[8];
          WT::decode(wv[u][r], (wsb[r] >> (8 * u)) & 0xffu, wf);
#pragma unroll
          for (int m = 0; m < M; ++m) acc[r][m] = WT::dot(wf, xv[u][m], acc[r][m]);
        }
    } else {
#pragma unroll
      for (int u = 0; u < LSM_U; ++u)
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
          for (int m = 0; m < M; ++m) acc[r][m] = WT::dot(wv[u][r], xv[u][m], acc[r][m]);
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float s = wave_sum(acc[r][m]);
      float s2 = 0.f;
      if (GLU) s2 = wave_sum(acc[RPW + r][m]);
      if constexpr (WT::SCALED) {                  // y = bf16(scale * acc + bias): the product is exact for a scale 2^e
        s = wscale[r] * s;
        if (GLU) s2 = wscale[RPW + r] * s2;
      }
      if (lane == 0 && row0 + r < N) {
        if (GLU) {
          const float gt = bf_round(s + (bias != nullptr ? bf2f(bias[row0 + r]) : 0.f));          // gate_proj output
          const float up = bf_round(s2 + (bias != nullptr ? bf2f(bias[N + row0 + r]) : 0.f));     // up_proj output
          const float g1[1] = {gt};
          float s1[1];
          siluf_n_(g1, s1);
          y[(size_t)m * N + row0 + r] = f2bf(bf_round(s1[0]) * up);                              // = silu_mul_kernel
        } else {
          y[(size_t)m * N + row0 + r] = f2bf(s + (bias != nullptr ? bf2f(bias[row0 + r]) : 0.f));
        }
      }
    }
}

template <class WT, int RPW, bool GLU, bool NORM>
static void launch_lsm(const bf16_t* x, typename WT::arg w, const bf16_t* bias, bf16_t* y, int M, int N, int K, const NormArgs& na,
                       hipStream_t st) {
  const int rows_per_wg = 4 * RPW;
  dim3 grid((N + rows_per_wg - 1) / rows_per_wg);
  if (NORM && K <= 2048) {
    switch (M) {
      case 1: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 1, GLU, NORM, 1>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
      case 2: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 2, GLU, NORM, 1>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
      case 3: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 3, GLU, NORM, 1>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
      default: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 4, GLU, NORM, 1>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
    }
    return;
  }
  switch (M) {
    case 1: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 1, GLU, NORM>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
    case 2: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 2, GLU, NORM>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
    case 3: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 3, GLU, NORM>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
    default: hipLaunchKernelGGL((linear_small_m_kernel<WT, RPW, 4, GLU, NORM>), grid, dim3(256), 0, st, x, w, bias, y, N, K, na); break;
  }
}

template <class WT, bool NORM>
static int lsm_dispatch(const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N, int K, bool glu, const NormArgs& na,
                        void* stream, const char* who) {
  IVL_REQUIRE(x && !WT::null(wp) && y, IVL_ERR_INVALID_ARG, "%s: NULL pointer", who);
  IVL_REQUIRE(M >= 1 && M <= 4, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..4 rows; use a GEMM)", who, M);
  IVL_REQUIRE(N > 0 && K > 0 && K % 8 == 0, IVL_ERR_INVALID_ARG, "%s: N=%d K=%d (K must be a multiple of 8)", who, N, K);
  if constexpr (WT::PACKED) {
    IVL_REQUIRE(K % 32 == 0, IVL_ERR_INVALID_ARG, "%s: K=%d (one block scale per 32 weights: K must be a multiple of 32)", who, K);
    IVL_REQUIRE(((size_t)wp.q & 15) == 0 && ((size_t)wp.s & 3) == 0, IVL_ERR_INVALID_ARG,
                "%s: wq must be 16-byte aligned and sq 4-byte aligned", who);
  }
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *xp = (const bf16_t*)x, *bp = (const bf16_t*)bias;
  bf16_t* yp = (bf16_t*)y;
  // rows per wave: enough workgroups to cover the chip (>= ~2 per CU) before amortising the x reads over more rows (mxfp4 keeps the
  // rule: 8 rows per wave from N = 32768 measured lm_head at 48 us against 44 with 4 in the same build -- DESIGN 4.14)
  if (glu) {
    if (N >= 4096) launch_lsm<WT, 2, true, NORM>(xp, wp, bp, yp, M, N, K, na, st);       // 4 weight rows per wave
    else launch_lsm<WT, 1, true, NORM>(xp, wp, bp, yp, M, N, K, na, st);
  } else {
    if (N >= 8192) launch_lsm<WT, 4, false, NORM>(xp, wp, bp, yp, M, N, K, na, st);
    else if (N >= 4096) launch_lsm<WT, 2, false, NORM>(xp, wp, bp, yp, M, N, K, na, st);
    else launch_lsm<WT, 1, false, NORM>(xp, wp, bp, yp, M, N, K, na, st);
  }
  return check_launch(who);
}

// ------------------------------------------------------------------------------------------------------------------------------
// GDN output projection of a decode step with the GATED RMSNorm in its prologue (round 5): x = o_norm(o, gate) is
// formed by every workgroup itself -- per head a 256-wide statistic of the un-normalised bf16 delta-rule output (8 KB per row,
// L2-resident) and the gate columns of the projection row -- through gated_norm_n_ with the element layout of
// gdn_decode_step_kernel's last block (lane l of a wave holds elements 4l .. 4l + 3 of a head), staged in LDS, then the o_proj weight
// stream reads x from there.  What makes it worth a kernel: the decode step itself can then run on 4 x as many workgroups
// (gdn_decode_split_kernel) because nothing spans a head any more.  The first workgroups also shift the conv states of q and k
// (new state = taps 1..3 + the step's raw projection value): every quarter workgroup of the split step READS those states, so
// they can only be written by the NEXT launch.
struct GdnOutArgs {
  const bf16_t* gate; long long gate_ld;           // gate[m][h * 256 + c] = gate[m * gate_ld + h * 256 + c]
  const bf16_t* norm_w; float eps; int H;
  const bf16_t* proj; long long proj_ld; int col_q, col_k;
  bf16_t* cq; bf16_t* ck; int Dq;                  // conv states [M, Dq, 4] of q and k
};
template <class WT, int M>
__global__ __launch_bounds__(256) void linear_gdn_out_kernel(const bf16_t* __restrict__ o_raw, typename WT::arg w,
                                                             const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int N, int K, GdnOutArgs ga) {
  __shared__ __attribute__((aligned(16))) u32x4 s_x[M * (LSM_NORM_KMAX / 8)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tid = threadIdx.x;
  const int nchunk = K >> 3;
  using piece_t = typename WT::piece;
  const int row = min((int)blockIdx.x * 4 + wave, N - 1);
  const piece_t* wrow = WT::row(w, (size_t)row, K);
  float wscale = 1.f;
  if constexpr (WT::SCALED) wscale = WT::scale(w, __builtin_amdgcn_readfirstlane(row));
  const unsigned int* wsrow = nullptr;             // (mxfp4: the row's block scales)
  if constexpr (WT::PACKED) wsrow = WT::srow(w, (size_t)row, K);
  // ---- conv-state shift of q and k (a few items per workgroup; independent of everything else here) ----
  {
    const int total = M * 2 * ga.Dq;
    for (int item = (int)blockIdx.x * 256 + tid; item < total; item += (int)gridDim.x * 256) {
      const int ch = item % ga.Dq, rest = item / ga.Dq, isk = rest & 1, m = rest >> 1;
      bf16_t* st = (isk ? ga.ck : ga.cq) + ((size_t)m * ga.Dq + ch) * 4;
      const u32x2 sv = *(const u32x2*)st;
      const bf16_t xr = ga.proj[(size_t)m * ga.proj_ld + (isk ? ga.col_k : ga.col_q) + ch];
      *(u32x2*)st = conv_state_shift1_(sv, xr);
    }
  }
  // ---- the rows' pieces first (o, gate, norm weight: 4 heads per wave), then the first weight batch, then the norm ----
  constexpr int HPW = 4;                           // heads per wave: head = wave + 4 i (H <= 16)
  u32x2 oraw[M][HPW], graw[M][HPW];
  const u32x2 wv = *(const u32x2*)(ga.norm_w + 4 * lane);
#pragma unroll
  for (int i = 0; i < HPW; ++i) {
    const int hh = min(wave + 4 * i, ga.H - 1);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      oraw[m][i] = *(const u32x2*)(o_raw + (size_t)m * K + hh * 256 + 4 * lane);
      graw[m][i] = *(const u32x2*)(ga.gate + (size_t)m * ga.gate_ld + hh * 256 + 4 * lane);
    }
  }
  float acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) acc[m] = 0.f;
  bool first = true;
  constexpr bool AHEAD = WT::PACKED && M > 1;      // (mxfp4: two trips in flight, as in linear_small_m_kernel; K >= 512: every lane has a trip 0)
  u32x4 qnext = {0u, 0u, 0u, 0u};
  unsigned int snext = 0;
  if constexpr (AHEAD) {
    qnext = WT::load_codes(wrow, 0, lane);
    snext = WT::load_scales(wsrow, 0, lane);
  }
  for (int c0 = lane; c0 < nchunk; c0 += 64 * LSM_U) {
    piece_t wvv[LSM_U];
    unsigned int wsb = 0;                          // (mxfp4: byte u = the block scale of piece u)
    if constexpr (WT::PACKED) {
      if constexpr (!AHEAD) {
        qnext = WT::load_codes(wrow, c0 >> 8, lane);
        snext = WT::load_scales(wsrow, c0 >> 8, lane);
      }
      wvv[0] = qnext.x; wvv[1] = qnext.y; wvv[2] = qnext.z; wvv[3] = qnext.w;
      wsb = snext;
      if constexpr (AHEAD) {
        if (c0 + 64 * LSM_U < nchunk) {
          qnext = WT::load_codes(wrow, (c0 >> 8) + 1, lane);
          snext = WT::load_scales(wsrow, (c0 >> 8) + 1, lane);
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < LSM_U; ++u) wvv[u] = __builtin_nontemporal_load(wrow + min(c0 + 64 * u, nchunk - 1));
    }
    if (first) {                                  // (workgroup-uniform trip count)
      const float wf[4] = {bflo(wv.x), bfhi(wv.x), bflo(wv.y), bfhi(wv.y)};
#pragma unroll
      for (int i = 0; i < HPW; ++i) {
        const int hh = wave + 4 * i;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const float o4[4] = {bflo(oraw[m][i].x), bfhi(oraw[m][i].x), bflo(oraw[m][i].y), bfhi(oraw[m][i].y)};
          const float gf[4] = {bflo(graw[m][i].x), bfhi(graw[m][i].x), bflo(graw[m][i].y), bfhi(graw[m][i].y)};
          const float ss = wave_sum(o4[0] * o4[0] + o4[1] * o4[1] + o4[2] * o4[2] + o4[3] * o4[3]);
          float y4[4];
          gated_norm_n_(o4, rms256_rstd_(ss, ga.eps), wf, gf, y4);
          if (hh < ga.H)
            *(u32x2*)((bf16_t*)s_x + (size_t)m * LSM_NORM_KMAX + hh * 256 + 4 * lane) = u32x2{pack2bf(y4[0], y4[1]), pack2bf(y4[2], y4[3])};
        }
      }
      __syncthreads();
      first = false;
    }
#pragma unroll
    for (int u = 0; u < LSM_U; ++u) {
      const int c = c0 + 64 * u;
      const int cc = min(c, nchunk - 1);
      float wf[WT::PACKED ? 8 : 1];
      if constexpr (WT::PACKED) WT::decode(wvv[u], (wsb >> (8 * u)) & 0xffu, wf);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const u32x4 xl = c < nchunk ? s_x[m * (LSM_NORM_KMAX / 8) + cc] : u32x4{0u, 0u, 0u, 0u};
        if constexpr (WT::PACKED) acc[m] = WT::dot(wf, xl, acc[m]);
        else acc[m] = WT::dot(wvv[u], xl, acc[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float sum = wave_sum(acc[m]);
    if constexpr (WT::SCALED) sum = wscale * sum;
    if (lane == 0 && (int)blockIdx.x * 4 + wave < N)
      y[(size_t)m * N + row] = f2bf(sum + (bias != nullptr ? bf2f(bias[row]) : 0.f));
  }
}

}  // namespace ivl

using namespace ivl;

// ---- the bf16 entry points -------------------------------------------------------------------------------------------------
extern "C" int ivl_linear_small_m_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K,
                                      void* stream) {
  return lsm_dispatch<WBf16, false>(x, (const bf16_t*)w, bias, y, M, N, K, false, NormArgs{}, stream, "ivl_linear_small_m_fwd");
}

extern "C" int ivl_linear_swiglu_small_m_fwd(const void* x, const void* w_gate_up, const void* bias, void* y, int M, int I,
                                             int K, void* stream) {
  return lsm_dispatch<WBf16, false>(x, (const bf16_t*)w_gate_up, bias, y, M, I, K, true, NormArgs{}, stream, "ivl_linear_swiglu_small_m_fwd");
}

template <class WT>
static int norm_linear(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out, typename WT::arg w,
                       const void* bias, void* y, int M, int N, int K, int glu, void* stream, const char* who) {
  IVL_REQUIRE(norm_weight != nullptr, IVL_ERR_INVALID_ARG, "%s: NULL norm weight", who);
  IVL_REQUIRE(residual == nullptr || h_out != nullptr, IVL_ERR_INVALID_ARG, "%s: residual needs h_out", who);
  // (K >= 512: every lane of a wave must enter the weight loop, whose first trip holds the workgroup barriers of the norm)
  IVL_REQUIRE(K >= 512 && K <= LSM_NORM_KMAX, IVL_ERR_UNSUPPORTED,
              "%s: K=%d (the normalised rows are staged in LDS by the whole workgroup: 512 <= K <= %d)", who, K, LSM_NORM_KMAX);
  NormArgs na;
  na.residual = (const bf16_t*)residual; na.weight = (const bf16_t*)norm_weight; na.h_out = (bf16_t*)h_out; na.eps = eps;
  return lsm_dispatch<WT, true>(x, w, bias, y, M, N, K, glu != 0, na, stream, who);
}

extern "C" int ivl_norm_linear_small_m_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                           const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream) {
  return norm_linear<WBf16>(x, residual, norm_weight, eps, h_out, (const bf16_t*)w, bias, y, M, N, K, glu, stream,
                            "ivl_norm_linear_small_m_fwd");
}

// o_proj of a GDN decode step with the gated RMSNorm in the prologue and the q / k conv-state shift riding along (see
// linear_gdn_out_kernel; pairs with ivl_gdn_decode_split_fwd).  o_raw bf16 [M, H*256] (un-normalised delta-rule output), gate =
// first gate element of row 0 (row stride gate_ld elements), proj = the step's projection rows (row stride proj_ld), conv states
// [M, Dq, 4] of q and k (updated in place).  y[M, N] = o_norm(o_raw, gate) W^T (+ bias).
template <class WT>
static int gdn_out_linear(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight, float eps, int H,
                          const void* proj, int64_t proj_ld, int col_q, int col_k, void* conv_state_q, void* conv_state_k,
                          typename WT::arg w, const void* bias, void* y, int M, int N, int K, void* stream, const char* who) {
  IVL_REQUIRE(o_raw && gate && norm_weight && proj && conv_state_q && conv_state_k && !WT::null(w) && y, IVL_ERR_INVALID_ARG,
              "%s: NULL pointer", who);
  IVL_REQUIRE(M >= 1 && M <= 4, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..4 rows)", who, M);
  // (H >= 2, i.e. K >= 512: every lane of a wave must enter the weight loop, whose first trip holds the gated norm and its
  // workgroup barrier -- as in the NORM form)
  IVL_REQUIRE(H >= 2 && H <= 16 && K == H * 256 && K <= LSM_NORM_KMAX && N > 0, IVL_ERR_UNSUPPORTED,
              "%s: H=%d K=%d N=%d (2 <= H <= 16, K = H * 256 <= %d: every lane must enter the weight loop, "
              "whose first trip holds the gated norm, as in the NORM form)", who, H, K, N, LSM_NORM_KMAX);
  IVL_REQUIRE(gate_ld % 4 == 0 && ((size_t)gate & 7) == 0 && ((size_t)o_raw & 7) == 0, IVL_ERR_INVALID_ARG,
              "%s: o_raw / gate rows must be 8-byte aligned", who);
  if constexpr (WT::PACKED)                        // (K = H * 256 is a multiple of 32)
    IVL_REQUIRE(((size_t)w.q & 15) == 0 && ((size_t)w.s & 3) == 0, IVL_ERR_INVALID_ARG,
                "%s: wq must be 16-byte aligned and sq 4-byte aligned", who);
  GdnOutArgs ga;
  ga.gate = (const bf16_t*)gate; ga.gate_ld = gate_ld; ga.norm_w = (const bf16_t*)norm_weight; ga.eps = eps; ga.H = H;
  ga.proj = (const bf16_t*)proj; ga.proj_ld = proj_ld; ga.col_q = col_q; ga.col_k = col_k;
  ga.cq = (bf16_t*)conv_state_q; ga.ck = (bf16_t*)conv_state_k; ga.Dq = H * 128;
  const dim3 grid((N + 3) / 4);
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *op = (const bf16_t*)o_raw, *bp = (const bf16_t*)bias;
  switch (M) {
    case 1: hipLaunchKernelGGL((linear_gdn_out_kernel<WT, 1>), grid, dim3(256), 0, st, op, w, bp, (bf16_t*)y, N, K, ga); break;
    case 2: hipLaunchKernelGGL((linear_gdn_out_kernel<WT, 2>), grid, dim3(256), 0, st, op, w, bp, (bf16_t*)y, N, K, ga); break;
    case 3: hipLaunchKernelGGL((linear_gdn_out_kernel<WT, 3>), grid, dim3(256), 0, st, op, w, bp, (bf16_t*)y, N, K, ga); break;
    default: hipLaunchKernelGGL((linear_gdn_out_kernel<WT, 4>), grid, dim3(256), 0, st, op, w, bp, (bf16_t*)y, N, K, ga); break;
  }
  return check_launch(who);
}

extern "C" int ivl_gdn_out_linear_small_m_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight, float eps,
                                              int H, const void* proj, int64_t proj_ld, int col_q, int col_k, void* conv_state_q,
                                              void* conv_state_k, const void* w, const void* bias, void* y, int M, int N, int K,
                                              void* stream) {
  return gdn_out_linear<WBf16>(o_raw, gate, gate_ld, norm_weight, eps, H, proj, proj_ld, col_q, col_k, conv_state_q, conv_state_k,
                               (const bf16_t*)w, bias, y, M, N, K, stream, "ivl_gdn_out_linear_small_m_fwd");
}

// ---- the e4m3 twins: wq uint8 [N,K] (GLU: [2I,K]) OCP e4m3fn codes, scale fp32 [N] / [2I]; everything else as above --------------
extern "C" int ivl_linear_small_m_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N,
                                         int K, void* stream) {
  return lsm_dispatch<WE4m3, false>(x, W8Arg{(const unsigned char*)wq, scale}, bias, y, M, N, K, false, NormArgs{}, stream,
                                    "ivl_linear_small_m_w8_fwd");
}

extern "C" int ivl_linear_swiglu_small_m_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M,
                                                int I, int K, void* stream) {
  return lsm_dispatch<WE4m3, false>(x, W8Arg{(const unsigned char*)wq, scale}, bias, y, M, I, K, true, NormArgs{}, stream,
                                    "ivl_linear_swiglu_small_m_w8_fwd");
}

extern "C" int ivl_norm_linear_small_m_w8_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                              const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K,
                                              int glu, void* stream) {
  return norm_linear<WE4m3>(x, residual, norm_weight, eps, h_out, W8Arg{(const unsigned char*)wq, scale}, bias, y, M, N, K, glu, stream,
                            "ivl_norm_linear_small_m_w8_fwd");
}

extern "C" int ivl_gdn_out_linear_small_m_w8_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight,
                                                 float eps, int H, const void* proj, int64_t proj_ld, int col_q, int col_k,
                                                 void* conv_state_q, void* conv_state_k, const void* wq, const float* scale,
                                                 const void* bias, void* y, int M, int N, int K, void* stream) {
  return gdn_out_linear<WE4m3>(o_raw, gate, gate_ld, norm_weight, eps, H, proj, proj_ld, col_q, col_k, conv_state_q, conv_state_k,
                               W8Arg{(const unsigned char*)wq, scale}, bias, y, M, N, K, stream, "ivl_gdn_out_linear_small_m_w8_fwd");
}

// ---- the MXFP4 twins: wq uint8 [N,Kp/2] e2m1 codes and sq uint8 [N,Kp/32] e8m0 block scales in the shuffled layout of the header ----
extern "C" int ivl_linear_small_m_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                         void* stream) {
  return lsm_dispatch<WMxfp4, false>(x, W4Arg{(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, N, K, false, NormArgs{},
                                     stream, "ivl_linear_small_m_w4_fwd");
}

extern "C" int ivl_linear_swiglu_small_m_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int I,
                                                int K, void* stream) {
  return lsm_dispatch<WMxfp4, false>(x, W4Arg{(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, I, K, true, NormArgs{},
                                     stream, "ivl_linear_swiglu_small_m_w4_fwd");
}

extern "C" int ivl_norm_linear_small_m_w4_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                              const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K, int glu,
                                              void* stream) {
  return norm_linear<WMxfp4>(x, residual, norm_weight, eps, h_out, W4Arg{(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M,
                             N, K, glu, stream, "ivl_norm_linear_small_m_w4_fwd");
}

extern "C" int ivl_gdn_out_linear_small_m_w4_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight,
                                                 float eps, int H, const void* proj, int64_t proj_ld, int col_q, int col_k,
                                                 void* conv_state_q, void* conv_state_k, const void* wq, const void* sq,
                                                 const void* bias, void* y, int M, int N, int K, void* stream) {
  return gdn_out_linear<WMxfp4>(o_raw, gate, gate_ld, norm_weight, eps, H, proj, proj_ld, col_q, col_k, conv_state_q, conv_state_k,
                                W4Arg{(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, N, K, stream,
                                "ivl_gdn_out_linear_small_m_w4_fwd");
}

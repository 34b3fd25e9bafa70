// y[M,N] = x[M,K] W[N,K]^T (+ bias), bf16 in / fp32 accumulate / bf16 out, for 1 <= M <= 64 rows: the projections of a decode step
// that advances 17 to 63 slots.  The 16-row kernel of linear_m16.hip with XT = ceil(M / 16) B operands instead of one:
// a wave still owns tiles of 16 weight rows and streams their K elements once, non-temporally, but a weight piece -- loaded and
// decoded to the bf16 pattern of W' ONCE -- is now the A operand of XT MFMAs, one per tile of 16 x rows.
//
// THE PLAN is that of linear_m16.hip, unchanged, and that is the contract: chunks, tiles and steps s = 16t + j, the four MFMAs
// u = 0..3 with chunk 256t + 4j + g + 64u in k-group g, the 8 contiguous slices of ceil(S / 8) steps, each accumulated from zero in
// ascending (s, u), the eight partials added in fp32 in ascending slice order in LDS, then the bias, then the one rounding; the GLU
// rounding points are those of linear_m16_kernel.  An accumulator here belongs to ONE (weight tile, x tile) pair and sees exactly the
// MFMA sequence that linear_m16_kernel issues for that weight tile with those 16 rows as its B operand; a column of D depends on its
// own column of B only.  So row m of an M-row call is, bit for bit, ivl_linear_m16*_fwd on that row alone -- in the three formats,
// plain and GLU.  What is a choice of speed: how many weight tiles a wave owns per x fragment (CT column tiles; the GLU form has the
// gate and the up tile of each), and how many steps it keeps in flight.
//
// Rows M .. 16 XT - 1 of the B operands are zeros: never read from x (the row index is clamped to M - 1 and the piece replaced by
// zeros), never written to y.  Weight rows past the last are neither read (clamped) nor stored.
//
// THE X SIDE.  A B fragment is 16 rows x 64 bytes, and in fragment shape the four lanes that share a row's 64 bytes are 16 lanes
// apart: every lane of a load instruction is a cache line request of its own, and that request rate -- not HBM, not the MFMAs -- bounds a
// workgroup that reads XT fragments per weight piece (measured: DESIGN 4.18).  So a wave loads a fragment ROW-MAJOR (lane l: row l >> 2,
// 16-byte piece l & 3 -- four adjacent lanes per 64 bytes), writes it to a 1 KB block of its OWN LDS region and reads it back in
// fragment shape (lane: row lane & 15, piece lane >> 4); the piece index is XOR-swizzled with bits 2..3 of the row, so that neither the
// write nor the read has a bank conflict.  Nothing is shared between waves -- every wave has its own K slice -- so the round trip
// needs no workgroup barrier, only wave-scope fences.  The same region holds the partial sums of the K split after the loop.  The wide
// plain projections own two tiles per fragment (as in linear_m16.hip), the GLU form two by construction; four tiles per wave and a
// K slab of x shared by the waves of a workgroup were not built ("not built").
#include "linear_m16.h"

namespace ivl {

constexpr int M64_XT = 4;         // x tiles of 16 rows: 64 rows at most

// steps in flight per wave: a step holds 16 XT registers of x pieces per lane, so two steps only up to two x tiles
template <int XT> constexpr int m64_pf() { return XT <= 2 ? 2 : 1; }

// CT: column tiles (of 16 output columns) per wave; GLU: each with its gate and its up tile.  N = number of OUTPUT columns (GLU: I;
// the weight then has 2N rows); per = steps per slice.  Accumulator (a, i): weight tile a = ct (GLU: 2 ct + half), x tile i.
constexpr int M64_STAGE = 4096;   // bytes of LDS per wave and x tile: the four fragments (u = 0..3) of one step

// the LDS of a workgroup: 8 waves x XT x 4 KB of staging, which the 7 x NA x XT KB of partial sums reuse (NA <= 4)
template <int XT> constexpr int m64_lds_bytes() { return M16_KS * XT * M64_STAGE; }

// what a wave wrote to its LDS region is visible to its own later reads, and the reverse (LDS serves a wave in order: no wait, only
// an order the compiler must keep)
__device__ __forceinline__ void m64_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class WT, bool GLU, int CT, int XT>
__global__ __launch_bounds__(64 * M16_KS) void linear_m64_kernel(const bf16_t* __restrict__ x, typename WT::arg w,
                                                                   const bf16_t* __restrict__ bias, bf16_t* __restrict__ y, int M, int N,
                                                                   int K, int per) {
  constexpr int NA = GLU ? 2 * CT : CT;            // weight tiles per wave
  constexpr int COLS = 16 * CT;                    // output columns per wave
  constexpr int PF = m64_pf<XT>();
  static_assert((M16_KS - 1) * NA * XT * 1024 <= m64_lds_bytes<XT>(), "the partial sums of 7 slices reuse the staging area");
  extern __shared__ __align__(16) unsigned char m64_lds[];
  f32x4 (*s_part)[NA * XT][64] = (f32x4 (*)[NA * XT][64])m64_lds;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int tile = (int)blockIdx.x, slice = wave;
  const int nchunk = K >> 3;
  const int n0 = tile * COLS;
  typename WT::row wr[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int ct = GLU ? a >> 1 : a, half = GLU ? a & 1 : 0;                  // (GLU: half = 1 is the "up" row)
    wr[a] = WT::open(w, min(n0 + 16 * ct + r16, N - 1) + half * N, K);
  }
  // x: loaded row-major (row lrow, piece lpc), staged at wofs of a fragment's block, read back in fragment shape at rofs
  const int lrow = lane >> 2, lpc = lane & 3;
  unsigned char* stage = m64_lds + wave * (XT * M64_STAGE);
  const unsigned int wofs = 64u * lrow + 16u * (lpc ^ ((lrow >> 2) & 3)), rofs = 64u * r16 + 16u * (g ^ ((r16 >> 2) & 3));
  const u32x4* xrow[XT];
  bool mlive[XT];
#pragma unroll
  for (int i = 0; i < XT; ++i) {
    xrow[i] = (const u32x4*)(x + (size_t)min(16 * i + lrow, M - 1) * K);
    mlive[i] = 16 * i + r16 < M;
  }
  f32x4 acc[NA][XT];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int i = 0; i < XT; ++i) acc[a][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};

  const int S = m16_steps(K);
  const int s_end = min(S, (slice + 1) * per);
  for (int s = slice * per; s < s_end; s += PF) {
    typename WT::raw wv[PF][NA];
    u32x4 xv[PF][XT][4];
#pragma unroll
    for (int p = 0; p < PF; ++p) {                 // (a step past the slice repeats the last one and is masked below)
      const int ss = min(s + p, s_end - 1), t = ss >> 4, j = ss & 15;
#pragma unroll
      for (int a = 0; a < NA; ++a) WT::load(w, wr[a], t, j, g, nchunk, wv[p][a]);
#pragma unroll
      for (int i = 0; i < XT; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[p][i][u] = xrow[i][min(256 * t + 4 * j + lpc + 64 * u, nchunk - 1)];
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int ss = min(s + p, s_end - 1), t = ss >> 4, j = ss & 15;
#pragma unroll
      for (int i = 0; i < XT; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) *(u32x4*)(stage + (i * 4 + u) * 1024 + wofs) = xv[p][i][u];
      m64_wave_sync();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = s + p < s_end && 256 * t + 4 * j + g + 64 * u < nchunk;
        bf16x8 b[XT];
#pragma unroll
        for (int i = 0; i < XT; ++i) b[i] = m16_frag(ok && mlive[i] ? *(const u32x4*)(stage + (i * 4 + u) * 1024 + rofs) : zero);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const bf16x8 wa = m16_frag(ok ? WT::bits(wv[p][a], wr[a], u) : zero);      // decoded once, the A operand of XT MFMAs
#pragma unroll
          for (int i = 0; i < XT; ++i) acc[a][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, b[i], acc[a][i], 0, 0, 0);
        }
      }
      m64_wave_sync();                             // (the next step's fragments overwrite the blocks)
    }
  }

  __syncthreads();                                 // every wave is done with its staging blocks: the partial sums take their place
  if (slice != 0) {                                // slices 1 .. 7 hand over, slice 0 adds them in ascending order
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int i = 0; i < XT; ++i) s_part[slice - 1][a * XT + i][lane] = acc[a][i];
  }
  __syncthreads();
  if (slice != 0) return;
#pragma unroll 1
  for (int k = 1; k < M16_KS; ++k)                 // (not unrolled: 7 x NA x XT partials at once would not fit the registers)
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int i = 0; i < XT; ++i) acc[a][i] += s_part[k - 1][a * XT + i][lane];

#pragma unroll
  for (int i = 0; i < XT; ++i) {
    if (!mlive[i]) continue;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = n0 + 16 * ct + 4 * g;          // this lane: x row 16 i + r16, output columns n .. n + 3
      if (n >= N) continue;
      float o[4];
      if constexpr (GLU) {
        float gt[4], sg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int col = min(n + r, N - 1);
          gt[r] = bf_round(acc[2 * ct][i][r] + (bias != nullptr ? bf2f(bias[col]) : 0.f));          // gate_proj output
          o[r] = bf_round(acc[2 * ct + 1][i][r] + (bias != nullptr ? bf2f(bias[N + col]) : 0.f));   // up_proj output
        }
        siluf_n_(gt, sg);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = bf_round(sg[r]) * o[r];                                   // = silu_mul_kernel
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = acc[ct][i][r] + (bias != nullptr ? bf2f(bias[min(n + r, N - 1)]) : 0.f);
      }
      bf16_t* yp = y + (size_t)(16 * i + r16) * N + n;
      if ((N & 3) == 0) {                          // (n is a multiple of 4: the four columns exist and the piece is 8-byte aligned)
        *(u32x2*)yp = u32x2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) yp[r] = f2bf(o[r]);
      }
    }
  }
}

// two column tiles per wave from 512 weight tiles on, as linear_m16.hip pairs them
static bool m64_pair(int R) { return R >= 8192; }

// more than 64 KB of dynamic LDS is an attribute of the function, set once (a host call: nothing is enqueued)
template <class KF, class... A>
static void m64_launch_one(KF kernel, int lds, dim3 grid, dim3 block, hipStream_t st, A... a) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  (void)attr;                                      // (a failure shows as the launch error that check_launch reports)
  hipLaunchKernelGGL(kernel, grid, block, lds, st, a...);
}

template <class WT, int XT>
static void m64_launch_xt(const bf16_t* x, typename WT::arg wp, const bf16_t* bias, bf16_t* y, int M, int N, int K, int glu, int per,
                          hipStream_t st) {
  const bool pair = !glu && m64_pair(N);
  const dim3 grid((N + (pair ? 31 : 15)) / (pair ? 32 : 16)), block(64 * M16_KS);       // one range of output columns per workgroup
  constexpr int lds = m64_lds_bytes<XT>();
  if (glu) m64_launch_one(linear_m64_kernel<WT, true, 1, XT>, lds, grid, block, st, x, wp, bias, y, M, N, K, per);
  else if (pair) m64_launch_one(linear_m64_kernel<WT, false, 2, XT>, lds, grid, block, st, x, wp, bias, y, M, N, K, per);
  else m64_launch_one(linear_m64_kernel<WT, false, 1, XT>, lds, grid, block, st, x, wp, bias, y, M, N, K, per);
}

template <class WT>
static int m64_launch(const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N, int K, int glu, void* stream,
                      const char* who) {
  const int per = (m16_steps(K) + M16_KS - 1) / M16_KS;
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *xp = (const bf16_t*)x, *bp = (const bf16_t*)bias;
  bf16_t* yp = (bf16_t*)y;
  static_assert(M64_XT == 4, "one instantiation per number of x tiles");
  switch ((M + 15) >> 4) {
    case 1: m64_launch_xt<WT, 1>(xp, wp, bp, yp, M, N, K, glu, per, st); break;
    case 2: m64_launch_xt<WT, 2>(xp, wp, bp, yp, M, N, K, glu, per, st); break;
    case 3: m64_launch_xt<WT, 3>(xp, wp, bp, yp, M, N, K, glu, per, st); break;
    default: m64_launch_xt<WT, 4>(xp, wp, bp, yp, M, N, K, glu, per, st); break;
  }
  return check_launch(who);
}

template <class WT>
static int m64_fwd(const char* who, const void* x, typename WT::arg wp, const void* bias, void* y, int M, int N, int K, int glu,
                   void* stream) {
  return m16_entry<WT>(who, x, wp, bias, y, M, N, K, glu, 16 * M64_XT,
                       [&] { return m64_launch<WT>(x, wp, bias, y, M, N, K, glu, stream, who); });
}

}  // namespace ivl

using namespace ivl;

extern "C" int ivl_linear_m64_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream) {
  return m64_fwd<W16Bf16>("ivl_linear_m64_fwd", x, (const bf16_t*)w, bias, y, M, N, K, glu, stream);
}

extern "C" int ivl_linear_m64_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K,
                                     int glu, void* stream) {
  return m64_fwd<W16E4m3>("ivl_linear_m64_w8_fwd", x, {(const unsigned char*)wq, scale}, bias, y, M, N, K, glu, stream);
}

extern "C" int ivl_linear_m64_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                     int glu, void* stream) {
  return m64_fwd<W16Mxfp4>("ivl_linear_m64_w4_fwd", x, {(const unsigned char*)wq, (const unsigned char*)sq}, bias, y, M, N, K, glu, stream);
}

// What the weight-stream MFMA kernels share (linear_m16.hip: 1..16 rows; linear_m64.hip: 1..64 rows): the K split,
// the weight element policies and the number of steps of THE PLAN that the head of linear_m16.hip describes.  One definition: the two
// kernels hand the MFMA the same operand bits in the same order.
#pragma once
#include "ivl_rowwise.h"

namespace ivl {

constexpr int M16_KS = 8;         // the K split: waves of a workgroup, which share one range of output columns

__device__ __forceinline__ bf16x8 m16_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

struct W16Bf16 {                                   // bf16 [R,K]: four 16-byte pieces per step
  using arg = const bf16_t*;
  struct row { unsigned int off; };
  struct raw { u32x4 p[4]; };
  static bool null(arg w) { return w == nullptr; }
  static size_t row_bytes(int K) { return (size_t)K * 2; }
  static bool aligned(arg w) { return ((size_t)w & 15) == 0; }
  static const char* misaligned() { return "%s: x / w / y must be 16-byte aligned"; }
  static __device__ __forceinline__ row open(arg, int r, int K) { return row{(unsigned int)r * (unsigned int)K * 2u}; }
  static __device__ __forceinline__ void load(arg w, row rw, int t, int j, int g, int nchunk, raw& o) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = min(256 * t + 4 * j + g + 64 * u, nchunk - 1);
      o.p[u] = __builtin_nontemporal_load((const u32x4*)((const unsigned char*)w + (rw.off + (unsigned int)c * 16u)));
    }
  }
  static __device__ __forceinline__ u32x4 bits(const raw& o, row, int u) { return o.p[u]; }
};

struct W16Arg8 { const unsigned char* q; const float* scale; };
struct W16E4m3 {                                   // e4m3fn codes [R,K] + one fp32 scale per row: four 8-byte pieces per step
  using arg = W16Arg8;
  struct row { unsigned int off; float scale; };
  struct raw { u32x2 p[4]; };
  static bool null(arg w) { return w.q == nullptr || w.scale == nullptr; }
  static size_t row_bytes(int K) { return (size_t)K; }
  static bool aligned(arg w) { return ((size_t)w.q & 15) == 0 && ((size_t)w.scale & 3) == 0; }
  static const char* misaligned() { return "%s: x / wq / y must be 16-byte aligned, scale 4-byte aligned"; }
  static __device__ __forceinline__ row open(arg w, int r, int K) { return row{(unsigned int)r * (unsigned int)K, w.scale[r]}; }
  static __device__ __forceinline__ void load(arg w, row rw, int t, int j, int g, int nchunk, raw& o) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = min(256 * t + 4 * j + g + 64 * u, nchunk - 1);
      o.p[u] = __builtin_nontemporal_load((const u32x2*)(w.q + (rw.off + (unsigned int)c * 8u)));
    }
  }
  // W' = bf16(float(code) * scale): v_cvt_pk_f32_fp8 decodes exactly, the product with a power of two is exact and has 4 significant bits
  static __device__ __forceinline__ u32x4 bits(const raw& o, row rw, int u) {
    const u32x2 a = o.p[u];
    const auto w01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.x, false), w23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.x, true);
    const auto w45 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.y, false), w67 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a.y, true);
    const float s = rw.scale;
    return u32x4{pack2bf(w01[0] * s, w01[1] * s), pack2bf(w23[0] * s, w23[1] * s), pack2bf(w45[0] * s, w45[1] * s),
                 pack2bf(w67[0] * s, w67[1] * s)};
  }
};

struct W16Arg4 { const unsigned char* q; const unsigned char* s; };
struct W16Mxfp4 {                                  // the shuffled MXFP4 layout of include/ivl_hip.h: one 16-byte load + one dword per step
  using arg = W16Arg4;
  struct row { unsigned int qoff, soff; };
  struct raw { u32x4 q; unsigned int s; };
  static bool null(arg w) { return w.q == nullptr || w.s == nullptr; }
  static __host__ __device__ __forceinline__ int kp(int K) { return (K + 2047) & ~2047; }        // a row is whole tiles of 2048 weights
  static size_t row_bytes(int K) { return (size_t)(kp(K) >> 1); }
  static bool aligned(arg w) { return ((size_t)w.q & 15) == 0 && ((size_t)w.s & 3) == 0; }
  static const char* misaligned() { return "%s: x / wq / y must be 16-byte aligned, sq 4-byte aligned"; }
  static __device__ __forceinline__ row open(arg, int r, int K) {
    return row{(unsigned int)r * (unsigned int)(kp(K) >> 1), (unsigned int)r * (unsigned int)(kp(K) >> 5)};
  }
  // position p = 4j + g of tile t: codes at byte 1024t + 16p of the row (chunks 256t + p + 64u, u = 0..3), their block scales
  // (blocks 64t + j + 16u) at byte 64t + 4j of the scale row; a padded row holds whole tiles: no clamp
  static __device__ __forceinline__ void load(arg w, row rw, int t, int j, int g, int, raw& o) {
    o.q = __builtin_nontemporal_load((const u32x4*)(w.q + (rw.qoff + (unsigned int)(1024 * t + 16 * (4 * j + g)))));
    o.s = __builtin_nontemporal_load((const unsigned int*)(w.s + (rw.soff + (unsigned int)(64 * t + 4 * j))));
  }
  // v_cvt_scalef32_pk_f32_fp4 decodes two codes and multiplies by 2^(sb - 127), exactly; 2 significant bits
  static __device__ __forceinline__ u32x4 bits(const raw& o, row, int u) {
    const unsigned int a = u == 0 ? o.q.x : u == 1 ? o.q.y : u == 2 ? o.q.z : o.q.w;
    const float s = __builtin_bit_cast(float, ((o.s >> (8 * u)) & 0xffu) << 23);
    const auto w01 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 0), w23 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 1);
    const auto w45 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 2), w67 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(a, s, 3);
    return u32x4{pack2bf(w01[0], w01[1]), pack2bf(w23[0], w23[1]), pack2bf(w45[0], w45[1]), pack2bf(w67[0], w67[1])};
  }
};

// steps of a row of K elements: tile t < T - 1 has all 16, the last one those whose first chunk 256t + 4j lies below K / 8
static __host__ __device__ __forceinline__ int m16_steps(int K) {
  const int nchunk = K >> 3, T = (nchunk + 255) >> 8, last = nchunk - 256 * (T - 1);
  const int sl = (last + 3) >> 2;
  return 16 * (T - 1) + (sl < 16 ? sl : 16);
}

// An entry point of either kernel, whatever the format: every refusal in ONE order and before anything is launched -- NULL, the rows
// (max_rows: 16, or the 64 of linear_m64.hip), N, K, the 32-bit offsets, the alignment that the format asks -- then launch(): the
// kernel's launch, behind the LoRA refusals and the shrink launch where the entry has an adapter.  What differs between the formats
// is the policy's: null(), row_bytes(K) (the bytes of a padded weight row), aligned() and the text of misaligned().
template <class WT, class Launch>
static int m16_entry(const char* who, const void* x, typename WT::arg wp, const void* bias, const void* y, int M, int N, int K, int glu,
                     int max_rows, Launch launch) {
  IVL_REQUIRE(x && !WT::null(wp) && y, IVL_ERR_INVALID_ARG, "%s: NULL pointer", who);
  IVL_REQUIRE(M >= 1 && M <= max_rows, IVL_ERR_UNSUPPORTED, "%s: M=%d (built for 1..%d rows)", who, M, max_rows);
  IVL_REQUIRE(N >= 1, IVL_ERR_INVALID_ARG, "%s: N=%d", who, N);
  IVL_REQUIRE(K >= 32 && K % 32 == 0, IVL_ERR_INVALID_ARG, "%s: K=%d (one MFMA spans 32 k: K must be a multiple of 32, at least 32)", who, K);
  const long long R = (long long)(glu ? 2 : 1) * N;
  // every weight offset is a 32-bit byte offset from the base: ONE bound for the three formats (the plan is theirs in common), and the
  // padded rows of the format at hand
  IVL_REQUIRE(R * K * 2 < (1ll << 32) && R * (long long)WT::row_bytes(K) < (1ll << 32), IVL_ERR_UNSUPPORTED,
              "%s: weight of %lld x %d does not fit 32-bit offsets", who, R, K);
  IVL_REQUIRE((((size_t)x | (size_t)y) & 15) == 0 && ((size_t)bias & 1) == 0 && WT::aligned(wp), IVL_ERR_INVALID_ARG, WT::misaligned(), who);
  return launch();
}

}  // namespace ivl

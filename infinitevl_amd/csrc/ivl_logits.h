// The formulas over a row of bf16 logits that more than one launch evaluates, each written ONCE: the sampling launch (sample.hip)
// and the guidance launch in front of it (guide.hip) agree on a row's maximum, its integer partition sum and a token's
// log-probability because both call the helpers below, and a change to a rounding point or an edge case is made here.
#pragma once
#include "ivl_common.h"

namespace ivl {

typedef unsigned long long u64;

constexpr unsigned SMP_KEY_NINF = 0x007Fu;     // key of -inf (and of NaN): the lowest key that occurs
constexpr u64 SMP_ONE = 1ull << 40;            // weight of the maximum
constexpr float SMP_LOG2E = 1.44269504088896341f;

// bf16 bits -> a 16-bit key whose unsigned order is the numeric order; NaN counts as -inf, -0 as +0
__device__ __forceinline__ unsigned smp_key(unsigned b) {
  if ((b & 0x7FFFu) > 0x7F80u) b = 0xFF80u;
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}
__device__ __forceinline__ float smp_key_value(unsigned k) {
  const unsigned b = (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu);
  return __uint_as_float(b << 16);
}

// Q40 weight of a key: 2^40 exactly at the maximum (also m = +-inf), 0 for -inf below it and below 2^-40
__device__ __forceinline__ u64 smp_weight(unsigned key, unsigned mkey, float xm, float c) {
  if (key == mkey) return SMP_ONE;
  if (key <= SMP_KEY_NINF) return 0ull;
  const float a = (smp_key_value(key) - xm) * c;
  if (!(a > -41.f)) return 0ull;               // also a NaN (0 x inf at a temperature outside what the host admits)
  return (u64)(__builtin_amdgcn_exp2f(a) * 0x1p40f);
}

// the log-partition of a row from the integer sum Z1 of its Q40 weights at temperature 1
// (2^40 <= Z1 < 2^63: the conversion rounds to nearest even, the scaling is exact)
__device__ __forceinline__ float smp_lse(u64 Z1) { return logf((float)Z1 * 0x1p-40f); }

// lp of a key: (x' - m) - lse in fp32; -lse at the maximum (also m = +-inf), -inf for -inf < m
__device__ __forceinline__ float smp_lp(unsigned key, unsigned mkey, float xm, float lse) {
  if (key == mkey) return -lse;
  if (key <= SMP_KEY_NINF) return -__builtin_inff();
  return (smp_key_value(key) - xm) - lse;
}

// fp32 -> bf16 bits, round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ unsigned smp_bf16_rne(float y) {
  unsigned u = __float_as_uint(y);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ u64 smp_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A row of V elements as 16-byte tiles from the 16-byte boundary at or below its start, whatever `ld` and the base: the (at
// most 7) elements in front of and behind the row inside its first and last tile lie in the same 16 bytes as row elements, so
// the loads stay inside the caller's allocation granule; the caller masks them out.
struct SmpRow {
  const u32x4* base;     // 16-byte boundary at or below the row start
  long long nt;          // tiles of 8 elements
  int off;               // row element 0 is element `off` of tile 0
  int V;
};
__device__ __forceinline__ SmpRow smp_row(const bf16_t* row, int V) {
  SmpRow r;
  r.off = (int)(((uintptr_t)row & 15u) >> 1);
  r.base = (const u32x4*)(row - r.off);
  r.V = V;
  r.nt = ((long long)r.off + V + 7) >> 3;
  return r;
}

}  // namespace ivl

// Classifier-free guidance / contrastive decoding in front of the sampling launch: a guided stream is TWO rows of the step's
// logits, the leader (the real prompt) and its partner (the negative prompt), and ONE small launch rewrites the leader's row in
// place from both (GUIDE-0 .. GUIDE-5 at ivl_logit_guide_fwd in include/ivl_hip.h):
//   out(v) = bf16( lu + s (lc - lu) ),  lc / lu = the log-softmax of the leader's / the partner's row,
// HF's UnbatchedClassifierFreeGuidanceLogitsProcessor, and with s = 1 + alpha and the cut ln(beta) visual contrastive decoding.
// The bans and the kernels of sample.hip know nothing of it: they see the edited row.  A second launch behind the draw,
// ivl_rows_follow_fwd, copies the leader's token and `done` code into the partner's row, so the partner's stream is "negative
// prompt + the leader's tokens" without a word going to the host.
//
// One workgroup per row; a row that is not a guided leader returns after reading its table entries.  Three passes over the two
// rows in the 16-byte tiles of sample.hip (the second and third hit L2: two rows are 608 KB at V = 151936):
//   1  the two maxima (keys)      2  the two integer sums of the Q40 weights at temperature 1 -> Lc, Lu      3  combine, store
// The maxima, the weights and the log-probabilities are those of the scoring form of the sampling launch (ivl_logits.h): integer
// sums, so a row's result is the same bits in any row position, among any neighbours, eager or replayed.  The partner's row may sit
// at another offset inside its tiles than the leader's: pass 3 takes the two partner tiles that cover a leader tile and shifts.
// No atomics; a full tile is one 16-byte store, an element of a head or tail tile a 2-byte store, and an element outside [0, V)
// is never stored.
#include "ivl_common.h"
#include "ivl_logits.h"

namespace ivl {

constexpr int GDE_THREADS = 1024;
constexpr int GDE_WAVES = GDE_THREADS / 64;
constexpr int GDE_ROWS_MAX = 63;               // S of either launch: the rows of a captured step

// bf16 bits of element e of a tile
__device__ __forceinline__ unsigned gde_elem(const unsigned (&w)[4], int e) { return (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }

// mask of the elements of tile j that belong to the row
__device__ __forceinline__ unsigned gde_valid(const SmpRow& r, long long j) {
  const long long i0 = j * 8 - r.off;
  unsigned valid = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const long long i = i0 + e;
    if (i >= 0 && i < r.V) valid |= 1u << e;
  }
  return valid;
}

// the largest key of a row, by every thread of the workgroup (wmax: GDE_WAVES words of LDS); ends on a barrier
__device__ __forceinline__ unsigned gde_row_max(const SmpRow& r, unsigned* wmax, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  unsigned best = 0u;                          // below every key that occurs; V >= 1: some thread finds one
  for (long long j = tid; j < r.nt; j += GDE_THREADS) {
    const u32x4 v = r.base[j];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const unsigned valid = gde_valid(r, j);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned k = smp_key(gde_elem(w, e));
      if ((valid >> e & 1u) && k > best) best = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)best, o, 64); best = t > best ? t : best; }
  if (lane == 0) wmax[wave] = best;
  __syncthreads();
  best = 0u;
#pragma unroll
  for (int w = 0; w < GDE_WAVES; ++w) best = wmax[w] > best ? wmax[w] : best;
  return best;
}

// GUIDE-1: the log-partition of a row whose largest key is mkey, by every thread of the workgroup; ends on a barrier
__device__ __forceinline__ float gde_row_lse(const SmpRow& r, unsigned mkey, u64* wsum, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const float xm = smp_key_value(mkey);
  u64 z = 0ull;
  for (long long j = tid; j < r.nt; j += GDE_THREADS) {
    const u32x4 v = r.base[j];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    const unsigned valid = gde_valid(r, j);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (valid >> e & 1u) z += smp_weight(smp_key(gde_elem(w, e)), mkey, xm, SMP_LOG2E);
  }
  z = smp_wave_sum(z);
  if (lane == 0) wsum[wave] = z;
  __syncthreads();
  u64 Z1 = 0ull;
#pragma unroll
  for (int w = 0; w < GDE_WAVES; ++w) Z1 += wsum[w];
  return smp_lse(Z1);
}

// Elements i0 .. i0 + 7 of row u as four words, i0 the first element of a leader tile (-7 <= i0 < V): the two tiles of u that
// hold them, shifted.  A tile index outside the row is clamped into it; what a clamped tile contributes belongs to elements
// outside [0, V), which the caller masks out -- an element inside the row lies in a tile of the row.
__device__ __forceinline__ int gde_partner_at(const SmpRow& u, long long i0, long long& ja, long long& jb) {
  const long long t = i0 + u.off + 8;          // >= 1
  const long long ju = (t >> 3) - 1, last = u.nt - 1;
  ja = ju < 0 ? 0 : (ju > last ? last : ju);
  jb = ju + 1 > last ? last : ju + 1;
  return (int)(t & 7);                         // element 0 of the result is element sh of tile ju
}
__device__ __forceinline__ void gde_partner_tile(u32x4 a, u32x4 b, int sh, unsigned (&o)[4]) {
  const unsigned W[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const int ws = sh >> 1;
  const bool odd = (sh & 1) != 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned lo = W[k], hi = W[k + 1];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (ws == q) { lo = W[k + q]; hi = W[k + q + 1]; }
    o[k] = odd ? ((lo >> 16) | (hi << 16)) : lo;
  }
}

__global__ __launch_bounds__(GDE_THREADS) void logit_guide_kernel(bf16_t* logits, long long ld, int S, int V, const int* partner,
                                                                  const float* scale, const float* cut, const int* done) {
  __shared__ unsigned wmax[2][GDE_WAVES];
  __shared__ u64 wsum[2][GDE_WAVES];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  // GUIDE-0: of a row that is off, only these table entries are read
  const int p = partner[r];
  if (p < 0 || p >= S || p == r) return;
  if (done && done[r] != 0) return;
  const float s = scale[r];
  if (!(fabsf(s) < __builtin_inff())) return;
  const int pp = partner[p];
  if (pp >= 0 && pp < S && pp != p) return;    // a partner is never a leader
  const float ct = cut[r];

  bf16_t* row = logits + (long long)r * ld;
  const SmpRow c = smp_row(row, V), u = smp_row(logits + (long long)p * ld, V);
  // ---- pass 1: the maxima
  const unsigned mkc = gde_row_max(c, wmax[0], tid), mku = gde_row_max(u, wmax[1], tid);
  const float xmc = smp_key_value(mkc), xmu = smp_key_value(mku);
  // ---- pass 2: the log-partitions
  const float Lc = gde_row_lse(c, mkc, wsum[0], tid), Lu = gde_row_lse(u, mku, wsum[1], tid);
  // ---- pass 3: combine and store.  Every thread reads the tile it writes and nothing else of the leader's row; the partner's
  // row is written by no workgroup (a partner is never a leader)
  const float ninf = -__builtin_inff();
  for (long long j = tid; j < c.nt; j += GDE_THREADS) {
    const u32x4 v = c.base[j];
    const unsigned wc[4] = {v.x, v.y, v.z, v.w};
    const long long i0 = j * 8 - c.off;
    long long ja, jb;
    const int sh = gde_partner_at(u, i0, ja, jb);
    unsigned wu[4];
    gde_partner_tile(u.base[ja], u.base[jb], sh, wu);
    const unsigned valid = gde_valid(c, j);
    unsigned out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned kc = smp_key(gde_elem(wc, e)), ku = smp_key(gde_elem(wu, e));
      const float lc = smp_lp(kc, mkc, xmc, Lc), lu = smp_lp(ku, mku, xmu, Lu);    // GUIDE-2: (x - m) - L
      float y;
      if (kc <= SMP_KEY_NINF || !(lc > ninf)) y = ninf;                            // GUIDE-3: c(v) = -inf (also a row of nothing else)
      else if (kc != mkc && __fsub_rn(smp_key_value(kc), xmc) < ct) y = ninf;      //          the cut; the maximum survives
      else if (ku <= SMP_KEY_NINF || !(lu > ninf)) y = lc;                         //          u(v) = -inf
      else y = __fmaf_rn(s, __fsub_rn(lc, lu), lu);
      out[e] = smp_bf16_rne(y);
    }
    if (valid == 0xFFu) {
      ((u32x4*)c.base)[j] = u32x4{out[0] | (out[1] << 16), out[2] | (out[3] << 16), out[4] | (out[5] << 16), out[6] | (out[7] << 16)};
    } else {                                   // GUIDE-4: a head or tail tile: only the elements of [0, V)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (valid >> e & 1u) row[i0 + e] = (bf16_t)out[e];
    }
  }
}

// One workgroup, thread p = row p: a partner takes the token and the done code of its lowest valid leader.  A leader's row is
// read only: the thread of a row that names a partner returns before it writes.
__global__ __launch_bounds__(64) void rows_follow_kernel(long long* token, long long token_stride, int* done, const int* partner, int S) {
  const int p = threadIdx.x;
  if (p >= S) return;
  const int pp = partner[p];
  if (pp >= 0 && pp < S && pp != p) return;    // a partner is never a leader
  for (int r = 0; r < S; ++r) {
    if (r == p || partner[r] != p) continue;
    token[p * token_stride] = token[r * token_stride];
    if (done) done[p] = done[r];
    return;                                    // the lowest leader wins
  }
}

}  // namespace ivl

extern "C" int ivl_logit_guide_fwd(void* logits, int64_t ld, int S, int V, const int32_t* partner, const float* scale,
                                   const float* cut, const int32_t* done, void* stream) {
  using namespace ivl;
  const char* fn = "ivl_logit_guide_fwd";
  IVL_REQUIRE(logits && partner && scale && cut, IVL_ERR_INVALID_ARG, "%s: NULL logits, partner, scale or cut", fn);
  IVL_REQUIRE(S >= 1 && V >= 1 && ld >= V, IVL_ERR_INVALID_ARG, "%s: S=%d V=%d ld=%lld", fn, S, V, (long long)ld);
  IVL_REQUIRE(V < (1 << 23), IVL_ERR_UNSUPPORTED, "%s: V=%d (below 2^23 only)", fn, V);
  IVL_REQUIRE(S <= GDE_ROWS_MAX, IVL_ERR_UNSUPPORTED, "%s: S=%d (at most %d rows)", fn, S, GDE_ROWS_MAX);
  hipLaunchKernelGGL(logit_guide_kernel, dim3((unsigned)S), dim3(GDE_THREADS), 0, (hipStream_t)stream, (bf16_t*)logits,
                     (long long)ld, S, V, partner, scale, cut, done);
  return check_launch(fn);
}

extern "C" int ivl_rows_follow_fwd(int64_t* token, int64_t token_stride, int32_t* done, const int32_t* partner, int S, void* stream) {
  using namespace ivl;
  const char* fn = "ivl_rows_follow_fwd";
  IVL_REQUIRE(token && partner, IVL_ERR_INVALID_ARG, "%s: NULL token or partner", fn);
  IVL_REQUIRE(S >= 1 && token_stride >= 1, IVL_ERR_INVALID_ARG, "%s: S=%d token_stride=%lld", fn, S, (long long)token_stride);
  IVL_REQUIRE(S <= GDE_ROWS_MAX, IVL_ERR_UNSUPPORTED, "%s: S=%d (at most %d rows)", fn, S, GDE_ROWS_MAX);
  hipLaunchKernelGGL(rows_follow_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)token, (long long)token_stride, done,
                     partner, S);
  return check_launch(fn);
}

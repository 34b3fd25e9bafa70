// Token sampling over the lm_head logits of a decode step: temperature, top-k and top-p per row, one launch, one workgroup per
// row (a row = a batch row of GraphedDecode or a slot of GraphedMultiStreamDecode).  Serves the generation arguments the
// reference hands to HF generate (src/llamafactory/api/chat.py:160-162, api/protocol.py:99-101, webui/runner.py:231-232,
// webui/components/chatbot.py:78-79); the semantics are written out at ivl_sample_rows_fwd in include/ivl_hip.h.
//
// No sort: bf16 has 65,536 values, so the top-k and the top-p thresholds come EXACTLY from histograms of an order-preserving
// 16-bit key -- a coarse level over the high 12 bits (4096 bins in LDS: real logits sit in a few binades, 8 bins each), then the 16
// keys of the one boundary bin.  No float sums: a weight is the integer q = floor(2^(( x - m) log2e / tau) 2^40) (Q40; a token more
// than 40 ln 2 = 27.7 nats below the maximum has weight 0), every histogram, sum and prefix is an integer add, so the token is the
// same bits whatever the order the waves arrive in, eager or replayed, alone or beside other rows.  Z <= V 2^40: below 2^58 at the
// model's V = 151936; the host refuses V >= 2^23, so every sum stays below 2^63.
//
// Passes over the row (304 KB at V = 151936, written by lm_head just before: L2 hits), only those the row's parameters need:
//   1  maximum and its lowest index (+ coarse counts if top-k)      greedy rows end here
//   2  top-k: counts of the 16 keys of the bin that holds the k-th largest value                -> t_k
//   3  top-p: coarse masses of the keys >= t_k                                                  -> Z_K, boundary bin
//   4  top-p: counts of the 16 keys of that bin (mass = count x weight)                         -> t_p
//   5  kept count and mass per wave (a wave owns a contiguous index range)                      -> |P|, Z_P, target = hi64(u64 Z_P)
//   6  the one wave whose range holds the target scans it again and walks the tile that holds it -> token
// Rows are read in 16-byte tiles from the 16-byte boundary at or below the row start, whatever `ld` and the base: the (at most 7)
// elements in front of and behind the row inside its first and last tile are masked out -- they lie in the same 16 bytes as row
// elements, so the loads stay inside the caller's allocation granule.
//
// Generation controls (the kernel is a template on them; the entry point launches the form without when none is given): a
// finished row returns its fill token before the first pass; the repetition penalty re-keys the seen elements of a
// tile where it is loaded (a bitmap of seen tokens, 8 bits a tile from two bytes), rounded back to bf16, so every pass sees the same
// penalised keys and nothing behind the key changes; the lane that writes the token then sets its bit, logs it, counts it and
// decides `done` from the stop ids and the budget.  ivl_token_mark_fwd marks a prompt's tokens in a row of the bitmap.
//
// Log-probabilities (a third form of the template, the two others are compiled without a line of it): the
// row's log-partition from the integer sum Z1 of the Q40 weights at temperature 1 and the n_top <= 20 largest keys, in three more
// passes placed where `hist` is free -- behind top-k's scan, in front of top-p's masses, or in front of a greedy row's write:
//   L1  Z1 and the coarse counts (a top-k row has them from pass 1)     L2  counts of the 16 keys of the bin that holds the n_top-th largest value -> t_N
//       (skipped where that bin and the bins above it hold at most 20 keys: they are all collected)
//   L3  collect: every key > t_N (fewer than n_top), and per wave (a wave owns a contiguous index range) its first ties == t_N
// then wave 0 takes the ties in wave = index order, ranks the <= 20 survivors against each other (no sort of the row) and leaves
// the ordered list in LDS for the lane that writes the token: it scores the token, logs and adds it up beside smp_after.
//
// Score only (score_only != 0; a fourth form, the three others are compiled without a line of it): a beam search step
// needs every beam's candidate list and no token.  The form takes the greedy row's path -- pass 1 for the maximum, L1-L3 -- writes
// the list and stops: no token, counter, seen bit, n_new, done, history or ring; its sampling parameters are not even read.
//
// Constrained (fsm_state != NULL; a fifth form, the four others are compiled without a line of it): a row in state q >= 0 of
// a token-level finite state machine IS its allowed sub-vocabulary.  The allowed-token bitmap of q has the layout of `seen` and
// comes through the same helper, and it is ANDed into the `valid` mask of smp_load: a disallowed token is absent from every pass,
// exactly as the elements in front of and behind the row are.  Pass 1 counts |A| beside the maximum (it takes V's place in top-k's
// switch and in the length of the top-N list); the lane that writes the token then advances the state by three dependent loads.
//
// Adjusted (ivl_sample_rows_adj_fwd with a group that is on; twins of the controlled, scoring and constrained forms, which are
// compiled without a line of it): frequency / presence penalties over a row of counts of the generated tokens and a logit-bias
// table per row, added where smp_load has re-keyed the tile and rounded back to bf16 -- nothing behind the key changes -- and
// min-p as one more predicate on the Q40 weight where passes 5 and 6 evaluate it.  The lane that writes the token counts it.
#include "ivl_common.h"
#include "ivl_logits.h"

#include <type_traits>

namespace ivl {

// (the key, the Q40 weight, the log-partition, the bf16 rounding, the wave sum and the tile view of a row: ivl_logits.h,
// shared with the guidance launch of guide.hip)
constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_BINS = 4096;                 // coarse level: key >> 4
constexpr int SMP_SUB = 16;                    // keys per coarse bin

// The repetition penalty of the controlled form: the row's bitmap of seen tokens as bytes (bit i & 7 of byte i >> 3 = bit i & 31 of
// word i >> 5) and the row's r; bits == NULL when r == 1 (uniform per workgroup: nothing is fetched then).  SmpNoPen: the
// control-free form, whose smp_load is the one it always had.
struct SmpNoPen {};
struct SmpPen {
  const unsigned char* bits;
  float r;
  float inv;             // RN(1 / r)
  bool fast;             // 2^-20 <= r < 2^21: smp_penalise_fast serves the logits of ordinary size
};

// bf16 bits of a seen logit -> bf16_rne(x < 0 ? x * r : x / r) in fp32 (a true division, one rounding); NaN stays NaN
__device__ __forceinline__ unsigned smp_penalise(unsigned b, float r) {
  const float x = __uint_as_float(b << 16);
  const float y = x < 0.f ? x * r : __fdiv_rn(x, r);
  unsigned u = __float_as_uint(y);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}
// The same value without a division or a branch, for a logit of ordinary size (2^-30 <= |x| < 2^31, checked by the caller) and
// 2^-20 <= r < 2^21: with y = RN(1 / r), q = RN(x y) is within an ulp of x / r, e = x - q r is exact in one fma, and
// RN(q + e y) = RN(x / r) (Markstein's theorem; the ranges keep q, e and every product away from overflow and underflow).  The
// passes are bound by their vector instructions, and a division costs about as many as the rest of an element's work.
__device__ __forceinline__ unsigned smp_penalise_fast(unsigned b, float r, float inv) {
  const float x = __uint_as_float(b << 16);
  const float q = __fmul_rn(x, inv);
  const float e = __fmaf_rn(-q, r, x);
  const float y = x < 0.f ? __fmul_rn(x, r) : __fmaf_rn(e, inv, q);
  unsigned u = __float_as_uint(y);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

// the seen bits of the 8 elements of tile j (bit e = element e).  The tile starts `off` elements before a byte boundary of the
// bitmap, so they come from bytes j - 1 and j.  Both indices are clamped into the ceil(V/8) bytes that hold a bit below V (no
// branch: the two loads leave with the tile's own); what a clamped byte contributes belongs to elements outside the row, which
// the caller masks out.
__device__ __forceinline__ unsigned smp_seen_bits(const SmpRow& r, const unsigned char* bits, long long j) {
  const long long last = ((long long)r.V - 1) >> 3;
  const unsigned lo = bits[j > 0 ? j - 1 : 0];
  const unsigned hi = bits[j < last ? j : last];
  return ((lo >> (8 - r.off)) | (hi << r.off)) & 0xFFu;
}

// keys of tile j; returns the mask of the elements that belong to the row
__device__ __forceinline__ unsigned smp_load(const SmpRow& r, const SmpNoPen&, long long j, unsigned (&key)[8]) {
  const u32x4 v = r.base[j];
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  const long long i0 = j * 8 - r.off;
  unsigned valid = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    key[e] = smp_key((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu);
    const long long i = i0 + e;
    if (i >= 0 && i < r.V) valid |= 1u << e;
  }
  return valid;
}
// the same with the seen elements re-keyed to their penalised value: every pass sees the same keys
__device__ __forceinline__ unsigned smp_load(const SmpRow& r, const SmpPen& pen, long long j, unsigned (&key)[8]) {
  const u32x4 v = r.base[j];
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
  const long long i0 = j * 8 - r.off;
  unsigned valid = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const long long i = i0 + e;
    if (i >= 0 && i < r.V) valid |= 1u << e;
  }
  if (pen.bits) {                                // uniform per workgroup
    const unsigned seen = smp_seen_bits(r, pen.bits, j) & valid;
    unsigned odd = pen.fast ? 0u : seen;         // seen elements outside the fast form's range: zeros, infinities, NaN, tiny, huge
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned b = (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
      const unsigned pb = smp_penalise_fast(b, pen.r, pen.inv);
      if (((b & 0x7F80u) - (97u << 7)) > (60u << 7)) odd |= seen & (1u << e);
      key[e] = (seen >> e & 1u) ? pb : b;
    }
    if (__any(odd != 0u)) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (odd >> e & 1u) key[e] = smp_penalise((w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu, pen.r);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) key[e] = (w[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) key[e] = smp_key(key[e]);
  return valid;
}

// The constrained form: the penalty's view plus the allowed-token bitmap of the row's state, bytes in the layout of `bits`
// (allow == NULL for a free row, uniform per workgroup).  A disallowed element leaves the mask: no pass ever looks at its key.
struct SmpPenFsm : SmpPen {
  const unsigned char* allow;
};
__device__ __forceinline__ unsigned smp_load(const SmpRow& r, const SmpPenFsm& pen, long long j, unsigned (&key)[8]) {
  unsigned valid = smp_load(r, static_cast<const SmpPen&>(pen), j, key);
  if (pen.allow) valid &= smp_seen_bits(r, pen.allow, j);
  return valid;
}

// The adjusted forms (ADJ-1 of include/ivl_hip.h): the constrained form's view, then the additive adjustments of the row -- the
// frequency / presence penalty on the seen elements that have been generated (count > 0) and the row's logit-bias table -- in
// plain fp32, each operation rounded once, and one rounding back to bf16.  cbits: the row's seen bitmap, NULL when (f, p) ==
// (0, 0); bbits / bval: the row's bias bitmap and values, NULL without a table (all uniform per workgroup: nothing is fetched
// then).  A count word is read only under a set seen bit, a bias value only under a set bias bit, both only inside the row.
// The arithmetic starts from the VALUE of the key: a NaN arrives as -inf and -0 as +0, and every result they can reach lies in
// the same key class as the one reached from the bits themselves (anything with a NaN is a NaN = -inf; -inf plus or minus
// anything is -inf or a NaN; a zero of either sign plus t is t, or a zero).  An untouched element keeps its key.  A penalised
// element whose penalty sums to zero (f c + p == 0) IS touched and re-keyed from its value: it keeps its key class, not its
// bits (-0 comes out as +0, the same key), which is all that the passes can see.
struct SmpPenAdj : SmpPenFsm {
  const unsigned char* cbits;
  const int* cnt;
  float f, p;
  const unsigned char* bbits;
  const float* bval;
};
__device__ __forceinline__ unsigned smp_load(const SmpRow& r, const SmpPenAdj& pen, long long j, unsigned (&key)[8]) {
  const unsigned valid = smp_load(r, static_cast<const SmpPenFsm&>(pen), j, key);
  if (pen.cbits || pen.bbits) {                  // uniform per workgroup
    const unsigned pm = pen.cbits ? smp_seen_bits(r, pen.cbits, j) & valid : 0u;
    const unsigned bm = pen.bbits ? smp_seen_bits(r, pen.bbits, j) & valid : 0u;
    if ((pm | bm) != 0u) {
      // The tile's loads leave together, one wait for all: an element without a bit reads the word of the tile's LOWEST set
      // bit in its place (a word the row may read, the same line) -- a load under a branch per element would wait for each
      // of them in turn, in every pass (measured: the sampled operator at V = 151936, 4 rows, 481 us that way).
      const long long i0 = j * 8 - r.off;
      int c[8] = {};
      float bv[8] = {};
      if (pm != 0u) {
        const int lo = __ffs((int)pm) - 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) c[e] = pen.cnt[i0 + ((pm >> e & 1u) ? e : lo)];
      }
      if (bm != 0u) {
        const int lo = __ffs((int)bm) - 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = pen.bval[i0 + ((bm >> e & 1u) ? e : lo)];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool pe = (pm >> e & 1u) && c[e] > 0, be = (bm >> e & 1u) != 0u;
        if (pe || be) {
          float t = smp_key_value(key[e]);
          if (pe) t = __fsub_rn(t, __fadd_rn(__fmul_rn(pen.f, (float)c[e]), pen.p));
          if (be) t = __fadd_rn(t, bv[e]);
          key[e] = smp_key(smp_bf16_rne(t));
        }
      }
    }
  }
  return valid;
}

__device__ __forceinline__ u64 smp_wave_incl_scan(u64 v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// hist[bin[e]] += val[e] for the elements of `mask`, called by every lane of a wave.  A wave whose elements all fall into one
// bin (a row of equal logits, a masked vocabulary range) adds once per wave, a thread whose elements do once per thread: all the
// row's atomics on one LDS word would otherwise run one after the other.
__device__ __forceinline__ void smp_hist_add(u64* hist, const unsigned (&bin)[8], const u64 (&val)[8], unsigned mask, int lane) {
  unsigned tb = 0xFFFFFFFFu;
  u64 tsum = 0ull;
  bool same = true;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (mask >> e & 1u) {
      if (tb == 0xFFFFFFFFu) tb = bin[e];
      if (bin[e] == tb) tsum += val[e]; else same = false;
    }
  const u64 have = __ballot(mask != 0u);
  if (have == 0ull) return;
  const unsigned wb = (unsigned)__shfl((int)tb, __ffsll((long long)have) - 1, 64);
  if (__all(mask == 0u || (same && tb == wb))) {
    const u64 s = smp_wave_sum(tsum);
    if (lane == 0 && s != 0ull) atomicAdd(&hist[wb], s);
  } else if (mask != 0u) {
    if (same) {
      if (tsum != 0ull) atomicAdd(&hist[tb], tsum);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((mask >> e & 1u) && val[e] != 0ull) atomicAdd(&hist[bin[e]], val[e]);
    }
  }
}

// Walk of the coarse bins from the top: thread t owns bins 4095-4t .. 4092-4t.  E_b = the sum of the bins above b.  Returns the
// total; `locate` then finds the lowest bin with E_b < T (the bin where the running sum crosses T) and leaves (bin, E_bin) in sh[].
struct SmpScan { u64 c[4]; u64 excl; u64 total; };
__device__ __forceinline__ void smp_scan(const u64* hist, u64* wsum, int tid, SmpScan& s) {
  const int lane = tid & 63, wave = tid >> 6;
  u64 local = 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) { s.c[i] = hist[SMP_BINS - 1 - 4 * tid - i]; local += s.c[i]; }
  const u64 incl = smp_wave_incl_scan(local, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  u64 woff = 0ull, total = 0ull;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) { const u64 x = wsum[w]; if (w < wave) woff += x; total += x; }
  s.excl = woff + incl - local;
  s.total = total;
}
__device__ __forceinline__ void smp_locate(const SmpScan& s, u64 T, int tid, unsigned* sh_bin, u64* sh_E) {
  u64 E = s.excl;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (E < T && E + s.c[i] >= T) { *sh_bin = (unsigned)(SMP_BINS - 1 - 4 * tid - i); *sh_E = E; }
    E += s.c[i];
  }
}

// The control group of ivl_sample_args; every group may be NULL (off)
struct SmpCtl {
  const float* rep_penalty;
  unsigned* seen;
  long long seen_ld;
  const long long* stop_ids;
  int n_stop;
  const long long* budget;
  const long long* fill;
  long long* n_new;
  int* done;
  long long* history;
  long long hist_ld;
};

// Bookkeeping of row s after its draw, by the one lane that wrote the token (no other thread touches the row's state: every
// read of `seen` by the passes lies before the barrier or the wave-wide shuffle in front of the token write)
__device__ __forceinline__ void smp_after(const SmpCtl& c, long long s, long long tok) {
  if (c.seen) {
    unsigned* w = c.seen + s * c.seen_ld + (tok >> 5);
    *w = *w | (1u << (tok & 31));
  }
  long long n = 0;
  if (c.n_new) {
    n = c.n_new[s];
    if (c.history) c.history[s * c.hist_ld + n % c.hist_ld] = tok;
    c.n_new[s] = ++n;
  }
  if (c.done) {
    int d = 0;
    for (int i = 0; i < c.n_stop; ++i) {
      const long long id = c.stop_ids[s * c.n_stop + i];
      if (id >= 0 && id == tok) d = 1;
    }
    if (d == 0 && c.budget) {
      const long long b = c.budget[s];
      if (b >= 0 && n >= b) d = 2;
    }
    if (d != 0) c.done[s] = d;
  }
}

// The score group of ivl_sample_args; every pointer may be NULL (off)
constexpr int SMP_TOP_MAX = 20;
struct SmpLp {
  float* logprob;
  int n_top;
  long long* top_ids;
  float* top_lp;
  double* cum;
  float* lp_hist;
  long long* top_hist_ids;
  float* top_hist_lp;
};
struct SmpLpLds {
  u64 cand[SMP_TOP_MAX];                   // the survivors in output order, as (key + 1) << 32 | ~index
  u64 gt[SMP_TOP_MAX];                     // keys above t_N, in the order the waves met them
  unsigned tie[SMP_WAVES][SMP_TOP_MAX];    // per wave: the lowest indices of its keys == t_N
  unsigned ntie[SMP_WAVES];
  unsigned ngt;
};
struct SmpNoLds {};

// Passes L1-L3, by every thread of the workgroup, while `hist`, `sub`, `wsum` and the sh_ words are free; returns lse and leaves
// the min(n_top, nrow) survivors in L.cand (nrow: the tokens of the row, V or a constrained row's |A|).  Ends on a barrier.
// counted: hist already holds the row's coarse counts (pass 1 made them for top-k, whose scan only read them).
template <typename PEN>
__device__ __forceinline__ float smp_lp_phase(const SmpRow& r, const PEN& pen, int nrow, unsigned mkey, float xm, int n_top, bool counted, int tid,
                                              u64* hist, u64* sub, u64* wsum, unsigned* sh_bin, u64* sh_E, unsigned* sh_key,
                                              SmpLpLds& L) {
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned nsel = (unsigned)(n_top < nrow ? n_top : nrow);
  const bool count = nsel > 0u && !counted;
  if (nsel > 0u) {
    if (count) {
#pragma unroll
      for (int i = 0; i < SMP_BINS / SMP_THREADS; ++i) hist[tid + i * SMP_THREADS] = 0ull;
    }
    if (tid < SMP_WAVES) L.ntie[tid] = 0u;
    if (tid == 0) L.ngt = 0u;
  }
  __syncthreads();
  // ---- L1: Z1 = the sum of the Q40 weights at temperature 1; coarse counts
  u64 z = 0ull;
  for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
    const long long j = j0 + lane;
    unsigned key[8] = {}, valid = 0u;
    if (j < r.nt) valid = smp_load(r, pen, j, key);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (valid >> e & 1u) z += smp_weight(key[e], mkey, xm, 1.44269504088896341f);
    if (count) {
      unsigned bin[8];
      u64 val[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bin[e] = key[e] >> 4; val[e] = 1ull; }
      smp_hist_add(hist, bin, val, valid, lane);
    }
  }
  z = smp_wave_sum(z);
  if (lane == 0) wsum[wave] = z;
  __syncthreads();
  u64 Z1 = 0ull;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) Z1 += wsum[w];
  const float lse = smp_lse(Z1);
  if (nsel == 0u) { __syncthreads(); return lse; }
  __syncthreads();                                     // wsum has been read by every thread
  // ---- the bin where the count from the top reaches nsel, then L2: the key inside it
  SmpScan sc;
  smp_scan(hist, wsum, tid, sc);
  smp_locate(sc, (u64)nsel, tid, sh_bin, sh_E);
  if (tid < SMP_SUB) sub[tid] = 0ull;
  __syncthreads();
  const unsigned B = *sh_bin;
  // The boundary bin and the bins above it hold `upto` >= nsel keys.  If they all fit the list (the usual case: the head of a
  // row of logits is sparse), L2 is skipped: every key of these bins is collected and the ranking keeps the first nsel.
  const u64 upto = *sh_E + hist[B];
  const bool whole = upto <= (u64)SMP_TOP_MAX;         // uniform over the workgroup
  unsigned tN, need;
  if (whole) {
    tN = B * SMP_SUB - 1u;                             // B >= 7 (the bin of -inf): every key of bin B is above it
    need = 0u;
  } else {
    for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
      const long long j = j0 + lane;
      unsigned key[8] = {}, valid = 0u;
      if (j < r.nt) valid = smp_load(r, pen, j, key);
      unsigned bin[8], m = 0u;
      u64 val[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bin[e] = key[e] & 15u; val[e] = 1ull; if ((key[e] >> 4) == B) m |= 1u << e; }
      if (__any((valid & m) != 0u)) smp_hist_add(sub, bin, val, valid & m, lane);
    }
    __syncthreads();
    if (tid == 0) {
      u64 E = *sh_E, above = 0ull;
      unsigned res = mkey;
      for (int i = SMP_SUB - 1; i >= 0; --i) {
        if (E < (u64)nsel) { res = B * SMP_SUB + i; above = E; }
        E += sub[i];
      }
      *sh_key = res;
      *sh_E = above;                                   // keys above t_N: fewer than nsel
    }
    __syncthreads();
    tN = *sh_key;
    need = nsel - (unsigned)*sh_E;                     // ties at t_N to take, lowest indices first: 1 .. nsel
  }
  // ---- L3: collect; wave w owns the tiles [w tpw, (w+1) tpw), its lanes interleaved: lane order = index order
  const long long tpw = (r.nt + SMP_WAVES - 1) / SMP_WAVES;
  const long long jbeg = wave * tpw, jend = (jbeg + tpw < r.nt) ? jbeg + tpw : r.nt;
  unsigned mytie = 0u;                                 // ties of this wave so far (uniform over the wave)
  for (long long j0 = jbeg; j0 < jend; j0 += 64) {
    const long long j = j0 + lane;
    unsigned key[8] = {}, valid = 0u;
    if (j < jend) valid = smp_load(r, pen, j, key);
    unsigned gm = 0u, tm = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (key[e] > tN) gm |= 1u << e;
      if (key[e] == tN) tm |= 1u << e;
    }
    gm &= valid;
    tm &= valid;
    if (gm != 0u) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (gm >> e & 1u) {
          const unsigned at = atomicAdd(&L.ngt, 1u);
          if (at < (unsigned)SMP_TOP_MAX) L.gt[at] = ((u64)(key[e] + 1u) << 32) | (u64)(0xFFFFFFFFu - (unsigned)(j * 8 - r.off + e));
        }
    }
    if (mytie < need && __any(tm != 0u)) {
      const unsigned c = (unsigned)__popc(tm);
      const unsigned incl = (unsigned)smp_wave_incl_scan((u64)c, lane);
      unsigned pos = mytie + incl - c;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (tm >> e & 1u) {
          if (pos < need) L.tie[wave][pos] = (unsigned)(j * 8 - r.off + e);
          ++pos;
        }
      mytie += (unsigned)__shfl((int)incl, 63, 64);
    }
  }
  if (lane == 0) L.ntie[wave] = mytie < need ? mytie : need;
  __syncthreads();
  // ---- wave 0: lane i holds candidate i, its rank = the candidates in front of it by (key descending, index ascending)
  if (wave == 0) {
    const unsigned ngt = L.ngt;                        // the keys above t_N; with `need` ties: the candidates
    const unsigned ncand = ngt + need;
    u64 mine = 0ull;
    if ((unsigned)lane < ngt) {
      mine = L.gt[lane];
    } else if ((unsigned)lane < ncand) {
      unsigned t = (unsigned)lane - ngt;
      bool found = false;
#pragma unroll
      for (int w = 0; w < SMP_WAVES; ++w) {
        const unsigned n = L.ntie[w];
        if (!found) {
          if (t < n) { mine = ((u64)(tN + 1u) << 32) | (u64)(0xFFFFFFFFu - L.tie[w][t]); found = true; }
          else t -= n;
        }
      }
    }
    unsigned rank = 0u;
    for (unsigned i = 0u; i < ncand; ++i) {
      const u64 other = __shfl(mine, (int)i, 64);
      if (other > mine) ++rank;
    }
    if ((unsigned)lane < ncand) L.cand[rank] = mine;
  }
  __syncthreads();
  return lse;
}

// Scores of row s, by the lane that writes the token, in front of smp_after (the ring index is n_new before its increment)
__device__ __forceinline__ void smp_lp_after(const SmpLp& lp, const SmpCtl& c, long long s, int V, unsigned tkey, unsigned mkey,
                                             float xm, float lse, const SmpLpLds& L) {
  const float v = smp_lp(tkey, mkey, xm, lse);
  if (lp.logprob) lp.logprob[s] = v;
  long long at = 0;
  if (lp.lp_hist || lp.top_hist_ids || lp.top_hist_lp) at = s * c.hist_ld + c.n_new[s] % c.hist_ld;
  if (lp.lp_hist) lp.lp_hist[at] = v;
  for (int j = 0; j < lp.n_top; ++j) {
    long long id = -1ll;
    float l = -__builtin_inff();
    if (j < V) {
      const u64 w = L.cand[j];
      id = (long long)(0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFull));
      l = smp_lp((unsigned)(w >> 32) - 1u, mkey, xm, lse);
    }
    lp.top_ids[s * lp.n_top + j] = id;
    lp.top_lp[s * lp.n_top + j] = l;
    if (lp.top_hist_ids) lp.top_hist_ids[at * lp.n_top + j] = id;
    if (lp.top_hist_lp) lp.top_hist_lp[at * lp.n_top + j] = l;
  }
  if (lp.cum) lp.cum[s] += (double)v;
}

// The constraint group of ivl_sample_args
struct SmpFsm {
  int* state;
  const unsigned* mask;
  long long mask_ld;
  int n_states;
  const long long* desc;
  const int* cls;
  const int* trans;
};

// The adjustment group of ivl_sample_adj_args; every pointer may be NULL (off)
struct SmpAdj {
  const float* min_p;
  const float* freq;
  const float* pres;
  int* count;
  long long count_ld;
  const int* bias_idx;
  const unsigned* bias_mask;
  long long bias_mask_ld;
  const float* bias_val;
  long long bias_ld;
  int n_bias;
};

// ADJ-4, by the one lane that wrote the token, beside smp_after (the passes' reads of the row's counts lie in front of it, as
// their reads of `seen` do)
__device__ __forceinline__ void smp_adj_after(const SmpAdj& a, long long s, long long tok) {
  if (a.count) a.count[s * a.count_ld + tok] += 1;
}

// A dead end in front of the draw (F5: no such state, or a state that allows nothing), by every thread of the workgroup: step
// A's outputs and done = 3; the counter, seen, n_new, the history, the scores' sums and rings and the state stay as they are
__device__ __forceinline__ void smp_fsm_dead(const SmpCtl& c, const SmpLp& lp, long long s, long long* token, long long token_stride,
                                             int* n_kept, float* prob) {
  if (threadIdx.x == 0) {
    token[s * token_stride] = c.fill ? c.fill[s] : 0ll;
    if (n_kept) n_kept[s] = 0;
    if (prob) prob[s] = 0.f;
    if (lp.logprob) lp.logprob[s] = 0.f;
    c.done[s] = 3;
  }
  if ((int)threadIdx.x < lp.n_top) {
    lp.top_ids[s * lp.n_top + threadIdx.x] = -1ll;
    lp.top_lp[s * lp.n_top + threadIdx.x] = -__builtin_inff();
  }
}

// F4, by the one lane that wrote the token, behind smp_after: the state advances by the token's class; no transition (-2) is
// a dead end behind the draw: the token stands, the state stays, done = 3
__device__ __forceinline__ void smp_fsm_after(const SmpFsm& f, const SmpCtl& c, long long s, int q, long long tok) {
  if (q < 0) return;
  const long long trans_off = f.desc[2 * q], cls_off = f.desc[2 * q + 1];
  const int next = f.trans[trans_off + f.cls[cls_off + tok]];
  if (next < -1) c.done[s] = 3; else f.state[s] = next;
}

// CTL: no type (the control-free form, with the parameter list it always had), SmpCtl, SmpCtl and SmpLp, or these two and
// SmpScore (the score-only form: steps A, B, L1 and L3, nothing committed) or SmpFsm (the constrained form); SmpAdj behind
// SmpCtl, SmpCtl and SmpLp, or these two and SmpFsm: the adjusted twin of that form
struct SmpScore {};
template <typename T, typename... U> constexpr bool smp_has = (std::is_same<T, U>::value || ...);
// the group of type T among the kernel's trailing parameters
template <typename T, typename H, typename... R>
__device__ __forceinline__ const T& smp_get(const H& h, const R&... r) {
  if constexpr (std::is_same<T, H>::value) return h; else return smp_get<T>(r...);
}

template <typename... CTL>
__global__ void __launch_bounds__(SMP_THREADS)
sample_rows_kernel(const bf16_t* __restrict__ logits, long long ld, int V, const float* __restrict__ temperature,
                   const int* __restrict__ top_k, const float* __restrict__ top_p, const long long* __restrict__ seed,
                   long long* __restrict__ counter, long long* __restrict__ token, long long token_stride,
                   int* __restrict__ n_kept, float* __restrict__ prob, const CTL... ctl_) {
  constexpr bool kCtl = smp_has<SmpCtl, CTL...>, kLp = smp_has<SmpLp, CTL...>, kScore = smp_has<SmpScore, CTL...>;
  constexpr bool kFsm = smp_has<SmpFsm, CTL...>, kAdj = smp_has<SmpAdj, CTL...>;
  typename std::conditional<kAdj, SmpPenAdj, typename std::conditional<kFsm, SmpPenFsm,
      typename std::conditional<kCtl, SmpPen, SmpNoPen>::type>::type>::type pen;
  [[maybe_unused]] int fsm_q = -1;                      // the row's state, read once: the lane that advances it writes last
  [[maybe_unused]] bool lp_on = true;                   // (the constrained form is launched with the score group off, too)
  if constexpr (kCtl) {
    const SmpCtl& ctl = smp_get<SmpCtl>(ctl_...);
    const long long s = blockIdx.x;
    if (ctl.done && ctl.done[s] != 0) {                 // a finished row: the fill token, nothing else read or written
      if constexpr (!kScore) {
        if (threadIdx.x == 0) {
          token[s * token_stride] = ctl.fill ? ctl.fill[s] : 0ll;
          if (n_kept) n_kept[s] = 0;
          if (prob) prob[s] = 0.f;
        }
      }
      if constexpr (kLp) {                              // no score: logprob 0, no alternatives, no ring or sum write
        const SmpLp& lp = smp_get<SmpLp>(ctl_...);
        if (threadIdx.x == 0 && lp.logprob) lp.logprob[s] = 0.f;
        if ((int)threadIdx.x < lp.n_top) {
          lp.top_ids[s * lp.n_top + threadIdx.x] = -1ll;
          lp.top_lp[s * lp.n_top + threadIdx.x] = -__builtin_inff();
        }
      }
      return;
    }
    pen.r = ctl.rep_penalty ? ctl.rep_penalty[s] : 1.f;
    pen.bits = pen.r != 1.f ? (const unsigned char*)(ctl.seen + s * ctl.seen_ld) : nullptr;
    pen.inv = __fdiv_rn(1.f, pen.r);
    pen.fast = ((__float_as_uint(pen.r) >> 23) & 0x1FFu) - 107u <= 40u;      // positive, exponent -20 .. 20
    if constexpr (kFsm) {
      const SmpFsm& f = smp_get<SmpFsm>(ctl_...);
      const SmpLp& lp = smp_get<SmpLp>(ctl_...);
      lp_on = lp.logprob || lp.n_top > 0 || lp.cum || lp.lp_hist;
      fsm_q = f.state[s];
      if (fsm_q >= f.n_states) {                        // no such state: a dead end, before a word of the tables is read
        smp_fsm_dead(ctl, lp, s, token, token_stride, n_kept, prob);
        return;
      }
      pen.allow = fsm_q >= 0 ? (const unsigned char*)(f.mask + (long long)fsm_q * f.mask_ld) : nullptr;
    }
    if constexpr (kAdj) {
      const SmpAdj& a = smp_get<SmpAdj>(ctl_...);
      if constexpr (!kFsm) pen.allow = nullptr;
      pen.f = a.freq ? a.freq[s] : 0.f;
      pen.p = a.pres ? a.pres[s] : 0.f;
      pen.cnt = a.count ? a.count + s * a.count_ld : nullptr;
      pen.cbits = pen.cnt && (pen.f != 0.f || pen.p != 0.f) ? (const unsigned char*)(ctl.seen + s * ctl.seen_ld) : nullptr;
      const int b = a.bias_idx ? a.bias_idx[s] : -1;
      const bool biased = b >= 0 && b < a.n_bias;
      pen.bbits = biased ? (const unsigned char*)(a.bias_mask + (long long)b * a.bias_mask_ld) : nullptr;
      pen.bval = biased ? a.bias_val + (long long)b * a.bias_ld : nullptr;
    }
  }
  __shared__ u64 hist[SMP_BINS];
  __shared__ u64 sub[SMP_SUB];
  __shared__ u64 wsum[SMP_WAVES];
  __shared__ u64 wbest[SMP_WAVES];
  __shared__ unsigned wcnt[SMP_WAVES];
  __shared__ unsigned sh_bin;
  __shared__ u64 sh_E;
  __shared__ unsigned sh_key;
  __shared__ typename std::conditional<kLp, SmpLpLds, SmpNoLds>::type lpl;
  [[maybe_unused]] float lse = 0.f;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long s = blockIdx.x;
  const bf16_t* row = logits + s * ld;
  const SmpRow r = smp_row(row, V);

  float tau = 0.f, p = 1.f;                             // the score-only form has no sampling parameters: it takes the greedy
  int k = 0;                                            // row's path to the scores and writes no token
  if constexpr (!kScore) { tau = temperature[s]; k = top_k[s]; p = top_p[s]; }
  const bool greedy = !(tau > 0.f);
  const bool count_k = !greedy && k > 0 && k < V;      // pass 1 counts for top-k (a constrained row may still turn it off: k >= |A|)
  const bool use_p = !greedy && p < 1.f;

  if (count_k) {
#pragma unroll
    for (int i = 0; i < SMP_BINS / SMP_THREADS; ++i) hist[tid + i * SMP_THREADS] = 0ull;
    __syncthreads();
  }

  // ---- pass 1: the maximum and its lowest index; coarse counts for top-k
  unsigned bkey = 0u, bidx = 0u;
  bool got = false;
  [[maybe_unused]] unsigned na = 0u;                    // the constrained form: this thread's share of |A|
  for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
    const long long j = j0 + lane;
    unsigned key[8] = {}, valid = 0u;
    if (j < r.nt) valid = smp_load(r, pen, j, key);
    if constexpr (kFsm) na += (unsigned)__popc(valid);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if ((valid >> e & 1u) && (!got || key[e] > bkey)) { bkey = key[e]; bidx = (unsigned)(j * 8 - r.off + e); got = true; }
    if (count_k) {
      unsigned bin[8];
      u64 val[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bin[e] = key[e] >> 4; val[e] = 1ull; }
      smp_hist_add(hist, bin, val, valid, lane);
    }
  }
  // (key, lowest index) as one ordered word: the larger key wins, then the smaller index
  u64 best = got ? ((u64)(bkey + 1u) << 32) | (u64)(0xFFFFFFFFu - bidx) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(best, o, 64); best = t > best ? t : best; }
  if (lane == 0) wbest[wave] = best;
  if constexpr (kFsm) {
    na = (unsigned)smp_wave_sum((u64)na);
    if (lane == 0) wcnt[wave] = na;                     // (pass 5 writes wcnt again, behind barriers)
  }
  __syncthreads();
  best = 0ull;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) best = wbest[w] > best ? wbest[w] : best;
  const unsigned mkey = (unsigned)(best >> 32) - 1u;
  const unsigned midx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
  int nrow = V;                                         // the tokens of the row: V, or |A| of a constrained row
  if constexpr (kFsm) {
    nrow = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) nrow += (int)wcnt[w];
    if (nrow == 0) {                                    // the state allows nothing (uniform: every thread sums the same words)
      smp_fsm_dead(smp_get<SmpCtl>(ctl_...), smp_get<SmpLp>(ctl_...), s, token, token_stride, n_kept, prob);
      return;
    }
  }
  const bool use_k = count_k && k < nrow;

  if (greedy) {
    if constexpr (kLp)
      if (lp_on)
        lse = smp_lp_phase(r, pen, nrow, mkey, smp_key_value(mkey), smp_get<SmpLp>(ctl_...).n_top, false, tid, hist, sub, wsum, &sh_bin,
                           &sh_E, &sh_key, lpl);
    if (tid == 0) {
      if constexpr (!kScore) {
        token[s * token_stride] = (long long)midx;
        if (n_kept) n_kept[s] = 1;
        if (prob) prob[s] = 1.f;
      }
      if constexpr (kLp)
        smp_lp_after(smp_get<SmpLp>(ctl_...), smp_get<SmpCtl>(ctl_...), s, nrow, mkey, mkey, smp_key_value(mkey), lse, lpl);
      if constexpr (kCtl && !kScore) smp_after(smp_get<SmpCtl>(ctl_...), s, (long long)midx);
      if constexpr (kAdj) smp_adj_after(smp_get<SmpAdj>(ctl_...), s, (long long)midx);
      if constexpr (kFsm) smp_fsm_after(smp_get<SmpFsm>(ctl_...), smp_get<SmpCtl>(ctl_...), s, fsm_q, (long long)midx);
    }
    return;
  }
  const float xm = smp_key_value(mkey);
  const float c = 1.44269504088896341f / tau;
  [[maybe_unused]] u64 qmin = 0ull;                     // ADJ-3: a kept element's weight is at least (u64)(min_p 2^40); above 1 as 1
  if constexpr (kAdj) {
    const SmpAdj& a = smp_get<SmpAdj>(ctl_...);
    const float mp = a.min_p ? a.min_p[s] : 0.f;
    qmin = mp > 0.f ? (mp < 1.f ? (u64)(mp * 0x1p40f) : SMP_ONE) : 0ull;
  }

  // ---- top-k: the bin where the count from the top reaches k, then the key inside it
  unsigned tk = 0u;
  if (use_k) {
    SmpScan sc;
    smp_scan(hist, wsum, tid, sc);
    smp_locate(sc, (u64)k, tid, &sh_bin, &sh_E);
    if (tid < SMP_SUB) sub[tid] = 0ull;
    __syncthreads();
    const unsigned B = sh_bin;
    for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
      const long long j = j0 + lane;
      unsigned key[8] = {}, valid = 0u;
      if (j < r.nt) valid = smp_load(r, pen, j, key);
      unsigned bin[8], m = 0u;
      u64 val[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bin[e] = key[e] & 15u; val[e] = 1ull; if ((key[e] >> 4) == B) m |= 1u << e; }
      if (__any((valid & m) != 0u)) smp_hist_add(sub, bin, val, valid & m, lane);
    }
    __syncthreads();
    if (tid == 0) {
      u64 E = sh_E;
      unsigned res = mkey;
      for (int i = SMP_SUB - 1; i >= 0; --i) {
        if (E < (u64)k) res = B * SMP_SUB + i;
        E += sub[i];
      }
      sh_key = res;
    }
    __syncthreads();
    tk = sh_key;
    __syncthreads();
  }
  if constexpr (kLp)                             // hist is free here: top-k has read its counts, top-p has not begun
    if (lp_on)
      lse = smp_lp_phase(r, pen, nrow, mkey, xm, smp_get<SmpLp>(ctl_...).n_top, count_k, tid, hist, sub, wsum, &sh_bin, &sh_E, &sh_key,
                         lpl);

  // ---- top-p: keep a class while the mass strictly above it is below p Z_K
  unsigned tp = 0u;
  if (use_p) {
#pragma unroll
    for (int i = 0; i < SMP_BINS / SMP_THREADS; ++i) hist[tid + i * SMP_THREADS] = 0ull;
    __syncthreads();
    for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
      const long long j = j0 + lane;
      unsigned key[8] = {}, valid = 0u;
      if (j < r.nt) valid = smp_load(r, pen, j, key);
      unsigned m = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (key[e] >= tk) m |= 1u << e;
      m &= valid;
      if (__any(m != 0u)) {
        unsigned bin[8];
        u64 val[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { bin[e] = key[e] >> 4; val[e] = (m >> e & 1u) ? smp_weight(key[e], mkey, xm, c) : 0ull; }
        smp_hist_add(hist, bin, val, m, lane);
      }
    }
    __syncthreads();
    SmpScan sc;
    smp_scan(hist, wsum, tid, sc);
    // mass above < p Z  <=>  mass above < ceil(p Z) for an integer mass; p Z in float64 (Z < 2^64: 2^-53 relative)
    const double pz = (double)p * (double)sc.total;
    const u64 T = pz > 0.0 ? (u64)ceil(pz) : 0ull;
    if (tid == 0) { sh_bin = mkey >> 4; sh_E = 0ull; }        // T == 0 (p <= 0): the top class alone
    __syncthreads();
    smp_locate(sc, T, tid, &sh_bin, &sh_E);
    if (tid < SMP_SUB) sub[tid] = 0ull;
    __syncthreads();
    const unsigned B = sh_bin;
    for (long long j0 = (long long)wave * 64; j0 < r.nt; j0 += SMP_THREADS) {
      const long long j = j0 + lane;
      unsigned key[8] = {}, valid = 0u;
      if (j < r.nt) valid = smp_load(r, pen, j, key);
      unsigned bin[8], m = 0u;
      u64 val[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { bin[e] = key[e] & 15u; val[e] = 1ull; if ((key[e] >> 4) == B && key[e] >= tk) m |= 1u << e; }
      if (__any((valid & m) != 0u)) smp_hist_add(sub, bin, val, valid & m, lane);
    }
    __syncthreads();
    if (tid == 0) {
      u64 E = sh_E;
      unsigned res = mkey;
      for (int i = SMP_SUB - 1; i >= 0; --i) {
        const unsigned key = B * SMP_SUB + i;
        if (E < T) res = key;
        E += sub[i] * smp_weight(key, mkey, xm, c);
      }
      sh_key = res < mkey ? res : mkey;
    }
    __syncthreads();
    tp = sh_key;
  }
  const unsigned t = tk > tp ? tk : tp;

  // ---- pass 5: kept count and mass; wave w owns the tiles [w tpw, (w+1) tpw), its lanes interleaved
  const long long tpw = (r.nt + SMP_WAVES - 1) / SMP_WAVES;
  const long long jbeg = wave * tpw, jend = (jbeg + tpw < r.nt) ? jbeg + tpw : r.nt;
  unsigned cnt = 0u;
  u64 mass = 0ull;
  for (long long j0 = jbeg; j0 < jend; j0 += 64) {
    const long long j = j0 + lane;
    if (j < jend) {
      unsigned key[8];
      const unsigned valid = smp_load(r, pen, j, key);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((valid >> e & 1u) && key[e] >= t) {
          if constexpr (kAdj) {
            const u64 w = smp_weight(key[e], mkey, xm, c);
            if (w >= qmin) { ++cnt; mass += w; }
          } else {
            ++cnt; mass += smp_weight(key[e], mkey, xm, c);
          }
        }
    }
  }
  mass = smp_wave_sum(mass);
  cnt = (unsigned)smp_wave_sum((u64)cnt);
  __syncthreads();                              // wsum of the last scan has been read by every thread
  if (lane == 0) { wsum[wave] = mass; wcnt[wave] = cnt; }
  __syncthreads();
  u64 Z = 0ull;
  unsigned kept = 0u;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) { Z += wsum[w]; kept += wcnt[w]; }

  // ---- the draw: splitmix64 finaliser over (seed, counter + 1)
  const long long ctr = counter[s];
  auto mix = [](u64 z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  const u64 u = mix(mix((u64)seed[s]) + ((u64)ctr + 1ull) * 0x9E3779B97F4A7C15ull);
  const u64 target = __umul64hi(u, Z);          // < Z
  u64 before = 0ull;
  int wstar = SMP_WAVES - 1;
#pragma unroll
  for (int w = SMP_WAVES - 1; w >= 0; --w) {
    u64 pre = 0ull;
#pragma unroll
    for (int v = 0; v < SMP_WAVES; ++v) if (v < w) pre += wsum[v];
    if (target >= pre && target < pre + wsum[w]) { wstar = w; before = pre; }
  }
  if (wave != wstar) return;

  // ---- pass 6: the wave that holds the target finds the tile, one lane walks it
  u64 rem = target - before;
  for (long long j0 = jbeg; j0 < jend; j0 += 64) {
    const long long j = j0 + lane;
    unsigned key[8] = {}, valid = 0u;
    u64 q[8];
    u64 m = 0ull;
    if (j < jend) valid = smp_load(r, pen, j, key);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      q[e] = ((valid >> e & 1u) && key[e] >= t) ? smp_weight(key[e], mkey, xm, c) : 0ull;
      if constexpr (kAdj) q[e] = q[e] >= qmin ? q[e] : 0ull;
      m += q[e];
    }
    const u64 incl = smp_wave_incl_scan(m, lane);
    const u64 tot = __shfl(incl, 63, 64);
    if (rem < tot) {
      const u64 hit = __ballot(rem < incl);
      if (lane == __ffsll((long long)hit) - 1) {
        u64 x = rem - (incl - m);
        int e = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i)
          if (e == i && x >= q[i]) { x -= q[i]; e = i + 1; }
        u64 qe = q[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) if (e == i) qe = q[i];
        token[s * token_stride] = j * 8 - r.off + e;
        if (n_kept) n_kept[s] = (int)kept;
        if (prob) prob[s] = (float)((double)qe / (double)Z);
        counter[s] = ctr + 1;
        if constexpr (kLp) {
          unsigned ke = key[0];
#pragma unroll
          for (int i = 1; i < 8; ++i) if (e == i) ke = key[i];
          smp_lp_after(smp_get<SmpLp>(ctl_...), smp_get<SmpCtl>(ctl_...), s, nrow, ke, mkey, xm, lse, lpl);
        }
        if constexpr (kCtl) smp_after(smp_get<SmpCtl>(ctl_...), s, j * 8 - r.off + e);
        if constexpr (kAdj) smp_adj_after(smp_get<SmpAdj>(ctl_...), s, j * 8 - r.off + e);
        if constexpr (kFsm) smp_fsm_after(smp_get<SmpFsm>(ctl_...), smp_get<SmpCtl>(ctl_...), s, fsm_q, j * 8 - r.off + e);
      }
      return;
    }
    rem -= tot;
  }
}

// seen_row |= the bits of ids[0..n) that lie in [0, V)
__global__ void __launch_bounds__(256)
token_mark_kernel(unsigned* __restrict__ seen_row, long long V, const long long* __restrict__ ids, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long id = ids[i];
    if (id >= 0 && id < V) atomicOr(&seen_row[id >> 5], 1u << (id & 31));
  }
}

}  // namespace ivl

// one launch statement for the five forms and their three adjusted twins: the groups G follow the twelve parameters that every form takes
template <typename... G>
static void sample_rows_launch(const ivl_sample_args& a, void* stream, const G&... g) {
  using namespace ivl;
  hipLaunchKernelGGL((sample_rows_kernel<G...>), dim3((unsigned)a.S), dim3(SMP_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)a.logits, (long long)a.ld, a.V, a.temperature, (const int*)a.top_k, a.top_p,
                     (const long long*)a.seed, (long long*)a.counter, (long long*)a.token, (long long)a.token_stride,
                     (int*)a.n_kept, a.prob, g...);
}

// Checks in the order base, controls, scores, constraint, adjustment; then the form rule of include/ivl_hip.h, written once.
// adj == NULL: ivl_sample_rows_fwd, whose five launches stand as they were.
static int sample_rows(const ivl_sample_args* args, const ivl_sample_adj_args* adj, void* stream, const char* fn) {
  using namespace ivl;
  IVL_REQUIRE(args, IVL_ERR_INVALID_ARG, "%s: NULL args", fn);
  const ivl_sample_args& a = *args;
  const bool score = a.score_only != 0;
  const bool ring = a.lp_history || a.top_hist_ids || a.top_hist_lp;
  // ---- base
  IVL_REQUIRE(a.logits && (score ? a.top_ids && a.top_logprobs
                                 : a.temperature && a.top_k && a.top_p && a.seed && a.counter && a.token),
              IVL_ERR_INVALID_ARG, "%s: NULL pointer", fn);
  IVL_REQUIRE(a.S >= 1 && a.V >= 1 && a.ld >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: S=%d V=%d ld=%lld", fn, a.S, a.V,
              (long long)a.ld);
  IVL_REQUIRE(a.V < (1 << 23), IVL_ERR_UNSUPPORTED, "%s: V=%d (the Q40 sums are sized for V < 2^23)", fn, a.V);
  if (score)                                             // nothing is committed: a field that says otherwise is refused
    IVL_REQUIRE(!a.temperature && !a.top_k && !a.top_p && !a.seed && !a.counter && !a.token && a.token_stride == 0 && !a.n_kept &&
                    !a.prob && !a.stop_ids && a.n_stop == 0 && !a.budget && !a.fill && !a.n_new && !a.history && a.hist_ld == 0 &&
                    !a.logprob && !a.cum_logprob && !ring && !a.fsm_state && !a.fsm_mask && a.mask_ld == 0 && a.n_states == 0 &&
                    !a.fsm_desc && !a.fsm_cls && !a.fsm_trans,
                IVL_ERR_INVALID_ARG, "%s: score_only takes logits, rep_penalty, seen, done and the top-N list alone", fn);
  // ---- controls
  IVL_REQUIRE(!a.rep_penalty || a.seen, IVL_ERR_INVALID_ARG, "%s: rep_penalty needs seen", fn);
  IVL_REQUIRE(!a.seen || a.seen_ld * 32 >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: seen_ld=%lld words hold fewer than V=%d bits", fn,
              (long long)a.seen_ld, a.V);
  IVL_REQUIRE(a.n_stop >= 0 && a.n_stop <= 16, IVL_ERR_INVALID_ARG, "%s: n_stop=%d outside 0..16", fn, a.n_stop);
  IVL_REQUIRE(a.n_stop == 0 || (a.stop_ids && a.done), IVL_ERR_INVALID_ARG, "%s: n_stop=%d needs stop_ids and done", fn, a.n_stop);
  IVL_REQUIRE(!a.budget || (a.n_new && a.done), IVL_ERR_INVALID_ARG, "%s: budget needs n_new and done", fn);
  IVL_REQUIRE(!a.history || (a.n_new && a.hist_ld >= 1), IVL_ERR_INVALID_ARG, "%s: history needs n_new and hist_ld >= 1 (%lld)", fn,
              (long long)a.hist_ld);
  // ---- scores
  IVL_REQUIRE(a.n_top >= (score ? 1 : 0) && a.n_top <= SMP_TOP_MAX, IVL_ERR_INVALID_ARG, "%s: n_top=%d outside %d..%d", fn, a.n_top,
              score ? 1 : 0, SMP_TOP_MAX);
  IVL_REQUIRE(a.n_top == 0 || (a.top_ids && a.top_logprobs), IVL_ERR_INVALID_ARG, "%s: n_top=%d needs top_ids and top_logprobs", fn,
              a.n_top);
  IVL_REQUIRE(!(a.top_hist_ids || a.top_hist_lp) || a.n_top > 0, IVL_ERR_INVALID_ARG, "%s: the top rings need n_top > 0", fn);
  IVL_REQUIRE(!ring || (a.n_new && a.hist_ld >= 1), IVL_ERR_INVALID_ARG,
              "%s: lp_history and the top rings need n_new and hist_ld >= 1 (%lld)", fn, (long long)a.hist_ld);
  // ---- constraint
  if (a.fsm_state) {
    IVL_REQUIRE(a.fsm_mask, IVL_ERR_INVALID_ARG, "%s: fsm_state needs fsm_mask", fn);
    IVL_REQUIRE(a.fsm_desc, IVL_ERR_INVALID_ARG, "%s: fsm_state needs fsm_desc", fn);
    IVL_REQUIRE(a.fsm_cls, IVL_ERR_INVALID_ARG, "%s: fsm_state needs fsm_cls", fn);
    IVL_REQUIRE(a.fsm_trans, IVL_ERR_INVALID_ARG, "%s: fsm_state needs fsm_trans", fn);
    IVL_REQUIRE(a.done, IVL_ERR_INVALID_ARG, "%s: fsm_state needs done (a dead end is reported there)", fn);
    IVL_REQUIRE(a.mask_ld * 32 >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: mask_ld=%lld words hold fewer than V=%d bits", fn,
                (long long)a.mask_ld, a.V);
    IVL_REQUIRE(a.n_states >= 1, IVL_ERR_INVALID_ARG, "%s: n_states=%d", fn, a.n_states);
  }
  // ---- adjustment
  bool adjusted = false;
  if (adj) {
    const ivl_sample_adj_args& j = *adj;
    IVL_REQUIRE(!j.count || a.seen, IVL_ERR_INVALID_ARG, "%s: count needs seen", fn);
    IVL_REQUIRE(!j.count || j.count_ld >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: count_ld=%lld below V=%d", fn, (long long)j.count_ld,
                a.V);
    IVL_REQUIRE(!(j.freq_penalty || j.pres_penalty) || j.count, IVL_ERR_INVALID_ARG, "%s: freq_penalty and pres_penalty need count",
                fn);
    if (j.bias_idx) {
      IVL_REQUIRE(j.bias_mask, IVL_ERR_INVALID_ARG, "%s: bias_idx needs bias_mask", fn);
      IVL_REQUIRE(j.bias_val, IVL_ERR_INVALID_ARG, "%s: bias_idx needs bias_val", fn);
      IVL_REQUIRE(j.n_bias >= 1, IVL_ERR_INVALID_ARG, "%s: n_bias=%d", fn, j.n_bias);
      IVL_REQUIRE(j.bias_mask_ld * 32 >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: bias_mask_ld=%lld words hold fewer than V=%d bits",
                  fn, (long long)j.bias_mask_ld, a.V);
      IVL_REQUIRE(j.bias_ld >= (int64_t)a.V, IVL_ERR_INVALID_ARG, "%s: bias_ld=%lld below V=%d", fn, (long long)j.bias_ld, a.V);
    }
    IVL_REQUIRE(!score, IVL_ERR_INVALID_ARG, "%s: score_only takes no adjustment group", fn);
    adjusted = j.min_p || j.freq_penalty || j.pres_penalty || j.count || j.bias_idx;      // else ADJ-0: the call without the group
  }
  if (adjusted) {
    const ivl_sample_adj_args& j = *adj;
    const SmpCtl c = {a.rep_penalty, a.seen, a.seen_ld, (const long long*)a.stop_ids, a.n_stop, (const long long*)a.budget,
                      (const long long*)a.fill, (long long*)a.n_new, a.done, (long long*)a.history, a.hist_ld};
    const SmpLp l = {a.logprob, a.n_top, (long long*)a.top_ids, a.top_logprobs, a.cum_logprob, a.lp_history,
                     (long long*)a.top_hist_ids, a.top_hist_lp};
    const SmpFsm f = {a.fsm_state, a.fsm_mask, a.mask_ld, a.n_states, (const long long*)a.fsm_desc, a.fsm_cls, a.fsm_trans};
    const SmpAdj d = {j.min_p, j.freq_penalty, j.pres_penalty, j.count, j.count_ld, j.bias_idx, j.bias_mask, j.bias_mask_ld,
                      j.bias_val, j.bias_ld, j.n_bias};
    // at least the controlled form, then the scoring or the constrained one by the rule below
    if (a.fsm_state)
      sample_rows_launch(a, stream, c, l, f, d);
    else if (a.logprob || a.n_top > 0 || a.top_ids || a.top_logprobs || a.cum_logprob || ring)
      sample_rows_launch(a, stream, c, l, d);
    else
      sample_rows_launch(a, stream, c, d);
    return check_launch(fn);
  }
  // ---- the device structs, each filled here and nowhere else, in the order of their fields (the score-only form reads seen
  //      and done and writes neither)
  const SmpCtl c = {a.rep_penalty, a.seen, a.seen_ld, (const long long*)a.stop_ids, a.n_stop, (const long long*)a.budget,
                    (const long long*)a.fill, (long long*)a.n_new, a.done, (long long*)a.history, a.hist_ld};
  const SmpLp l = {a.logprob, a.n_top, (long long*)a.top_ids, a.top_logprobs, a.cum_logprob, a.lp_history,
                   (long long*)a.top_hist_ids, a.top_hist_lp};
  const SmpFsm f = {a.fsm_state, a.fsm_mask, a.mask_ld, a.n_states, (const long long*)a.fsm_desc, a.fsm_cls, a.fsm_trans};
  // ---- the form: `fill` and the scalars (seen_ld, hist_ld, mask_ld, n_states) select nothing
  if (score)
    sample_rows_launch(a, stream, c, l, SmpScore{});
  else if (a.fsm_state)
    sample_rows_launch(a, stream, c, l, f);
  else if (a.logprob || a.n_top > 0 || a.top_ids || a.top_logprobs || a.cum_logprob || ring)
    sample_rows_launch(a, stream, c, l);
  else if (a.rep_penalty || a.seen || a.n_stop > 0 || a.budget || a.n_new || a.done || a.history)
    sample_rows_launch(a, stream, c);
  else
    sample_rows_launch(a, stream);
  return check_launch(fn);
}

extern "C" int ivl_sample_rows_fwd(const ivl_sample_args* args, void* stream) {
  return sample_rows(args, nullptr, stream, "ivl_sample_rows_fwd");
}

extern "C" int ivl_sample_rows_adj_fwd(const ivl_sample_args* args, const ivl_sample_adj_args* adj, void* stream) {
  return sample_rows(args, adj, stream, "ivl_sample_rows_adj_fwd");
}

extern "C" int ivl_token_mark_fwd(uint32_t* seen_row, int64_t V, const int64_t* ids, int64_t n, void* stream) {
  using namespace ivl;
  IVL_REQUIRE(seen_row && V >= 1 && n >= 0 && (n == 0 || ids), IVL_ERR_INVALID_ARG, "ivl_token_mark_fwd: seen_row=%p V=%lld n=%lld",
              (void*)seen_row, (long long)V, (long long)n);
  if (n == 0) return IVL_OK;
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(token_mark_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream,
                     (unsigned*)seen_row, (long long)V, (const long long*)ids, (long long)n);
  return check_launch("ivl_token_mark_fwd");
}

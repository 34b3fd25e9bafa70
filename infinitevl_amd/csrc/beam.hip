// Beam search bookkeeping of a graphed decode step (ivl_beam_select_fwd, ivl_beam_commit_fwd): G groups of B beams in the slots
// [g B, (g+1) B) of a multi-stream cache.  One wave per group; everything the step decides -- the beams' parents, their next
// tokens, the finished hypotheses, the group's done flag -- stays on the device, so a captured step makes no host round trip.
// The semantics (HF BeamSearchScorer.process / BeamHypotheses / finalize, with a total tie order) are written out in
// include/ivl_hip.h.  All score arithmetic is float64: cum + (double)lp of an fp32 lp is one correctly rounded add of two values
// whose order does not matter; nothing here depends on the order in which lanes or waves arrive.
#include "ivl_common.h"

namespace ivl {

constexpr int BM_THREADS = 64;
constexpr int BM_MAX_B = 8;
constexpr int BM_MAX_K = 20;

struct BeamHyp {                  // a group's finished hypotheses, in insertion order (HF's list)
  double score[BM_MAX_B];
  double sum[BM_MAX_B];
  long long len[BM_MAX_B];
  int n;
};

struct BeamTables {               // per group [G,B] / [G,B,L]
  int* beam_done;
  int* n_hyp;
  double* hyp_score;
  double* hyp_sum;
  long long* hyp_len;
  long long* hyp_tokens;
  long long L;
};

// sum / n^lp in float64: lp == 1 a plain IEEE division, lp == 0 the sum itself
__device__ __forceinline__ double beam_hyp_score(double sum, long long n, double lp) {
  if (lp == 0.0) return sum;
  if (lp == 1.0) return sum / (double)n;
  return sum / pow((double)n, lp);
}

__device__ __forceinline__ void beam_load(BeamHyp& H, const BeamTables& t, long long g, int B, int lane) {
  if (lane < B) {
    H.score[lane] = t.hyp_score[g * B + lane];
    H.sum[lane] = t.hyp_sum[g * B + lane];
    H.len[lane] = t.hyp_len[g * B + lane];
  }
  if (lane == 0) {                                   // (a count outside 0..B cannot index past the table)
    const int n = t.n_hyp[g];
    H.n = n < 0 ? 0 : (n > B ? B : n);
  }
  __syncthreads();
}
__device__ __forceinline__ void beam_store(const BeamHyp& H, const BeamTables& t, long long g, int B, int lane) {
  __syncthreads();
  if (lane < B) {
    t.hyp_score[g * B + lane] = H.score[lane];
    t.hyp_sum[g * B + lane] = H.sum[lane];
    t.hyp_len[g * B + lane] = H.len[lane];
  }
  if (lane == 0) t.n_hyp[g] = H.n;
}

// BeamHypotheses.add, called by every lane of the wave with the same arguments: insert if the table holds fewer than B or
// score > the worst; over B the worst (lowest score, the earliest of equals) leaves and the later ones move up.  The
// hypothesis' tokens are src[0 .. n_src) and then `last` (when >= 0).  Lane t owns the token positions t mod 64 of every row,
// in the shift and in the copy alike: a position is read and written by one lane, in program order.
__device__ __forceinline__ void beam_insert(BeamHyp& H, int B, double score, double sum, long long n, const long long* src,
                                            long long n_src, long long last, long long* rows, long long L, int lane) {
  __syncthreads();
  const int nh = H.n;
  if (nh >= B) {
    int w = 0;
    for (int i = 1; i < nh; ++i)
      if (H.score[i] < H.score[w]) w = i;
    if (!(score > H.score[w])) return;
    for (int i = w; i + 1 < nh; ++i) {
      const long long m = H.len[i + 1] < L ? H.len[i + 1] : L;
      for (long long t = lane; t < m; t += BM_THREADS) rows[(long long)i * L + t] = rows[(long long)(i + 1) * L + t];
    }
    __syncthreads();
    if (lane == 0) {
      for (int i = w; i + 1 < nh; ++i) { H.score[i] = H.score[i + 1]; H.sum[i] = H.sum[i + 1]; H.len[i] = H.len[i + 1]; }
      H.n = nh - 1;
    }
    __syncthreads();
  }
  const int at = H.n;
  if (n_src > L) n_src = L;
  for (long long t = lane; t < n_src; t += BM_THREADS) rows[(long long)at * L + t] = src[t];
  if (lane == 0) {
    if (last >= 0 && n_src >= 0 && n_src < L) rows[(long long)at * L + n_src] = last;
    H.score[at] = score;
    H.sum[at] = sum;
    H.len[at] = n;
    H.n = at + 1;
  }
  __syncthreads();
}

struct BeamSelectArgs {
  int B, K, n_stop;
  unsigned long long mask;
  const long long* top_ids;
  const float* top_lp;
  const double* cum;
  const long long* n_new;
  const long long* history;
  const long long* stop_ids;
  const double* length_penalty;
  const int* early_stopping;
  BeamTables t;
  int* parent;
  long long* next_token;
  double* next_score;
};

__global__ void __launch_bounds__(BM_THREADS) beam_select_kernel(const BeamSelectArgs a) {
  const long long g = blockIdx.x;
  const int lane = threadIdx.x;
  if (!(a.mask >> g & 1ull) || a.t.beam_done[g] != 0) return;      // uniform
  __shared__ double cs[BM_MAX_B * BM_MAX_K];
  __shared__ unsigned char cv[BM_MAX_B * BM_MAX_K];
  __shared__ int order[BM_MAX_K];
  __shared__ int nvalid_s;
  __shared__ BeamHyp H;
  const int B = a.B, K = a.K, n = B * K;
  const long long slot0 = g * B, L = a.t.L;
  if (lane == 0) nvalid_s = 0;
  beam_load(H, a.t, g, B, lane);
  // the candidates: (beam b, rank j) = c = b K + j, of beams with a finite sum, ids >= 0
  for (int c = lane; c < n; c += BM_THREADS) {
    const int b = c / K;
    const long long id = a.top_ids[slot0 * K + c];
    const double cb = a.cum[slot0 + b];
    const bool ok = id >= 0 && cb > -__builtin_inf() && cb < __builtin_inf();
    cs[c] = ok ? cb + (double)a.top_lp[slot0 * K + c] : -__builtin_inf();
    cv[c] = ok ? 1 : 0;
    if (ok) atomicAdd(&nvalid_s, 1);
  }
  __syncthreads();
  // rank = the candidates in front by (score descending, beam ascending, rank ascending); the first K are the walk
  for (int c = lane; c < n; c += BM_THREADS) {
    if (!cv[c]) continue;
    const double s = cs[c];
    int rank = 0;
    for (int o = 0; o < n; ++o)
      if (cv[o] && (cs[o] > s || (cs[o] == s && o < c))) ++rank;
    if (rank < K) order[rank] = c;
  }
  __syncthreads();
  const int nvalid = nvalid_s;
  const int nw = nvalid < K ? nvalid : K;
  const double lpv = a.length_penalty[g];
  int nb = 0;
  for (int r = 0; r < nw && nb < B; ++r) {
    const int c = order[r], b = c / K;
    const long long tok = a.top_ids[slot0 * K + c];
    const double sc = cs[c];
    bool stop = false;
    for (int i = 0; i < a.n_stop; ++i) {
      const long long id = a.stop_ids[g * a.n_stop + i];
      if (id >= 0 && id == tok) stop = true;
    }
    if (stop) {
      if (r >= B) continue;
      const long long len = a.n_new[slot0 + b] + 1;
      beam_insert(H, B, beam_hyp_score(sc, len, lpv), sc, len, a.history + (slot0 + b) * L, len - 1, tok,
                  a.t.hyp_tokens + slot0 * L, L, lane);
    } else {
      if (lane == 0) {
        a.parent[slot0 + nb] = b;
        a.next_token[slot0 + nb] = tok;
        a.next_score[slot0 + nb] = sc;
      }
      ++nb;
    }
  }
  if (lane == 0)
    for (int d = nb; d < B; ++d) {                   // fewer than B continuations: no beam there
      a.parent[slot0 + d] = d;
      a.next_token[slot0 + d] = 0;
      a.next_score[slot0 + d] = -__builtin_inf();
    }
  __syncthreads();
  // the done rule, after the walk
  bool done = false;
  if (H.n >= B) {
    if (a.early_stopping[g] != 0) {
      done = true;
    } else {
      double worst = H.score[0];
      for (int i = 1; i < H.n; ++i) worst = H.score[i] < worst ? H.score[i] : worst;
      const double best = nvalid > 0 ? cs[order[0]] : -__builtin_inf();
      done = worst >= beam_hyp_score(best, a.n_new[slot0] + 1, lpv);
    }
  }
  if (done && lane == 0) {
    a.t.beam_done[g] = 1;
    for (int d = 0; d < B; ++d) a.parent[slot0 + d] = d;
  }
  beam_store(H, a.t, g, B, lane);
}

struct BeamCommitArgs {
  int B;
  unsigned long long mask;
  const long long* next_token;
  const double* next_score;
  long long* token;
  long long token_stride;
  unsigned* seen;
  long long seen_ld;
  long long V;
  long long* history;
  long long* n_new;
  double* cum;
  const long long* budget;
  const double* length_penalty;
  int* parent;
  BeamTables t;
};

__global__ void __launch_bounds__(BM_THREADS) beam_commit_kernel(const BeamCommitArgs a) {
  const long long g = blockIdx.x;
  const int lane = threadIdx.x;
  if (!(a.mask >> g & 1ull) || a.t.beam_done[g] != 0) return;      // uniform
  __shared__ BeamHyp H;
  const int B = a.B;
  const long long slot0 = g * B, L = a.t.L;
  beam_load(H, a.t, g, B, lane);
  if (lane < B) {
    const long long s = slot0 + lane;
    const long long tok = a.next_token[s];
    a.token[s * a.token_stride] = tok;
    if (a.seen && tok >= 0 && tok < a.V) {
      unsigned* w = a.seen + s * a.seen_ld + (tok >> 5);
      *w = *w | (1u << (tok & 31));
    }
    const long long n = a.n_new[s];
    a.history[s * L + ((n % L) + L) % L] = tok;
    a.n_new[s] = n + 1;
    a.cum[s] = a.next_score[s];
  }
  __threadfence();
  __syncthreads();
  const long long bud = a.budget[g];
  if (bud >= 0 && a.n_new[slot0] >= bud) {           // HF finalize: every live beam becomes a hypothesis, in beam order
    const double lpv = a.length_penalty[g];
    for (int d = 0; d < B; ++d) {
      const double cd = a.cum[slot0 + d];
      if (!(cd > -__builtin_inf() && cd < __builtin_inf())) continue;
      const long long len = a.n_new[slot0 + d];
      beam_insert(H, B, beam_hyp_score(cd, len, lpv), cd, len, a.history + (slot0 + d) * L, len, -1ll,
                  a.t.hyp_tokens + slot0 * L, L, lane);
    }
    if (lane == 0) {                                 // a finished group's map is the identity: the next gather moves nothing
      a.t.beam_done[g] = 2;
      for (int d = 0; d < B; ++d) a.parent[slot0 + d] = d;
    }
  }
  beam_store(H, a.t, g, B, lane);
}

}  // namespace ivl

using namespace ivl;

static int beam_check(const char* fn, int G, int B, int64_t hist_ld, const void* beam_done, const void* n_hyp, const void* hyp_score,
                      const void* hyp_sum, const void* hyp_len, const void* hyp_tokens) {
  IVL_REQUIRE(G >= 1 && G <= 63, IVL_ERR_INVALID_ARG, "%s: G=%d outside 1..63", fn, G);
  IVL_REQUIRE(B >= 1 && B <= BM_MAX_B, IVL_ERR_INVALID_ARG, "%s: B=%d outside 1..%d", fn, B, BM_MAX_B);
  IVL_REQUIRE(hist_ld >= 1, IVL_ERR_INVALID_ARG, "%s: hist_ld=%lld must be >= 1", fn, (long long)hist_ld);
  IVL_REQUIRE(beam_done && n_hyp && hyp_score && hyp_sum && hyp_len && hyp_tokens, IVL_ERR_INVALID_ARG,
              "%s: NULL hypothesis table", fn);
  return IVL_OK;
}

static BeamTables beam_tables(int32_t* beam_done, int32_t* n_hyp, double* hyp_score, double* hyp_sum, int64_t* hyp_len,
                              int64_t* hyp_tokens, int64_t hist_ld) {
  BeamTables t;
  t.beam_done = beam_done;
  t.n_hyp = n_hyp;
  t.hyp_score = hyp_score;
  t.hyp_sum = hyp_sum;
  t.hyp_len = (long long*)hyp_len;
  t.hyp_tokens = (long long*)hyp_tokens;
  t.L = hist_ld;
  return t;
}

extern "C" int ivl_beam_select_fwd(int G, int B, int K, int64_t group_mask, const int64_t* top_ids, const float* top_logprobs,
                                   const double* cum_logprob, const int64_t* n_new, const int64_t* history, int64_t hist_ld,
                                   const int64_t* stop_ids, int n_stop, const double* length_penalty,
                                   const int32_t* early_stopping, int32_t* beam_done, int32_t* n_hyp, double* hyp_score,
                                   double* hyp_sum, int64_t* hyp_len, int64_t* hyp_tokens, int32_t* parent, int64_t* next_token,
                                   double* next_score, void* stream) {
  const char* fn = "ivl_beam_select_fwd";
  const int rc = beam_check(fn, G, B, hist_ld, beam_done, n_hyp, hyp_score, hyp_sum, hyp_len, hyp_tokens);
  if (rc != IVL_OK) return rc;
  IVL_REQUIRE(K >= 1 && K <= BM_MAX_K, IVL_ERR_INVALID_ARG, "%s: K=%d outside 1..%d", fn, K, BM_MAX_K);
  IVL_REQUIRE(n_stop >= 0 && n_stop <= 16, IVL_ERR_INVALID_ARG, "%s: n_stop=%d outside 0..16", fn, n_stop);
  IVL_REQUIRE(n_stop == 0 || stop_ids, IVL_ERR_INVALID_ARG, "%s: n_stop=%d needs stop_ids", fn, n_stop);
  IVL_REQUIRE(top_ids && top_logprobs && cum_logprob && n_new && history && length_penalty && early_stopping && parent &&
                  next_token && next_score,
              IVL_ERR_INVALID_ARG, "%s: NULL pointer", fn);
  if (group_mask == 0) return IVL_OK;
  BeamSelectArgs a;
  a.B = B;
  a.K = K;
  a.n_stop = n_stop;
  a.mask = (unsigned long long)group_mask;
  a.top_ids = (const long long*)top_ids;
  a.top_lp = top_logprobs;
  a.cum = cum_logprob;
  a.n_new = (const long long*)n_new;
  a.history = (const long long*)history;
  a.stop_ids = (const long long*)stop_ids;
  a.length_penalty = length_penalty;
  a.early_stopping = early_stopping;
  a.t = beam_tables(beam_done, n_hyp, hyp_score, hyp_sum, hyp_len, hyp_tokens, hist_ld);
  a.parent = parent;
  a.next_token = (long long*)next_token;
  a.next_score = next_score;
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)G), dim3(BM_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(fn);
}

extern "C" int ivl_beam_commit_fwd(int G, int B, int64_t group_mask, const int64_t* next_token, const double* next_score,
                                   int64_t* token, int64_t token_stride, uint32_t* seen, int64_t seen_ld, int64_t V,
                                   int64_t* history, int64_t hist_ld, int64_t* n_new, double* cum_logprob, const int64_t* budget,
                                   const double* length_penalty, int32_t* beam_done, int32_t* n_hyp, double* hyp_score,
                                   double* hyp_sum, int64_t* hyp_len, int64_t* hyp_tokens, int32_t* parent, void* stream) {
  const char* fn = "ivl_beam_commit_fwd";
  const int rc = beam_check(fn, G, B, hist_ld, beam_done, n_hyp, hyp_score, hyp_sum, hyp_len, hyp_tokens);
  if (rc != IVL_OK) return rc;
  IVL_REQUIRE(next_token && next_score && token && history && n_new && cum_logprob && budget && length_penalty && parent,
              IVL_ERR_INVALID_ARG, "%s: NULL pointer", fn);
  IVL_REQUIRE(token_stride >= 1, IVL_ERR_INVALID_ARG, "%s: token_stride=%lld must be >= 1", fn, (long long)token_stride);
  IVL_REQUIRE(!seen || (V >= 1 && seen_ld * 32 >= V), IVL_ERR_INVALID_ARG, "%s: seen_ld=%lld words hold fewer than V=%lld bits", fn,
              (long long)seen_ld, (long long)V);
  if (group_mask == 0) return IVL_OK;
  BeamCommitArgs a;
  a.B = B;
  a.mask = (unsigned long long)group_mask;
  a.next_token = (const long long*)next_token;
  a.next_score = next_score;
  a.token = (long long*)token;
  a.token_stride = token_stride;
  a.seen = seen;
  a.seen_ld = seen_ld;
  a.V = V;
  a.history = (long long*)history;
  a.n_new = (long long*)n_new;
  a.cum = cum_logprob;
  a.budget = (const long long*)budget;
  a.length_penalty = length_penalty;
  a.parent = parent;
  a.t = beam_tables(beam_done, n_hyp, hyp_score, hyp_sum, hyp_len, hyp_tokens, hist_ld);
  hipLaunchKernelGGL(beam_commit_kernel, dim3((unsigned)G), dim3(BM_THREADS), 0, (hipStream_t)stream, a);
  return check_launch(fn);
}

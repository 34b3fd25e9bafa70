// Token bans in front of the sampling launch: no_repeat_ngram_size, bad_words_ids and min_new_tokens of HF generate as ONE small
// launch that writes bf16 -inf into a row's logits in place (BAN-0 .. BAN-5 at ivl_token_ban_fwd in include/ivl_hip.h).  The
// kernels of sample.hip know nothing of it: they see the edited row.
//
// One workgroup per row.  A row that is finished or has every rule off returns before it reads anything else.  The row's
// sequence -- the context ring, then the history ring, each oldest first -- is staged once into LDS as int32 (an id outside
// [0, V) becomes -1 and equals nothing, not even itself), then the lanes stride over the n-gram start positions and over the
// rows of the row's sequence table.  A ban is one 2-byte store of 0xFF80 to the element's own address: nothing of the row is
// read, so a neighbour's ban in the same dword cannot be lost and the call is idempotent.
#include "ivl_common.h"

namespace ivl {

constexpr int BAN_THREADS = 256;
constexpr int BAN_WINDOW = 12288;              // tokens of hist_ld + ctx_ld the kernel stages (48 KiB of LDS)
constexpr int BAN_SEQ_MAX = 16;                // seq_ld of a sequence table
constexpr unsigned short BAN_NINF = 0xFF80u;   // bf16 -inf

struct BanArgs {
  unsigned short* logits;
  long long ld;
  int V;
  const int* done;
  const long long* n_new;
  const long long* history;
  long long hist_ld;
  const long long* ctx;
  long long ctx_ld;
  const long long* n_ctx;
  const int* ngram;
  const long long* min_new;
  const long long* stop_ids;
  int n_stop;
  const int* ban_idx;
  const long long* ban_seq;
  int n_tables, n_seq, seq_ld;
};

// how many entries of a ring count: min(n, ld), nothing for n < 0
__device__ __forceinline__ int ban_ring_len(long long n, long long ld) { return (int)(n < 0 ? 0 : (n < ld ? n : ld)); }

// entries [0, len) of a ring of `n` entries written so far, oldest first, into dst: entry number i sits at i % ld
__device__ __forceinline__ void ban_stage(int* dst, const long long* ring, long long n, long long ld, int len, int V) {
  const long long first = n - len;             // the number of the oldest entry that is still there
  for (int k = threadIdx.x; k < len; k += BAN_THREADS) {
    const long long id = ring[(first + k) % ld];
    dst[k] = (id >= 0 && id < V) ? (int)id : -1;
  }
}

__global__ __launch_bounds__(BAN_THREADS) void token_ban_kernel(const BanArgs a) {
  extern __shared__ int win[];                 // the row's sequence, oldest first
  const long long s = blockIdx.x;
  if (a.done && a.done[s] != 0) return;        // BAN-0: nothing of a finished row beyond done[s] is read
  const int g = a.ngram ? a.ngram[s] : 0;
  const int b = a.ban_idx ? a.ban_idx[s] : -1;
  const bool table = b >= 0 && b < a.n_tables;
  const bool early = a.min_new && a.n_new[s] < a.min_new[s];
  if (g < 1 && !table && !early) return;       // BAN-0: every rule off
  unsigned short* row = a.logits + s * a.ld;
  if (early) {                                 // BAN-3
    if ((int)threadIdx.x < a.n_stop) {
      const long long id = a.stop_ids[s * a.n_stop + threadIdx.x];
      if (id >= 0 && id < a.V) row[id] = BAN_NINF;
    }
  }
  if (g < 1 && !table) return;
  const int c = a.ctx ? ban_ring_len(a.n_ctx[s], a.ctx_ld) : 0;
  const long long n_new = a.n_new[s];
  const int h = ban_ring_len(n_new, a.hist_ld);
  const int L = c + h;
  if (c > 0) ban_stage(win, a.ctx + s * a.ctx_ld, a.n_ctx[s], a.ctx_ld, c, a.V);
  if (h > 0) ban_stage(win + c, a.history + s * a.hist_ld, n_new, a.hist_ld, h, a.V);
  __syncthreads();
  if (g >= 1 && L >= g) {                      // BAN-1
    const int p = g - 1;                       // the prefix: the last p tokens of the sequence
    for (int i = threadIdx.x; i <= L - g; i += BAN_THREADS) {
      bool eq = true;
      for (int k = 0; k < p && eq; ++k) {
        const int x = win[i + k];
        eq = x >= 0 && x == win[L - p + k];
      }
      const int t = win[i + p];
      if (eq && t >= 0) row[t] = BAN_NINF;
    }
  }
  if (table) {                                 // BAN-2
    for (int r = threadIdx.x; r < a.n_seq; r += BAN_THREADS) {
      const long long* q = a.ban_seq + ((long long)b * a.n_seq + r) * a.seq_ld;
      const long long t = q[a.seq_ld - 1];
      if (t < 0) continue;                     // an unused row
      bool eq = true;
      for (int k = 1; k < a.seq_ld && eq; ++k) {         // the k-th token in front of t against the k-th from the end
        const long long id = q[a.seq_ld - 1 - k];
        if (id < 0) break;                     // the sequence ends here
        eq = k <= L && id < a.V && (int)id == win[L - k];
      }
      if (eq && t < a.V) row[t] = BAN_NINF;
    }
  }
}

}  // namespace ivl

extern "C" int ivl_token_ban_fwd(const ivl_ban_args* args, void* stream) {
  using namespace ivl;
  const char* fn = "ivl_token_ban_fwd";
  IVL_REQUIRE(args && args->logits, IVL_ERR_INVALID_ARG, "%s: NULL args or logits", fn);
  const ivl_ban_args& a = *args;
  IVL_REQUIRE(a.S >= 1 && a.V >= 1 && a.ld >= a.V, IVL_ERR_INVALID_ARG, "%s: S=%d V=%d ld=%lld", fn, a.S, a.V, (long long)a.ld);
  IVL_REQUIRE(!(a.ngram || a.ban_idx) || (a.n_new && a.history && a.hist_ld >= 1), IVL_ERR_INVALID_ARG,
              "%s: ngram and ban_idx need n_new and history with hist_ld >= 1 (%lld)", fn, (long long)a.hist_ld);
  IVL_REQUIRE(!a.ctx || (a.n_ctx && a.ctx_ld >= 1), IVL_ERR_INVALID_ARG, "%s: ctx needs n_ctx and ctx_ld >= 1 (%lld)", fn,
              (long long)a.ctx_ld);
  IVL_REQUIRE(!a.ban_idx || (a.ban_seq && a.n_tables >= 1 && a.n_seq >= 1 && a.seq_ld >= 1 && a.seq_ld <= BAN_SEQ_MAX),
              IVL_ERR_INVALID_ARG, "%s: ban_idx needs ban_seq with n_tables, n_seq >= 1 and seq_ld in 1..%d (%d, %d, %d)", fn,
              BAN_SEQ_MAX, a.n_tables, a.n_seq, a.seq_ld);
  IVL_REQUIRE(!a.min_new || (a.n_new && a.stop_ids && a.n_stop >= 1 && a.n_stop <= 16), IVL_ERR_INVALID_ARG,
              "%s: min_new needs n_new and stop_ids with n_stop in 1..16 (%d)", fn, a.n_stop);
  IVL_REQUIRE(a.V < (1 << 23), IVL_ERR_UNSUPPORTED, "%s: V=%d (below 2^23 only)", fn, a.V);
  const bool window = a.ngram || a.ban_idx;
  const long long hist_ld = window ? a.hist_ld : 0, ctx_ld = window && a.ctx ? a.ctx_ld : 0;
  IVL_REQUIRE(hist_ld <= BAN_WINDOW && ctx_ld <= BAN_WINDOW && hist_ld + ctx_ld <= BAN_WINDOW, IVL_ERR_UNSUPPORTED,
              "%s: a window of hist_ld + ctx_ld = %lld + %lld tokens (at most %d)", fn, (long long)a.hist_ld, (long long)a.ctx_ld,
              BAN_WINDOW);
  const BanArgs k = {(unsigned short*)a.logits, a.ld, a.V, a.done, (const long long*)a.n_new, (const long long*)a.history, a.hist_ld,
                     window ? (const long long*)a.ctx : nullptr, a.ctx_ld, (const long long*)a.n_ctx, a.ngram,
                     (const long long*)a.min_new, (const long long*)a.stop_ids, a.n_stop, a.ban_idx, (const long long*)a.ban_seq,
                     a.n_tables, a.n_seq, a.seq_ld};
  hipLaunchKernelGGL(token_ban_kernel, dim3((unsigned)a.S), dim3(BAN_THREADS), (size_t)(hist_ld + ctx_ld) * sizeof(int),
                     (hipStream_t)stream, k);
  return check_launch(fn);
}

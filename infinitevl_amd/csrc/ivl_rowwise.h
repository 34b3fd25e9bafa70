// The row-wise formulas that more than one kernel evaluates, each written ONCE: the fused kernels (decode step, prologue,
// norm-in-projection, split step) equal the single-purpose ones bit for bit because both sides call the helper below, and a
// change to a rounding point or an edge case is made here.  Every helper is a plain inlined expression: operation order, the
// explicit fmaf and the expressions hipcc contracts (a * b + c) are part of the contract, not style.
#pragma once
#include "ivl_common.h"

namespace ivl {

// ---- GDN gate math (std:1293-1294): g = -exp(A_log) softplus(a + dt_bias), softplus as torch (the argument itself above 20);
// beta = sigmoid(b), fp32 and UNROUNDED: the caller rounds it to bf16 where the reference stores bf16.  A_log comes as the
// address of the head's value: it is read behind the softplus branch, as the decode kernels always did (read in front of it
// with the other inputs, thread 0 of gdn_decode_split_kernel measured 0.010 us slower per launch, two same-box ABAB calls) ------
__device__ __forceinline__ void gdn_gate_(float a, float dt_bias, float b, const float* A_log, float& g, float& beta) {
  const float av = a + dt_bias;
  const float sp = av > 20.f ? av : log1pf(expf(av));
  g = -expf(*A_log) * sp;
  beta = sigmoid_exact_(b);
}

// ---- causal conv of width 4 over 8 channels (fla's ShortConvolution): y[t] = act(bias + sum_j w[j] ext[t + 1 + j]),
// ext = [state(4), x(T)], new state = ext[T .. T + 3].  gdn_chunk.hip's conv4_silu is the packed form of conv4_taps_ + SiLU -------
constexpr int CONV_W = 4;

// a [8 channels][4 taps] bf16 block (conv taps, or a carried state) as its four 16-byte pieces -> fp32
__device__ __forceinline__ void unpack_taps8_(u32x4 p0, u32x4 p1, u32x4 p2, u32x4 p3, float (&f)[8][CONV_W]) {
  const unsigned int ww[16] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w, p3.x, p3.y, p3.z, p3.w};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    f[c][0] = bflo(ww[2 * c]); f[c][1] = bfhi(ww[2 * c]); f[c][2] = bflo(ww[2 * c + 1]); f[c][3] = bfhi(ww[2 * c + 1]);
  }
}

// one channel, one token: one product and three fma in tap order; with a bias the accumulator starts from it (causal_conv1d)
__device__ __forceinline__ float conv4_taps_(float w0, float w1, float w2, float w3, float x0, float x1, float x2, float x3,
                                             bool has_bias = false, float bias = 0.f) {
  float a = has_bias ? fmaf(w0, x0, bias) : w0 * x0;
  a = fmaf(w1, x1, a);
  a = fmaf(w2, x2, a);
  a = fmaf(w3, x3, a);
  return a;
}

// one token of 8 channels: out[c] from the window (the three inputs before `cur`) and `cur`; the window then slides by one
__device__ __forceinline__ void conv4_step8_(const float (&wf)[8][CONV_W], float (&win)[3][8], const float (&cur)[8], bool silu,
                                             float (&out)[8], bool has_bias = false, const float* bias8 = nullptr) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float a = conv4_taps_(wf[c][0], wf[c][1], wf[c][2], wf[c][3], win[0][c], win[1][c], win[2][c], cur[c], has_bias, has_bias ? bias8[c] : 0.f);
    if (silu) a = a * sigmoidf_(a);
    out[c] = a;
    win[0][c] = win[1][c]; win[1][c] = win[2][c]; win[2][c] = cur[c];
  }
}

// the window in front of token 0: times -3, -2, -1 are the carried state's slots 1..3 (newest last)
__device__ __forceinline__ void conv_window_from_state_(const float (&st)[8][CONV_W], float (&win)[3][8]) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 8; ++c) win[k][c] = st[c][k + 1];
}

// new_state[c][j] = ext[T + j] of 8 channels -> out [8][4] bf16; row t of x for these channels at xb + t * ld; st = the old state
__device__ __forceinline__ void conv_store_state8_(const float (&st)[8][CONV_W], const bf16_t* xb, long long ld, int T, bf16_t* out) {
  float ns[8][CONV_W];
#pragma unroll
  for (int j = 0; j < CONV_W; ++j) {
    const int e = T + j;            // index into ext
    if (e >= CONV_W) {
      float xv[8];
      unpack8(*(const u32x4*)(xb + (long long)(e - CONV_W) * ld), xv);
#pragma unroll
      for (int c = 0; c < 8; ++c) ns[c][j] = xv[c];
    } else {
#pragma unroll
      for (int e2 = 0; e2 < CONV_W; ++e2)
        if (e == e2) {
#pragma unroll
          for (int c = 0; c < 8; ++c) ns[c][j] = st[c][e2];
        }
    }
  }
  u32x4* op = (u32x4*)out;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    op[i] = u32x4{pack2bf(ns[2 * i][0], ns[2 * i][1]), pack2bf(ns[2 * i][2], ns[2 * i][3]),
                  pack2bf(ns[2 * i + 1][0], ns[2 * i + 1][1]), pack2bf(ns[2 * i + 1][2], ns[2 * i + 1][3])};
}

// T == 1: the state of one channel (4 bf16, oldest first) loses its oldest slot and takes the raw input x
__device__ __forceinline__ u32x2 conv_state_shift1_(u32x2 sv, bf16_t x) {
  return u32x2{(sv.x >> 16) | (sv.y << 16), (sv.y >> 16) | ((unsigned int)x << 16)};
}

// ---- gated RMSNorm of a 256-wide row (fla's FusedRMSNormGated): y = x * rstd * w * g * sigmoid(g) in fp32, rounded once by
// the caller's store; ss = the row's sum of squares -------------------------------------------------------------------------------
__device__ __forceinline__ float rms256_rstd_(float ss, float eps) { return 1.0f / sqrtf(ss * (1.0f / 256.0f) + eps); }

template <int N_>
__device__ __forceinline__ void gated_norm_n_(const float (&x)[N_], float rstd, const float (&w)[N_], const float (&g)[N_], float (&out)[N_]) {
#pragma unroll
  for (int i = 0; i < N_; ++i) out[i] = x[i] * rstd * w[i] * g[i] * sigmoidf_(g[i]);
}

// ---- (residual add +) RMSNorm with the Qwen2RMSNorm rounding points: h = bf16(x + residual);
// y = bf16(w * bf16(h * rsqrt(mean(h^2) + eps))) ----------------------------------------------------------------------------------
__device__ __forceinline__ float add_round_(float x, float r) { return bf_round(x + r); }      // h = bf16(x + residual)
__device__ __forceinline__ float sumsq8_(const float (&h)[8], float ss) {         // ss + sum h^2, accumulated in element order
#pragma unroll
  for (int i = 0; i < 8; ++i) ss = fmaf(h[i], h[i], ss);
  return ss;
}
__device__ __forceinline__ float qwen_rstd_(float sumsq, int N, float eps) { return rsqrtf(sumsq / (float)N + eps); }
__device__ __forceinline__ float qwen_norm_(float h, float rstd, float w) { return w * bf_round(h * rstd); }

}  // namespace ivl

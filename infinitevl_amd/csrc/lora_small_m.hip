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
// The device code lives in ivl_lora.h, shared with the 16-row entry (lora_m16.hip) and the LoRA epilogue of linear_m16.hip.
#include "ivl_lora.h"

using namespace ivl;

extern "C" int ivl_lora_add_small_m_fwd(const ivl_lora_args* a, void* stream) {
  const char* who = "ivl_lora_add_small_m_fwd";
  LoraSegs segs;
  const int chk = lora_check(who, a, 4, true, segs);
  if (chk != IVL_OK) return chk;
  const bool norm = a->norm_weight != nullptr;
  hipStream_t st = (hipStream_t)stream;
  const bf16_t *x = (const bf16_t*)a->x, *A = (const bf16_t*)a->A;
  const bf16_t *res = (const bf16_t*)a->residual, *nw = (const bf16_t*)a->norm_weight;
  bf16_t* t_ws = (bf16_t*)a->t_ws;
  const int* idx = (const int*)a->adapter_idx;
  const int nrank = a->n_seg * a->R;
  const dim3 sgrid((nrank + 4 * LORA_JPW - 1) / (4 * LORA_JPW), a->M);
  if (!norm)
    lora_launch_shrink(x, idx, A, t_ws, a->M, a->K, nrank, a->n_adapters, st);
  else if (a->K <= 2048)
    hipLaunchKernelGGL((lora_shrink_kernel<true, 1>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, a->K, nrank, a->n_adapters, res, nw, a->eps);
  else
    hipLaunchKernelGGL((lora_shrink_kernel<true, 2>), sgrid, dim3(256), 0, st, x, idx, A, t_ws, a->K, nrank, a->n_adapters, res, nw, a->eps);
  const int rc = check_launch("ivl_lora_add_small_m_fwd (shrink)");
  if (rc != IVL_OK) return rc;
  lora_launch_expand(a, segs, st);
  return check_launch("ivl_lora_add_small_m_fwd (expand-add)");
}

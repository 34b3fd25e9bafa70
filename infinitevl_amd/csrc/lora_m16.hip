// Per-row LoRA adapters for a decode step of up to 16 rows, as two launches behind a base projection (ivl_lora_add_m16_fwd, DESIGN
// 4.17): the non-NORM shrink and the expand-add of ivl_lora_add_small_m_fwd on grids of M <= 16 rows -- the same kernels (ivl_lora.h),
// so a row is the same bits as through the small-M entry called on that row alone.  The 5..16-row step materialises its norms: there
// is no NORM group.  The fused form, where the expand-add rides in the epilogue of the base projection, is linear_m16.hip's.
#include "ivl_lora.h"

using namespace ivl;

extern "C" int ivl_lora_add_m16_fwd(const ivl_lora_args* a, void* stream) {
  const char* who = "ivl_lora_add_m16_fwd";
  LoraSegs segs;
  const int chk = lora_check(who, a, 16, false, segs);
  if (chk != IVL_OK) return chk;
  hipStream_t st = (hipStream_t)stream;
  lora_launch_shrink((const bf16_t*)a->x, (const int*)a->adapter_idx, (const bf16_t*)a->A, (bf16_t*)a->t_ws, a->M, a->K,
                     a->n_seg * a->R, a->n_adapters, st);
  const int rc = check_launch("ivl_lora_add_m16_fwd (shrink)");
  if (rc != IVL_OK) return rc;
  lora_launch_expand(a, segs, st);
  return check_launch("ivl_lora_add_m16_fwd (expand-add)");
}

/*
 * ivl_hip.h -- C ABI of libivl_hip.so: MI355X (gfx950 / CDNA4) kernels for the
 * InfiniteVL hybrid-attention hot path (Gated DeltaNet + sliding-window attention, and the
 * vision tower's window attention).
 *
 * This is the drop-in boundary.  Each entry point replaces one
 * operator the reference reaches through a third-party CUDA/Triton package; the
 * reference call site it serves is cited as `std:<line>` =
 * infinitevl/infinitevl_standard/modeling_infinitevl.py, `strm:` = the same file of
 * infinitevl/infinitevl_streaming/, and `fla:` =
 * src/llamafactory/model/fla/ (vendored snapshot of flash-linear-attention).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller;
 *     the library never allocates, frees, synchronises or branches on device data on the
 *     host, so every call is hipGraph-capturable (SURVEY.md section 8b "Threading / streams").
 *     (One exception, ownership: the first GDN chunk call on a device makes ONE hipHostMalloc of 512 bytes of pinned,
 *     device-mapped host memory -- 64 status slots of two words for ivl_gdn_sync_status -- owned by the library and kept
 *     for the life of the process; if it fails the library runs without it.  ivl_gdn_sync_status(sync != NULL) is the
 *     one blocking call.)
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - layouts are the reference's time-major ones: q,k [B,T,H,K], v,o [B,T,H,V],
 *     g,beta [B,T,H], recurrent state [B,H,K,V]; bf16 activations, fp32 g.
 *   - return value: 0 = ok, negative = error code below; never throws, never exits.
 *     ivl_last_error() returns a thread-local human-readable message for the last failure.
 */
#ifndef IVL_HIP_H
#define IVL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVL_ABI_VERSION 12

/* The library is built with -fvisibility=hidden: the entry points declared here are its ONLY exported symbols. */
#define IVL_API __attribute__((visibility("default")))

/* element type codes for the arguments that accept more than one */
#define IVL_BF16 0
#define IVL_F32 2
#define IVL_FP8_E4M3 3   /* OCP e4m3fn (gfx950); accepted only as `mma_dtype`: operand format of the MFMA products */

/* error codes */
#define IVL_OK 0
#define IVL_ERR_INVALID_ARG (-1)   /* NULL pointer / non-positive size / bad dtype code        */
#define IVL_ERR_UNSUPPORTED (-2)   /* shape outside what the kernels are built for             */
#define IVL_ERR_WORKSPACE (-3)     /* workspace too small (see the *_workspace_bytes helpers)  */
#define IVL_ERR_LAUNCH (-4)        /* hipLaunch / hipGetLastError failure                      */
#define IVL_ERR_SYNC (-5)          /* a wait inside a single-launch GDN call ran out (ivl_gdn_sync_status / _reset) */

IVL_API int ivl_abi_version(void);
IVL_API const char* ivl_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Gated DeltaNet, token-recurrent form.
 * Replaces fla.ops.gated_delta_rule.fused_recurrent_gated_delta_rule
 *   (call site std:1309-1320; kernel fla:ops/gated_delta_rule/fused_recurrent.py:21-112).
 * Per token: S *= exp(g); d = beta*(v - S^T k); S += k d^T; o = S^T (q*scale); l2norm(q), l2norm(k)
 * first when use_qk_l2norm != 0 (eps 1e-6, result rounded to bf16 like fla's l2norm_fwd).
 * h0 (may be NULL = zeros) and ht (may be NULL = not stored) are [B,H,K,V] in h0_dtype/ht_dtype
 * (IVL_F32 or IVL_BF16); ht may alias h0 (in-place state update: each element is read once, then
 * written once by the same thread).  Requires K == 128, V % 64 == 0.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_gdn_recurrent_fwd(const void* q, const void* k, const void* v, const float* g, const void* beta,
                          void* o, const void* h0, int h0_dtype, void* ht, int ht_dtype,
                          int B, int T, int H, int K, int V, float scale, int use_qk_l2norm, void* stream);
/* The same rule on IEEE-half activations (q, k, v, beta, o fp16; g fp32; the state in its own dtype): fla's operators take fp16 as
 * well as bf16 (fla:ops/gated_delta_rule/chunk.py:352 refuses fp32 only).  The package serves BOTH GDN operators with it when
 * handed fp16 tensors -- fp32 arithmetic on the fp16 inputs, token by token, whatever T: the function the chunkwise form
 * evaluates, without that form's intermediate roundings (the MFMA kernels of the chunk path are bf16 / e4m3 only). */
IVL_API int ivl_gdn_recurrent_f16_fwd(const void* q, const void* k, const void* v, const float* g, const void* beta,
                              void* o, const void* h0, int h0_dtype, void* ht, int ht_dtype,
                              int B, int T, int H, int K, int V, float scale, int use_qk_l2norm, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gated DeltaNet, chunkwise form (chunk = 64 tokens).
 * Replaces fla.ops.gated_delta_rule.chunk_gated_delta_rule (call site std:1297-1308;
 *   fla:ops/gated_delta_rule/chunk.py:18-71 = l2norm + cumsum + WY transform + state scan + output,
 *   kernels K1-K6 of SURVEY.md section 2.1) with two launches: a chunk-parallel pre-pass and a fused
 *   state-scan + output pass (the per-chunk state snapshots never reach HBM).
 * `workspace` holds the pre-pass results; size from ivl_gdn_chunk_workspace_bytes.
 * Requires K == 128, V == 256 (the InfiniteVL head shape), any T >= 1 (zero-padded last chunk).
 * mma_dtype = IVL_BF16: the reference's precision (bf16 operands at the reference's rounding points, fp32 accumulation).
 * mma_dtype = IVL_FP8_E4M3 (BASELINE.json configs[4]; the reference has no such path): the four products of the serial
 *   pass (w S, q S, k^T v_new, A v_new) take e4m3 operands -- w e^gamma, q_hat, k_hat e^{gl-gamma}, A, the state and v_new
 *   are rounded to e4m3 (clamped to +-448) -- with fp32 accumulators, fp32 carried state and bf16 u / o: half the LDS and
 *   L2 operand traffic of the scan.  Tolerance: tests/test_gpu_parity.py (fp8 section).
 * ------------------------------------------------------------------------------------------- */
IVL_API size_t ivl_gdn_chunk_workspace_bytes(int B, int T, int H, int K, int V);
IVL_API int ivl_gdn_chunk_fwd(const void* q, const void* k, const void* v, const float* g, const void* beta,
                      void* o, const void* h0, int h0_dtype, void* ht, int ht_dtype,
                      int B, int T, int H, int K, int V, float scale, int use_qk_l2norm, int mma_dtype,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Chunked gated delta rule WITH its front end, from the mixer's single projection buffer: the three causal short
 * convolutions (+SiLU, carry-in from / carry-out to the conv states) and the gate math run inside the chunk-parallel
 * pre-pass, so q / k / v / g / beta never reach HBM and ivl_gdn_prologue_fwd's launch disappears.
 * Replaces std:1253-1283 (q/k/v_conv1d), std:1293-1294 (beta, g) and std:1299-1323 (chunk_gated_delta_rule with
 *   use_qk_l2norm_in_kernel=True) of Qwen3NextGatedDeltaNet.forward in one call; bit-identical to ivl_gdn_prologue_fwd
 *   followed by ivl_gdn_chunk_fwd (same arithmetic, same bf16 rounding points).
 * proj bf16 [B*T, ld]; col_q / col_k / col_v = first column of head 0 of the q / k / v blocks ([H*K], [H*K], [H*V]),
 * col_a / col_b = first column of the a / b gate inputs ([H]); conv taps wq / wk / wv bf16 [D, 1, 4]; conv states
 * [B, D, 4] bf16 (in: NULL = zero history; out: NULL = not wanted; out may alias in).  The rest as ivl_gdn_chunk_fwd
 * (q/k l2norm always on, as the reference calls it).
 * `sync` (optional, NULL = always two launches): IVL_GDN_SYNC_BYTES of device memory, 16-byte aligned, that the CALLER
 *   zeroed (hipMemset or ivl_gdn_sync_reset) before its first use and that nothing but this library has written since; ONE
 *   AREA PER STREAM of concurrent calls.  With it the call runs as ONE launch per 4096-token segment whenever the grid can
 *   be resident at once (occupancy query x CU count; ivl_gdn_resident_blocks overrides it, 0 = always two
 *   launches) and B*H <= 32:
 *     - B*H*(T/64 + 8) workgroups fit (the 256-token streaming step): pre-pass and scan workgroups side by side, the scan
 *       waiting on flags in this area; with room for twice the pre-pass workgroups the pre-pass is split in a k and a q side;
 *     - longer calls, when the device holds 2 * 8*B*H workgroups: persistent pre-pass workgroups in front of the scan
 *       workgroups, the scan consuming the records chunk by chunk as they are published.
 *   The launch clears its flags again (all-zero between launches: replayable from a hipGraph).  Results are bit-identical to
 *   the two-launch form.  Contract of the in-launch waits (csrc/gdn_chunk.hip, scan_wait_records): a workgroup only waits for
 *   workgroups with lower block ids; every wait is bounded; a wait that runs out raises a sticky error word in the area and in
 *   a host-visible status word, and the waiting workgroup stores NO output / state computed from records it has not seen.
 *   After that this entry point returns IVL_ERR_SYNC for every call with THAT sync area (and launches nothing) until
 *   ivl_gdn_sync_reset of the area; calls with other areas -- other streams, other graphs -- go on (an area reports into
 *   its own host status slot: the 64 most recently used area addresses of a device own a slot each, and a failed area never loses
 *   its slot); workgroups of launches already queued (a hipGraph) stop at once when they find
 *   the area failed.
 * ------------------------------------------------------------------------------------------- */
#define IVL_GDN_SYNC_BYTES 16384
IVL_API int ivl_gdn_chunk_fused_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_a, int col_b,
                            const void* wq, const void* wk, const void* wv, const void* sq_in, const void* sk_in,
                            const void* sv_in, void* sq_out, void* sk_out, void* sv_out, const float* A_log,
                            const float* dt_bias, void* o, const void* h0, int h0_dtype, void* ht, int ht_dtype, int B,
                            int T, int H, int K, int V, int conv_width, float scale, int mma_dtype, void* workspace,
                            size_t workspace_bytes, void* sync, void* stream);
/* ivl_gdn_chunk_fused_fwd with A TOKEN COUNT PER BATCH ROW: row b takes the first n_b = clamp(n_rows[b], 0, T) tokens of its T rows
 * of proj and nothing else of them touches its states.  n_rows: device int32 [B], never read on the host (each workgroup reads its
 * row's count as it starts).  Scope: mma_dtype IVL_BF16, K = 128, V = 256, conv width 4, one segment (T <= 4096), states updated in
 * place (each s*_out and ht aliases its input -- ht with h0's dtype -- or is NULL); other shapes IVL_ERR_UNSUPPORTED, other
 * arguments IVL_ERR_INVALID_ARG.  Always the two-launch form (no sync area: a workgroup that has left is never waited for).
 * n_rows == NULL: the call IS ivl_gdn_chunk_fused_fwd with sync = NULL, same kernels, same bits.
 *   RAG-1 for every row b, o[b, :n_b], the recurrent state and the three conv states (also for n_b of 1, 2 or 3, where old and new
 *         inputs mix in a conv state) are bit-equal to row b of ivl_gdn_chunk_fused_fwd(sync = NULL) on the same arguments with the
 *         same B and T = n_b.
 *   RAG-2 a row depends on its own first n_b tokens only.  Tokens t >= n_b of proj are never read (they may hold NaN); o[b, n_b:] is
 *         unspecified; what other rows hold, or how long they are, changes no bit of row b.
 *   RAG-3 for n_b = 0 no byte the row owns is written and none is read (its states may hold NaN).
 *   RAG-4 the counts are read when the launch RUNS: one captured call serves every tick, the same bits eager or replayed. */
IVL_API int ivl_gdn_chunk_fused_rows_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_a, int col_b,
                                 const void* wq, const void* wk, const void* wv, const void* sq_in, const void* sk_in,
                                 const void* sv_in, void* sq_out, void* sk_out, void* sv_out, const float* A_log,
                                 const float* dt_bias, void* o, const void* h0, int h0_dtype, void* ht, int ht_dtype, int B,
                                 int T, int H, int K, int V, int conv_width, float scale, int mma_dtype, void* workspace,
                                 size_t workspace_bytes, const int32_t* n_rows, void* stream);
/* Status of the single-launch forms on the CURRENT device: IVL_OK or IVL_ERR_SYNC (ivl_last_error(): which wait, head, chunk).
 * sync == NULL: what the kernels of ANY area have reported so far through the host-visible status slots -- no stream work,
 *   callable at any time, also during capture (a failure shows up once the failing kernel has run: check after a
 *   synchronisation point).
 * sync != NULL: that area's slot, and additionally the area's own error word copied back behind `stream` (blocking; not capturable).
 * ivl_gdn_sync_reset zeroes the area behind `stream` and clears the area's status slot (also the way to initialise an area). */
IVL_API int ivl_gdn_sync_status(const void* sync, void* stream);
IVL_API int ivl_gdn_sync_reset(void* sync, void* stream);
/* The number of single-launch workgroups the library takes to be resident at once on the current device (occupancy query x CU
 * count: 256 on a whole MI355X).  override_blocks >= 0 replaces it process-wide -- 0 = always the two-launch form, a small
 * number = a partitioned / shared device; < 0 restores the query; IVL_GDN_RESIDENT_QUERY changes nothing (a pure read).  Returns
 * the number in force. */
#define IVL_GDN_RESIDENT_QUERY (-2147483647 - 1)
IVL_API int ivl_gdn_resident_blocks(int override_blocks);

/* ---------------------------------------------------------------------------------------------
 * Gate math: beta = sigmoid(b) (bf16), g = -exp(A_log) * softplus(a + dt_bias) (fp32).
 * Replaces the torch glue at std:1293-1294.  a,b bf16 [rows,H] (a_proj / b_proj outputs);
 * A_log, dt_bias fp32 [H].
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_gdn_gate_fwd(const void* a, const void* b, const float* A_log, const float* dt_bias,
                     float* g, void* beta, int rows, int H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Causal depthwise short convolution (+ optional SiLU) with state carry-in.
 * Replaces fla.modules.ShortConvolution.forward / .step (call sites std:1263-1280;
 *   fla:modules/convolution.py:195-293; CUDA ext causal_conv1d_fn / causal_conv1d_update).
 * x,y bf16 [B,T,D]; weight bf16 [D,W] (W == 4); state [B,D,W] bf16 = last W raw inputs, newest
 * last.  state_in == NULL means zero history; state_out == NULL means "do not store";
 * state_out may alias state_in.  T == 1 is the decode step.  D % 8 == 0.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_short_conv_fwd(const void* x, const void* weight, const void* state_in, void* y, void* state_out,
                       int B, int T, int D, int W, int apply_silu, void* stream);
/* The same with fla's `bias=True` option (fla:modules/convolution.py:128-160; InfiniteVL uses conv_bias = False): bias bf16 [D]
 * (NULL = none); y = act(bias + sum_j w[.,j] x[t - W + 1 + j]), the accumulator starting from the bias as in causal_conv1d. */
IVL_API int ivl_short_conv_bias_fwd(const void* x, const void* weight, const void* bias, const void* state_in, void* y, void* state_out,
                            int B, int T, int D, int W, int apply_silu, void* stream);

/* ---------------------------------------------------------------------------------------------
 * y = rmsnorm(x) * weight * gate * sigmoid(gate), rows of N == 256, statistics in fp32.
 * Replaces fla.modules.FusedRMSNormGated.forward (call site std:1338;
 *   fla:modules/fused_norm_gate.py:27-95).  x, gate, y bf16 [rows,N]; weight bf16 [N].
 * gate == NULL: y = rmsnorm(x) * weight with fla's rounding (x * rstd * w in fp32, one rounding at the store) =
 *   fla.modules.RMSNorm.forward (fla:modules/layernorm.py:103-143), the mixer's output norm when use_gate=False (std:1213).
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_rmsnorm_swish_gate_fwd(const void* x, const void* gate, const void* weight, void* y,
                               int rows, int N, float eps, void* stream);
/* The same with fla's residual= / prenorm= / residual_in_fp32= options (fla:modules/fused_norm_gate.py:54-60, 98-155; not used by
 * InfiniteVL): the row is x + residual in fp32 (residual [rows,N] IVL_BF16 or IVL_F32; NULL = none), written to residual_out
 * ([rows,N] IVL_BF16 or IVL_F32; NULL = not wanted); statistics and output are those of the unrounded fp32 row. */
IVL_API int ivl_rmsnorm_swish_gate_res_fwd(const void* x, const void* gate, const void* weight, const void* residual, int residual_dtype,
                                   void* residual_out, int residual_out_dtype, void* y, int rows, int N, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multimodal rotary embedding applied in place to q [B,T,Hq,d] and k [B,T,Hkv,d] (bf16,
 * contiguous time-major, i.e. the projection outputs before the reference's transpose).
 * Replaces apply_multimodal_rotary_pos_emb (std:949-984, call site std:1057-1064).
 * cos,sin bf16 [3,B,T,d] as produced by InfiniteVLRotaryEmbedding (std:918-930); sections s0,s1,s2
 * (sum == d/2) pick the t/h/w table per channel block.  Products and the sum are each rounded to
 * bf16 like the reference's eager bf16 arithmetic (bit-identical result).
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_mrope_fwd(void* q, void* k, const void* cos, const void* sin,
                  int B, int T, int Hq, int Hkv, int d, int s0, int s1, int s2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window attention over (ring-buffer cache ++ new tokens), GQA, d == 128.
 * Replaces ALL_ATTENTION_FUNCTIONS["flash_attention_2"] (call site std:1092-1108) together with
 * the torch.cat cache maintenance of StaticSlidingWindowLayerPrealloc.update (std:126-173).
 *
 * Query row i of the call (absolute position pos+i) sees call-local keys
 *     lo(i) = max(0, n_prev + i - window + 1) .. hi(i) = n_prev + i          (inclusive),
 * where n_prev = min(cache_capacity, pos) cached keys precede the T new ones.
 * Cached token with absolute position p lives in ring slot p % cache_capacity.
 *
 * All strides are in ELEMENTS.  k_new/v_new hold `T_new` >= T keys; when T_new > T the first
 * T_new - T of them are additional already-seen keys in chronological order (this is how the
 * operator-level call with a concatenated full_k/full_v is expressed: k_cache = NULL,
 * T_new = S).  `pos` = tokens seen before this call; when pos_dev != NULL the kernels read the value
 * from device memory instead (one hipGraph then serves every step).
 * Workspace (split-KV partials): ivl_swa_workspace_bytes.
 * ------------------------------------------------------------------------------------------- */
typedef struct ivl_swa_args {
  const void* q;            /* bf16, element (b,t,h,:) at q + b*q_sb + t*q_st + h*q_sh            */
  const void* k_new;        /* bf16, element (b,j,hk,:) at k_new + b*kn_sb + j*kn_st + hk*kn_sh  */
  const void* v_new;        /* same strides as k_new                                              */
  const void* k_cache;      /* bf16 ring [B,Hkv,cache_capacity,d] contiguous, or NULL            */
  const void* v_cache;
  void* o;                  /* bf16 [B,T,Hq,d] contiguous                                          */
  int64_t q_sb, q_st, q_sh;
  int64_t kn_sb, kn_st, kn_sh;
  int B, T, T_new, Hq, Hkv, d;
  int cache_capacity;       /* C (= window-1 in the reference's cache); 0 when k_cache == NULL     */
  int window;               /* W; <= 0 means plain causal                                          */
  int64_t pos;              /* tokens seen before this call (ignored when pos_dev != NULL)         */
  const int64_t* pos_dev;   /* optional device scalar                                              */
  float scaling;
  void* workspace;
  size_t workspace_bytes;
  const void* rope_cos;     /* optional fused M-RoPE (std:949-984): cos / sin tables bf16 [3,B,T,d] as produced by  */
  const void* rope_sin;     /* InfiniteVLRotaryEmbedding; q and k_new are then the UN-rotated projections and are rotated while   */
  int rope_s0, rope_s1;     /* they are loaded (bit-identical to ivl_mrope_fwd).  Needs T_new == T; sections s0|s1|rest, multiples */
                            /* of 8.  NULL: q / k_new are already rotated.                                                         */
  int mma_dtype;            /* IVL_BF16 (the reference's precision) or IVL_FP8_E4M3: the single-token decode step
                               (T * Hq/Hkv <= 64 packed rows) rounds q, K, V and the probabilities to e4m3 for the two
                               products (BASELINE.json configs[4]); longer calls always run in bf16                  */
  int append_new;           /* != 0: after the attention, also append the call's T tokens to the ring (what ivl_swa_cache_append
                               does, same rope arguments) - inside the split-KV combine launch when there is one, so that a
                               layer costs one launch less.  Needs a ring cache and T_new == T.                      */
  int64_t pos_min;          /* a lower bound of the position the CALLER guarantees (0: none).  The position itself may live in
                               device memory (pos_dev), but a long call over a FULL ring (pos_min >= cache_capacity, window ==
                               cache_capacity + 1, T a multiple of 256, >= 256 workgroups of 256 rows, workspace of
                               ivl_swa_ring256_workspace_bytes) takes the 256-row form: the pre-pass lays the ring out in
                               chronological order in front of the call's keys (and appends), the attention kernel has no
                               ring / band arithmetic in its steady state.  Never set it for a call recorded into a graph that
                               may be replayed from an earlier position.                                                  */
} ivl_swa_args;

IVL_API size_t ivl_swa_workspace_bytes(int B, int T, int Hq, int d);
/* Workspace of the 256-row form of a long call over a full ring (see ivl_swa_args.pos_min); 0: the shape does not qualify. */
IVL_API size_t ivl_swa_ring256_workspace_bytes(int B, int T, int Hq, int Hkv, int d, int cache_capacity);
IVL_API int ivl_swa_fwd(const ivl_swa_args* args, void* stream);
/* The packed decode step of ivl_swa_fwd with ONE RING POSITION PER BATCH ROW (independent streams in the rows of one
 * cache).  pos_rows: device int64[B]; row b attends exactly as ivl_swa_fwd does at pos = pos_rows[b] (n_ring =
 * min(pos_rows[b], C), key 0 in ring slot (pos_rows[b] - n_ring) mod C, same band), and with append_new its tokens go to
 * slots (pos_rows[b] + t) % C.  args->pos, pos_dev and pos_min are ignored; pos_rows is never written (advancing the
 * positions is the caller's job).  Scope: a ring cache, T_new == T, T * Hq/Hkv <= 64, mma_dtype IVL_BF16; fused rope and
 * append_new as in ivl_swa_fwd.  Workspace: ivl_swa_workspace_bytes(B, T, Hq, d).  Two launches (split-KV attention, then the
 * combine with the append folded in), with the split count of ivl_swa_fwd: a row's output and ring are bit-identical to a
 * B = 1 ivl_swa_fwd of that row.  Other shapes: IVL_ERR_UNSUPPORTED; NULL pos_rows: IVL_ERR_INVALID_ARG. */
IVL_API int ivl_swa_decode_rows_fwd(const ivl_swa_args* args, const int64_t* pos_rows, void* stream);
/* ivl_swa_fwd with ONE RING POSITION PER BATCH ROW for every T >= 1: a T-token frame for each of B independent streams in one call.
 * pos_rows: device int64[B], never written.  args->pos, pos_dev and pos_min are ignored; the 256-row form of a full ring is never
 * taken.  Scope: a ring cache, T_new == T, mma_dtype IVL_BF16; fused rope and append_new as in ivl_swa_fwd.  Workspace:
 * ivl_swa_workspace_bytes(B, T, Hq, d).  The launch plan is ivl_swa_fwd's for the same B, T, Hq, Hkv, window and capacity (form,
 * split count, rope pre-pass, combine with the append folded in; the stand-alone append launch when there is one split): packed
 * shapes (T * Hq/Hkv <= 64) run the launches of ivl_swa_decode_rows_fwd, T <= 64 the 64-row kernel, longer calls the 128-row kernel,
 * each reading pos_rows[b] where its twin reads the scalar position.
 *   ROWS-1 row b's rows of o and its ring row are bit-equal to row b of ivl_swa_fwd on the same arguments with every row at
 *          pos = pos_rows[b].
 *   ROWS-2 a row depends on its own row only (its q, keys, ring row and position): what the other rows hold changes no bit of it.
 *   ROWS-3 the positions are read when the launch RUNS: one captured call serves every step, the same bits eager or replayed.
 *   ROWS-4 with append_new and T > cache_capacity only the last cache_capacity tokens of a row reach its ring, as in ivl_swa_fwd.
 * Refusals are ivl_swa_decode_rows_fwd's minus the packing rule. */
IVL_API int ivl_swa_rows_fwd(const ivl_swa_args* args, const int64_t* pos_rows, void* stream);
/* ivl_swa_rows_fwd with A TOKEN COUNT PER BATCH ROW: row b brings n_b = clamp(n_rows[b], 0, T) tokens, the first n_b of its T.  n_rows:
 * device int32 [B], never read on the host.  Same arguments, same rules, same launch plan (which reads no length); n_rows == NULL IS
 * ivl_swa_rows_fwd.  Scope: the unpacked forms, T * Hq/Hkv > 64 (a packed shape is IVL_ERR_UNSUPPORTED: the decode step has its hold
 * twin).  Causality keeps a query t < n_b from the keys of tokens >= n_b, so the valid rows attend as before; what changes: with
 * append_new only tokens t < n_b go to slots (pos_rows[b] + t) % C (the last C of them when n_b > C); query tiles wholly at or beyond
 * n_b, and their rows of the merge, do nothing.
 *   RAG-5  o[b, :n_b] is bit-equal to ivl_swa_rows_fwd on the same arguments with ZEROS in q, k_new and v_new at the tokens t >= n_b
 *          (which is what the kernels compute, without reading them; with other finite values there the 128-row kernel of
 *          ivl_swa_rows_fwd may move a row's lazily updated softmax reference when a neighbouring row of its wavefront outgrows its
 *          own -- the same value up to the rounding of the rescale).  o[b, n_b:] is unspecified.
 *   RAG-6  row b's ring row is bit-equal to its ring row after ivl_swa_rows_fwd with T = n_b (rope tables of the same positions).
 *   RAG-7  with n_b = 0 no byte of the row's ring row is written or read.
 *   RAG-8  pos_rows is never written.
 *   RAG-9  q / k_new / v_new at t >= n_b and unread ring slots may hold NaN.
 *   RAG-10 the counts are read when the launch RUNS: one captured call serves every tick, the same bits eager or replayed. */
IVL_API int ivl_swa_rows_n_fwd(const ivl_swa_args* args, const int64_t* pos_rows, const int32_t* n_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-row HOLD of a multi-stream step.  `frozen`: device int32 [B], read when the launch RUNS (at replay); row b is frozen when
 * frozen[b] != 0.  frozen == NULL means "no row is frozen": the call IS its twin without the argument, same kernels, same bits.
 * The three entry points that take it -- ivl_gdn_decode_step_rows_fwd, ivl_swa_decode_rows_hold_fwd, ivl_rows_advance_fwd -- keep:
 *   HOLD-1 a frozen row is untouched.  No byte of what the row owns is written: its GDN recurrent state, its three conv states, its
 *          K / V ring row, pos_rows[b], its three M-RoPE positions.  Nothing of it needs to be read (it may hold NaN or inf).  The
 *          outputs of that row (y, o, and the logits computed from them) are unspecified.
 *   HOLD-2 running rows do not notice.  Every output and every state byte of a running row is bit-equal to the same call with
 *          frozen == NULL, and so to the call in which the frozen rows hold anything at all (a row depends on its own row only).
 *   HOLD-3 graph.  The mask is read on the device; changing it between replays of a captured call needs no recapture, and the same
 *          bits result eager or replayed.
 * The sampling launch's `done` (int32 [S]) has exactly this layout: a decoder may pass it as the mask, so that a row that ends (codes
 * 1, 2, 3) freezes on the next replay with no host involved; code 4 is "held by the host" (to the sampling kernels: a finished row).
 * ------------------------------------------------------------------------------------------- */
/* ivl_swa_decode_rows_fwd with the hold mask: same scope, argument rules, split count, grids and merge.  The attention workgroups
 * of a frozen row leave at once, its combine blocks skip the merge and the o store, and with append_new its slots
 * (pos_rows[b] + t) % C are not written. */
IVL_API int ivl_swa_decode_rows_hold_fwd(const ivl_swa_args* args, const int64_t* pos_rows, const int32_t* frozen, void* stream);

/* The counters of a multi-stream step, one launch: pos_rows[s] += delta (int64 [S]) and position_ids[a * pid_stride + s] += delta
 * for a = 0, 1, 2 (int64 [3, S], row stride pid_stride >= S) where row s runs.  Either pointer may be NULL (that counter is left
 * alone).  S < 1 or pid_stride < S: IVL_ERR_INVALID_ARG. */
IVL_API int ivl_rows_advance_fwd(int64_t* pos_rows, int64_t* position_ids, int64_t pid_stride, const int32_t* frozen, int S,
                                 int64_t delta, void* stream);

/* Append the T new tokens to the ring (slot (pos+t) % C) -- after ivl_swa_fwd of the same call.
 * Replaces the tail copy-back of std:146-172.  k_new,v_new bf16 with the strides given.  With rope_cos / rope_sin
 * (same meaning as in ivl_swa_args) the keys are rotated on the way into the ring. */
IVL_API int ivl_swa_cache_append(const void* k_new, const void* v_new, int64_t kn_sb, int64_t kn_st, int64_t kn_sh,
                         void* k_cache, void* v_cache, int B, int T, int Hkv, int d, int cache_capacity,
                         int64_t pos, const int64_t* pos_dev, const void* rope_cos, const void* rope_sin,
                         int rope_s0, int rope_s1, void* stream);

/* 3-D rotary tables cos / sin bf16 [rows, 2*half_dim] from position ids (int64 [rows], rows = 3*B*T in (axis, batch,
 * token) order) and the inverse frequencies fp32 [half_dim]: cos(pos * inv_freq) in fp32, the frequencies repeated over
 * both halves of the channels, times attention_scaling, rounded to bf16.
 * Replaces InfiniteVLRotaryEmbedding.forward (std:896-930: cast, K=1 matmul, cat, cos, sin, scaling, cast) with one launch. */
IVL_API int ivl_rope_tables_fwd(const int64_t* position_ids, const float* inv_freq, void* cos_out, void* sin_out, int rows,
                        int half_dim, float attention_scaling, void* stream);

/* Vision-tower window attention: NON-causal softmax attention inside each segment
 * [cu_seqlens[s], cu_seqlens[s+1]) of one packed patch sequence, with the vision rotary embedding folded into the Q / K
 * loads.  Replaces apply_rotary_pos_emb_vision (strm:657-671) + the per-window attention_interface loop / the
 * flash-attention varlen call of InfiniteVLVisionAttention.forward (strm:752-796 = std:623-664).
 *   q, k, v : bf16, token t / head h at element offset t * x_st + h * x_sh (the three slices of the fused qkv projection
 *             output [S, 3, H, d] are passed without a copy); o : bf16 with its own strides ([S, H, d] contiguous for proj)
 *   cu_seqlens : device int32 [n_seg + 1], ascending, cu_seqlens[0] = 0 (strm:1076-1077); never read on the host
 *   max_seqlen : an upper bound of the segment lengths (the grid is sized from it; longer segments are NOT processed)
 *   d          : head_dim, 64 / 80 / 128 built (80 = the 3B vision tower: 1280 / 16)
 *   rope_cos, rope_sin : fp32 [S, d] (emb.cos(), emb.sin() of strm:1073-1074) or both NULL when q, k are already
 *             rotated; the rotation is done in fp32 with separately rounded products and sum, rounded to bf16 once:
 *             bit-identical to the reference's eager arithmetic.
 *   S          : number of tokens (patches) in the packed sequence
 *   workspace  : ivl_vision_attn_workspace_bytes(S, H, d, max_seqlen) bytes (0 when max_seqlen <= 64) or NULL.  With rope
 *             tables and segments longer than one 64-row query tile, the keys are rotated ONCE into it by a pre-pass;
 *             without it the rotation is redone in every query tile's loads (same results, slower).
 * Scores and the softmax statistics are fp32, the probabilities are rounded to bf16 for the PV product, fp32 accumulation. */
IVL_API size_t ivl_vision_attn_workspace_bytes(int S, int H, int d, int max_seqlen);
IVL_API int ivl_vision_attn_fwd(const void* q, const void* k, const void* v, void* o,
                        int64_t q_st, int64_t q_sh, int64_t k_st, int64_t k_sh, int64_t v_st, int64_t v_sh,
                        int64_t o_st, int64_t o_sh, const int32_t* cu_seqlens, int n_seg, int max_seqlen,
                        int S, int H, int d, float scaling, const float* rope_cos, const float* rope_sin,
                        void* workspace, size_t workspace_bytes, void* stream);

/* *counter += delta on the device (graph-replayable position bookkeeping). */
IVL_API int ivl_counter_add(int64_t* counter, int64_t delta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused prologue / epilogue entry points: the same arithmetic as the
 * single-purpose entry points above, but reading the column blocks of ONE fused projection output
 * (row stride `ld` elements) so that a Gated DeltaNet layer needs one projection GEMM and one
 * prologue launch instead of six GEMMs + 3 conv + gate launches (call sites std:1261-1294).
 * ------------------------------------------------------------------------------------------- */

/* 3 short convs (+SiLU, carry-in, state in/out as in ivl_short_conv_fwd) + gate math (ivl_gdn_gate_fwd).
 * proj bf16 [B*T, ld]; q|k|v|a|b start at columns col_*; outputs q [B,T,Dq], k [B,T,Dk], v [B,T,Dv] bf16
 * contiguous, g fp32 [B,T,H], beta bf16 [B,T,H]. */
IVL_API int ivl_gdn_prologue_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_a, int col_b,
                         const void* w_q, const void* w_k, const void* w_v,
                         const void* sq_in, const void* sk_in, const void* sv_in,
                         void* sq_out, void* sk_out, void* sv_out,
                         const float* A_log, const float* dt_bias,
                         void* q, void* k, void* v, float* g, void* beta,
                         int B, int T, int H, int Dq, int Dk, int Dv, int W, int apply_silu, void* stream);

/* ivl_rmsnorm_swish_gate_fwd with the gate read in place: gate element (token, head, c) at
 * gate + token*gate_ld + head*N + c; x,y [rows = tokens*H, N] contiguous. */
IVL_API int ivl_rmsnorm_swish_gate_strided_fwd(const void* x, const void* gate, int64_t gate_ld, int H,
                                       const void* weight, void* y, int rows, int N, float eps, void* stream);

/* ivl_mrope_fwd on column blocks of a fused qkv projection: q element (b,t,h,c) at
 * q + (b*T+t)*q_ld + h*d + c, k likewise with k_ld. */
IVL_API int ivl_mrope_strided_fwd(void* q, void* k, int64_t q_ld, int64_t k_ld, const void* cos, const void* sin,
                          int B, int T, int Hq, int Hkv, int d, int s0, int s1, int s2, void* stream);

/* Decoder-layer norm (std:1400-1420 / Qwen2RMSNorm) fused with the residual add:
 *   h = bf16(x + residual) -> h_out   (skipped when residual == NULL: h = x)
 *   y = bf16(weight * bf16(h * rsqrt(mean(h^2) + eps)));  x,residual,y,h_out bf16 [rows,N], N%8==0, N<=8192. */
IVL_API int ivl_add_rmsnorm_fwd(const void* x, const void* residual, const void* weight, void* y, void* h_out,
                        int rows, int N, float eps, void* stream);

/* SwiGLU gate over a fused gate|up projection: y[r,i] = bf16(bf16(silu(gu[r,i])) * gu[r,I+i]) (std:945). */
IVL_API int ivl_silu_mul_fwd(const void* gate_up, void* y, int64_t rows, int I, void* stream);

/* Gated DeltaNet mixer core for ONE new token per sequence (GatedDeltaNet.forward, std:1215-1347, q_len == 1):
 * = ivl_gdn_prologue_fwd + ivl_gdn_recurrent_fwd(use_qk_l2norm=1) + ivl_rmsnorm_swish_gate_strided_fwd in one launch,
 * same rounding points.  proj [B, ld] bf16 is the fused projection row (columns col_q|col_k: H*128 each, col_v|col_g:
 * H*256 each, col_a|col_b: H each); conv weights [D,4] bf16; conv states [B,D,4] bf16 and the recurrent state
 * [B,H,128,256] (IVL_F32 / IVL_BF16) are updated IN PLACE; y [B, H*256] bf16 is the gated-norm output (o_proj input). */
IVL_API int ivl_gdn_decode_step_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_g, int col_a,
                            int col_b, const void* conv_wq, const void* conv_wk, const void* conv_wv,
                            void* conv_state_q, void* conv_state_k, void* conv_state_v, const float* A_log,
                            const float* dt_bias, const void* norm_weight, float eps, void* state, int state_dtype,
                            void* y, int B, int H, int K, int V, float scale, void* stream);

/* ivl_gdn_decode_step_fwd with the hold mask (HOLD-1..3 above): the workgroups of a frozen row leave before their first state load;
 * the row's recurrent state and conv states are neither read nor written and its y is not written.  Same argument rules. */
IVL_API int ivl_gdn_decode_step_rows_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_g, int col_a,
                            int col_b, const void* conv_wq, const void* conv_wk, const void* conv_wv,
                            void* conv_state_q, void* conv_state_k, void* conv_state_v, const float* A_log,
                            const float* dt_bias, const void* norm_weight, float eps, void* state, int state_dtype,
                            void* y, int B, int H, int K, int V, float scale, const int32_t* frozen, void* stream);

/* The same step on 4 x as many workgroups (round 5): a workgroup = (sequence, head, quarter of the 256 value columns); the delta
 * rule is column-local, so the quarters exchange nothing.  What spans a head moves into the NEXT launch
 * (ivl_gdn_out_linear_small_m_fwd, the o_proj weight stream): the gated RMSNorm, and the shift of the q / k conv states (every
 * quarter reads them).  Here: conv states of q and k are READ ONLY, the v conv state and the recurrent state are updated in
 * place, o_raw [B, H*256] bf16 receives the delta rule's UN-NORMALISED output (the bf16 rounding point of the recurrent kernel).
 * ivl_gdn_decode_split_fwd + ivl_gdn_out_linear_small_m_fwd == ivl_gdn_decode_step_fwd + ivl_linear_small_m_fwd, bit for bit
 * (outputs, recurrent state, all three conv states).  Replaces std:1241-1342 at q_len == 1. */
IVL_API int ivl_gdn_decode_split_fwd(const void* proj, int64_t ld, int col_q, int col_k, int col_v, int col_a, int col_b,
                             const void* conv_wq, const void* conv_wk, const void* conv_wv, const void* conv_state_q,
                             const void* conv_state_k, void* conv_state_v, const float* A_log, const float* dt_bias,
                             void* state, int state_dtype, void* o_raw, int B, int H, int K, int V, float scale, void* stream);
/* y[M,N] = bf16(o_norm(o_raw, gate)[M, H*256] W[N, H*256]^T + bias): the GDN output projection of a decode step (std:1336-1342)
 * with FusedRMSNormGated (fla:modules/fused_norm_gate.py:778-796; 256-wide heads, eps) in the prologue of the weight stream.
 * gate = first gate element of row 0 of the fused projection (row stride gate_ld elements); norm_weight bf16 [256].  Also shifts
 * the conv states [M, H*128, 4] of q and k by the step's raw projection values (proj + col_q / col_k, row stride proj_ld): the
 * second half of ivl_gdn_decode_split_fwd's state update.  M <= 4, 2 <= H <= 16 (IVL_ERR_UNSUPPORTED otherwise: at H = 1 half of
 * every wave would skip the weight loop whose first trip holds the norm). */
IVL_API int ivl_gdn_out_linear_small_m_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight, float eps,
                                   int H, const void* proj, int64_t proj_ld, int col_q, int col_k, void* conv_state_q,
                                   void* conv_state_k, const void* w, const void* bias, void* y, int M, int N, int K, void* stream);

/* nn.Linear for the single-token decode step (M <= 4 rows): y[M,N] = bf16(x[M,K] W[N,K]^T + bias[N]).
 * Replaces the q/k/v/o, GDN in/out, MLP and tied lm_head projections (std:1047-1054, 1215-1240, 945, 2091-2092)
 * when q_len == 1: a pure weight stream bounded by HBM.  x,W,bias,y bf16, row-major contiguous; fp32 accumulation;
 * bias may be NULL.  K % 8 == 0.  IVL_ERR_UNSUPPORTED for M > 4 (callers use a GEMM there). */
IVL_API int ivl_linear_small_m_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, void* stream);

/* SwiGLU MLP head of a decode step (std:945: act_fn(gate_proj(x)) * up_proj(x)), fused gate|up weight [2I,K]:
 *   y[M,I] = bf16( bf16(silu(bf16(x Wg^T))) * bf16(x Wu^T) ),  Wg = w_gate_up[:I], Wu = w_gate_up[I:]
 * = ivl_linear_small_m_fwd on the fused weight followed by ivl_silu_mul_fwd, bit for bit.  bias [2I] or NULL. */
IVL_API int ivl_linear_swiglu_small_m_fwd(const void* x, const void* w_gate_up, const void* bias, void* y, int M, int I, int K,
                                  void* stream);

/* (Residual add +) RMSNorm in the prologue of the decode step's projection: ivl_add_rmsnorm_fwd followed by
 * ivl_linear_small_m_fwd (glu == 0) or ivl_linear_swiglu_small_m_fwd (glu != 0, N = I), bit for bit, in ONE launch --
 * the decoder layer's input_layernorm -> q|k|v / GDN in-projection, post_attention_layernorm -> gate|up, and the final
 * norm -> lm_head (std:1350-1429, 1573, 2091-2092) at q_len == 1.  (The package routes the 72 per-layer norms of a decode token through
 * it; the final norm in front of lm_head stays a launch of its own.)
 *   h = bf16(x + residual) (residual NULL: h = x; else written to h_out [M,K]);  xn = bf16(norm_weight * bf16(h * rstd(h)));
 *   y = linear(xn).  x, residual, h_out bf16 [M,K]; norm_weight bf16 [K]; 512 <= K <= 4096; the rest as the two entry points above. */
IVL_API int ivl_norm_linear_small_m_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream);

/* WEIGHT-ONLY E4M3: the e4m3 twins of the four decode projections above -- the same argument lists, with
 *   wq     uint8 [N,K] row-major, 16-byte aligned (GLU: [2I,K]): OCP e4m3fn codes (the gfx950 encoding, not e4m3fnuz) in place of w,
 *   scale  fp32 [N] (GLU: [2I]): one scale per weight row.
 *   y[m,n] = bf16(scale[n] * acc[m,n] + bias[n]),   acc[m,n] = the fp32 sum of float(code) * x (the decode of a code is exact).
 * The summation ORDER is that of the bf16 kernels (linear_small_m_kernel / linear_gdn_out_kernel are ONE template over the weight
 * element): per (weight row, x row) lane l of a wave adds the 8 products of chunk l + 64 i (8 elements = 8 bytes here) in element
 * order with fmaf, i ascending, from 0; pieces past the row end add fmaf(w, 0, acc); then wave_sum.  scale * acc + bias is
 * formed in fp32 (the product is exact for a power of two).  GLU, NORM and the gated norm with the conv-state shift are those of the bf16 forms;
 * the x side is untouched.
 * THE CONTRACT: with every scale[n] a power of two, each entry point equals its bf16 twin called on W' = dequantize(wq, scale)
 * (W'[n,k] = float(code) * scale[n], exact in bf16) BIT FOR BIT -- y, h_out and the conv states -- because scaling an fp32 fmaf chain
 * by a power of two commutes with every rounding in it (short of underflow / overflow).  The ABI does not check that a scale is a
 * power of two: a general scale computes the formula above and loses the equality.  No e4m3 NaN code (0x7F / 0xFF) is expected.
 * Ranges and refusals are those of the twins (M 1..4, K % 8 == 0, 512 <= K <= 4096 for NORM, 2 <= H <= 16 for the GDN form), NULL
 * scale: IVL_ERR_INVALID_ARG; every check runs before anything is launched. */
IVL_API int ivl_linear_small_m_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N,
                              int K, void* stream);
IVL_API int ivl_linear_swiglu_small_m_w8_fwd(const void* x, const void* wq_gate_up, const float* scale, const void* bias, void* y,
                                     int M, int I, int K, void* stream);
IVL_API int ivl_norm_linear_small_m_w8_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                   const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K, int glu,
                                   void* stream);
IVL_API int ivl_gdn_out_linear_small_m_w8_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight,
                                      float eps, int H, const void* proj, int64_t proj_ld, int col_q, int col_k,
                                      void* conv_state_q, void* conv_state_k, const void* wq, const float* scale,
                                      const void* bias, void* y, int M, int N, int K, void* stream);

/* WEIGHT-ONLY MXFP4: the 4-bit twins of the four decode projections -- the argument lists of the *_w8 twins, with
 *   wq   uint8 [N, Kp/2] (GLU: [2I, Kp/2]), 16-byte aligned: OCP microscaling FP4 codes (e2m1: sign, 2 exponent bits, 1 mantissa
 *        bit -- the magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6 --, two per byte, the element of the lower index in the LOW nibble),
 *   sq   uint8 [N, Kp/32] (GLU: [2I, Kp/32]), 4-byte aligned: one e8m0 scale byte b per block of 32 consecutive K elements,
 *        the scale 2^(b - 127),
 * both in the SHUFFLED layout the kernels read (below), Kp = 2048 ceil(K / 2048).  K % 32 == 0.
 *   W'[n,k] = e2m1(code[n,k]) * 2^(b[n, k/32] - 127)        (2 significant bits: exact in bf16)
 *   y[m,n]  = bf16(acc[m,n] + bias[n]),   acc[m,n] = the fp32 sum of W'[n,k] * x[m,k] in the bf16 kernels' ORDER (see the w8 twins: one
 *             template over the weight element): v_cvt_scalef32_pk_f32_fp4 decodes two codes and applies the block scale, exactly.
 * THE CONTRACT: each entry point equals its bf16 twin called on W' BIT FOR BIT -- y, h_out and the conv states.  There is no per-row
 * scale and no scaled epilogue: the block scale is part of the weight.
 * THE LAYOUT (ops.mxfp4_shuffle / mxfp4_unshuffle convert from / to plain row-major OCP, where byte j of a row holds elements 2j, 2j + 1
 * and scale byte i belongs to elements 32i .. 32i + 31).  A CHUNK is 8 consecutive K elements = 4 bytes; TILE t of a row is the chunks
 * [256t, 256t + 256) = one trip of the weight loop of a wave.  In a row of wq (Kp/2 bytes) the chunk 256t + l + 64u (l in 0..63, u in
 * 0..3) sits at byte 1024t + 16l + 4u: lane l fetches the four pieces of a trip with ONE 16-byte load, in the order it adds them.  In a
 * row of sq (Kp/32 bytes) the scale of block 64t + (l >> 2) + 16u -- the block of that chunk -- sits at byte 64t + 4(l >> 2) + u: one
 * dword per lane holds the scales of its four pieces.  Chunks and blocks past K are padding: code 0x0, scale byte 127; they meet
 * x = 0 like every piece past the row end.  A scale byte is used as the fp32 bit pattern b << 23: b = 0 and b = 255 are not expected
 * (ops.quantize_rows_mxfp4 keeps |b - 127| <= 100).
 * The exponent rule is the producer's business: ops.quantize_rows_mxfp4 takes the SMALLEST e with amax(block) <= 6 * 2^e, which never
 * saturates; the OCP reference rule, e = floor(log2 amax) - 2, is one smaller where amax > 6 * 2^e and then clamps such elements to +-6.
 * Codes made by either rule (any e8m0 in 1..254) are decoded the same way here.
 * Ranges and refusals are those of the twins, plus K % 32 == 0, wq 16-byte and sq 4-byte aligned (IVL_ERR_INVALID_ARG); NULL sq:
 * IVL_ERR_INVALID_ARG; every check runs before anything is launched. */
IVL_API int ivl_linear_small_m_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N,
                              int K, void* stream);
IVL_API int ivl_linear_swiglu_small_m_w4_fwd(const void* x, const void* wq_gate_up, const void* sq, const void* bias, void* y,
                                     int M, int I, int K, void* stream);
IVL_API int ivl_norm_linear_small_m_w4_fwd(const void* x, const void* residual, const void* norm_weight, float eps, void* h_out,
                                   const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K, int glu,
                                   void* stream);
IVL_API int ivl_gdn_out_linear_small_m_w4_fwd(const void* o_raw, const void* gate, int64_t gate_ld, const void* norm_weight,
                                      float eps, int H, const void* proj, int64_t proj_ld, int col_q, int col_k,
                                      void* conv_state_q, void* conv_state_k, const void* wq, const void* sq,
                                      const void* bias, void* y, int M, int N, int K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PER-ROW LoRA ADAPTERS on the output of a decode projection, UNMERGED: y[m] += s_a B_a (A_a x[m]) with a = adapter_idx[m] read on
 * the device, so that every row (decode slot) of a captured step follows its own fine-tune and the base weight -- bf16 or packed --
 * stays what it is.  Replaces peft's bf16 lora.Linear.forward, `result + lora_B(lora_A(x)) * scaling`, which the reference only
 * reaches merged (src/llamafactory/model/adapter.py: PeftModel.from_pretrained -> merge_and_unload), at its rounding points:
 *     t[m,j] = bf16( sum_k A_a[j,k] x[m,k] )        fp32 accumulation (lane l of a wave: the 8-element chunks l + 64 i, i ascending,
 *                                                     one fmaf per element from 0, then wave_sum)
 *     d[m,n] = bf16( sum_j B_a[n,j] t[m,j] )        fp32, one fmaf per j, j ascending from 0
 *     e[m,n] = bf16( scaling[a] * d[m,n] )          one fp32 multiply
 *     y[m,n] = bf16( y[m,n] + e[m,n] )              one fp32 add, in place
 *   x [M,K] bf16; y [M,N] bf16 in and out; adapter_idx int32 [M]; scaling fp32 [n_adapters] (alpha / r, or alpha / sqrt r).
 *   SEGMENTS: a fused weight (q|k|v, the GDN q|k|v|g|a|b, gate|up) has one adapter pair per sub-projection.  Segment i < n_seg owns
 *   the output columns [seg_col<i>, seg_col<i+1>) -- the nine fields seg_col0 .. seg_col8 are one int[9] by value, entries past
 *   n_seg unused -- and reads t[m, i R .. i R + R), R the rank capacity of the table:
 *     A bf16 [n_adapters, n_seg R, K] (the segments' A stacked), B bf16 [n_adapters, N, R] (row n = the B row of n's segment).
 *   An adapter of rank r < R is stored zero-padded: zero terms add exactly, the result is the rank-r computation bit for bit.
 *   NOT TOUCHED (no read-modify-write: -0.0 + 0.0 would flip a sign bit): every row m with adapter_idx[m] outside [0, n_adapters)
 *   -- -1 = no adapter -- and every column in no segment (below seg_col0, from seg_col<n_seg> on).
 *   NORM group (norm_weight != NULL): x is the raw input of the (residual add +) RMSNorm in front of the projection, and the
 *   kernel forms xn = bf16(norm_weight * bf16(h rstd)), h = bf16(x + residual) (residual NULL: h = x) itself, with the thread ->
 *   element mapping and summation order of ivl_add_rmsnorm_fwd / ivl_norm_linear_small_m_fwd: bit-identical rows, no norm launch.
 *   h is not written (the base launch owns h_out).  512 <= K <= 4096.
 *   t_ws: bf16 [4, 512] owned by the caller; afterwards t_ws[m*512 + j] = t[m,j] for j < n_seg R of every row WITH an adapter.
 * Two launches (shrink: one wave per two rows of A and x row; expand-add: one thread per output column); no atomics, a fixed
 * order: the same bits eager or replayed, and for a row alone or among other rows.  Everything 16-byte aligned.
 * IVL_ERR_INVALID_ARG: NULL args, x, y, adapter_idx, A, B, scaling or t_ws; a pointer off 16 bytes; N < 1, K < 8, K % 8 != 0;
 *   n_adapters < 1; n_seg outside 1..8; seg_col not non-decreasing within [0, N]; residual without norm_weight.
 * IVL_ERR_UNSUPPORTED: M outside 1..4; R not 8, 16, 32 or 64; NORM with K outside [512, 4096].  Checked before any launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct ivl_lora_args {
  const void* x; void* y; const int32_t* adapter_idx;
  const void* A; const void* B; const float* scaling;
  int M, N, K, R, n_adapters, n_seg;
  int seg_col0, seg_col1, seg_col2, seg_col3, seg_col4, seg_col5, seg_col6, seg_col7, seg_col8;
  /* NORM */
  const void* residual; const void* norm_weight; float eps;
  void* t_ws;
} ivl_lora_args;
IVL_API int ivl_lora_add_small_m_fwd(const ivl_lora_args* args, void* stream);

/* nn.Linear for the wide projections of a prefill chunk of up to 256 rows: y[M,N] = bf16(x[M,K] W[N,K]^T + bias[N]), or with
 * glu != 0 the SwiGLU MLP head on the fused gate|up weight [2N,K] (N = I):
 *   y[M,I] = bf16( bf16(silu(bf16(x Wg^T + bg))) * bf16(x Wu^T + bu) ),  Wg = w[:I], Wu = w[I:], bias [2I] or NULL
 * = the glu == 0 call on the fused weight followed by ivl_silu_mul_fwd, bit for bit.  One workgroup per column range with all rows
 * (no K split: the same bits on every run).  x, W, bias, y bf16 row-major contiguous, fp32 accumulation, one rounding.
 * 1 <= M <= 256, K % 64 == 0 and K <= 16384, N % 4 == 0, x / W 16-byte aligned: else IVL_ERR_UNSUPPORTED / IVL_ERR_INVALID_ARG. */
IVL_API int ivl_linear_m256_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream);

/* nn.Linear for a decode step of up to 16 rows (5 to 16 slots of a multi-stream step): y[M,N] = bf16(x[M,K] W[N,K]^T + bias[N]), or
 * with glu != 0 the SwiGLU MLP head on the fused gate|up weight [2N,K] (N = I), with the formula and rounding points of
 * ivl_linear_swiglu_small_m_fwd:  y[M,I] = bf16( bf16(silu(bf16(x Wg^T + bg))) * bf16(x Wu^T + bu) ),  bias [2I] or NULL.
 * A weight stream on v_mfma_f32_16x16x32_bf16: 16 weight rows are the A operand, the (zero-padded) 16 rows of x the B operand; fp32
 * accumulation, one rounding.  x, bias, y bf16 row-major contiguous.
 *   ivl_linear_m16_fwd     w  bf16 [N,K] (GLU: [2I,K]);
 *   ivl_linear_m16_w8_fwd  wq uint8 [N,K] OCP e4m3fn codes + scale fp32 [N] (GLU: [2I,K] / [2I]), W'[n,k] = bf16(float(code) * scale[n]);
 *   ivl_linear_m16_w4_fwd  wq / sq: the SHUFFLED MXFP4 layout of the *_small_m_w4 twins above, unchanged (uint8 [N,Kp/2] and [N,Kp/32],
 *                          Kp = 2048 ceil(K / 2048)), W'[n,k] = e2m1(code) * 2^(b - 127).
 * ONE SUMMATION PLAN for the three, a function of K only -- not of M, not of N, not of the format.  A chunk is 8 consecutive k;
 * step s = 16t + j (t = tile of 2048 k, j in 0..15) is four MFMAs u = 0..3 whose k-group g in 0..3 holds the chunk
 * 256t + 4j + g + 64u (chunks past K/8: zeros); the S steps that hold a chunk below K/8 are cut into 8 contiguous slices of
 * ceil(S / 8) steps, each slice is accumulated from 0 in ascending (s, u) order by one wave of the workgroup that owns the output
 * columns, and the slices are added in ascending order in fp32 in LDS; then the bias, then the rounding.
 * No split across workgroups, no atomics, one launch.  THE CONTRACTS:
 *  1. Determinism: every run gives the same bits, eager or replayed from a graph.
 *  2. Row independence: row m of y depends on row m of x only -- the same bits for every M, at every row index, whatever the other
 *     rows hold (NaN, Inf); rows >= M of the B operand are zeros, never read from x and never written to y.  Weight rows past the
 *     last are neither read nor stored.
 *  3. Packed equals bf16 on W': ivl_linear_m16_w8_fwd with power-of-two scales, and ivl_linear_m16_w4_fwd, equal ivl_linear_m16_fwd
 *     called on W' = dequantize(packed copy) bit for bit, plain and GLU: every policy hands the MFMA the bf16 bit pattern of W'
 *     (exact in bf16 for both formats).  A general e4m3 scale computes the W' above (rounded to bf16) and loses nothing but the name.
 *  4. GLU equals plain plus gate: the glu != 0 call equals the glu == 0 call on the fused weight (N = 2I) followed by
 *     ivl_silu_mul_fwd, bit for bit.
 *  5. NO bit-equality with the small-M (M <= 4) or 256-row kernels: their summation orders differ; the agreement is numerical.
 * 1 <= M <= 16 (else IVL_ERR_UNSUPPORTED); N >= 1, K >= 32 and K % 32 == 0 -- tails in N are predicated, nothing is padded by the
 * caller --, x / w (wq) / y 16-byte aligned, scale / sq 4-byte aligned, no NULL x, w, wq, scale, sq or y (else IVL_ERR_INVALID_ARG);
 * every weight offset is a 32-bit byte offset: R K 2 < 2^32 and R (bytes of a padded row) < 2^32 (else IVL_ERR_UNSUPPORTED).  Every
 * check runs before anything is launched. */
IVL_API int ivl_linear_m16_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream);
IVL_API int ivl_linear_m16_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K,
                                  int glu, void* stream);
IVL_API int ivl_linear_m16_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                  int glu, void* stream);

/* nn.Linear for a decode step of up to 64 rows (17 to 63 slots of a multi-stream step): the three entries above with the row bound
 * moved -- the same argument lists, formulas, rounding points, weight formats and layouts (the same packed copies: no new layout and
 * no second copy).  The 64 rows of x are XT = ceil(M / 16) B operands of v_mfma_f32_16x16x32_bf16; a lane's weight piece is loaded
 * and decoded to the bf16 pattern of W' once and is the A operand of all XT.
 * THE SUMMATION PLAN IS THAT OF THE 16-ROW ENTRIES, UNCHANGED: the chunks, tiles and steps s = 16t + j, the four MFMAs u = 0..3 with
 * chunk 256t + 4j + g + 64u, the 8 contiguous slices of ceil(S / 8) steps, each accumulated from 0 in ascending (s, u), the eight
 * partials added in fp32 in ascending slice order, then the bias, then the one rounding.  Which wave computes which slice of which
 * (weight tile, x tile) is a choice of speed; the value of an output element is not.  No split across workgroups, no atomics, one
 * launch, no scratch.  THE CONTRACTS:
 *  C1. Determinism: every run gives the same bits, eager or replayed from a graph.
 *  C2. Row m of an M-row call equals ivl_linear_m16_fwd / _w8_fwd / _w4_fwd called on row m alone (M = 1), bit for bit, plain and
 *      GLU: a row depends on its own row of x only -- the same bits for every M, at every row index, whatever the other rows hold
 *      (NaN, Inf).
 *  C3. Packed equals bf16 on W': contract 3 of the 16-row entries, on the same terms.
 *  C4. GLU equals plain plus gate: the glu != 0 call equals the glu == 0 call on the fused weight (N = 2I) followed by
 *      ivl_silu_mul_fwd, bit for bit.
 *  C5. Rows M .. 16 XT - 1 of the B operands are zeros: never read from x, never written to y.  Weight rows past the last are
 *      neither read nor stored.
 * 1 <= M <= 64 (else IVL_ERR_UNSUPPORTED); every other refusal is that of the 16-row entry of the same format, with the same code:
 * N >= 1, K >= 32 and K % 32 == 0, alignment, no NULL pointer (IVL_ERR_INVALID_ARG); 32-bit weight byte offsets
 * (IVL_ERR_UNSUPPORTED).  Every check runs before anything is launched.  There is no LoRA form: ivl_linear_m16_lora*_fwd stop at 16
 * rows. */
IVL_API int ivl_linear_m64_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu, void* stream);
IVL_API int ivl_linear_m64_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N, int K,
                                  int glu, void* stream);
IVL_API int ivl_linear_m64_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                  int glu, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PER-ROW LoRA ADAPTERS FOR 5 TO 16 ROWS (the args, chain, segments, rank padding and NOT TOUCHED rule of
 * ivl_lora_add_small_m_fwd above, its t order included; t_ws is bf16 [16, 512] here).
 *
 * ivl_lora_add_m16_fwd: the two-launch form (shrink on a grid of (ceil(n_seg R / 8), M), expand-add) for 1 <= M <= 16.  There is no
 * NORM group -- the 5..16-row step materialises its norms: norm_weight != NULL is IVL_ERR_UNSUPPORTED, residual without a norm
 * weight IVL_ERR_INVALID_ARG as above; M outside 1..16 is IVL_ERR_UNSUPPORTED; every other refusal is the small-M entry's, checked
 * before any launch.
 *  L1. Row m of y and of t_ws equals what ivl_lora_add_small_m_fwd writes for that row called alone (M = 1, its x row, y row and
 *      index), bit for bit: independent of M, of the row's position and of the other rows' contents and adapters.
 *  L2. A row with an index outside [0, n_adapters) and a column in no segment are not read-modify-written (-0.0 keeps its sign);
 *      t_ws keeps its contents outside the rows and rank rows of the call.
 *  L3. The same bits eager or replayed.
 *
 * ivl_linear_m16_lora_fwd / _w8_fwd / _w4_fwd: the argument lists of the three ivl_linear_m16* entries plus `lora`.  Two launches:
 * the shrink of the x rows into lora->t_ws, then the m16 kernel with a LoRA epilogue -- after the LDS combine and the bias the lane
 * that owns an element forms y0 = bf16(acc + bias) and, where its row has an adapter and its WEIGHT ROW lies in a segment, applies
 * d, e and the add above; with glu != 0 to the gate row c and the up row I + c, before the gate.
 *   lora->x, y, M and K must be the call's; lora->N must be the number of weight rows (N, or 2N with glu: the segments live in the
 *   fused row space); the norm fields must be NULL; lora and every table pointer non-NULL: else IVL_ERR_INVALID_ARG.  The refusals of
 *   the m16 entries come first and are unchanged; those of ivl_lora_add_m16_fwd follow; all before any launch.
 *  F1. glu == 0: y and t_ws equal ivl_linear_m16*_fwd(glu = 0) followed by ivl_lora_add_m16_fwd on its output, bit for bit -- in
 *      both tile modes, with N tails, for every weight format.
 *  F2. glu != 0: equals the glu == 0 call of the same entry on the fused weight (N -> 2N) followed by ivl_silu_mul_fwd, bit for bit.
 *  F3. A row without an adapter and a column in no segment carry the bits of ivl_linear_m16*_fwd.
 *  F4. Contracts 1 to 3 of the m16 block carry over: determinism; row m depends on row m of x and on adapter_idx[m] only; packed
 *      equals bf16 on W'.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_lora_add_m16_fwd(const ivl_lora_args* args, void* stream);
IVL_API int ivl_linear_m16_lora_fwd(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int glu,
                                    const ivl_lora_args* lora, void* stream);
IVL_API int ivl_linear_m16_lora_w8_fwd(const void* x, const void* wq, const float* scale, const void* bias, void* y, int M, int N,
                                       int K, int glu, const ivl_lora_args* lora, void* stream);
IVL_API int ivl_linear_m16_lora_w4_fwd(const void* x, const void* wq, const void* sq, const void* bias, void* y, int M, int N, int K,
                                       int glu, const ivl_lora_args* lora, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring GIVEN tokens under lm_head: the log-probability of target[r] in the distribution of row r, the [M,N] logits never
 * written anywhere.  Replaces logits -> float log_softmax -> gather (HF `labels=`, CrossEntropyLoss(reduction="none") of
 * scripts/stat_utils/cal_ppl.py:111-124, `echo` + `logprobs` of the OpenAI protocol, likelihood ranking of candidate answers).
 * x [M,K], w [N,K], bias [N] or NULL: bf16, the shapes and alignments of the plain form of ivl_linear_m256_fwd (1 <= M <= 256,
 * K % 64 == 0 and K <= 16384, N % 4 == 0, 32-bit weight offsets, x / w 16-byte aligned).  target int64 [M]; logprob fp32 [M];
 * top1 int64 [M] and lse fp32 [M] may be NULL.  Per row r:
 *   S1 the logits.  xl[c] = bf16(x[r] . W[c] + bias[c]): the bits ivl_linear_m256_fwd (glu == 0) writes for that element -- the
 *      same K order, one rounding.  A NaN counts as -inf (step 1 of the sampling contract below).  m = max_c xl[c].
 *   S2 the partition sum.  Z = sum_c w_c, w_c = exp(xl[c] - m): exactly 1 where xl[c] == m (also at m = +-inf), 0 where
 *      xl[c] = -inf < m.  The real-valued definition behind L1 of the sampling launch's scores, without its 2^-40 weight floor.
 *      A row of nothing but -inf / NaN has Z = N.
 *   S3 lse[r] = m + logf(Z); lse[r] = m when m is infinite.
 *   S4 logprob[r] = (xl[target[r]] - m) - logf(Z): -logf(Z) where the target's logit equals m, -inf where it is -inf < m,
 *      -logf((float)N) in the all -inf row.  A target outside [0, N) -- IGNORE_INDEX = -100 -- is not scored: logprob[r] = 0.0f.
 *   S5 top1[r] = the lowest index with xl == m (the greedy token of step 2); written for ignored rows too; 0 in the all -inf row.
 * Two launches.  (1) linear_m256's kernel with a SCORE epilogue, 64 columns x all rows per workgroup: per (column block j, row)
 * one partial {m_j, z_j = sum exp(xl - m_j) in fp32, idx_j = the lowest index attaining m_j} goes to the workspace as one
 * 16-byte store, and the one lane that owns column target[r] stores that logit; no atomics.  (2) one workgroup per row:
 * M_r = max_j m_j, top1 = the smallest idx_j among m_j == M_r, Z = sum_j z_j exp(m_j - M_r) in float64 in a fixed order (blocks
 * with m_j == M_r unscaled, blocks at -inf nothing).  Every output is a pure function of (x[r], W, bias, target[r]): the same
 * bits on every run, eager or in a replayed graph, for any M and whichever row of the call the row sits in.
 * Error against the real number, from the bf16 logits on: |err| <= 1e-5 + 2^-22 |value| for logprob and lse (<= 2 ulp per expf,
 * 64-term fp32 partial sums, a float64 combine, 1 ulp of logf, one rounding of the difference).
 * workspace: ivl_linear_logprob_workspace_bytes(M, N) = ceil(N/64) * M * 16 + M * 4 bytes rounded up to 256 (0 for M < 1 or
 * N < 1), 16-byte aligned; its contents are scratch.  No allocation, no synchronisation, capturable.
 * Errors as ivl_linear_m256_fwd; IVL_ERR_INVALID_ARG also for NULL target, logprob or workspace; IVL_ERR_WORKSPACE: too small.
 * ------------------------------------------------------------------------------------------- */
IVL_API size_t ivl_linear_logprob_workspace_bytes(int M, int N);
IVL_API int ivl_linear_logprob_m256_fwd(const void* x, const void* w, const void* bias, const int64_t* target, float* logprob,
                                int64_t* top1, float* lse, int M, int N, int K, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Next-token sampling over lm_head logits: temperature, top-k, top-p, one random stream per row, one launch.
 * Replaces the logits warpers + multinomial of HF generate, which the reference drives with do_sample / temperature / top_p /
 * top_k (src/llamafactory/api/chat.py:160-162, api/protocol.py:99-101, webui/runner.py:231-232,
 * webui/components/chatbot.py:78-79).  Row s (a batch row or a decode slot) = the V bf16 logits at logits + s*ld.
 *   1 a NaN logit counts as -inf; order = numeric order of the bf16 values; m = max x.
 *   2 temperature[s] <= 0: token = the LOWEST index with x == m, n_kept = 1, prob = 1, counter[s] unchanged.
 *   3 top-k (0 < top_k[s] < V): K = {i : x_i >= the k-th largest value} (ties at the threshold stay, TopKLogitsWarper); else all.
 *   4 w_i = exp((x_i - m) / temperature), exactly 1 where x_i == m (also m = +-inf), 0 for x_i = -inf < m.  Evaluated as the
 *     integer q_i = floor(exp2f((x_i - m) * (log2e / temperature)) * 2^40): a token more than 40 ln 2 = 27.7 nats (after the
 *     temperature) below the maximum has weight 0 and is never drawn.
 *   5 top-p (top_p[s] < 1): with A(v) = sum{w_i : i in K, x_i > v} / sum{w_i : i in K}, P = {i in K : A(x_i) < p}
 *     (TopPLogitsWarper behind temperature and top-k: the top class always survives) -- except that tokens with EQUAL logits
 *     are kept or dropped together, where HF's cut inside a tie follows its sort order; else P = K.
 *   6 u64 = mix(mix(seed[s]) + (counter[s] + 1) * 0x9E3779B97F4A7C15) mod 2^64, mix = splitmix64's finaliser
 *     (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31);
 *     token = the first i in P, in vocabulary order, whose inclusive sum of q over P exceeds floor(u64 * Z_P / 2^64);
 *     then counter[s] += 1.
 * All sums are integer adds: the token is a pure function of (x, temperature, top_k, top_p, seed, counter) -- the same bits on
 * every run, eager or in a replayed graph, whichever row of a larger call the logits sit in.
 * token[s * token_stride] int64 is written; n_kept [S] int32 (= |P|) and prob [S] fp32 (= q_token / Z_P) may be NULL.
 * Any V >= 1 and ld >= V, any alignment (16-byte loads from the boundary at or below each row).  V >= 2^23: IVL_ERR_UNSUPPORTED.
 *
 * The call takes ONE struct, ivl_sample_args: the row and the sampling arguments above, then three optional groups and the
 * score-only switch.  Every field of a group may be NULL / 0 (off).  THE FORM of the launch follows from what is set:
 *     score_only != 0                                                                          -> the score-only form
 *     else fsm_state                                                                           -> the constrained form
 *     else any of logprob, n_top > 0, top_ids, top_logprobs, cum_logprob, lp_history, top_hist_ids, top_hist_lp
 *                                                                                              -> the scoring form
 *     else any of rep_penalty, seen, n_stop > 0, budget, n_new, done, history                  -> the controlled form
 *     else                                                                                     -> the control-free form
 *   `fill` alone and the scalars (seen_ld, hist_ld, mask_ld, n_states) select nothing.  Turning a group on never changes the
 *   outputs of the groups below it: with the scores on, token, counter, seen, n_new, done, history, n_kept and prob are bit for bit
 *   those of the same call without them; a row with fsm_state[s] < 0 behaves as in the call without the constraint group; and with
 *   every group off the outputs are those of steps 1-6 alone.
 *
 * CONTROLS: the generation controls the reference hands to HF generate beside the sampling arguments
 * (src/llamafactory/chat/hf_engine.py:128-156: repetition_penalty, eos_token_id, max_new_tokens), inside the same one launch.
 * Per row s, in order:
 *   A finished row.  done[s] != 0 on entry: token = fill[s] (0 when fill == NULL), n_kept = 0, prob = 0, and nothing else of the
 *     row is read or written -- not the counter, seen, n_new or the history; the workgroup returns before its first pass.
 *   B repetition penalty (HF RepetitionPenaltyLogitsProcessor, which runs before the warpers).  seen: a bitmap of uint32 words,
 *     row s at seen + s*seen_ld; bit (i & 31) of word (i >> 5) = token i has occurred.  For a seen token and
 *     r = rep_penalty[s] != 1:   x' = bf16_rne(x < 0 ? x * r : x / r),
 *     fp32 arithmetic on the widened bf16 value, a true IEEE division, one rounding to bf16.  NaN stays NaN (= -inf), +-inf stay,
 *     -0 stays in the class of +0.  Unseen tokens and rows with r == 1 (or rep_penalty == NULL) use x unchanged.  Steps 1-6
 *     then run on x' (the greedy arg-max is that of x'); because x' is a bf16 value again, the histograms,
 *     the integer weights and the bit-reproducible draw are what they are for any other row.  HF keeps the penalised logit in
 *     fp32; here it is rounded to bf16: half a bf16 ulp, at most 2^-8 relative, on a penalised logit.
 *   C bookkeeping after the draw, by the one lane that writes the token:
 *       seen != NULL: the token's bit is set (also at r == 1);
 *       history != NULL: history[s*hist_ld + n_new[s] % hist_ld] = token  (int64; a ring of the last hist_ld tokens: hist_ld is
 *         both the ring's length and its row pitch);
 *       n_new != NULL: n_new[s] += 1;
 *       done[s] = 1 if the token equals any of stop_ids[s*n_stop .. +n_stop) (int64; entries < 0 are unused);
 *       else done[s] = 2 if budget[s] >= 0 and n_new[s] >= budget[s] (after the increment).  A stop id wins over the budget.
 *   D bounds.  Bits at or above V in a row's last word, the words between ceil(V/32) and seen_ld and other rows are never
 *     modified and never influence a result; nothing outside a row's seen_ld words is read.
 * done codes: 0 running, 1 ended on a stop id, 2 ended on its budget, 3 a dead end of the constraint, 4 held by the host (never
 * written by a kernel; a decoder with holds sets and clears it between replays); the host clears done[s] to
 * restart a row.
 *
 * SCORES: the scores of what the call generates, inside the same one launch: the log-probability of the token, the
 * n_top most likely alternatives, a running sum and rings beside the token history (`logprobs` / `top_logprobs` of the OpenAI
 * protocol the reference's api/ serves; output_scores of HF generate).  Per row s:
 *   L1 the scored distribution.  x' = the row as the kernel keys it: after the repetition penalty of step B, before temperature,
 *      top-k and top-p (HF's processed scores in front of the warpers; with r == 1 the raw model distribution).  NaN counts as
 *      -inf (step 1); m = max x'.
 *        Z1  = sum_i floor(exp2f((x'_i - m) * log2e) * 2^40),  log2e = 1.44269504088896341f, the product rounded to fp32;
 *              an integer sum, exact in any order.  The weight is exactly 2^40 where x'_i == m (also at m = +-inf), 0 for
 *              x'_i = -inf < m and for (x'_i - m) * log2e <= -41 (step 4 at temperature 1).  2^40 <= Z1 <= V 2^40 < 2^63.
 *        lse = logf(RN_fp32(Z1) * 2^-40): the uint64 -> fp32 conversion rounds to nearest even, the scaling by 2^-40 is exact,
 *              logf is the device library's fp32 logarithm (1 ulp).  0 <= lse <= ln V.
 *        lp(i) = (x'_i - m) - lse, two fp32 subtractions in this order; lp(i) = -lse where x'_i == m; lp(i) = -inf where
 *              x'_i = -inf < m.  A token below the 27.7-nat weight floor of step 4 still gets its finite lp from this formula.
 *              A row of nothing but -inf / NaN gives every token -logf((float)V).
 *   L2 logprob[s] = lp(token written), for greedy and drawn rows alike (a greedy row makes the Z1 pass too, in this form only).
 *   L3 top-N.  The min(n_top, V) tokens with the largest x', ties to the lowest index, listed by (x' descending, index ascending):
 *      top_ids[s*n_top + j] int64, top_logprobs[s*n_top + j] = lp(top_ids[..]) fp32, bit-equal to what logprob would hold for that
 *      token; entries j >= V are id -1 / lp -inf.  Selected by the 4096 + 16 histogram threshold of top-k, no sort of the row.
 *   L4 bookkeeping, by the one lane that writes the token, in front of step C, at the ring index of the token history
 *      a = s*hist_ld + n_new[s] % hist_ld (n_new before its increment):
 *        lp_history[a] = logprob;  top_hist_ids[a*n_top + j] = top_ids[j];  top_hist_lp[a*n_top + j] = top_logprobs[j];
 *        cum_logprob[s] += (double)logprob  (float64; one add per step, in step order).
 *   L5 a finished row (done[s] != 0 on entry): logprob = 0, top_ids = -1, top_logprobs = -inf; no ring or cum_logprob write, and
 *      nothing else of the row is touched, as in step A.
 * logprob [S] fp32; n_top 0..20; top_ids / top_logprobs [S, n_top]; cum_logprob [S] float64; lp_history [S, hist_ld] fp32;
 * top_hist_ids int64 / top_hist_lp fp32 [S, hist_ld, n_top].  hist_ld is the one of `history` (which may itself be NULL).
 * The scores are a pure function of (x, rep_penalty, seen) and the token: the same bits eager or in a replayed graph, alone or as
 * any row of a larger call.
 *
 * CONSTRAINT: a token-level finite state machine per row, inside the same one launch: constrained decoding (what
 * HF generate takes as prefix_allowed_tokens_fn or a logits processor, with the token on the host after every step) without a
 * host round trip per token.
 *   fsm_state int32 [S]: per row a state index q >= 0, or -1 = an unconstrained row;
 *   fsm_mask uint32 [n_states, mask_ld], mask_ld*32 >= V: bit (i & 31) of word (i >> 5) of row q = token i is allowed in state q
 *     (the layout of `seen`);
 *   fsm_desc int64 [n_states, 2] = {trans_off, cls_off} of state q's grammar;  fsm_cls int32, flat: the class of token i in that
 *     grammar = fsm_cls[cls_off + i];  fsm_trans int32, flat: next = fsm_trans[trans_off + class]: a state >= 0, -1 = the row
 *     becomes unconstrained, -2 = no transition.  States are global indices: several grammars share the tables.
 * Per row s, with q = fsm_state[s] read ONCE at kernel entry (behind step A: a finished row is not looked at):
 *   F0 group off or row free.  fsm_state == NULL: the form rule above decides, as if the group's fields did not exist.  A row with
 *      q < 0 behaves as in the call without the group and its state stays as it is.
 *   F1 the row is its allowed sub-vocabulary.  A = {i < V : bit i of mask row q}.  Steps 1-6, B and L1-L3 run over i in A only: a
 *      token outside A is not keyed to -inf, it is ABSENT -- no part in the maximum, the counts, the masses, Z1, the top-N or the
 *      walk -- and can never be emitted or listed, also when every allowed logit is -inf or NaN and a disallowed one is +inf.
 *      Bits at or above V in a mask row's last word and the words between ceil(V/32) and mask_ld are ignored.
 *   F2 what follows: |A| takes V's place throughout.  top_k >= |A| keeps all of A; entries j >= |A| of the top-N list are -1 /
 *      -inf; a set A whose logits are all -inf or NaN gives each of its tokens -logf((float)|A|) (Z1 = |A| 2^40); n_kept, prob
 *      and logprob are those of the distribution renormalised over A.
 *   F3 all sums are integers and the draw is the first index in vocabulary order, so every output equals, bit for bit, that of
 *      the unconstrained call on the gathered row x[A] (A ascending) with the gathered seen bits: token and top_ids (mapped back
 *      through A), counter, n_kept, prob, logprob, top_logprobs, the rings and cum_logprob.
 *   F4 advance, by the lane that writes the token, behind step C:  c = fsm_cls[cls_off + token];
 *      fsm_state[s] = fsm_trans[trans_off + c].  `done` is decided by step C as before: a stop id that an accepting state allows
 *      ends the row through the stop rule.
 *   F5 dead end: done[s] = 3.
 *      A is empty, or q >= n_states (then no word of the tables is read): token = fill[s] (0 without fill), n_kept = 0, prob = 0,
 *      logprob = 0, top_ids = -1, top_logprobs = -inf; the counter, seen, n_new, the history, the rings, cum_logprob and the
 *      state stay unchanged (step A's treatment).  "A is empty" is decided uniformly for the workgroup after pass 1.
 *      The transition read in F4 is -2 (tables whose mask and transitions disagree): the token stands as drawn with step C's
 *      bookkeeping, the state stays unchanged, and done[s] = 3 replaces what step C decided.
 * Tables are the caller's to keep consistent (bit set <=> transition != -2) and in bounds: cls_off + i and trans_off + class are
 * not checked on the device.
 *
 * SCORE ONLY (score_only != 0): the scores without a token: per row s, steps A (a finished row), B (the repetition penalty on
 * `seen`), L1 and L3, and nothing else -- the candidate lists of a beam search step.
 *   top_ids[s*n_top + j] / top_logprobs[s*n_top + j]: the min(n_top, V) tokens with the largest x', ties to the lowest index,
 *   by (x' descending, index ascending), with lp of L1; entries j >= V are -1 / -inf.  Bit-equal to what the scoring form
 *   writes to its top_ids / top_logprobs for the same (logits, rep_penalty, seen), whatever that call's sampling parameters.
 *   A row with done[s] != 0 gets ids -1 and lp -inf (L5).  done may be NULL (no row is finished).
 * Nothing is committed: no token, counter, n_kept or prob; `seen` and `done` are only read and no n_new, history or ring exists here.
 * The form takes logits, ld, S, V, rep_penalty, seen, seen_ld, done, n_top (1..20), top_ids and top_logprobs; any other field that
 * is set is refused, not ignored.
 *
 * Refused before anything is launched, checked in the order base, controls, scores, constraint.
 * IVL_ERR_INVALID_ARG: NULL args, logits, temperature, top_k, top_p, seed, counter or token (score only: logits, top_ids or
 * top_logprobs); S < 1, V < 1, ld < V; score_only with a field outside its list; rep_penalty without seen; seen with
 * seen_ld*32 < V; n_stop outside 0..16; n_stop > 0 without stop_ids or done; budget without n_new or done; history without n_new or
 * with hist_ld < 1; n_top outside 0..20 (score only: 1..20); n_top > 0 without top_ids or top_logprobs; lp_history or a top ring
 * without n_new or with hist_ld < 1; a top ring with n_top == 0; fsm_state with fsm_mask, fsm_desc, fsm_cls, fsm_trans or done NULL,
 * mask_ld*32 < V or n_states < 1.  IVL_ERR_UNSUPPORTED: V >= 2^23.
 * ------------------------------------------------------------------------------------------- */
typedef struct ivl_sample_args {
  /* row */
  const void* logits; int64_t ld; int S, V;
  /* sampling */
  const float* temperature; const int32_t* top_k; const float* top_p; const int64_t* seed; int64_t* counter;
  int64_t* token; int64_t token_stride; int32_t* n_kept; float* prob;
  /* controls */
  const float* rep_penalty; uint32_t* seen; int64_t seen_ld;
  const int64_t* stop_ids; int n_stop; const int64_t* budget; const int64_t* fill;
  int64_t* n_new; int32_t* done; int64_t* history; int64_t hist_ld;
  /* scores */
  float* logprob; int n_top; int64_t* top_ids; float* top_logprobs; double* cum_logprob;
  float* lp_history; int64_t* top_hist_ids; float* top_hist_lp;
  /* constraint */
  int32_t* fsm_state; const uint32_t* fsm_mask; int64_t mask_ld; int n_states;
  const int64_t* fsm_desc; const int32_t* fsm_cls; const int32_t* fsm_trans;
  int score_only;
} ivl_sample_args;

IVL_API int ivl_sample_rows_fwd(const ivl_sample_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ADJUSTMENT: logit bias, frequency / presence penalties and min-p inside the same one launch -- `logit_bias`,
 * `frequency_penalty` and `presence_penalty` of the OpenAI chat-completion protocol the reference's api/ serves, and HF's
 * MinPLogitsWarper.  ivl_sample_args is unchanged: the group is a second struct, handed to a second entry point beside it.
 *   min_p fp32 [S]: 0 = off for the row; NULL = off for all rows;
 *   freq_penalty, pres_penalty fp32 [S]: f and p of the row; NULL = 0;
 *   count int32 [S, count_ld], count_ld >= V: c_i = how often token i has been GENERATED in row s (the prompt's tokens are marked
 *     in `seen` and not counted: the OpenAI / vLLM convention);
 *   bias_idx int32 [S]: the row's bias table b, outside [0, n_bias) = no bias;
 *   bias_mask uint32 [n_bias, bias_mask_ld], bias_mask_ld*32 >= V: bit (i & 31) of word (i >> 5) of row b = token i has a bias in
 *     table b (the layout of `seen`);  bias_val fp32 [n_bias, bias_ld], bias_ld >= V: that bias.
 * Per row s:
 *   ADJ-0 off is identity.  adj == NULL, or every field of it NULL / 0: every output is bit-equal to ivl_sample_rows_fwd(args)
 *      (it IS that call).  A row whose min_p is 0, whose f and p are 0 and whose bias_idx is out of range gets the bits of the call
 *      without the group; its counts are still kept when count != NULL (ADJ-4).
 *   ADJ-1 the adjusted row.  x' = the bf16 row after step B (the repetition penalty, rounded to bf16), c_i = count[s*count_ld + i].
 *        an element whose seen bit is set, with c_i > 0 and (f, p) != (0, 0):   t = x' - RN(RN(f * (float)c_i) + p)
 *        an element whose bit is set in bias_mask row b:                         t = RN(t + bias_val[b*bias_ld + i])
 *        then                                                                    x'' = bf16_rne(t)
 *      plain fp32 operations in this order, each rounded once to nearest even, no fused multiply-add; (float)c_i rounds to
 *      nearest even above 2^24.  A NaN result counts as -inf (step 1) and +-inf behave as IEEE says: a bias of -inf bans a
 *      token, +inf forces it (several forced tokens: the lowest index, or a draw among them by step 4's weights of 1).  An element
 *      touched by neither keeps the bits of x' (nothing is read, modified and written back; -0 stays what it is).  count is read
 *      only where the seen bit is set: a count word under a clear seen bit never influences a result.  Bits and words at or
 *      beyond V and other rows and tables are never read or written.
 *   ADJ-2 what follows.  Steps 1-6, the scores L1-L3 and the constraint F1-F5 run on x'' exactly as they run on x' without the
 *      group: every output is, bit for bit, what ivl_sample_rows_fwd writes for the row x'' with rep_penalty == 1 and the same
 *      seen / state tensors.  THE SCORED DISTRIBUTION IS THE ADJUSTED ONE: logprob, the top-N list and cum_logprob are those of
 *      x'' (HF's processed scores behind all its logits processors, in front of the warpers).
 *   ADJ-3 min-p (MinPLogitsWarper behind temperature, top-k and top-p, min_tokens_to_keep = 1).  With q_i the Q40 integer of
 *      step 4 at the row's temperature and qmin = (u64)(min_p * 2^40) (the product is exact in fp32):
 *        P' = {i in P : q_i >= qmin};
 *      the maximum (q = 2^40) always survives; min_p above 1 acts as 1, below 0 or NaN as 0.  Z_P, n_kept, prob and the walk of
 *      step 6 are over P'.  The rule is evaluated element by element where the weight is; a greedy row ignores it.
 *   ADJ-4 bookkeeping.  The one lane that writes the token, in step C:  count[s*count_ld + token] += 1.  A finished row (step A)
 *      and a dead end in front of the draw (F5) touch nothing.
 * THE FORM: with a group that is on, the launch takes at least the controlled form, then the scoring or the constrained form
 * by the rule of ivl_sample_rows_fwd; the kernels launched without the group are the ones they were.  Penalties inside a beam
 * search are not served: score_only with adj is refused.
 * Refused before anything is launched, after the checks of ivl_sample_rows_fwd (IVL_ERR_INVALID_ARG): count without seen or
 * with count_ld < V; freq_penalty or pres_penalty without count; bias_idx with bias_mask or bias_val NULL, n_bias < 1,
 * bias_mask_ld*32 < V or bias_ld < V; score_only != 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct ivl_sample_adj_args {
  const float* min_p;
  const float* freq_penalty; const float* pres_penalty;
  int32_t* count; int64_t count_ld;
  const int32_t* bias_idx;
  const uint32_t* bias_mask; int64_t bias_mask_ld;
  const float* bias_val; int64_t bias_ld; int n_bias;
} ivl_sample_adj_args;

IVL_API int ivl_sample_rows_adj_fwd(const ivl_sample_args* args, const ivl_sample_adj_args* adj, void* stream);

/* Sets the bits of ids[0..n) (int64, device) in ONE row of a seen bitmap: the prompt's tokens, before the first draw.  Ids outside
 * [0, V) are ignored, duplicates are fine; n == 0 is a no-op.  seen_row NULL, V < 1, n < 0 or ids NULL with n > 0:
 * IVL_ERR_INVALID_ARG. */
IVL_API int ivl_token_mark_fwd(uint32_t* seen_row, int64_t V, const int64_t* ids, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TOKEN BANS: `no_repeat_ngram_size`, `bad_words_ids` and `min_new_tokens` of HF generate -- the logits processors that set
 * scores to -inf in front of the warpers -- as ONE small launch in front of the sampling launch.  It writes bf16 -inf into the
 * rows of `logits` IN PLACE; the sampling entry points are unchanged and see the edited rows.
 *   logits bf16 [S, ld], ld >= V; done int32 [S], may be NULL;
 *   n_new int64 [S] and history int64 [S, hist_ld]: the ring of the row's generated tokens that ivl_sample_rows_fwd keeps;
 *   ctx int64 [S, ctx_ld] and n_ctx int64 [S]: a second ring of the same rule, the tokens in front of them (the prompt), n_ctx of
 *     them pushed so far; may be NULL;
 *   ngram int32 [S]: the row's n-gram size g, <= 0 = off; NULL = off for all rows;
 *   min_new int64 [S] with stop_ids int64 [S, n_stop]; NULL = off;
 *   ban_idx int32 [S]: the row's sequence table b, outside [0, n_tables) = none; NULL = none for all rows;
 *   ban_seq int64 [n_tables, n_seq, seq_ld]: a sequence of m <= seq_ld tokens occupies the LAST m columns of its row; the first
 *     negative entry from the right ends it; a row whose last column is negative is unused.
 * THE ROW'S SEQUENCE seq[0 .. L): the c = min(n_ctx[s], ctx_ld) newest entries of the context ring, oldest first (c = 0 when ctx
 * is NULL or n_ctx[s] < 0), then the h = min(n_new[s], hist_ld) newest entries of the history ring, oldest first; L = c + h.
 * Entry number i of a ring sits at i % ld.  The window is what the rings hold: a token that has been overwritten no longer counts.
 * An id outside [0, V) in a ring or a table equals nothing, not even itself: a prefix that holds one never matches.
 * Per row s:
 *   BAN-0 finished rows and rows that are off.  A row with done[s] != 0 is not touched, and nothing of it beyond done[s] is read
 *      (step A of the sampling launch, HOLD-1..3).  A row with ngram <= 0, ban_idx out of range and n_new >= min_new has no byte
 *      written, and neither its rings nor any table are read.
 *   BAN-1 n-gram rule (NoRepeatNGramLogitsProcessor), g = ngram[s] >= 1.  For every i in [0, L - g]: if seq[i .. i+g-2] equals the
 *      last g - 1 tokens of seq, token seq[i+g-1] is banned.  g = 1 bans every token of seq; L < g bans nothing.
 *   BAN-2 sequence rule (NoBadWordsLogitsProcessor), for every used row of table b: t is its last token, the m - 1 tokens in
 *      front of it the prefix.  If m - 1 <= L and the prefix equals the last m - 1 tokens of seq, t is banned; m = 1 always bans
 *      t.  (HF skips a sequence that is LONGER than the ids so far, one token too early: its prefix may fit.  Here a prefix that
 *      fits is matched.)
 *   BAN-3 minimum length rule (MinNewTokensLengthLogitsProcessor).  While n_new[s] < min_new[s], every entry of stop_ids[s, :]
 *      in [0, V) is banned.
 *   BAN-4 the edit.  Banned: logits[s*ld + t] = bf16 -inf (0xFF80), for 0 <= t < V only -- no id is used as an address before it
 *      is known to lie in [0, V).  Every other element keeps its bits (NaN payloads, -0); columns V..ld and other rows are never
 *      written.  A ban is a 2-byte store to the element itself, never a read-modify-write of the word around it, and the row is
 *      not read: the call is idempotent.  A row's result depends on that row's inputs alone: the same bits eager or replayed,
 *      alone or as any row of a larger call.
 *   BAN-5 composition.  The sampling launch that follows runs step 1, the scores L1-L3, the adjustments ADJ-1..3 and the
 *      constraint on the edited row; a row that is banned entirely follows the all -inf rules it has.
 * Refused before anything is launched (IVL_ERR_INVALID_ARG): NULL args or logits; S < 1, V < 1, ld < V; ngram or ban_idx
 * without n_new and history or with hist_ld < 1; ctx without n_ctx or with ctx_ld < 1; ban_idx without ban_seq or with
 * n_tables, n_seq or seq_ld < 1 or seq_ld > 16; min_new without n_new or stop_ids or with n_stop outside 1..16.
 * IVL_ERR_UNSUPPORTED: V >= 2^23; with ngram or ban_idx, hist_ld + ctx_ld > 12288 (the window the kernel stages).
 * ------------------------------------------------------------------------------------------- */
typedef struct ivl_ban_args {
  void* logits; int64_t ld; int S, V;
  const int32_t* done;
  const int64_t* n_new; const int64_t* history; int64_t hist_ld;
  const int64_t* ctx; int64_t ctx_ld; const int64_t* n_ctx;
  const int32_t* ngram;
  const int64_t* min_new; const int64_t* stop_ids; int n_stop;
  const int32_t* ban_idx;
  const int64_t* ban_seq; int n_tables, n_seq, seq_ld;
} ivl_ban_args;

IVL_API int ivl_token_ban_fwd(const ivl_ban_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GUIDANCE ON PAIRED ROWS: `guidance_scale` with `negative_prompt_ids` of HF generate (UnbatchedClassifierFreeGuidanceLogits-
 * Processor) and visual contrastive decoding (VCD: cd_alpha, cd_beta) -- the one logits processor that needs TWO rows.  A guided
 * stream is a leader row r (the real prompt) and its partner row p = partner[r] (the negative prompt).  ivl_logit_guide_fwd is ONE
 * small launch in front of the bans and the sampling launch; it rewrites the leader's row of `logits` IN PLACE from both rows.
 * ivl_rows_follow_fwd is one launch behind the sampling launch; it keeps the partner on the leader's tokens.
 *   logits bf16 [S, ld], ld >= V, rows at any alignment, as in the sampling launch;
 *   partner int32 [S]; scale fp32 [S]; cut fp32 [S]: ln(beta) of the plausibility rule, -inf = off (the host takes the
 *     logarithm); done int32 [S], may be NULL.
 *   GUIDE-0 which rows are guided.  Row r is guided when p = partner[r] lies in [0, S), p != r, partner[p] is not itself in
 *      [0, S) other than p (a partner is never a leader), scale[r] is finite, and done is NULL or done[r] == 0.  Any other row is
 *      OFF: no byte of it is written and nothing of it beyond those table entries is read; it keeps its bits whatever they are.
 *   GUIDE-1 log-partitions.  c = row r, u = row p, a NaN read as -inf.  mc, mu: the row maxima.  Lc, Lu: the log-partitions as
 *      the scoring form of the sampling launch computes its lse (L1): Z = the INTEGER sum of the Q40 weights at temperature 1,
 *      2^40 exactly at the maximum, L = logf((float)Z * 2^-40).  An integer sum does not depend on the order of the reduction.
 *   GUIDE-2 the combination, in fp32, one rounding per operation: dc = c(v) - mc, du = u(v) - mu; lc = dc - Lc, lu = du - Lu;
 *      y = fmaf(s, lc - lu, lu), s = scale[r]; out(v) = bf16_rne(y).  This is HF's uncond + s (cond - uncond) on log-softmaxes;
 *      with s = 1 + alpha it is VCD's (1 + alpha) c - alpha u up to a constant per row, which is kept so that what runs behind
 *      it (the repetition penalty) sees HF's values.
 *   GUIDE-3 infinities and the cut.  c(v) = -inf: out(v) = -inf.  u(v) = -inf with c(v) finite: out(v) = lc (HF produces a NaN
 *      there).  dc < cut[r]: out(v) = -inf -- VCD's adaptive plausibility constraint p_c(v) >= beta max p_c.  The leader's
 *      maximum always survives, whatever cut[r] holds.
 *   GUIDE-4 the edit.  Only elements [0, V) of guided leader rows are written; columns V..ld, partner rows and off rows keep
 *      every bit.  A row's result depends on its two input rows alone: the same bits eager or replayed, in any pair of row
 *      positions, among any neighbours.  The call is NOT idempotent: it is meant for freshly written logits.
 *   GUIDE-5 composition.  The bans and every form of the sampling launch run on the edited row: scores and logprobs are those
 *      of the guided distribution.
 * ivl_rows_follow_fwd: token int64, row s at token[s * token_stride]; done int32 [S], may be NULL.  For every row p that is the
 * partner of a valid leader r (GUIDE-0 without the done and scale clauses): token[p * stride] = token[r * stride], and
 * done[p] = done[r] if done is given.  If several leaders name p the lowest r wins.  Every other element is untouched.
 * Refused before anything is launched (IVL_ERR_INVALID_ARG): NULL logits, partner, scale, cut or token; S < 1, V < 1, ld < V,
 * token_stride < 1.  IVL_ERR_UNSUPPORTED: V >= 2^23 or S > 63.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_logit_guide_fwd(void* logits, int64_t ld, int S, int V, const int32_t* partner, const float* scale,
                                const float* cut, const int32_t* done, void* stream);
IVL_API int ivl_rows_follow_fwd(int64_t* token, int64_t token_stride, int32_t* done, const int32_t* partner, int S, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row fork: row `src_row` of every tensor of a table goes to a set of rows of the partner tensors, in one launch.  The state of
 * a stream (ring rows, conv and recurrent states, position, sampler rows) is one row each of many tensors: this is the clone of
 * the reference's streaming demo (inference_examples/demo_streaming_inference.py:357-398) and the fan-out behind
 * num_return_sequences (src/llamafactory/api/chat.py:164), between two replays of a captured step.
 * table: DEVICE int64 [n_entries][6], built once by the caller and kept:
 *     {src_base, dst_base, src_row_stride_bytes, dst_row_stride_bytes, row_bytes, first_piece}
 *   Row r of an entry is the row_bytes >= 1 bytes at base + r * row_stride_bytes.  A row is cut into pieces of 16384 bytes;
 *   first_piece is the number of pieces of all entries before this one (entry 0: 0), which makes the pieces of the table one
 *   flat work list that the workgroups share evenly, whatever the mix of entry sizes.
 * dst_mask: bit r set = row r of every entry's destination tensor is written.  Every source byte is read once and stored to
 *   every destination; 16-byte accesses where the source and all destinations of a piece sit at the same offset in a 16-byte
 *   line (bytes before and after), single bytes otherwise; no byte outside a destination row is written, none outside the source
 *   row read.  An entry whose src_base == dst_base never copies src_row onto itself (that bit is skipped in the kernel; a caller
 *   that can see the table refuses it: the host side of this call cannot, the table is device memory).  Overlapping source and
 *   destination rows are the caller's to exclude.
 * max_row_bytes: the largest row_bytes of the table (it bounds the grid).  No allocation, copy or synchronisation: capturable.
 * IVL_ERR_INVALID_ARG: NULL table, n_entries < 1, max_row_bytes < 1, src_row < 0, dst_mask == 0.
 * IVL_ERR_UNSUPPORTED: src_row >= 63 or bit 63 of dst_mask (rows 0..62 only).
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_rows_copy_fwd(const int64_t* table, int n_entries, int64_t max_row_bytes, int src_row, int64_t dst_mask,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row gather: the rows [row0, row0 + n_rows) of every tensor of a table are permuted / duplicated IN PLACE by a map that lives on
 * the device -- the reorder of a beam search step (HF generate's cache reorder by beam_idx; num_beams of the reference's
 * hparams/generating_args.py), whose parents are decided inside the captured step.
 * table: the format of ivl_rows_copy_fwd, every entry with src_base == dst_base and equal strides (only dst_base, the destination
 *   stride, row_bytes and first_piece are read).
 * parent: DEVICE int32 [n_rows].  For every entry and every d < n_rows at once:
 *     row row0 + d  <-  the OLD row row0 + parent[d].
 *   Rows with parent[d] == d are neither loaded nor stored (an identity map moves no byte); a parent[d] outside [0, n_rows) counts
 *   as d: nothing outside the group is ever read or written.
 * No shadow copy and no barrier: for its own 16-byte lanes of a piece (and its edge bytes) a thread first loads that lane from
 *   every row some d != parent[d] names, and only then stores to every such d.  A thread only overwrites bytes it has itself
 *   already loaded, and one offset of a row belongs to one thread, so cycles ([1,2,3,0]), swaps and fan-out ([0,0,0,0], the fork)
 *   need no ordering between threads.  16-byte accesses where the row stride is a multiple of 16 (bytes at the unaligned head and
 *   tail of a piece), single bytes otherwise, in the same load-all-then-store order.  n_rows <= 4: 16384-byte pieces, 4 x 4
 *   16-byte registers; n_rows 5..8: the piece is walked in two halves, 8 x 2 registers.  No LDS.
 * 1 <= n_rows <= 8, row0 >= 0, row0 + n_rows <= 63.  No allocation, copy or synchronisation: capturable, and a replay follows the
 * current contents of `parent`.
 * IVL_ERR_INVALID_ARG: NULL table or parent, n_entries < 1, max_row_bytes < 1, row0 < 0, n_rows outside 1..8.
 * IVL_ERR_UNSUPPORTED: row0 + n_rows > 63.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_rows_gather_fwd(const int64_t* table, int n_entries, int64_t max_row_bytes, int row0, int n_rows,
                                const int32_t* parent, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Beam search (num_beams / length_penalty / early_stopping of HF generate, which the reference sets through
 * hparams/generating_args.py and train/sft/workflow.py:94): G groups of B beams; group g owns the rows (slots) [g B, (g+1) B) of
 * every per-slot tensor.  One step = score (ivl_sample_rows_fwd with score_only and n_top = K) -> ivl_beam_select_fwd ->
 * ivl_rows_gather_fwd(parent + g B) over everything a slot owns -> ivl_beam_commit_fwd.  Both calls here process group g only if
 * bit g of the HOST group_mask is set and beam_done[g] == 0; a skipped group has nothing read or written.
 * Per slot: top_ids int64 / top_logprobs fp32 [S,K]; cum_logprob float64 [S], the beam's sum of log-probabilities, -inf = no beam
 *   here; n_new int64 [S]; history int64 [S,L] (L = hist_ld; token i of a beam at history[s*L + i % L]); seen uint32 [S,seen_ld];
 *   token int64 at token + s*token_stride.
 * Per group: length_penalty float64 [G]; early_stopping int32 [G]; budget int64 [G] (< 0: none); stop_ids int64 [G,n_stop]
 *   (entries < 0 unused); beam_done int32 [G] (0 running, 1 finished by the stopping rule, 2 by its budget); n_hyp int32 [G];
 *   hyp_score / hyp_sum float64 [G,B]; hyp_len int64 [G,B]; hyp_tokens int64 [G,B,L]; parent int32, next_token int64 and next_score
 *   float64 [G,B].  The first n_hyp entries of the hyp_* tables are the group's finished hypotheses in insertion order.
 *
 * ivl_beam_select_fwd (HF BeamSearchScorer.process, BeamHypotheses.add / is_done):
 *   S1 candidates: (beam b, rank j < K) with top_ids >= 0, of beams with a finite cum_logprob; score = cum_logprob[b] + (double)lp,
 *      one float64 add of an fp32 value.
 *   S2 they are ranked by (score descending, beam ascending, rank ascending) -- a total order -- and the first K are walked:
 *        a stop id at walk position >= B is skipped;
 *        a stop id at walk position < B becomes a hypothesis: tokens = the parent's history (as it is BEFORE the gather) followed
 *          by the stop token, length n = n_new[parent] + 1, sum = the candidate's score, score = hyp(sum, n);
 *        any other candidate becomes the next beam d = 0, 1, ...: parent[d] = b, next_token[d], next_score[d]; the walk ends when
 *          B beams are taken.  Beams left over (fewer candidates than needed) get parent d, token 0, score -inf.
 *   S3 hyp(sum, n) = sum / n^length_penalty in float64: length_penalty == 1 is a plain IEEE division, == 0 the sum itself, anything
 *      else sum / pow((double)n, length_penalty).
 *   S4 insert: if n_hyp < B or score > the worst score; over B, the worst (the lowest score, the earliest inserted of equals) leaves
 *      and the later entries move up.
 *   S5 done, evaluated after the walk: never while n_hyp < B; with early_stopping once n_hyp == B; else when
 *      worst >= hyp(the best candidate's score, n_new + 1).  A done group gets beam_done = 1 and parent = the identity; it is
 *      not committed, so its tokens and scores freeze while its slots go on computing.
 * ivl_beam_commit_fwd, after the gather, for every beam d of a running group: token = next_token[d]; its bit of `seen` is set (seen
 *   may be NULL); history[n_new % L] = token; n_new += 1; cum_logprob = next_score[d].  Then, if budget[g] >= 0 and n_new has
 *   reached it: every beam with a finite sum becomes a hypothesis in beam order by S4 (tokens = its history, n = n_new; HF
 *   finalize), beam_done = 2 and parent = the identity.  Whichever way a group ends, its parent row is the identity from then
 *   on: the gather of a later step, which runs for every group, moves none of its rows.
 * K = max(2, 1 + n_stop) B makes the first K candidates hold B that are no stop id; the host computes it and refuses K > 20.
 * Deliberate differences from HF: the scores are those of the penalised bf16 row x' (L1; HF penalises log-softmax values; with
 * r == 1 the two agree); the tie order of S2 (torch.topk leaves it open); a hypothesis includes its stop token;
 * early_stopping = "never" and beam sampling are not offered.
 * IVL_ERR_INVALID_ARG (before anything is launched): G outside 1..63, B outside 1..8, K outside 1..20, n_stop outside 0..16 or
 * without stop_ids, hist_ld < 1, token_stride < 1, seen with seen_ld*32 < V, a NULL pointer other than seen and stop_ids.
 * ------------------------------------------------------------------------------------------- */
IVL_API int ivl_beam_select_fwd(int G, int B, int K, int64_t group_mask,
                                const int64_t* top_ids, const float* top_logprobs, const double* cum_logprob,
                                const int64_t* n_new, const int64_t* history, int64_t hist_ld,
                                const int64_t* stop_ids, int n_stop, const double* length_penalty, const int32_t* early_stopping,
                                int32_t* beam_done, int32_t* n_hyp, double* hyp_score, double* hyp_sum, int64_t* hyp_len,
                                int64_t* hyp_tokens, int32_t* parent, int64_t* next_token, double* next_score, void* stream);
IVL_API int ivl_beam_commit_fwd(int G, int B, int64_t group_mask,
                                const int64_t* next_token, const double* next_score, int64_t* token, int64_t token_stride,
                                uint32_t* seen, int64_t seen_ld, int64_t V, int64_t* history, int64_t hist_ld, int64_t* n_new,
                                double* cum_logprob, const int64_t* budget, const double* length_penalty,
                                int32_t* beam_done, int32_t* n_hyp, double* hyp_score, double* hyp_sum, int64_t* hyp_len,
                                int64_t* hyp_tokens, int32_t* parent, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IVL_HIP_H */

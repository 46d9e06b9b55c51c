/* aki_mi355x.h - C ABI of the MI355X-native AKI modality-mutual-attention (MMA) path: forward, KV-cache decode, the
 * pre-training step (backward, loss, optimizer) and the fp8 (e4m3) projection variants.
 *
 * The reference (sony/aki) has no FFI layer: its boundary is Python object protocol
 * (SURVEY.md section 8(b)).  Each entry point below names the reference function whose work it
 * replaces (paths relative to /root/reference/codes/open_flamingo/, "HF:" = the transformers
 * dependency the reference delegates to).  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.
 *
 * Conventions
 *  - Plain C: raw DEVICE pointers, sizes and strides in ELEMENTS, no torch/HIP types.
 *    `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - Ownership: the caller owns every buffer, including workspaces.  Kernels allocate nothing,
 *    keep no state between calls (one documented exception: the decode-attention workspace holds arrival counters
 *    that the kernel re-arms itself), never synchronise the host and are graph-capturable.
 *  - Errors: int return, 0 = AKI_OK, < 0 = aki_status code; never throws or aborts.  Shapes and
 *    alignment are validated on the host before anything is launched.
 *  - Threading: re-entrant; ordering only through `stream`.
 *  - dtype: AKI_DT_BF16 (MFMA path, fp32 accumulate/softmax) or AKI_DT_F32 (exact-f32 parity path, forward only);
 *    AKI_DT_FP8_E4M3 / AKI_DT_W8A16 where an entry point says so.  The backward / optimizer entry points are bf16.
 */
#ifndef AKI_MI355X_H
#define AKI_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AKI_ABI_VERSION 17   /* not bumped for the fp8 KV-cache functions (aki_kv_cache_quant_fp8, aki_decode_attn_fused_fp8kv_fwd): purely additive */

typedef enum {
  AKI_OK = 0,
  AKI_ERR_INVALID_ARG = -1,  /* null pointer, non-positive size, inconsistent shapes           */
  AKI_ERR_UNSUPPORTED = -2,  /* dtype / head_dim / size outside what the kernels are built for  */
  AKI_ERR_ALIGNMENT = -3,    /* pointer or leading dimension not 16-byte aligned                */
  AKI_ERR_WORKSPACE = -4,    /* workspace missing or too small                                  */
  AKI_ERR_LAUNCH = -5        /* hipGetLastError() after launch was not hipSuccess               */
} aki_status;

typedef enum {
  AKI_DT_BF16 = 0,
  AKI_DT_F32 = 1,
  AKI_DT_FP8_E4M3 = 2, /* e4m3 x and w with per-row scales (aki_linear_args / aki_mma_attn_args) */
  AKI_DT_W8A16 = 3,    /* weight-only fp8: e4m3 w + w_scale, bf16 x; decode rows (aki_linear_fwd: M <= 16, aki_decode_linear_fwd: M <= 8) */
  AKI_DT_W4A16 = 4     /* weight-only MXFP4: e2m1 nibbles + one e8m0 scale byte per block of 32 k (the layout of aki_linear_w4_fwd), bf16 x;
                          accepted by aki_decode_chain_fwd only (the per-layer calls take MXFP4 through aki_linear_w4_fwd) */
} aki_dtype;

/* Activation fused into aki_linear_fwd. */
typedef enum {
  AKI_ACT_NONE = 0,
  AKI_ACT_GELU_ERF = 1,  /* torch.nn.GELU()            - src/helpers.py:37                    */
  AKI_ACT_GELU_TANH = 2, /* gelu_pytorch_tanh          - HF:siglip MLP                        */
  AKI_ACT_SWIGLU = 3     /* out = up * silu(gate), W = [gate; up] - HF:phi3/modeling_phi3.py:49-64 */
} aki_act;

const char* aki_strerror(int status);
int aki_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Mask description.  The reference materialises a dense (B,1,L,L) int64 0/1 tensor
 * (src/vlm.py:410-443 `_make_modality_mutual_mask`, stacked by src/utils.py:99-108).  Here the
 * same information travels as a tiny table:
 *   visible(r,c) = valid(c) && ( c <= r || exists k: row_lo_k <= r < row_hi_k && col_lo_k <= c < col_hi_k )
 * `rects` is [B][max_rects]; unused entries are all-zero.  Row ranges of one sample's rectangles
 * must not overlap.  One rectangle per sample reproduces the reference; more are build-defined.
 * `col_valid_bits` is [B][ceil(L/64)] uint64, bit (c & 63) of word (c >> 6) = attention mask of
 * column c (bits at c >= L must be 0); NULL = every column < L valid.
 * `seq_lens` is [B] int32: rows r >= seq_lens[b] are the all-zero rows that batch stacking adds at
 * the bottom of a shorter sample's mask (src/utils.py:99-108) and are treated as rows with no
 * visible column; NULL = L for every sample.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t row_lo, row_hi, col_lo, col_hi;
} aki_mma_rect;

#define AKI_MAX_RECTS 8
#define AKI_PLAN_STRIDE 12 /* int32 per sample in the splice plan */

/* Rows with no visible column: the reference's additive finfo.min mask (transformers==4.41.2
 * `_prepare_4d_causal_attention_mask`, implicit at src/aki.py:125) yields a uniform softmax over
 * all L columns.  AKI_DEAD_ROWS_UNIFORM reproduces that; AKI_DEAD_ROWS_ZERO writes zeros. */
typedef enum { AKI_DEAD_ROWS_ZERO = 0, AKI_DEAD_ROWS_UNIFORM = 1 } aki_dead_rows;

/* ------------------------------------------------------------------------------------------------
 * aki_mma_attn_core_fwd - span-driven block-sparse softmax(QK^T * scale + mask) V.
 * Replaces: HF:phi3/modeling_phi3.py:145-167 `eager_attention_forward` as called from
 * `Phi3Attention.forward` (:218-263) under the reference's mask (src/vlm.py:556-564), plus the
 * 4-D mask inversion of transformers==4.41.2.  No L x L tensor is ever formed.
 *   q,k,v : [B,H,L,Dh] contiguous (k already rotated);  o : [B,L,H*Dh];  lse : [B,H,L] f32 or NULL
 *   workspace: aki_mma_attn_core_workspace_bytes() bytes, 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;
  const aki_mma_rect* rects;
  const uint64_t* col_valid_bits;
  const int32_t* seq_lens;
  int32_t max_rects;
  int32_t B, H, L, Dh;
  float scale;
  int32_t dtype;     /* aki_dtype */
  int32_t dead_rows; /* aki_dead_rows */
  int32_t kv_capacity; /* rows allocated per (batch, head) in k and v ([B,H,kv_capacity,Dh], a KV cache); 0 = L */
} aki_mma_attn_core_args;

size_t aki_mma_attn_core_workspace_bytes(int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype);
int aki_mma_attn_core_fwd(const aki_mma_attn_core_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * aki_mma_attn_fwd - the fused MMA op: QKV projection + RoPE + span-driven attention.
 * Replaces: `Phi3Attention.forward` up to (not including) o_proj, HF:phi3/modeling_phi3.py:218-258:
 *   qkv = x W_qkv^T ; split ; rotate-half RoPE with (cos,sin) ; attention core as above.
 *   x      : [B*L, d_model] (the RMS-normed hidden states), ldx elements between rows
 *   w_qkv  : [3*H*Dh, d_model] = `self_attn.qkv_proj.weight`, row-major, ldw
 *   cos,sin: f32 [pos_rows, Dh] tables (HF `Phi3RotaryEmbedding`; default or LongRoPE computed by the host)
 *   position_ids: int32 [B*L] row index into cos/sin per token, or NULL for (token index mod L)
 *   o      : [B, L, H*Dh]
 * Two stream-ordered launches inside one call (projection+RoPE epilogue, then attention); the
 * rotated Q/K and V live in the caller-owned workspace in head-major [B,H,L,Dh] order.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;
  const void* w_qkv;
  const float* cos;
  const float* sin;
  const int32_t* position_ids;
  void* o;
  float* lse;
  const aki_mma_rect* rects;
  const uint64_t* col_valid_bits;
  const int32_t* seq_lens;
  int32_t max_rects;
  int32_t B, H, L, Dh, d_model;
  int32_t ldx, ldw;
  int32_t pos_rows;
  float scale;
  int32_t dtype;
  int32_t dead_rows;
  int32_t kv_capacity; /* aki_qkv_rope_fwd: rows per (batch, head) of k_out / v_out (prefill straight into a KV cache); 0 = L */
  /* dtype == AKI_DT_FP8_E4M3: x / w_qkv are e4m3 bytes with per-row scales (see aki_linear_args); q, k, v, o are bf16 and
   * the attention core runs exactly as in the bf16 path. */
  const float* x_scale;
  const float* w_scale;
  const float* row_scale;  /* folded input RMSNorm (see aki_linear_args): x is the RAW hidden state, w_qkv = W diag(gain); NULL = none */
} aki_mma_attn_args;

size_t aki_mma_attn_workspace_bytes(int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype);
int aki_mma_attn_fwd(const aki_mma_attn_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* Stage 1 of the fused op on its own (KV-cache prefill, tests): q_out [B,H,L,Dh]; k_out / v_out [B,H,kv_capacity,Dh]
 * (kv_capacity = 0 means L).  AKI_DT_F32 needs a workspace of B*L*3*H*Dh floats; bf16 needs none. */
int aki_qkv_rope_fwd(const aki_mma_attn_args* args, void* q_out, void* k_out, void* v_out, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * aki_attn_fwd - plain (unmasked) multi-head attention softmax(Q K^T * scale) V for the vision side.
 * Replaces: SigLIP `eager_attention_forward` (HF:siglip/modeling_siglip.py:226-247, 16 heads x 72; call site
 * src/vlm.py:202-203) and the softmax attention of `PerceiverAttention.forward` (src/helpers.py:93-100, 8 x 64,
 * 144 latent queries over 729+144 keys).
 *   q/k/v are read in place through ELEMENT strides (batch, head, token; channel stride 1), so the fused QKV / KV
 *   projection outputs need no transposition;  o : [B, Lq, H*Dh] contiguous.  Dh in {32, 64, 72, 96}.
 *   AKI_DT_F32 needs contiguous head-major [B,H,L,Dh] inputs and a workspace of B*H*Dh floats.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int64_t q_stride_b, q_stride_h, q_stride_t;
  int64_t k_stride_b, k_stride_h, k_stride_t;
  int64_t v_stride_b, v_stride_h, v_stride_t;
  int32_t B, H, Lq, Lk, Dh;
  float scale;
  int32_t dtype;
  float* lse;          /* optional [B,H,Lq] f32 log-sum-exp of the scaled scores (bf16 path; consumed by aki_attn_bwd) */
} aki_attn_args;

int aki_attn_fwd(const aki_attn_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * aki_linear_fwd - y = act(x W^T + bias) [+ residual]   (torch.nn.functional.linear semantics)
 * Replaces: every nn.Linear on the path - o_proj / gate_up_proj / down_proj
 * (HF:phi3/modeling_phi3.py:49-64,215-216), Perceiver to_q/to_kv/to_out and FeedForward linears
 * (src/helpers.py:32-39,72-74), projection (src/helpers.py:147), DecoupledLinear pieces (src/helpers.py:594-603).
 *   x [M,K] ldx ; w [N,K] ldw ; y [M,N_out] ldy (N_out = N/2 for AKI_ACT_SWIGLU, else N)
 *   bias [N] or NULL ; residual [res_rows? , N_out] ldr or NULL, row index = m % res_row_mod when res_row_mod > 0
 *   K must be a multiple of 64 (bf16) ; N_out a multiple of 4.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;
  const void* w;
  const void* bias;
  const void* residual;
  void* y;
  int32_t M, N, K;
  int32_t ldx, ldw, ldy, ldr;
  int32_t res_row_mod;
  int32_t act;   /* aki_act */
  int32_t dtype; /* aki_dtype */
  /* AKI_DT_FP8_E4M3 (BASELINE configs[4]): x and w hold OCP e4m3 bytes (ldx / ldw in bytes, multiples of 16; K a multiple
   * of 128) produced by aki_quant_rows_fp8, with one f32 dequantisation scale per x row / per w row; bias, residual and
   * y stay bf16.  act: NONE or SWIGLU.  Ignored for the other dtypes. */
  const float* x_scale;
  const float* w_scale;
  /* Two-segment weight (bf16 MFMA GEMM, act NONE): logical weight row r comes from w[r] for r < w2_row0 and from
   * w2[min(r - w2_row0, w2_rows - 1)] beyond it (same ldw) - `DecoupledLinear` (src/helpers.py:594-603: the original
   * vocabulary rows ++ the rows of the added tokens) as ONE GEMM without a concatenated copy of the 197 MB head weight.
   * N counts logical rows and may exceed w2_row0 + w2_rows (padding columns repeat the last w2 row).  w2 = NULL: plain. */
  const void* w2;
  int32_t w2_row0;
  int32_t w2_rows;
  /* Normalisation folded into the GEMMs (bf16 MFMA path; HF:phi3/modeling_phi3.py:266-284 RMSNorm, torch.nn.LayerNorm of
   * HF:siglip/modeling_siglip.py:329-354) - the pre-norm of a block costs no launch and no pass over the activations:
   *   consumer   y = act( row_scale[m] * (x W'^T - row_shift[m] * col_shift[n]) + bias ) [+ residual]
   *              RMSNorm: W' = W diag(gain), row_scale = 1/rms(x_m), row_shift = NULL.
   *              LayerNorm: W' = W diag(gain), row_scale = 1/std(x_m), row_shift = mean(x_m), col_shift[n] = sum_k W'[n][k] (f32),
   *              bias = W beta + b.  (W', col_shift and that bias are prepared once per weight by the caller.)
   *   producer   stats_rstd != NULL: while writing y, the GEMM also computes the row statistics of y AS STORED (bf16):
   *              stats_rstd[m] = 1/sqrt(mean(y_m^2) + eps)                      (stats_mean == NULL: RMSNorm of the next block)
   *              stats_mean[m] = mean(y_m), stats_rstd[m] = 1/sqrt(var(y_m) + eps)   (stats_mean != NULL: LayerNorm)
   *              Accuracy: the variance is s2 / N - mean^2 in f32, so the relative error of the LayerNorm stats_rstd grows as
   *              1 + 2 (mean/std)^2 of the row - about 2e-7 at mean = 0, 3e-4 at 32 and 5e-3 at 128 standard deviations
   *              (tests/norm_fold_cases.py derives the bound); aki_row_stats takes the variance in two passes and has no such growth.
   *              stats_workspace: aki_linear_stats_workspace_bytes(M, N_out) bytes, 16-byte aligned, ZERO-FILLED ONCE by the
   *              caller before its first use (arrival counters at its front, which every launch puts back to zero; launches
   *              sharing a workspace must be stream-ordered).  The counter area has a fixed size -
   *              aki_linear_stats_counter_bytes(M) is the same 1 MiB for every M - so one buffer sized for the largest
   *              (M, N_out) serves any sequence of smaller and larger launches without being zero-filled again.
   *              M <= 16 777 216 rows; act must not be SWIGLU.
   * All NULL: plain GEMM. */
  const float* row_scale;
  const float* row_shift;
  const float* col_shift;
  float* stats_rstd;
  float* stats_mean;
  float stats_eps;
  void* stats_workspace;
  size_t stats_workspace_bytes;
  /* Split-K workspace (optional; bf16, act NONE).  Launches with few rows (a one-sample prefill: M = 655 / 207 against N = 3072) have
   * too few output tiles to fill the chip; given this buffer the library may split the K range of a tile over several workgroups
   * whose f32 partial sums meet here and are added in a FIXED order by the last one to arrive (bit-reproducible).  256-byte aligned,
   * aki_linear_splitk_workspace_bytes(M, N, K) bytes or more (0: this shape is never split), ZERO-FILLED ONCE by the caller (tickets
   * at its front, put back to zero by every launch; launches sharing it must be stream-ordered).  NULL / too small: no split. */
  void* splitk_workspace;
  size_t splitk_workspace_bytes;
  /* Training forward of the gated MLP (bf16, act SWIGLU; HF:phi3/modeling_phi3.py:49-64 under autograd): besides y = silu(g) * u the
   * launch leaves the pre-activations [g | u] as bf16 [M, N] (row stride ld_preact elements, a multiple of 4, >= N; 8-byte aligned) for the
   * backward pass, and takes the activation OF those bf16 values - the same numbers aki_linear_fwd (act NONE) followed by aki_swiglu_fwd
   * produce, without the second pass over [M, N].  NULL: not kept (inference). */
  void* preact_out;
  int64_t ld_preact;
} aki_linear_args;

int aki_linear_fwd(const aki_linear_args* args, void* stream);
size_t aki_linear_stats_workspace_bytes(int32_t M, int32_t N_out);
size_t aki_linear_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K);
size_t aki_linear_stats_counter_bytes(int32_t M);
/* aki_row_stats - the same statistics for a tensor no GEMM of this library produced (the first block's input): rstd[m] (and,
 * when mean != NULL, mean[m]) of x [rows, cols] bf16. */
int aki_row_stats(const void* x, int32_t rows, int32_t cols, int32_t ldx, float eps, float* rstd, float* mean, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Normalisation.  rmsnorm: HF:phi3/modeling_phi3.py:266-284 (fp32 statistics, result cast to the
 * input dtype BEFORE the gain multiply).  layernorm: torch.nn.LayerNorm (src/helpers.py:35,69-70,168).
 * ---------------------------------------------------------------------------------------------- */
int aki_rmsnorm_fwd(const void* x, const void* weight, void* y, int32_t rows, int32_t cols, int32_t ldx, int32_t ldy,
                    float eps, int32_t dtype, void* stream);
int aki_layernorm_fwd(const void* x, const void* weight, const void* bias, void* y, int32_t rows, int32_t cols,
                      int32_t ldx, int32_t ldy, float eps, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * aki_patch_embed_fwd - SigLIP patch embedding: Conv2d(3->E, k=P, s=P, valid) + flatten + pos-emb.
 * Replaces: `SiglipVisionEmbeddings.forward`, HF:siglip/modeling_siglip.py:175-185 (call site src/vlm.py:202-203).
 *   pixels [N,3,S,S] ; w [E, Kp] = conv weight flattened to [E,3*P*P] and zero-padded to Kp = roundup(3*P*P,64)
 *   bias [E] ; pos [G*G,E] (G = S/P) ; out [N,G*G,E] ; workspace = aki_patch_embed_workspace_bytes().
 * ---------------------------------------------------------------------------------------------- */
size_t aki_patch_embed_workspace_bytes(int32_t N, int32_t S, int32_t P, int32_t dtype);
int aki_patch_embed_fwd(const void* pixels, const void* w, const void* bias, const void* pos, void* out, int32_t N,
                        int32_t S, int32_t P, int32_t E, int32_t Kp, int32_t dtype, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Connector MLP (the Perceiver FeedForward block and the final projection).
 * aki_connector_mlp_fwd : out = x + W2 gelu(W1 LN(x))          - src/helpers.py:32-39,194
 * aki_connector_proj_fwd: out = Wp LN(x) + bp                   - src/helpers.py:196-197
 *   x [rows,d] ; w1 [4d,d] ; w2 [d,4d] ; workspace rows*(d+4d) elements.
 * ---------------------------------------------------------------------------------------------- */
size_t aki_connector_mlp_workspace_bytes(int32_t rows, int32_t d, int32_t d_inner, int32_t dtype);
int aki_connector_mlp_fwd(const void* x, const void* ln_w, const void* ln_b, const void* w1, const void* w2, void* out,
                          int32_t rows, int32_t d, int32_t d_inner, float eps, int32_t dtype, void* workspace,
                          size_t workspace_bytes, void* stream);
int aki_connector_proj_fwd(const void* x, const void* ln_w, const void* ln_b, const void* w, const void* b, void* out,
                           int32_t rows, int32_t d, int32_t d_out, float eps, int32_t dtype, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Language-stream fusion (integer / byte work).
 * aki_splice_plan : per sample, count <image> placeholders, find the first id == assistant_token_id
 *                   and the expanded length L_i = T - n_img + Nv*n_img   (src/vlm.py:488-496)
 *                   plan [B][AKI_PLAN_STRIDE] int32 = {n_img, q_idx, L_i, 0, t_0 .. t_7} with t_k the
 *                   index of the k-th placeholder (more than AKI_MAX_RECTS images per sample: unsupported)
 * aki_splice_fwd  : DecoupledEmbedding gather (src/helpers.py:445-484) + vision-token splice
 *                   (src/vlm.py:539-577) + padding with the scalar pad_token_id / -100
 *                   (src/vlm.py:584-598, src/utils.py:62-96) + the mask table (rects, valid bits).
 *   lang_x/attention_mask/labels int64 [B,T] ; embed_weight [V,d] ; embed_additional [n_add,d] or NULL
 *   vision_tokens [B,T_img,Nv,d] ; outputs sized for L_out = max_i L_i (right or left padding).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const int64_t* lang_x;
  const int64_t* attention_mask; /* NULL = all ones */
  const int64_t* labels;         /* NULL = no labels */
  const void* embed_weight;
  const void* embed_additional;
  const void* vision_tokens;
  const int32_t* plan; /* from aki_splice_plan */
  void* inputs_embeds; /* [B,L_out,d] */
  int64_t* labels_out; /* [B,L_out] or NULL */
  int64_t* mask_1d_out;/* [B,L_out] spliced 1-D mask, zero padded (always right-aligned like the reference's 2-D masks) */
  aki_mma_rect* rects; /* [B][max_rects] */
  uint64_t* col_valid_bits; /* [B][ceil(L_out/64)] */
  int32_t* seq_lens;        /* [B] = L_i */
  int64_t max_original_id;
  int64_t media_token_id;
  int64_t pad_token_id;
  int32_t B, T, T_img, Nv, d, L_out;
  int32_t max_rects;
  int32_t padding_side; /* 0 = right, 1 = left (embeds/labels only, src/utils.py:88-92) */
  int32_t dtype;
} aki_splice_args;

int aki_splice_plan(const int64_t* lang_x, int32_t B, int32_t T, int64_t media_token_id, int64_t assistant_token_id,
                    int32_t Nv, int32_t* plan, void* stream);
int aki_splice_fwd(const aki_splice_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decode path (after the MMA prefill): one new token per sequence.
 * Replaces the per-token steps of `lang_model.generate` as driven by src/aki.py:136-209 and the patched
 * `_update_model_kwargs_for_generation` (src/aki_generation.py:36-86): after the prefill the mask is all ones, i.e.
 * the new token attends to everything cached.  aki_linear_fwd streams weights with a GEMV kernel when M <= 8.
 * aki_rope_append_fwd : qkv [B,3*H*Dh] of the new tokens -> rotated q [B,H,Dh]; rotated k and v appended to the caches
 *                       [B,H,capacity,Dh] at index cache_len[b] (device int32); pos[b] = row into cos/sin.
 * aki_decode_attn_fwd : o [B,H*Dh] = softmax(q K^T * scale) V over the first n_keys[b] cache rows (device int32),
 *                       optional valid bits [B][nwords] of the prefill columns (padding), NULL = all valid; columns at
 *                       and past 64 * nwords count as valid.  A row with no visible key at all (every one of its
 *                       n_keys[b] columns lies inside the words with its bit clear) gets o = 0, not NaN.
 *                       bf16/Dh=96 runs split over the keys (flash-decoding) and needs the workspace below; max_keys is
 *                       a HOST upper bound of max_b n_keys[b] (<= capacity; 0 = capacity) that sizes the grid - keys
 *                       beyond it are not visited.
 * aki_decode_attn_fused_fwd : the two calls above in one launch (bf16, Dh=96): qkv rows in, rotated k / v appended at
 *                       cache_len[b] (which is also the RoPE position), attention over cache_len[b]+1 keys.
 *                       Returns AKI_ERR_UNSUPPORTED for f32 / other head sizes (use the two separate calls).
 * Workspace: aki_decode_attn_workspace_bytes(B,H,Dh,capacity) bytes, caller-owned, ZERO-FILLED ONCE before its first
 *                       use and then passed unchanged from call to call (it holds per-row arrival counters that the
 *                       kernel re-arms itself); calls sharing one workspace must be stream-ordered.
 * aki_decode_linear_fwd : aki_linear_fwd for M <= 8 bf16 rows with the layer's RMSNorm applied to x on the way in:
 *                       y = act(rmsnorm(x; rms_weight, eps) W^T + bias) [+ residual]  (HF:phi3/modeling_phi3.py:266-284
 *                       pre-norm followed by qkv_proj / gate_up_proj).  AKI_ERR_UNSUPPORTED if M > 8 or M*K > 64 Ki.
 * ---------------------------------------------------------------------------------------------- */
int aki_rope_append_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* pos, const int32_t* cache_len,
                        void* q_out, void* k_cache, void* v_cache, int32_t B, int32_t H, int32_t Dh, int32_t capacity,
                        int32_t dtype, void* stream);
size_t aki_decode_attn_workspace_bytes(int32_t B, int32_t H, int32_t Dh, int32_t capacity);
int aki_decode_attn_fwd(const void* q, const void* k_cache, const void* v_cache, void* o, const int32_t* n_keys,
                        const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H, int32_t Dh, int32_t capacity,
                        int32_t max_keys, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream);
int aki_decode_attn_fused_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, void* k_cache,
                              void* v_cache, void* o, const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H,
                              int32_t Dh, int32_t capacity, int32_t max_keys, float scale, int32_t dtype, void* ws,
                              size_t ws_bytes, void* stream);
int aki_decode_linear_fwd(const aki_linear_args* args, const void* rms_weight, float rms_eps, void* stream);

/* fp8 (e4m3) KV cache - an opt-in format for batched and long-context decode (Phi3ForCausalLM.set_kv_cache_dtype("fp8_e4m3")).
 * A cache row (one head, one position, Dh = 96 values) is 96 e4m3 bytes plus one f32 dequantisation scale:
 *   s = max(amax, 1e-12) / 448 over the row,  byte = e4m3(x / s) rounded to nearest even, saturating at +-448
 * (the rule of aki_quant_rows_fp8).  Caches are k/v [B, H, capacity, 96] uint8 and k_scale/v_scale [B, H, capacity] f32.
 * aki_kv_cache_quant_fp8 : rows [0, rows) of every slab of a bf16 cache src [slabs, src_capacity, 96] -> dst [slabs, dst_capacity, 96]
 *                       bytes + scale [slabs, dst_capacity]: the prefill's K/V (written in bf16 by the unchanged prefill kernels into
 *                       a staging cache) converted in one launch (slabs = 2 * layers * B * H).
 * aki_decode_attn_fused_fp8kv_fwd : aki_decode_attn_fused_fwd on the e4m3 cache - the rotated k (rounded to bf16) and v of the new
 *                       token are quantised per head and appended (bytes + scales) at cache_len[b], then attended through their
 *                       quantised copy like every cached key: score = (q . k8) * s_k * scale, row j of V weighted by p_j * s_v[j].
 *                       Same workspace (aki_decode_attn_workspace_bytes) and max_keys as aki_decode_attn_fused_fwd.
 * Both: NULL pointers -> AKI_ERR_INVALID_ARG; Dh != 96 or dtype != AKI_DT_BF16 -> AKI_ERR_UNSUPPORTED.
 * AKI_ABI_VERSION was not bumped for these two functions: they are purely additive (no existing symbol or struct changed). */
int aki_kv_cache_quant_fp8(const void* src, int32_t src_capacity, void* dst, float* scale, int32_t dst_capacity, int32_t slabs, int32_t rows,
                           int32_t Dh, int32_t dtype, void* stream);
int aki_decode_attn_fused_fp8kv_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, void* k_cache,
                                    void* v_cache, float* k_scale, float* v_scale, void* o, const uint64_t* col_valid_bits, int32_t nwords,
                                    int32_t B, int32_t H, int32_t Dh, int32_t capacity, int32_t max_keys, float scale, int32_t dtype, void* ws,
                                    size_t ws_bytes, void* stream);

/* Grouped decode attention - N returned rows per prompt sample over ONE copy of the prompt's K/V (AKI.generate(num_return_sequences=N);
 * bf16, Dh = 96).  The cache has two parts:
 *   k_prefix / v_prefix [B0, H, prefix_capacity, 96]   the prompt's rows as the prefill wrote them, one slab per prompt sample; READ-ONLY here
 *   k_suffix / v_suffix [B0*N, H, suffix_capacity, 96] one slab per returned row: the tokens decoded so far
 * Row r belongs to sample b = r / N.  Its keys are prefix rows [0, prefix_len[b]) - filtered by the sample's col_valid_bits words
 * ([B0][nwords], NULL = all valid) - followed by suffix rows [0, cache_len[r] - prefix_len[b]].  The last of those is the new token: its k is
 * rotated at position cache_len[r] (= the cos/sin row) and appended with its v at suffix row cache_len[r] - prefix_len[b], which must lie
 * in [0, suffix_capacity) (a row outside it is not appended and sees its prefix only).  qkv [B0*N, 3*H*96] un-rotated, o [B0*N, H*96].
 * A 64-key prefix tile is loaded once per (sample, head, chunk of 16 rows) and dotted with all of the chunk's queries.
 * max_prefix_keys / max_suffix_keys: HOST upper bounds of prefix_len[b] and of the suffix keys (new token included); 0 = the capacity.
 * They size the grid only: the result does not depend on them, bit for bit, while they cover the keys.
 * Workspace: aki_decode_attn_group_workspace_bytes(...) bytes, caller-owned, ZERO-FILLED ONCE, then passed unchanged (stream-ordered).
 * NULL pointers -> AKI_ERR_INVALID_ARG; Dh != 96 or dtype != AKI_DT_BF16 -> AKI_ERR_UNSUPPORTED; a short workspace -> AKI_ERR_WORKSPACE.
 * Purely additive: AKI_ABI_VERSION was not bumped. */
size_t aki_decode_attn_group_workspace_bytes(int32_t B0, int32_t N, int32_t H, int32_t Dh, int32_t prefix_capacity, int32_t suffix_capacity);
int aki_decode_attn_group_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, const int32_t* prefix_len,
                              const void* k_prefix, const void* v_prefix, void* k_suffix, void* v_suffix, void* o,
                              const uint64_t* col_valid_bits, int32_t nwords, int32_t B0, int32_t N, int32_t H, int32_t Dh,
                              int32_t prefix_capacity, int32_t suffix_capacity, int32_t max_prefix_keys, int32_t max_suffix_keys, float scale,
                              int32_t dtype, void* ws, size_t ws_bytes, void* stream);

/* Chunk attention - T new tokens per sample appended to a KV cache and attended in one pass (the continuation of a cached sequence by
 * more than one token; bf16, Dh = 96, MHA).  qkv [B*T, 3*H*96] un-rotated, row b*T + t = token t of sample b.  Two launches on `stream`:
 *   1. for every t < n_new[b]: q and k rotated at position cache_len[b] + t (= the cos/sin row), q to the workspace, k / v to cache row
 *      cache_len[b] + t of k_cache / v_cache [B, H, capacity, 96]; rows t >= n_new[b] write nothing.
 *   2. query t attends to keys j < cache_len[b] whose bit in col_valid_bits ([B][nwords], NULL = all valid; columns past nwords*64 are
 *      valid) is set, and to the chunk's keys cache_len[b] + u with u <= t.  o [B*T, H*96]; rows t >= n_new[b] are written as zeros.
 * n_new: [B] real tokens per sample of a right-padded chunk, NULL = T everywhere.  max_new: HOST upper bound of n_new (0 = T); rows of o
 * from the 32-row block past it on are NOT written.  cache_len is not advanced.  The caller guarantees cache_len[b] + n_new[b] <= capacity
 * (rows past the capacity are neither appended nor read).  The result is a function of the inputs alone, bit for bit.
 * Workspace: aki_chunk_attn_workspace_bytes(B, H, T, Dh) bytes (0 for unsupported sizes), no initialisation needed.
 * NULL pointers, B / H / T / capacity < 1 -> AKI_ERR_INVALID_ARG; Dh != 96 or dtype != AKI_DT_BF16 -> AKI_ERR_UNSUPPORTED; a short
 * workspace -> AKI_ERR_WORKSPACE.  Purely additive: AKI_ABI_VERSION was not bumped (it stays 17). */
size_t aki_chunk_attn_workspace_bytes(int32_t B, int32_t H, int32_t T, int32_t Dh);
int aki_chunk_attn_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, const int32_t* n_new, void* k_cache,
                       void* v_cache, void* o, const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H, int32_t Dh, int32_t T,
                       int32_t max_new, int32_t capacity, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream);

/* aki_decode_chain_fwd - ALL decoder layers of one decode step for ONE sequence (batch 1) in one launch (bf16 weights, or
 * AKI_DT_W8A16: e4m3 weights with one f32 scale per weight row).  Same arithmetic as the per-layer calls above
 * (aki_decode_linear_fwd -> aki_decode_attn_fused_fwd -> aki_linear_fwd + residual -> aki_decode_linear_fwd SwiGLU -> aki_linear_fwd
 * + residual), bit for bit; what changes is the schedule: every workgroup issues its weight loads before it waits for its
 * input vector, so the weight stream runs ahead of the dependency chain across phase and layer seams (decode_chain.hip).
 *   layers        DEVICE array of n_layers descriptors (weights as stored by nn.Linear, [N, K] row-major, K contiguous;
 *                 k_cache / v_cache [1, H, capacity, 96] bf16; s_* = per-row scales for AKI_DT_W8A16, else NULL)
 *   h_in / h_out  [d] bf16: the new token's embedding in, the residual stream after the last layer out (PRE final norm)
 *   cache_len     device int32 [1]: tokens cached so far = the new token's position and append index (not advanced here)
 *   max_keys      host upper bound of cache_len + 1 that sizes the attention split (0 = capacity)
 *   workspace     aki_decode_chain_workspace_bytes(...) bytes, 256-byte aligned, ZERO-FILLED ONCE by the caller before its
 *                 first use and owned by the calls from then on (one call in flight per workspace): it holds two sets of arrival
 *                 counters and the count of completed calls - a call uses the set of its parity and leaves the other one zeroed
 *                 for its successor, so a decode step is ONE launch.  The 32-bit word at aki_decode_chain_error_offset(...) is
 *                 sticky: 0 = every wait of every call so far was satisfied; otherwise (layer << 8 | phase) of a wait that gave
 *                 up after its bounded spin (the launch then drains and h_out is garbage) - read it after synchronising, and
 *                 zero-fill the workspace again before any further call on it.
 * Supported: Dh = 96, d = H * 96 = 3072, F = 8192 (Phi-3.5-mini); AKI_ERR_UNSUPPORTED otherwise (use the per-layer calls).
 * AKI_DT_W4A16 (batch 1 only; batch > 1 -> AKI_ERR_UNSUPPORTED): MXFP4 weights in the layout of aki_quant_mxfp4 - w_* are the nibbles
 * [N, K/2] bytes, dense, 16-byte aligned, and the s_* slots carry the e8m0 scale BYTES ws [N, K/32] (cast the uint8_t pointers to the
 * slots' type; nothing is read through them as float).  The step then reproduces the per-layer aki_linear_w4_fwd calls at M = 1 bit for bit.
 * The descriptors live in DEVICE memory, so the entry point cannot see their pointers: a NULL s_* under AKI_DT_W8A16 / AKI_DT_W4A16 is the
 * caller's error to prevent, for both formats alike (ops.DecodeChain checks it on the host before it builds the table).
 * AKI_DT_W4A16 is purely additive: AKI_ABI_VERSION was not bumped. */
typedef struct {
  const void* w_qkv;
  const void* w_o;
  const void* w_gate_up;
  const void* w_down;
  const void* norm1;
  const void* norm2;
  void* k_cache;
  void* v_cache;
  const float* s_qkv;
  const float* s_o;
  const float* s_gate_up;
  const float* s_down;
} aki_decode_chain_layer;

typedef struct {
  const aki_decode_chain_layer* layers;
  const void* h_in;
  void* h_out;
  const float* cos;
  const float* sin;
  const int32_t* cache_len;
  const uint64_t* col_valid_bits;
  void* workspace;
  size_t workspace_bytes;
  int32_t n_layers;
  int32_t nwords;
  int32_t d;
  int32_t H;
  int32_t Dh;
  int32_t F;
  int32_t capacity;
  int32_t max_keys;
  float scale;
  float rms_eps;
  int32_t dtype;
  int32_t batch; /* 0 or 1: one sequence.  2..8 (bf16): that many sequences per step - h_in / h_out are [batch, d] rows, cache_len [batch],
                    col_valid_bits [batch][nwords], k_cache / v_cache [batch, H, capacity, 96]; the GEMV phases become 16-feature MFMA tiles and
                    the step reproduces the per-layer batched calls (aki_decode_linear_fwd / aki_linear_fwd at 2-8 rows,
                    aki_decode_attn_fused_fwd) bit for bit.  Workspace: the *_batch_* functions below. */
} aki_decode_chain_args;

size_t aki_decode_chain_workspace_bytes(int32_t n_layers, int32_t d, int32_t H, int32_t F, int32_t capacity);
size_t aki_decode_chain_error_offset(int32_t n_layers, int32_t H);
size_t aki_decode_chain_batch_workspace_bytes(int32_t n_layers, int32_t d, int32_t H, int32_t F, int32_t capacity, int32_t batch);
size_t aki_decode_chain_batch_error_offset(int32_t n_layers, int32_t H, int32_t batch);
int aki_decode_chain_fwd(const aki_decode_chain_args* args, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training step (BASELINE configs[2]).  The reference's backward is torch autograd over its
 * eager forward under bf16 autocast, followed by clip_grad_norm_(1.0) and AdamW (train/train_utils.py:242-266,
 * train/train.py:330-337, train/losses.py:83-116).  These entry points are the kernels an autograd wrapper of the
 * forward ops needs; all of them are bf16 (dtype must be AKI_DT_BF16), caller-owned buffers, stream-ordered.
 * GEMM-shaped gradients: dX = dY W runs through aki_linear_fwd on W^T (aki_transpose, once per optimizer step), dW = dY^T X through aki_gemm_tn.
 *
 * aki_attn_bwd      backward of aki_mma_attn_core_fwd (masked = 1; needs Lq == Lk) or of aki_attn_fwd (masked = 0):
 *                   q,k,v [B,H,L,Dh] (k rotated) as the forward saw them, o and d_o [B,Lq,H*Dh], lse [B,H,Lq] from the
 *                   forward -> dq,dk,dv [B,H,L,Dh].  Dh 96 or 64.  Rows >= seq_lens[b] get zero gradient.
 * aki_transpose     y[C][ldy] = x[R][C]^T with columns R..Rpad-1 of y zero-filled (Rpad <= ldy).
 * aki_gemm_tn       c[I][ldc] = sum over the Kc rows of a[Kc][lda]^T b[Kc][ldb]: the weight gradient dW = dY^T X on dY [M,N] and X [M,K] AS THEY LIE
 *                   (contraction over the row index of both; the operands are staged row-major and read transposed from LDS - no
 *                   aki_transpose pass).  I, J, lda, ldb multiples of 8, ldc of 4; a, b 16-byte aligned, c 8-byte aligned.
 * aki_norm_bwd      RMSNorm (rms=1) / LayerNorm backward: dx [rows,cols] (+ dres when given: the gradient arriving through
 *                   the residual branch of a pre-norm block, so the two are summed without a separate pass); dw (and db
 *                   for LayerNorm) [cols], written or accumulated (accumulate=1).  cols % 8 == 0, cols <= 4096.
 * aki_colsum        out[c] (+)= sum_r x[r][c]   (bias gradients)
 * aki_swiglu_fwd/_bwd   a = up * silu(gate) on gate_up [rows, 2F] (gate first), and its backward to d(gate_up)
 * aki_gelu_fwd/_bwd     erf GELU (src/helpers.py:32-39), n elements, n % 8 == 0
 * aki_rope_bwd_merge    dq,dk,dv [B,H,L,Dh] -> d(qkv) [B*L, 3*H*Dh] through the transpose of the rotate-half RoPE
 * aki_ce_loss_fwd_bwd   HF shifted cross-entropy: row (b,t) against labels[b][t+1], ignore_index -100;
 *                       loss_rows [B*L] f32 (sum / *n_valid = loss), n_valid: device int32 (written),
 *                       dlogits (may alias logits, may be NULL) = d(mean loss)/d(logits) * gscale
 *                       Only columns 0..V-1 of a row are read or written: columns V..ldl-1 of logits and V..lddl-1 of dlogits
 *                       keep whatever they held (ignored rows get zeros in columns 0..V-1 only).
 * aki_ce_rows_fwd_bwd   the same arithmetic for an arbitrary CHUNK of rows: targets[r] is the (already shifted) class of row r
 *                       (< 0 or >= V: ignored row), *n_valid (device int32) is an INPUT - the number of scored rows of the
 *                       whole batch.  With it the lm_head and the loss run chunk by chunk and the [B, L, V] logits tensor
 *                       is never formed (src/helpers.py:594-603 + train/losses.py:83-116).
 * aki_grad_sqnorm       *out (+)= sum g^2 over a gradient buffer (n % 8 == 0; dtype AKI_DT_BF16, or AKI_DT_F32 for the fp32 exchange)
 * aki_adamw_step        fp32 master weights p, moments m, v; bf16 gradients g -> updated p/m/v and bf16 weights w16.
 *                       g is scaled by gscale (1/world, 1/grad_accum) and, when sqnorm != NULL and max_norm > 0, clipped by
 *                       min(1, max_norm / (sqrt(*sqnorm) * gscale + 1e-6))  (torch.nn.utils.clip_grad_norm_ semantics).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; const void* k; const void* v;
  const void* o; const void* d_o;
  const float* lse;
  void* dq; void* dk; void* dv;
  const aki_mma_rect* rects; int32_t max_rects;
  const uint64_t* col_valid_bits;
  const int32_t* seq_lens;
  int32_t masked;
  int32_t B, H, Lq, Lk, Dh;
  float scale;
  int32_t dtype;
} aki_attn_bwd_args;

size_t aki_attn_bwd_workspace_bytes(int32_t B, int32_t H, int32_t Lq);
int aki_attn_bwd(const aki_attn_bwd_args* args, void* workspace, size_t workspace_bytes, void* stream);
int aki_transpose(const void* x, void* y, int32_t R, int32_t C, int32_t ldx, int32_t ldy, int32_t Rpad, int32_t dtype, void* stream);
int aki_gemm_tn(const void* a, const void* b, void* c, int32_t Kc, int32_t I, int32_t J, int64_t lda, int64_t ldb, int64_t ldc, int32_t dtype,
                void* stream);
size_t aki_norm_bwd_workspace_bytes(int32_t cols);
int aki_norm_bwd(int32_t rms, const void* x, const void* w, const void* dy, const void* dres, void* dx, void* dw, void* db,
                 int32_t rows, int32_t cols, int32_t ldx, int32_t lddy, int32_t lddr, int32_t lddx, float eps, int32_t accumulate,
                 int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);
size_t aki_colsum_workspace_bytes(int32_t cols);
int aki_colsum(const void* x, void* out, int32_t rows, int32_t cols, int32_t ldx, int32_t accumulate, int32_t dtype, void* workspace,
               size_t workspace_bytes, void* stream);
int aki_swiglu_fwd(const void* gate_up, void* a, int32_t rows, int32_t F, int32_t ldg, int32_t lda, int32_t dtype, void* stream);
int aki_swiglu_bwd(const void* gate_up, const void* da, void* dgate_up, int32_t rows, int32_t F, int32_t ldg, int32_t ldda,
                   int32_t lddg, int32_t dtype, void* stream);
int aki_gelu_fwd(const void* x, void* y, size_t n, int32_t dtype, void* stream);
int aki_gelu_bwd(const void* x, const void* dy, void* dx, size_t n, int32_t dtype, void* stream);
int aki_rope_bwd_merge(const void* dq, const void* dk, const void* dv, const float* cos, const float* sin, const int32_t* position_ids,
                       void* dqkv, int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype, void* stream);
int aki_ce_loss_fwd_bwd(const void* logits, const int64_t* labels, int32_t* n_valid, float* loss_rows, void* dlogits, int32_t B,
                        int32_t L, int32_t V, int32_t ldl, int32_t lddl, float gscale, int32_t dtype, void* stream);
int aki_ce_rows_fwd_bwd(const void* logits, const int64_t* targets, const int32_t* n_valid, float* loss_rows, void* dlogits,
                        int32_t rows, int32_t V, int32_t ldl, int32_t lddl, float gscale, int32_t dtype, void* stream);
size_t aki_grad_sqnorm_workspace_bytes(void);
int aki_grad_sqnorm(const void* g, size_t n, float* out, int32_t accumulate, int32_t dtype, void* workspace, size_t workspace_bytes,
                    void* stream);
int aki_adamw_step(float* p, float* m, float* v, const void* g, void* w16, size_t n, const float* sqnorm, float max_norm, float gscale,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);
/* aki_adamw_step for ONE 2-D weight [N, K] (K % 4 == 0) that also writes W^T [K, ldT] (ldT = N rounded up to x64, padding columns zero) -
 * what aki_transpose would make of the updated bf16 weight, in the same pass (the backward's input-gradient GEMMs read W^T).
 * grad_dtype: AKI_DT_BF16 or AKI_DT_F32. */
int aki_adamw_step_t(float* p, float* m, float* v, const void* g, void* w16, void* wT, int32_t N, int32_t K, int32_t ldT, const float* sqnorm,
                     float max_norm, float gscale, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                     int32_t grad_dtype, void* stream);
/* the same update from FP32 gradients: the reference's DDP path under `--precision amp_bf16` keeps fp32 parameters, so the gradients
 * it all-reduces and its optimizer consumes are fp32 (train/train.py:311-312, train/train_utils.py:56-65) - AkiTrainer(reduce_dtype=float32) */
int aki_adamw_step_g32(float* p, float* m, float* v, const float* g, void* w16, size_t n, const float* sqnorm, float max_norm, float gscale,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* aki_quant_rows_fp8 - q[r][c] = e4m3(y[r][c] / scale[r]), scale[r] = max_c |y[r][c]| / 448, with y = x (bf16 [rows, cols])
 * or, when rms_weight != NULL, y = Phi3RMSNorm(x; rms_weight, rms_eps) (HF:phi3/modeling_phi3.py:266-284) - the input side
 * of the fp8 projections of BASELINE configs[4].  Also used once per nn.Linear weight (one scale per output feature).
 * cols % 8 == 0, cols <= 8192; q is [rows, ldq] bytes. */
int aki_quant_rows_fp8(const void* x, const void* rms_weight, float rms_eps, void* q, float* scale, int32_t rows, int32_t cols,
                       int32_t ldx, int32_t ldq, void* stream);

/* MXFP4 weight-only decode - an opt-in 4.25-bit weight format for the decode rows (Phi3ForCausalLM.enable_mxfp4()).  OCP microscaling: a weight
 * row [K] (K % 32 == 0) is cut into blocks of 32 consecutive k; a block is 32 e2m1 nibbles (sign in bit 3; magnitudes 0, 0.5, 1, 1.5, 2, 3,
 * 4, 6) and one e8m0 scale byte, value = nibble * 2^(byte - 127).  wq is [N, K/2] bytes (byte j of a row: k = 2j in the low nibble, k = 2j+1
 * in the high one), ws is [N, K/32] bytes, both dense.
 * aki_quant_mxfp4   : bf16 w [N, ldw] -> wq, ws.  Per block: e = floor(log2(amax)) - 2, byte = clamp(e + 127, 0, 254) (never 255), elements
 *                     v / 2^e rounded to the nearest e2m1 value, ties to the even code, saturating at +-6; an all-zero block gets byte 127 and
 *                     zero nibbles.  Inputs must be finite (the caller checks).  ldw % 8 == 0; w and wq 16-byte aligned.
 * aki_linear_w4_fwd : y = act(x W^T + bias) [+ residual] for M <= 16 bf16 rows on such weights, optionally with the RMSNorm of
 *                     aki_decode_linear_fwd applied to x first (rms_weight != NULL; M <= 8 and narrow outputs only, as there).
 *                     args->w = the nibbles, args->ldw in BYTES (% 16), args->dtype = AKI_DT_BF16 (x and y), args->w_scale is ignored;
 *                     w_scale_e8m0 = ws.  M = 1: a dot-product GEMV; 2..16: the skinny MFMA GEMM with the K / N / alignment limits of the
 *                     AKI_DT_W8A16 one.  K % 32 != 0, M > 16 or a shape outside those limits -> AKI_ERR_UNSUPPORTED; NULL pointers ->
 *                     AKI_ERR_INVALID_ARG; x / w / rms_weight not 16-byte aligned -> AKI_ERR_ALIGNMENT.  Nothing is launched on an error.
 * Purely additive: AKI_ABI_VERSION was not bumped. */
int aki_quant_mxfp4(const void* w, int32_t N, int32_t K, int32_t ldw, uint8_t* wq, uint8_t* ws, void* stream);
int aki_linear_w4_fwd(const aki_linear_args* args, const uint8_t* w_scale_e8m0, const void* rms_weight, float rms_eps, void* stream);

/* aki_mma_mask_dense - materialise the reference's (B,1,L,L) int64 0/1 mask from the table, for
 * callers that still want it (bit-exact vs src/vlm.py:410-443 + src/utils.py:99-108). */
int aki_mma_mask_dense(const aki_mma_rect* rects, int32_t max_rects, const uint64_t* col_valid_bits,
                       const int32_t* seq_lens, int32_t B, int32_t L, int64_t* out, void* stream);

/* aki_mma_mask_to_table - the inverse: the reference's LM hand-off type, `attention_mask` (B,1,L,L) int64 0/1 as returned
 * by `_prepare_inputs_for_forward` (src/vlm.py:589-603) and passed to `lang_model(...)` (src/aki.py:125-130), converted on
 * the device into the table the attention kernels consume.
 *   mask [B,1,L,L] int64 (non-zero = visible) -> rects [B][max_rects], col_valid_bits [B][ceil(L/64)], seq_lens [B],
 *   status [B] device int32: 0 = ok, n > max_rects = the sample needs n row groups (its rects are then incomplete).
 *   workspace: aki_mma_mask_to_table_workspace_bytes(B, L) bytes.
 * The result is a CANDIDATE: only masks of the family {causal triangle + row-interval rectangles + invalid columns +
 * empty bottom rows} are representable.  The caller proves it by materialising the table again with aki_mma_mask_dense
 * and comparing with the input bit for bit (aki_amd/phi3.py does; anything else is refused, never approximated). */
size_t aki_mma_mask_to_table_workspace_bytes(int32_t B, int32_t L);
int aki_mma_mask_to_table(const int64_t* mask, int32_t B, int32_t L, int32_t max_rects, aki_mma_rect* rects,
                          uint64_t* col_valid_bits, int32_t* seq_lens, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream);

/* aki_sft_collate_pad - the SFT collate (train/sft_data_utils/loader_utils.py:11-91 `_pad_trunc` + `batch_collate_pad`) on the
 * device: B ragged samples, concatenated (sample b = elements offsets[b] .. offsets[b+1]-1 of ids / labels / attention_mask),
 * -> [B, T_out] int64 arrays.  A sample of T_out tokens or more keeps its FIRST T_out tokens; a shorter one is padded on the
 * right (padding_side 0) or left (1) with pad_token_id / ignore_index / 0.  T_out is the caller's: `max_length + 1` for
 * padding="max_length" (loader_utils.py:78-82), the longest sample for "longest" (:30-31).  labels / attention_mask and their
 * outputs may be NULL together. */
int aki_sft_collate_pad(const int64_t* ids, const int64_t* labels, const int64_t* attention_mask, const int32_t* offsets, int32_t B,
                        int32_t T_out, int64_t pad_token_id, int64_t ignore_index, int32_t padding_side, int64_t* out_ids,
                        int64_t* out_labels, int64_t* out_mask, void* stream);

/* aki_greedy_pick - the step between two decode steps of a greedy `generate` (HF GenerationMixin's greedy branch, which
 * src/aki.py:136-209 drives through src/aki_generation.py:36-86): per row b of bf16 logits [B, ld], V columns used,
 *   next = done[b] ? pad_token_id : argmax_v logits[b, v]     (ties: the lower index; a NaN outranks every number - torch.argmax)
 *   t = cache_len[b] + advance - start_len[b]                 (0 when cache_len is NULL; start_len NULL = zeros)
 *   tokens[b, t] = next (when tokens != NULL and 0 <= t < tokens_ld);  next_ids[b] = next
 *   a row that was not done and whose next is one of eos_ids becomes done (done[b] = 1, done_at[b] = t)
 *   advance = 1: cache_len[b] += 1 (the decode step's own advance, folded into this launch)
 * done / tokens / cache_len / start_len / done_at may be NULL.  One launch, no host value: it sits inside the replayed hipGraph
 * of a decode step, so a greedy token is one replay and the host looks at `done` every few tokens. */
int aki_greedy_pick(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                    uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                    int32_t advance, int32_t* done_at, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layer loops issued from ONE call (host code; csrc/stack.hip).  A one-sample prefill - the shape the reference's callers run
 * (local_demo.py:75-87, eval_cv_bench/eval.py:92-104) - is ~400 launches of 10-70 us: issued one by one from Python the HOST was 9 ms
 * of a 15 ms first token.  These two functions issue, on `stream`, exactly the launches of the per-layer entry points above, in
 * the order of HF:phi3/modeling_phi3.py `Phi3Model.forward` (:287-328 per layer) and HF:siglip/modeling_siglip.py:329-354 -
 * bf16 inference with the normalisations folded into the GEMMs (aki_linear_args: row_scale / row_shift / stats_*).
 *
 * aki_decoder_stack_fwd: per layer  q,k,v = RoPE(rstd (h W_qkv'^T)) -> span attention -> h1 = h + o W_o^T -> act = SwiGLU(rstd1 (h1 W_gu'^T))
 * -> h2 = h1 + act W_down^T, every h-writing GEMM leaving 1/rms of its rows for the next one.  W' = W diag(RMSNorm gain), prepared by the
 * caller.  k_cache / v_cache ([B,H,kv_capacity,Dh], all layers or none): rotated keys and values are written there (KV-cache prefill).
 *   h_in, h_out [B*L, d] bf16 (may not alias); rstd_out [B*L] f32 or NULL: 1/rms(h_out) for the final norm folded into the head;
 *   workspace: aki_decoder_stack_workspace_bytes() bytes, 256-byte aligned, scratch; stats_workspace / splitk_workspace as in
 *   aki_linear_args (zero-filled once by the caller; splitk optional).  `layers` is a HOST array. */
typedef struct {
  const void* w_qkv;     /* [3*H*Dh, d] */
  const void* w_o;       /* [d, H*Dh] */
  const void* w_gate_up; /* [2F, d] */
  const void* w_down;    /* [d, F] */
  void* k_cache;
  void* v_cache;
} aki_decoder_layer;

typedef struct {
  const aki_decoder_layer* layers;
  int32_t n_layers;
  const void* h_in;
  void* h_out;
  float* rstd_out;
  const float* cos;
  const float* sin;
  const int32_t* position_ids;
  int32_t pos_rows;
  const aki_mma_rect* rects;
  const uint64_t* col_valid_bits;
  const int32_t* seq_lens;
  int32_t max_rects;
  int32_t B, H, L, Dh, d, F;
  int32_t kv_capacity;   /* rows per (batch, head) of the caches; 0 with no caches */
  float scale;
  float rms_eps;
  int32_t dead_rows;
  void* workspace;
  size_t workspace_bytes;
  void* stats_workspace;
  size_t stats_workspace_bytes;
  void* splitk_workspace;
  size_t splitk_workspace_bytes;
} aki_decoder_stack_args;

size_t aki_decoder_stack_workspace_bytes(int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t d, int32_t F, int32_t keep_kv);
int aki_decoder_stack_fwd(const aki_decoder_stack_args* args, void* stream);

/* aki_siglip_stack_fwd: per layer  qkv = LN1(h) W_qkv^T + b (folded: rstd (h W'^T - mean c) + b') -> 16-head attention read in place out
 * of qkv -> h1 = h + out_proj -> fc1 + GELU with LN2 folded, into fc1_out -> h2 = h1 + fc2.  W', b', c = fold of the LayerNorm gain /
 * bias into the weight (see aki_linear_args), prepared by the caller; w_fc2 is K-padded to Ip (a multiple of 64) with zero columns.
 *   h_in, h_out [N*L, E] bf16; fc1_out [N*L, Ip] bf16, caller-owned, its pad columns [I, Ip) ZERO (nothing here writes them);
 *   workspace: aki_siglip_stack_workspace_bytes() bytes, 256-byte aligned, scratch.  `layers` is a HOST array. */
typedef struct {
  const void* w_qkv;  /* [3E, E] */
  const void* b_qkv;  /* [3E] */
  const float* c_qkv; /* [3E] f32 */
  const void* w_out;  /* [E, E] */
  const void* b_out;  /* [E] or NULL */
  const void* w_fc1;  /* [I, E] */
  const void* b_fc1;  /* [I] */
  const float* c_fc1; /* [roundup(I, 4)] f32 */
  const void* w_fc2;  /* [E, Ip] */
  const void* b_fc2;  /* [E] or NULL */
} aki_siglip_layer;

typedef struct {
  const aki_siglip_layer* layers;
  int32_t n_layers;
  const void* h_in;
  void* h_out;
  void* fc1_out;
  int32_t N, L, E, heads, I, Ip;
  int32_t act;       /* AKI_ACT_GELU_TANH (SigLIP) or AKI_ACT_GELU_ERF */
  float ln_eps;
  float scale;       /* softmax scale, (E / heads)^-0.5 as the caller's module computed it */
  void* workspace;
  size_t workspace_bytes;
  void* stats_workspace;
  size_t stats_workspace_bytes;
  void* splitk_workspace;
  size_t splitk_workspace_bytes;
} aki_siglip_stack_args;

size_t aki_siglip_stack_workspace_bytes(int32_t N, int32_t L, int32_t E, int32_t heads);
int aki_siglip_stack_fwd(const aki_siglip_stack_args* args, void* stream);

/* aki_perceiver_stack_fwd: the Perceiver connector (src/helpers.py:170-199: `depth` x [PerceiverAttention + residual, FeedForward + residual],
 * final LayerNorm, projection) for ONE (sample, image) pair - the one-sample case, where issuing its ~55 launches from Python takes longer than
 * they run.  x [n1, D] media features, latents [n2, D] (the learned latents), out [n2, D_out] (D_out = D without a projection).  Every
 * LayerNorm uses `eps`; the attention is softmax(scale q k^T) over the n1 + n2 keys LN_media(x) ++ LN_latents(latents).  Same launches as
 * aki_layernorm_fwd / aki_linear_fwd / aki_attn_fwd / aki_connector_mlp_fwd / aki_connector_proj_fwd issued one by one. */
typedef struct {
  const void* norm_media_w;
  const void* norm_media_b;
  const void* norm_latents_w;
  const void* norm_latents_b;
  const void* w_q;   /* [heads*dim_head, D] */
  const void* w_kv;  /* [2*heads*dim_head, D] */
  const void* w_out; /* [D, heads*dim_head] */
  const void* ff_ln_w;
  const void* ff_ln_b;
  const void* ff_w1; /* [d_ff, D] */
  const void* ff_w2; /* [D, d_ff] */
} aki_perceiver_layer;

typedef struct {
  const aki_perceiver_layer* layers;
  int32_t n_layers;
  const void* x;
  const void* latents;
  const void* norm_w;
  const void* norm_b;
  const void* proj_w; /* [D_out, D] or NULL */
  const void* proj_b;
  void* out;
  int32_t n1, n2, D, heads, dim_head, d_ff, D_out;
  float scale;
  float eps;
  void* workspace;
  size_t workspace_bytes;
} aki_perceiver_stack_args;

size_t aki_perceiver_stack_workspace_bytes(int32_t n1, int32_t n2, int32_t D, int32_t heads, int32_t dim_head, int32_t d_ff);
int aki_perceiver_stack_fwd(const aki_perceiver_stack_args* args, void* stream);

/* aki_greedy_pick_embed - aki_greedy_pick + the embedding lookup of the token it picked (`DecoupledEmbedding.forward`,
 * src/helpers.py:440-492, which HF's generate loop runs at the top of the next step): next_embeds[b, :] = bf16 row `next` of embed_weight
 * [max_original_id + 1 or more rows, d], or row `next - max_original_id - 1` of additional_weight [num_additional, d] when
 * next > max_original_id (additional_weight NULL: one table).  d % 8 == 0, 16-byte aligned tables; V may not exceed the number of rows.
 * next_embeds is what the following decode step takes as h_in: a greedy token is decode chain + head + this launch. */
int aki_greedy_pick_embed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                          uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                          int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                          int64_t num_additional, int32_t d, void* next_embeds, void* stream);

/* aki_logits_process - HF `generate`'s logits processors on one decode step's scores, in the order of
 * GenerationMixin._get_logits_processor, for a decoder-only model called with inputs_embeds only (src/aki.py:192-207): the processors'
 * input_ids are the row's GENERATED tokens h = tokens[b, 0:n), never the prompt.  logits [B, ld] (AKI_DT_BF16 or AKI_DT_F32, V columns
 * used) -> out f32 [B, ld_out] (out == logits is allowed for f32):
 *   repetition_penalty   every distinct token g of h: s = s < 0 ? s * penalty : s / penalty      (1.0 = off)
 *   no_repeat_ngram_size every token that completes an n-gram of h: -inf                            (0 = off)
 *   bad words            word w = bad_ids[bad_offsets[i] : bad_offsets[i + 1]], i < n_bad: its last token -inf when |w| == 1, or when
 *                        n >= |w| and h ends with w's first |w| - 1 tokens (bad_offsets: n_bad + 1 ascending entries in [0, n_bad_ids])
 *   min_length           every eos id -inf while n < min_length                                      (0 = off)
 *   suppress ids         -inf; begin-suppress ids -inf at n == 0
 *   n = step + (cache_len ? cache_len[b] - start_len[b] : 0), clamped to [0, tokens_ld] (0 when tokens is NULL): the greedy loop's device
 *   counters, so the launch can sit inside a replayed hipGraph.  Rows with done[b] != 0 are copied unprocessed.  Ids outside [0, V)
 *   are skipped.  V <= AKI_LOGITS_PROCESS_MAX_V.  One launch, no host value read. */
#define AKI_LOGITS_PROCESS_MAX_V 131072
int aki_logits_process(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out, const int64_t* tokens,
                       int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step, const uint8_t* done,
                       float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* eos_ids, int32_t n_eos,
                       const int64_t* suppress_ids, int32_t n_suppress, const int64_t* begin_suppress_ids, int32_t n_begin_suppress,
                       const int64_t* bad_ids, const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, void* stream);

/* aki_greedy_pick_processed - aki_greedy_pick_embed over the processed scores, in ONE launch: the row is processed as aki_logits_process
 * does (with n = cache_len[b] + advance - start_len[b], the index the pick writes, and eos_ids as the minimum length's eos ids) into the
 * f32 scratch scores [B, ld_scores] (16-byte aligned, ld_scores % 4 == 0), and the pick scans it.  embed_weight NULL: no embedding row
 * (as aki_greedy_pick; additional_weight and next_embeds NULL too).  A greedy token with processors stays chain + head + this launch. */
int aki_greedy_pick_processed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, void* stream);

/* aki_sample_pick - the `do_sample` step of HF `generate` with aki_greedy_pick_processed's bookkeeping, in ONE launch (one workgroup per
 * row): processors (neutral arguments: none) -> y = x / temperature (correctly rounded f32) -> top-k -> top-p -> softmax -> one draw.
 *   top_k        0 < top_k < V: keep y >= the top_k-th largest y, ties at the threshold all kept (TopKLogitsWarper); 0 or >= V: off
 *   top_p        < 1: among what top-k kept, keep token i iff the softmax mass of the tokens with strictly larger y is < top_p
 *                (TopPLogitsWarper's set; equal values stay together, the maximum is always kept); 1: off
 *   draw         w = exp(y - max) over the kept set, C = its inclusive cumulative sum in index order; the token is the smallest kept i
 *                with C_i > u * C_total (the last kept index if rounding leaves none), u = ((x0 >> 8) + 0.5) * 2^-24, x0 = the first word
 *                of Philox4x32-10 with key (seed lo, seed hi) and counter (n, b, offset lo, offset hi)
 *   n            = step + (cache_len ? cache_len[b] + advance - start_len[b] : 0): the generated-token index, which is also where the pick
 *                writes tokens[b, n] and what the processors take as the history length.  A replayed graph or a rewind redraws the same u.
 * Rows with done[b] take pad_token_id; a row whose maximum is NaN or +-inf, and every row when top_k == 1, takes aki_greedy_pick's id.
 * Both filters are exact threshold selections (radix select on order-preserving keys, 64-bit integer histograms): no sort, and the
 * same inputs give the same bits on every run.  scores: f32 scratch [B, ld_scores] as in aki_greedy_pick_processed, always needed (it
 * holds y).  probs_out (may be NULL): f32 [B, ld_probs], the normalised filtered distribution the draw was made from, 0 for removed
 * tokens; one-hot for the greedy rows, all 0 for finished rows.  embed_weight NULL: no embedding row.  V <= AKI_LOGITS_PROCESS_MAX_V. */
int aki_sample_pick(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                    uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                    int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                    int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                    int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                    const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                    int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                    uint64_t offset, float* probs_out, int64_t ld_probs, void* stream);

/* aki_sample_pick_rows - aki_sample_pick with the sampling parameters per ROW: the scalars temperature, top_k, top_p, seed and offset are
 * replaced by four device arrays of B entries (float, int32, float, uint64), read by the launch itself, so a captured graph serves rows
 * whose parameters are rewritten in place between replays.  Purely additive: AKI_ABI_VERSION was not bumped (it stays 17).
 * Row b runs exactly aki_sample_pick's step with temperature[b], top_k[b] and top_p[b], and draws with
 *   x0 = the first word of Philox4x32-10 with key seed[b] and counter (n, 0, 0, 0),
 * n as above: the draw row 0 of a B = 1 aki_sample_pick call with seed = seed[b] and offset = 0 makes.  The random stream belongs to the
 * row's seed, never to the row index, so a request keeps its stream whichever row serves it.  A row with top_k[b] == 1 takes
 * aki_greedy_pick's id (lowest index among equal maxima): a greedy row inside a sampled batch.
 * The entry point cannot read the arrays; the caller validates what it writes there.  Bad bits stay inside their row: a temperature that
 * is not > 0 (0, negative, NaN) takes the greedy id, top_k[b] <= 0 or >= V is no top-k filter, top_p[b] >= 1 no top-p filter.
 * Host checks as for aki_sample_pick (non-null pointers, B >= 1, V <= AKI_LOGITS_PROCESS_MAX_V, the scratch's alignment). */
int aki_sample_pick_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                         uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                         int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                         int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                         int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                         const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                         int32_t n_bad, int32_t n_bad_ids, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                         const uint64_t* seed, float* probs_out, int64_t ld_probs, void* stream);

/* ---- constrained decoding: a deterministic automaton over token ids, applied on the pick path.  Purely additive: AKI_ABI_VERSION was
 * not bumped (it stays 17).  The three entry points below are aki_logits_process, aki_greedy_pick_processed and aki_sample_pick with
 * five more arguments in front of `stream`; everything else is as documented there.
 *   table      int16 [n_states, table_ld] on the device, table_ld >= V: table[s, v] = the state behind token v in state s, negative = v is
 *              not allowed in s.  Rows are scanned with 16-byte loads when table is 16-byte aligned and table_ld % 8 == 0, else one
 *              entry at a time.  0 < n_states <= 32767.
 *   states     int32 [B, states_ld] on the device, states_ld >= 1: the state HISTORY of every row - states[b, n] is the state in which
 *              generated token n is picked; column 0 holds the row's start state (the caller fills it).
 * The mask is the last processor stage: with n the generated-token index of the entry point (before it is clamped to tokens_ld) and
 * s = states[b, n], every column v < V with table[s, v] < 0 becomes -inf; the other columns are left as the earlier stages made them.
 * Rows with done[b] != 0 are copied unprocessed; n outside [0, states_ld) or s outside [0, n_states) leaves the row unmasked.
 * The two picks also store states[b, n + 1] = done[b] ? s : table[s, next] (where n + 1 < states_ld), next to tokens[b, n]: the state is
 * addressed by the token index like the history, never carried in a counter, so a replayed graph, a rewind of cache_len and a repeated
 * step read and write the right column.  The caller makes sure that every state a row can reach allows at least one token. */
int aki_logits_process_constrained(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                   const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                                   const uint8_t* done, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length,
                                   const int64_t* eos_ids, int32_t n_eos, const int64_t* suppress_ids, int32_t n_suppress,
                                   const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                   const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, void* stream);

int aki_greedy_pick_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                                int32_t states_ld, void* stream);

int aki_sample_pick_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                uint64_t offset, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld, int32_t n_states,
                                int32_t* states, int32_t states_ld, void* stream);

/* ---- constrained decoding, one automaton per ROW (generate_many: a slot's request, and so its automaton, changes at admit under a
 * captured step).  Purely additive: AKI_ABI_VERSION was not bumped (it stays 17).  aki_greedy_pick_constrained_rows is
 * aki_greedy_pick_constrained, and aki_sample_pick_rows_constrained is aki_sample_pick_rows with the constraint's five arguments, each
 * with two more device arrays of B entries in front of `stream`, read by the launch itself (no host value is read: capturable):
 *   table      int16 [n_states, table_ld]: a POOL - several automata one behind the other, each with its own state numbers from 0
 *              (nothing is renumbered).  n_states is the pool's row count, any positive number: the 32767 limit holds per automaton.
 *   row_base   int32 [B]: the pool row at which row b's automaton begins.
 *   row_states int32 [B]: the number of states of row b's automaton.
 * With s = states[b, n], row b is masked by pool row row_base[b] + s when 0 <= s < row_states[b] and row_base[b] + s < n_states;
 * otherwise (s = -1: an unconstrained row; row_states[b] = 0; a slice that leaves the pool; a negative base) the row is left untouched
 * and its next state is -1.  The state the picks store in states[b, n + 1] is the table entry as it stands, a number LOCAL to the row's
 * automaton; a row with done[b] != 0 keeps its state.  The caller rewrites row_base[b], row_states[b] and states[b, :] in place when
 * the row changes hands; everything else is as documented for the entry points these extend. */
int aki_greedy_pick_constrained_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                     int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                     int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                     const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                     void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                     int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                     const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                     const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld,
                                     int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base,
                                     const int32_t* row_states, void* stream);

int aki_sample_pick_rows_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                     int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                     int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                     const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                     void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                     int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                     const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                     const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, int32_t step, const float* temperature,
                                     const int32_t* top_k, const float* top_p, const uint64_t* seed, float* probs_out, int64_t ld_probs,
                                     const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                                     const int32_t* row_base, const int32_t* row_states, void* stream);

/* ---- logits processors, one SET of settings per ROW (generate_many: a slot's request, and so its settings, changes at admit under a
 * captured step).  Purely additive: AKI_ABI_VERSION was not bumped (it stays 17).  aki_logits_process_rows is
 * aki_logits_process_constrained, aki_greedy_pick_rows is aki_greedy_pick_constrained_rows and aki_sample_pick_rows_processed is
 * aki_sample_pick_rows_constrained, each with the eleven scalar processor arguments (repetition_penalty ... n_bad_ids) replaced by a
 * pool of settings and one set index per row, all device arrays read by the launch itself (no host value is read: capturable):
 *   sets        int32 [n_sets, AKI_PROCESSOR_SET_WORDS], n_sets >= 1: one record per distinct setting -
 *               word 0 the repetition penalty (the bits of a float), 1 no_repeat_ngram_size, 2 min_length,
 *               3, 4 the suppress ids set_ids[w3, w4), 5, 6 the begin-suppress ids set_ids[w5, w6), 7, 8 the bad words [w7, w8).
 *   row_set     int32 [B]: row b is processed with record row_set[b].
 *   set_ids     int64 [n_set_ids]: every record's suppress, begin-suppress and bad-word ids, one list behind the other.
 *   bad_offsets int32 [n_words + 1], ascending: bad word w is set_ids[bad_offsets[w], bad_offsets[w + 1]).
 * The stages, their order and their arithmetic are those of aki_logits_process; the minimum length bans the call's eos_ids.  Nothing
 * validates the arrays on the device, and bad bits stay inside their row: a set index outside [0, n_sets) processes the row with the
 * neutral set (the plain f32 copy), every range is cut at its pool's end (an empty or reversed one holds nothing), a penalty that is
 * not a finite positive float is read as 1, a negative n-gram size as 0, ids outside [0, V) are skipped.  The caller rewrites
 * row_set[b] in place when the row changes hands.
 * The token constraint is the per-row form of aki_greedy_pick_constrained_rows and stays the last stage; table == NULL means no
 * constraint, and the six arguments behind it are then ignored.  aki_logits_process_rows takes row_base / row_states too (its
 * constrained sibling has no per-row form) and AKI_DT_BF16 or AKI_DT_F32 logits; the two picks take bf16 logits.  In
 * aki_sample_pick_rows_processed every row runs through the processors (a neutral row is the plain copy), so rows with top_k[b] == 1
 * take aki_greedy_pick_rows' token.  Everything else is as documented for the entry points these extend. */
#define AKI_PROCESSOR_SET_WORDS 9

int aki_logits_process_rows(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                            const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                            const uint8_t* done, const int64_t* eos_ids, int32_t n_eos, const int32_t* sets, int32_t n_sets,
                            const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets, int32_t n_words,
                            const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                            const int32_t* row_base, const int32_t* row_states, void* stream);

int aki_greedy_pick_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                         uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                         int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                         int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets,
                         int32_t n_sets, const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                         int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                         const int32_t* row_base, const int32_t* row_states, void* stream);

int aki_sample_pick_rows_processed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                                   const uint64_t* seed, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                   void* stream);

/* ---- min_p and the frequency / presence penalties (HF MinPLogitsWarper; the OpenAI penalties in vLLM's order).  Purely additive:
 * AKI_ABI_VERSION was not bumped (it stays 17).  Six entry points: aki_logits_process_penalized, aki_greedy_pick_penalized and
 * aki_sample_pick_penalized are aki_logits_process_constrained, aki_greedy_pick_constrained and aki_sample_pick_constrained, and the
 * three *_rows_penalized are aki_logits_process_rows, aki_greedy_pick_rows and aki_sample_pick_rows_processed, each with two or three
 * more arguments in front of the stream - device arrays of B floats, read by the launch itself (capturable), each of which may be NULL:
 *   frequency_penalty, presence_penalty   stage 1b of the processors, directly behind the repetition penalty and before every ban: for
 *               every distinct token g of the row's generated history h[0, n) with 0 <= g < V and c occurrences,
 *               x = x - fl(frequency_penalty[b] * (float)c) when frequency_penalty[b] != 0, then x = x - presence_penalty[b] when
 *               presence_penalty[b] != 0; each ONE correctly rounded f32 operation (no FMA).  The counts are recomputed from the
 *               history in every launch: nothing is carried between steps, no float atomics, the same bits on every run.  Rows with
 *               done[b] keep the plain copy; -inf stays -inf.  A value that is not finite reads as 0; NULL is 0 for every row.
 *   min_p       (the two sample forms) behind temperature, top-k and top-p: a token those kept stays iff
 *               expf(y - ymax) >= min_p[b], y = x / T.  The maximum always stays (and its ties at min_p = 1); top-p's mass is decided
 *               before it; the draw and probs_out are made over what remains.  A value outside (0, 1] is no filter; NULL is none for
 *               every row.  Rows that take the greedy branch take it as before.
 * In the three call-wide forms table == NULL means no constraint (the four arguments behind it are then ignored), as in the per-row
 * forms.  The hosts' checks are those of the entry points these extend; the arrays' values are the caller's to validate. */
int aki_logits_process_penalized(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                 const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                                 const uint8_t* done, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length,
                                 const int64_t* eos_ids, int32_t n_eos, const int64_t* suppress_ids, int32_t n_suppress,
                                 const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                 const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld,
                                 int32_t n_states, int32_t* states, int32_t states_ld, const float* frequency_penalty,
                                 const float* presence_penalty, void* stream);

int aki_greedy_pick_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                              int32_t states_ld, const float* frequency_penalty, const float* presence_penalty, void* stream);

int aki_sample_pick_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                              uint64_t offset, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld, int32_t n_states,
                              int32_t* states, int32_t states_ld, const float* frequency_penalty, const float* presence_penalty,
                              const float* min_p, void* stream);

int aki_logits_process_rows_penalized(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                      const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len,
                                      int32_t step, const uint8_t* done, const int64_t* eos_ids, int32_t n_eos, const int32_t* sets,
                                      int32_t n_sets, const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids,
                                      const int32_t* bad_offsets, int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states,
                                      int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                      const float* frequency_penalty, const float* presence_penalty, void* stream);

int aki_greedy_pick_rows_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                                   int32_t states_ld, const int32_t* row_base, const int32_t* row_states, const float* frequency_penalty,
                                   const float* presence_penalty, void* stream);

int aki_sample_pick_rows_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                                   const uint64_t* seed, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                   const float* frequency_penalty, const float* presence_penalty, const float* min_p, void* stream);

/* ---- beam search on the device (beam.hip).  HF `GenerationMixin` beam search with a `BeamSearchScorer`, the algorithm AKI._beam_search
 * runs on the host: 2K candidates per step, hypotheses normalised by generated_length ** length_penalty, at most K per sample.
 * Purely additive: AKI_ABI_VERSION was not bumped (it stays 17). */
#define AKI_BEAM_MAX_K 16
#define AKI_BEAM_MAX_EOS 8
#define AKI_KV_BEAM_REORDER_CHUNK 16   /* cache positions one workgroup of aki_kv_beam_reorder owns */

/* aki_beam_logprob - out[r, v] = x - (m + log(sum_v exp(x - m))), m = max_v x, for rows r < rows of logits [rows, ld] (AKI_DT_BF16 or
 * AKI_DT_F32, V columns used) -> out f32 [rows, ld_out].  f32 arithmetic, one workgroup per row, a fixed reduction order (no atomics):
 * the same inputs give the same bits on every run.  out == logits is allowed for f32. */
int aki_beam_logprob(const void* logits, int32_t dtype, int32_t rows, int32_t V, int64_t ld, float* out, int64_t ld_out, void* stream);

/* aki_beam_step - one step of the search for every sample, one launch, no host value read.  logp f32 [B*K, ld] holds the (processed)
 * log-probabilities of the beams' next token, beam_scores f32 [B, K] the running sums (in / out), t the number of tokens generated so
 * far (the step writes token t), 1 <= K <= AKI_BEAM_MAX_K, 2 <= V, K * V < 2^31, 0 <= t < max_new, n_eos <= AKI_BEAM_MAX_EOS.
 *   candidates   the 2K best of logp[b*K + k, v] + beam_scores[b, k] (one f32 addition), ranked by score, descending; among exactly equal
 *                scores the lower flat index k * V + v comes first.  The ranking does not depend on how the work is laid out.
 *   walk         in rank order: an eos candidate of rank < K becomes a hypothesis with score sum / (t + 1) ** length_penalty (f32), one of
 *                rank >= K is dropped; the first K others become the running beams: beam_scores[b, n], next_ids[b*K + n],
 *                parent[b*K + n] = the GLOBAL row b*K + beam, seqs_out[b*K + n] = seqs_in[parent] + [token].  Unfilled slots: -1e9,
 *                pad_token_id, parent b*K.
 *   hypotheses   at most K per sample in hyp_score f32 [B, K], hyp_len int32 [B, K], hyp_tokens int64 [B, K, max_new], hyp_count int32 [B]
 *                (all zero before step 0): a new one takes a free slot, or - when its score is strictly better than the worst held -
 *                the worst one's slot (among equal worst scores the lowest slot).
 *   done         when K hypotheses are held: early_stopping 1 -> done; 0 -> done when the worst held score >= the best running score /
 *                (t + 1) ** length_penalty; any other value -> never.  A sample with done[b] != 0 at entry is frozen: nothing of its state
 *                is touched, next_ids = pad_token_id, parent = the identity, seqs_out = seqs_in + [pad_token_id].
 *   last != 0    the closing step: the running beams of a sample not done, with score > -1e8, become hypotheses with this step's token.
 * seqs_in / seqs_out: int64 [B*K, max_new], two different buffers (the caller swaps them every step; seqs_in may be NULL at t == 0). */
int aki_beam_step(const float* logp, int64_t ld, int32_t B, int32_t K, int32_t V, int32_t t, int32_t max_new, float* beam_scores,
                  const int64_t* seqs_in, int64_t* seqs_out, float* hyp_score, int32_t* hyp_len, int64_t* hyp_tokens, int32_t* hyp_count,
                  uint8_t* done, int64_t* next_ids, int32_t* parent, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                  float length_penalty, int32_t early_stopping, int32_t last, void* stream);

/* aki_kv_beam_reorder - beam search's cache re-ordering (HF `_reorder_cache`) in place, for the rows written since the prefill only:
 * for each of the n_tensors tensors [B*K, H, capacity, row_bytes] whose base addresses `table` holds (DEVICE memory: the K and V
 * tensors of every layer), dst[b*K + n, h, pos, :] = src[parent[b*K + n], h, pos, :] for start_len[row] <= pos < cache_len[row] (row: both the
 * destination's and the source's).  Rows move as bytes: 16-byte vectors when row_bytes % 16 == 0 (bases 16-byte aligned), 4-byte words when
 * row_bytes % 4 == 0.  [pos_lo, pos_hi): host bounds of the positions any row may move (the grid's extent; the device lengths decide).
 * A sample whose parents are the identity is skipped; a parent outside [b*K, b*K + K) is read as the identity.  Positions outside
 * [start_len, cache_len) are neither read nor written.  One launch; n_tensors * B <= 65535, H <= 65535, K <= AKI_BEAM_MAX_K. */
int aki_kv_beam_reorder(void* const* table, int32_t n_tensors, const int32_t* parent, const int32_t* start_len, const int32_t* cache_len,
                        int32_t B, int32_t K, int32_t H, int32_t capacity, int32_t row_bytes, int32_t pos_lo, int32_t pos_hi, void* stream);

/* ---- per-token log-probabilities (logprob.hip): what `generate(output_logprobs=True)` and `score` launch behind every pick.
 * Purely additive: AKI_ABI_VERSION was not bumped (it stays 17). */
#define AKI_LOGPROB_MAX_TOP 8        /* alternatives per position */
#define AKI_LOGPROB_MAX_V 262144     /* columns per row */

/* aki_token_logprob - for each row r < rows of logits [rows, ld] (AKI_DT_BF16 or AKI_DT_F32, V <= AKI_LOGPROB_MAX_V columns used), one
 * workgroup, one launch, no host value read, no workspace:
 *   lse       m + log(sum_v exp(x_v - m)), m = max_v x_v: f32, a fixed reduction order, no float atomics - the same inputs give the same
 *             bits on every run.  Columns may hold -inf, never a whole row; NaN inputs are unspecified (nothing is written out of bounds).
 *             The raw model distribution: HF's compute_transition_scores(sequences, logits, normalize_logits=True).
 *   position  t = step + (cache_len ? cache_len[r] - start_len[r] : 0) (cache_len and start_len: both or neither), evaluated on the
 *             device: behind aki_greedy_pick / aki_sample_pick that is the index the pick just wrote, so one captured graph serves every
 *             replay.  t outside [0, out_cols): the row writes nothing.
 *   token     ids[r] when ids is given, else tokens[r * tokens_ld + t] (int64).  out_logprob[r * out_ld + t] = x_id - lse; an id outside
 *             [0, V) (or t >= tokens_ld) writes NaN and reads nothing outside the row.
 *   top_k     0 .. AKI_LOGPROB_MAX_TOP alternatives: the top_k columns with the largest input values (ranked on the inputs, which are exact;
 *             equal values: the lower column first) go to out_top_ids[(r * out_ld + t) * top_k + j] (int64) with x - lse in
 *             out_top_logprobs[...]; -inf columns come last with logprob -inf; a row with fewer than top_k columns ends with id -1, -inf.
 *   skipped   a row with skip[r] != 0, or with done_at[r] >= 0 && done_at[r] < t (it finished at an earlier step and carries pad tokens;
 *             the step that picked its EOS, done_at[r] == t, is scored): logprob 0.0, top ids -1, top logprobs 0.0.
 * Rows are read with 16-byte vectors when logits and ld * element size are 16-byte aligned, column by column otherwise.
 * AKI_ERR_INVALID_ARG: null logits / out_logprob, neither ids nor tokens, one of cache_len / start_len alone, top_k > 0 without both top
 * outputs, rows / V < 1, ld < V, step < 0, out_cols < 1, out_ld < out_cols, tokens_ld < 1 with tokens.  AKI_ERR_UNSUPPORTED: dtype, top_k
 * outside 0 .. AKI_LOGPROB_MAX_TOP, V > AKI_LOGPROB_MAX_V. */
int aki_token_logprob(const void* logits, int32_t dtype, int32_t rows, int32_t V, int64_t ld, const int64_t* ids, const int64_t* tokens,
                      int64_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step, const uint8_t* skip,
                      const int32_t* done_at, int32_t top_k, float* out_logprob, int64_t* out_top_ids, float* out_top_logprobs,
                      int64_t out_ld, int32_t out_cols, void* stream);

/* ---- in-flight batching (slots.hip): what `generate_many` launches to refill a finished row of a batch from a queue of requests.
 * Purely additive: AKI_ABI_VERSION was not bumped (it stays 17). */
#define AKI_SLOT_MAX_ROWS 16         /* rows of one aki_slot_tick: the decode batch the skinny decode GEMMs take */

/* aki_kv_slot_admit - one prefilled sequence copied into row `slot` of a larger cache, every tensor in one launch.  `table` (DEVICE memory)
 * holds 2 * n_tensors base addresses: first the sources [1, H, cap_src, row_bytes], then the destinations [B, H, cap_dst, row_bytes], pairwise
 * (the K and V tensors of every layer; for an fp8_e4m3 cache the f32 scales are tensors with row_bytes 4, a launch of their own).
 *   dst[slot, h, pos, :] = src[0, h, pos, :] for 0 <= pos < len, len = min(src_len[0], cap_src, cap_dst) read on the device (the source's
 * cache_len); every other byte of a destination stays as it was.  Bytes only, nothing is converted.  vec_bytes is the unit the rows move in:
 * 16 (row_bytes % 16 == 0 and every address in the table 16-byte aligned) or 4 (row_bytes % 4 == 0, addresses 4-byte aligned) - the caller,
 * who wrote the table, states which.  host_len: a host bound of len (it sizes the grid only), 0 <= host_len <= min(cap_src, cap_dst); 0
 * launches nothing.  AKI_ERR_INVALID_ARG: a null pointer, a count below 1, slot outside [0, B), host_len out of range.
 * AKI_ERR_UNSUPPORTED: vec_bytes other than 4 / 16, row_bytes no multiple of it, H or n_tensors above 65535. */
int aki_kv_slot_admit(void* const* table, int32_t n_tensors, const int32_t* src_len, int32_t H, int32_t cap_src, int32_t cap_dst, int32_t B,
                      int32_t slot, int32_t row_bytes, int32_t vec_bytes, int32_t host_len, void* stream);

/* aki_slot_tick - the per-row token budget of B <= AKI_SLOT_MAX_ROWS rows, one thread per row, launched right behind aki_greedy_pick (inside
 * the captured step).  generated = cache_len[b] - start_len[b] + 1 is the number of tokens row b has picked (token 0 is picked from the
 * prefill's logits with advance = 0).  A live row (done[b] == 0) with generated >= limit[b] gets done[b] = 1, done_at[b] = generated - 1.
 * A done row with done_at[b] >= 0 - marked here or by the pick's eos check - is parked: cache_len[b] = start_len[b] + done_at[b], the cache
 * row of the token it never feeds, so the pad-token steps a loop still gives it overwrite one dead row and never walk past its slab.  A live
 * row under its budget is not touched.  done uint8, the others int32, all [B]. */
int aki_slot_tick(uint8_t* done, int32_t* done_at, int32_t* cache_len, const int32_t* start_len, const int32_t* limit, int32_t B, void* stream);

/* ---- stop sequences (slots.hip): a row ends when its generated tokens end with one of the token-id sequences of its stop set.
 * Purely additive: AKI_ABI_VERSION was not bumped (it stays 17). */
#define AKI_STOP_MAX_SEQS 64         /* sequences of one stop set: one lane of a wave each */
#define AKI_STOP_MAX_LEN 32          /* ids of one stop sequence */

/* The pool (DEVICE memory, all int32): ids[n_ids] holds every sequence one behind the other; sequence s is ids[seq_off[s] .. seq_off[s + 1]),
 * seq_off[n_seqs + 1]; set k is the sequences set_first[k] .. set_first[k + 1], set_first[n_sets + 1], at most AKI_STOP_MAX_SEQS of 1 to
 * AKI_STOP_MAX_LEN ids each, order significant; row b is checked against set row_set[b].  The device range-checks every index it reads
 * against the counts: a row_set outside [0, n_sets) and a set or sequence whose offsets leave the pool are an empty set, never a read
 * outside the arrays.
 *
 * aki_stop_check - launched right behind aki_greedy_pick / the sampling picks (and behind aki_token_logprob where there is one), inside the
 * captured step.  One wave per row.  t = cache_len[b] - start_len[b] is the index the pick just wrote (with advance 0 or 1).  A done row
 * and a row with t outside [0, tokens_ld) are skipped.  A live row whose tokens[b, t - n + 1 .. t] equal a sequence of n <= t + 1 ids of
 * its set gets done[b] = 1, done_at[b] = t and stop_hit[b] = the index within the set of the LOWEST-numbered sequence that matches at t;
 * nothing else is written (stop_hit of a row that does not match keeps its value: the caller presets -1).  Only the t + 1 generated
 * tokens of the row are read.  tokens int64 [B, tokens_ld], done uint8 [B], the others int32 [B].  No host value is read.
 * AKI_ERR_INVALID_ARG: a null pointer (ids may be null when n_ids == 0), B < 1, tokens_ld outside [1, 2^31), a count below zero. */
int aki_stop_check(const int64_t* tokens, int64_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, uint8_t* done,
                   int32_t* done_at, int32_t* stop_hit, const int32_t* ids, int32_t n_ids, const int32_t* seq_off, int32_t n_seqs,
                   const int32_t* set_first, int32_t n_sets, const int32_t* row_set, int32_t B, void* stream);

/* aki_slot_tick_stops - aki_stop_check followed by aki_slot_tick in ONE launch, for B <= AKI_SLOT_MAX_ROWS rows: on every input its effect on
 * done, done_at, cache_len and stop_hit is that of the two calls one behind the other (a stop and the budget at one token is a stop).
 * AKI_ERR_INVALID_ARG as for both; AKI_ERR_UNSUPPORTED: B above AKI_SLOT_MAX_ROWS. */
int aki_slot_tick_stops(uint8_t* done, int32_t* done_at, int32_t* cache_len, const int32_t* start_len, const int32_t* limit,
                        const int64_t* tokens, int64_t tokens_ld, int32_t* stop_hit, const int32_t* ids, int32_t n_ids,
                        const int32_t* seq_off, int32_t n_seqs, const int32_t* set_first, int32_t n_sets, const int32_t* row_set, int32_t B,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AKI_MI355X_H */

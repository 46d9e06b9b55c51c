// api.hip - extern "C" entry points of libaki_mi355x.so (include/aki_mi355x.h).
// Host-side validation only; every launch goes to the stream the caller passes.
#include "aki_device.h"
#include "pick_params.h"

namespace aki {
int linear_bf16(const aki_linear_args* a, hipStream_t stream);
size_t linear_stats_ws_bytes(int M, int n_out);
size_t linear_stats_cnt_bytes(int M);
int row_stats_launch(const void* x, int rows, int cols, int ldx, float eps, float* rstd, float* mean, hipStream_t s);
int linear_f32(const aki_linear_args* a, hipStream_t stream);
int qkv_rope_bf16(const aki_mma_attn_args* a, void* q, void* k, void* v, hipStream_t stream);
int qkv_rope_fp8(const aki_mma_attn_args* a, void* q, void* k, void* v, hipStream_t stream);
int linear_fp8(const aki_linear_args* a, hipStream_t stream);
int quant_rows_fp8_launch(const void* x, const void* rms_w, float eps, void* q, float* scale, int rows, int cols, int ldx, int ldq,
                          hipStream_t s);
int qkv_rope_f32(const aki_mma_attn_args* a, void* q, void* k, void* v, float* tmp, hipStream_t stream);
int attn_core_bf16(const aki_mma_attn_core_args* a, void* ws, size_t ws_bytes, hipStream_t stream);
int attn_core_f32(const aki_mma_attn_core_args* a, void* ws, size_t ws_bytes, hipStream_t stream, int causal);
int attn_nc_bf16(const aki_attn_args* a, hipStream_t stream);
int gemv_bf16(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream);
int skinny_gemm_bf16(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream);
int skinny_gemm_w8(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream);
int quant_mxfp4_launch(const void* w, int N, int K, int ldw, uint8_t* wq, uint8_t* ws, hipStream_t s);
int gemv_w4(const aki_linear_args* a, const uint8_t* ws, const void* rms_w, float eps, hipStream_t stream);
int skinny_gemm_w4(const aki_linear_args* a, const uint8_t* ws, const void* rms_w, float eps, hipStream_t stream);
size_t decode_attn_ws_bytes(int B, int H, int Dh, int cap);
int decode_attn_split_launch(const void* q_or_qkv, const float* cos, const float* sin, const int* len, void* kc, void* vc, void* o,
                             const uint64_t* vbits, int nwords, int B, int H, int cap, int max_keys, float scale, bool fused,
                             void* ws, size_t ws_bytes, hipStream_t s);
int rope_append_launch(const void* qkv, const float* cos, const float* sin, const int* pos, const int* cache_len, void* q_out,
                       void* k_cache, void* v_cache, int B, int H, int Dh, int cap, int dtype, hipStream_t s);
int kv_cache_quant_fp8_launch(const void* src, int src_cap, void* dst, float* scale, int dst_cap, int slabs, int rows, hipStream_t s);
int decode_attn_split_fp8kv_launch(const void* qkv, const float* cos, const float* sin, const int* len, void* kc, void* vc, float* ks, float* vs,
                                   void* o, const uint64_t* vbits, int nwords, int B, int H, int cap, int max_keys, float scale, void* ws,
                                   size_t ws_bytes, hipStream_t s);
size_t decode_attn_group_ws_bytes(int B0, int N, int H, int pcap, int scap);
int decode_attn_group_launch(const void* qkv, const float* cos, const float* sin, const int* len, const int* plen, const void* kp,
                             const void* vp, void* ks, void* vs, void* o, const uint64_t* vbits, int nwords, int B0, int N, int H, int pcap,
                             int scap, int max_pkeys, int max_skeys, float scale, void* ws, size_t ws_bytes, hipStream_t s);
size_t chunk_attn_ws_bytes(int B, int H, int T);
int chunk_attn_launch(const void* qkv, const float* cos, const float* sin, const int* cache_len, const int* n_new, void* k_cache, void* v_cache,
                      void* o, const uint64_t* vbits, int nwords, int B, int H, int T, int max_new, int cap, float scale, void* ws,
                      size_t ws_bytes, hipStream_t s);
size_t decode_chain_ws_bytes(int n_layers, int d, int H, int F, int cap);
size_t decode_chain_err_offset(int n_layers, int H);
size_t decode_chain_b_ws_bytes(int n_layers, int d, int H, int F, int cap, int B);
size_t decode_chain_b_err_offset(int n_layers, int H, int B);
int decode_chain_launch(const aki_decode_chain_args* a, hipStream_t stream);
int decode_attn_launch(const void* q, const void* kc, const void* vc, void* o, const int* n_keys, const uint64_t* vbits, int nwords,
                       int B, int H, int Dh, int cap, float scale, int dtype, hipStream_t s);
int norm_launch(bool rms, const void* x, const void* w, const void* b, void* y, int rows, int cols, int ldx, int ldy,
                float eps, int dtype, hipStream_t stream);
int splice_plan_launch(const int64_t* lang_x, int B, int T, int64_t media, int64_t assistant, int Nv, int* plan, hipStream_t s);
int splice_launch(const aki_splice_args* a, hipStream_t s);
int mask_dense_launch(const aki_mma_rect* rects, int max_rects, const uint64_t* vbits, const int* seq_lens, int B, int L,
                      int64_t* out, hipStream_t s);
int im2col_launch(const void* pix, void* out, int N, int S, int P, int Kp, int dtype, hipStream_t s);
int pick_call_launch(const PickCall& c, hipStream_t s);
int logits_process_call_launch(const ProcParams& q, const ProcSetParams* ps, int B, hipStream_t s);
int beam_logprob_launch(const void* logits, int in_f32, int rows, int V, int ld, float* out, int ld_out, hipStream_t s);
int beam_step_launch(const float* logp, int ld, int B, int K, int V, int t, int max_new, float* beam_scores, const int64_t* seqs_in,
                     int64_t* seqs_out, float* hyp_score, int* hyp_len, int64_t* hyp_tokens, int* hyp_count, unsigned char* done,
                     int64_t* next_ids, int* parent, const int64_t* eos, int n_eos, int64_t pad, float length_penalty, int early, int last,
                     hipStream_t s);
int kv_beam_reorder_launch(void* const* table, int n_tensors, const int* parent, const int* start_len, const int* cache_len, int B, int K,
                           int H, int cap, int row_bytes, int pos_lo, int pos_hi, hipStream_t s);
int token_logprob_launch(const void* logits, int in_f32, int rows, int V, int ld, const int64_t* ids, const int64_t* tokens, int tokens_ld,
                         const int* cache_len, const int* start_len, int step, const unsigned char* skip, const int* done_at, int top_k,
                         float* out_logprob, int64_t* out_top_ids, float* out_top_logprobs, int out_ld, int out_cols, hipStream_t s);
int kv_slot_admit_launch(void* const* table, int n_tensors, const int* src_len, int H, int cap_src, int cap_dst, int slot, int row_bytes,
                         int vec_bytes, int host_len, hipStream_t s);
int slot_tick_launch(unsigned char* done, int* done_at, int* cache_len, const int* start_len, const int* limit, int B, hipStream_t s);
int stop_check_launch(const int64_t* tokens, int tokens_ld, const int* cache_len, const int* start_len, unsigned char* done, int* done_at,
                      int* stop_hit, const int* ids, int n_ids, const int* seq_off, int n_seqs, const int* set_first, int n_sets,
                      const int* row_set, int B, hipStream_t s);
int slot_tick_stops_launch(unsigned char* done, int* done_at, int* cache_len, const int* start_len, const int* limit, const int64_t* tokens,
                           int tokens_ld, int* stop_hit, const int* ids, int n_ids, const int* seq_off, int n_seqs, const int* set_first,
                           int n_sets, const int* row_set, int B, hipStream_t s);
int sft_collate_launch(const int64_t* ids, const int64_t* labels, const int64_t* mask, const int* offsets, int B, int T_out,
                       int64_t pad_id, int64_t ignore_index, int left, int64_t* out_ids, int64_t* out_labels, int64_t* out_mask,
                       hipStream_t s);
size_t mask_to_table_ws_bytes(int B, int L);
int mask_to_table_launch(const int64_t* mask, int B, int L, int max_rects, aki_mma_rect* rects, uint64_t* vbits, int* seq_lens,
                         int* status, void* ws, hipStream_t s);
size_t linear_splitk_plan_ws_bytes(int M, int N, int K);
#ifdef AKI_LAB_HOOKS
extern int g_sk_slice_major;
extern int g_force_tile;
extern int g_deep_ring;
extern int g_res_prefetch;
extern int g_deepx;
extern int g_attn_variant;
extern long long* g_clock_probe;
extern int g_probe_block;
extern int g_gemm_dry_run;
void gemm_log_reset();
int gemm_log_copy(int* out, int cap);
extern int g_decode_dry_run;
void decode_log_reset();
int decode_log_copy(int* out, int cap);
#endif
size_t attn_bwd_ws_bytes(int B, int H, int Lq);
int attn_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, void* dq, void* dk,
                  void* dv, const aki_mma_rect* rects, int max_rects, const uint64_t* vbits, const int* seq_lens, int masked, int B,
                  int H, int Lq, int Lk, int Dh, float scale, void* ws, size_t ws_bytes, hipStream_t s);
int transpose_bf16_launch(const void* x, void* y, int R, int C, int ldx, int ldy, int Rpad, hipStream_t s);
int gemm_tn_launch(const void* a, const void* b, void* c, int Kc, int I, int J, long lda, long ldb, long ldc, hipStream_t stream);
size_t norm_bwd_ws_bytes(int cols);
int norm_bwd_launch(bool rms, const void* x, const void* w, const void* dy, const void* dres, void* dx, void* dw, void* db, int rows,
                    int cols, int ldx, int lddy, int lddx, int lddr, float eps, int accumulate, void* ws, size_t ws_bytes, hipStream_t s);
size_t colsum_ws_bytes(int cols);
int colsum_launch(const void* x, void* out, int rows, int cols, int ldx, int accumulate, void* ws, size_t ws_bytes, hipStream_t s);
int swiglu_launch(int bwd, const void* gu, const void* da, void* out, int rows, int F, int ldg, int ldda, int ldo, hipStream_t s);
int gelu_launch(int bwd, const void* x, const void* dy, void* out, size_t n, hipStream_t s);
int rope_bwd_merge_launch(const void* dq, const void* dk, const void* dv, const float* cos, const float* sin, const int* pos, void* dqkv,
                          int B, int H, int L, int Dh, hipStream_t s);
int ce_launch(const void* logits, const int64_t* labels, int* n_valid, float* loss_rows, void* dlogits, int B, int L, int V, int ldl,
              int lddl, float gscale, hipStream_t s);
int ce_rows_launch(const void* logits, const int64_t* targets, const int* n_valid, float* loss_rows, void* dlogits, int rows, int V,
                   int ldl, int lddl, float gscale, hipStream_t s);
size_t grad_sqnorm_ws_bytes();
int grad_sqnorm_launch(const void* g, size_t n, float* out, int accumulate, void* ws, size_t ws_bytes, bool g32, hipStream_t s);
int adamw_t_launch(float* p, float* m, float* v, const void* g, void* w16, void* wT, int N, int K, int ldT, const float* sqnorm, float max_norm,
                   float gscale, float lr, float beta1, float beta2, float eps, float wd, int step, bool g32, hipStream_t s);
int adamw_launch(float* p, float* m, float* v, const void* g, void* w16, size_t n, const float* sqnorm, float max_norm, float gscale,
                 float lr, float beta1, float beta2, float eps, float wd, int step, bool g32, hipStream_t s);
}  // namespace aki

using namespace aki;

static inline bool dtype_ok(int dt) { return dt == AKI_DT_BF16 || dt == AKI_DT_F32; }

extern "C" {

const char* aki_strerror(int status) {
  switch (status) {
    case AKI_OK: return "ok";
    case AKI_ERR_INVALID_ARG: return "invalid argument (null pointer, non-positive size or inconsistent shapes)";
    case AKI_ERR_UNSUPPORTED: return "unsupported dtype / head_dim / size for the gfx950 kernels";
    case AKI_ERR_ALIGNMENT: return "pointer or leading dimension is not 16-byte aligned";
    case AKI_ERR_WORKSPACE: return "workspace missing or too small";
    case AKI_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown aki status";
  }
}

int aki_abi_version(void) { return AKI_ABI_VERSION; }

#ifdef AKI_LAB_HOOKS
// Lab build only (libaki_mi355x_lab.so, `python -m aki_amd.build --lab`): force the bf16 GEMM tile configuration
// (0 = heuristic, 1 = 256x256, 2 = 128x128, 3 = 128 features x 96 tokens where that tile exists, else 128x128, 5 = 64x64 on a
// four-stage ring where that tile exists, else 128x128); +256 switches off the 4-stage / 64-feature variant of single-row launches,
// +1024 the residual prefetch of the 256x256 tile, +4096 / +8192 force / forbid the three-deep ring on the tokens of residual GEMMs.
// Process-global, not thread safe - which is why the product library does not carry it.
void aki_lab_set_gemm_tile(int mode) {
  aki::g_deep_ring = (mode & 256) ? 0 : 1;
  aki::g_deepx = (mode & 4096) ? 1 : ((mode & 8192) ? 2 : 0);
  aki::g_res_prefetch = (mode & 1024) ? 0 : 1;
  mode &= 255;
  aki::g_force_tile = (mode >= 1 && mode <= 5 && mode != 4) ? mode : 0;
}
// split-K workgroup order: 0 = tile-major (product), 1 = slice-major
void aki_lab_set_slice_major(int on) { aki::g_sk_slice_major = on ? 1 : 0; }
// attention core (mma_attn_bf16.hip, g_attn_variant): 0 = product choice, 1 / 2 = the 32-row core at every length, 9 / 10 = the 64-row core
void aki_lab_set_attn_variant(int v) { aki::g_attn_variant = v; }
// device pointer to two int64: every bf16 GEMM launch then leaves {shader cycles, 100 MHz wall ticks} of its workgroup 0 there
void aki_lab_set_probe_block(int b) { aki::g_probe_block = b; }   // which workgroup of a GEMM launch stamps
void aki_lab_set_clock_probe(void* int64x32) { aki::g_clock_probe = (long long*)int64x32; }   // 32 int64 (layout: GemmParams::clock_probe)
// route log of the bf16 / fp8 GEMM (gemm_bf16.hip, launch_gemm): 14 int32 per launch {NF, NT, WN, WM, EPI, ACT, FP8, NST, PIPE, SK, ksplit,
// M, m_offset, grid}; aki_lab_gemm_log copies up to `cap` records and returns the number of launches since the last reset
void aki_lab_gemm_log_reset(void) { aki::gemm_log_reset(); }
int aki_lab_gemm_log(int32_t* out, int cap) { return aki::gemm_log_copy(out, cap); }
// 1: every GEMM launch is recorded and returns AKI_OK before any HIP call (the planner without a GPU)
void aki_lab_set_gemm_dry_run(int on) { aki::g_gemm_dry_run = on ? 1 : 0; }
// route log of the decode linears (decode.hip, launch_gemv_cfg / launch_skinny / launch_skinny_w8): 9 int32 per launch {family, M or KS, SWIGLU,
// FPW or FT, W8 or NORM, norm, grid, feature groups per workgroup, dynamic LDS bytes}; family 0 = gemv_bf16_kernel, 1 = skinny_gemm_bf16_kernel,
// 2 = skinny_gemm_w8_kernel.  aki_lab_decode_log copies up to `cap` records and returns the number of launches since the last reset
void aki_lab_decode_log_reset(void) { aki::decode_log_reset(); }
int aki_lab_decode_log(int32_t* out, int cap) { return aki::decode_log_copy(out, cap); }
// 1: every decode-linear launch is recorded and returns AKI_OK before any HIP call
void aki_lab_set_decode_dry_run(int on) { aki::g_decode_dry_run = on ? 1 : 0; }
#endif

// ---- attention core --------------------------------------------------------------------------------
size_t aki_mma_attn_core_workspace_bytes(int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype) {
  AKI_CLEAR_ERR();
  (void)L; (void)dtype;
  return aki_align_up((size_t)B * H * Dh * sizeof(float), 256);
}

int aki_mma_attn_core_fwd(const aki_mma_attn_core_args* a, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->q && a->k && a->v && a->o);
  AKI_CHECK_ARG(a->B > 0 && a->H > 0 && a->L > 0 && a->Dh > 0 && a->scale > 0.f);
  AKI_CHECK_ARG(dtype_ok(a->dtype));
  AKI_CHECK_ARG(a->max_rects >= 0 && (a->max_rects == 0 || a->rects));
  if (a->dtype == AKI_DT_BF16) return attn_core_bf16(a, ws, ws_bytes, (hipStream_t)stream);
  return attn_core_f32(a, ws, ws_bytes, (hipStream_t)stream, 1);
}

// ---- plain attention (vision side) ---------------------------------------------------------------------
int aki_attn_fwd(const aki_attn_args* a, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->q && a->k && a->v && a->o);
  AKI_CHECK_ARG(a->B > 0 && a->H > 0 && a->Lq > 0 && a->Lk > 0 && a->Dh > 0 && a->scale > 0.f && dtype_ok(a->dtype));
  if (a->dtype == AKI_DT_BF16) return attn_nc_bf16(a, (hipStream_t)stream);
  // f32 parity path: the simple kernel wants contiguous head-major tensors and Lq == Lk (ops.attention pads shorter queries to Lk rows and
  // refuses longer ones); anything else is UNSUPPORTED
  const int64_t Dh = a->Dh;
  if (a->q_stride_t != Dh || a->k_stride_t != Dh || a->v_stride_t != Dh || a->q_stride_h != (int64_t)a->Lq * Dh ||
      a->k_stride_h != (int64_t)a->Lk * Dh || a->v_stride_h != (int64_t)a->Lk * Dh || a->Lq != a->Lk)
    return AKI_ERR_UNSUPPORTED;
  aki_mma_attn_core_args c = {};
  c.q = a->q; c.k = a->k; c.v = a->v; c.o = a->o; c.B = a->B; c.H = a->H; c.L = a->Lq; c.Dh = a->Dh; c.scale = a->scale;
  c.dtype = AKI_DT_F32; c.dead_rows = AKI_DEAD_ROWS_ZERO;
  return attn_core_f32(&c, ws, ws_bytes, (hipStream_t)stream, 0);
}

// ---- fused MMA op ------------------------------------------------------------------------------------
static size_t qkv_bytes(int B, int H, int L, int Dh, int dtype) {
  return aki_align_up((size_t)B * H * L * Dh * aki_elt_size(dtype), 256);
}

size_t aki_mma_attn_workspace_bytes(int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype) {
  size_t n = 3 * qkv_bytes(B, H, L, Dh, dtype) + aki_mma_attn_core_workspace_bytes(B, H, L, Dh, dtype);
  if (dtype == AKI_DT_F32) n += 3 * qkv_bytes(B, H, L, Dh, dtype);  // un-rotated qkv scratch
  return n;
}

static int check_fused(const aki_mma_attn_args* a) {
  AKI_CHECK_ARG(a && a->x && a->w_qkv && a->cos && a->sin);
  AKI_CHECK_ARG(a->B > 0 && a->H > 0 && a->L > 0 && a->Dh > 0 && a->d_model > 0);
  AKI_CHECK_ARG(a->ldx >= a->d_model && a->ldw >= a->d_model && a->pos_rows > 0);
  AKI_CHECK_ARG(a->position_ids || a->pos_rows >= a->L);
  AKI_CHECK_ARG(dtype_ok(a->dtype) || (a->dtype == AKI_DT_FP8_E4M3 && a->x_scale && a->w_scale));
  AKI_CHECK_ARG(!a->row_scale || a->dtype == AKI_DT_BF16);
  return AKI_OK;
}

int aki_qkv_rope_fwd(const aki_mma_attn_args* a, void* q, void* k, void* v, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  int rc = check_fused(a);
  if (rc) return rc;
  AKI_CHECK_ARG(q && k && v);
  AKI_CHECK_ARG(a->kv_capacity == 0 || a->kv_capacity >= a->L);
  if (a->dtype == AKI_DT_BF16) return qkv_rope_bf16(a, q, k, v, (hipStream_t)stream);
  if (a->dtype == AKI_DT_FP8_E4M3) return qkv_rope_fp8(a, q, k, v, (hipStream_t)stream);
  // f32 parity path: scratch for the un-rotated projection
  if (!ws || ws_bytes < (size_t)a->B * a->L * 3 * a->H * a->Dh * sizeof(float)) return AKI_ERR_WORKSPACE;
  return qkv_rope_f32(a, q, k, v, (float*)ws, (hipStream_t)stream);
}

int aki_mma_attn_fwd(const aki_mma_attn_args* a, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  int rc = check_fused(a);
  if (rc) return rc;
  AKI_CHECK_ARG(a->o && a->scale > 0.f);
  AKI_CHECK_ARG(a->max_rects >= 0 && (a->max_rects == 0 || a->rects));
  const int cdt = a->dtype == AKI_DT_FP8_E4M3 ? AKI_DT_BF16 : a->dtype;     // q, k, v, o and the core are bf16 on the fp8 path
  if (!ws || ws_bytes < aki_mma_attn_workspace_bytes(a->B, a->H, a->L, a->Dh, cdt)) return AKI_ERR_WORKSPACE;
  AKI_CHECK_ALIGN16(ws);
  const size_t qb = qkv_bytes(a->B, a->H, a->L, a->Dh, cdt);
  char* w = (char*)ws;
  void* q = w; void* k = w + qb; void* v = w + 2 * qb;
  char* rest = w + 3 * qb;
  if (a->dtype == AKI_DT_BF16) {
    rc = qkv_rope_bf16(a, q, k, v, (hipStream_t)stream);
  } else if (a->dtype == AKI_DT_FP8_E4M3) {
    rc = qkv_rope_fp8(a, q, k, v, (hipStream_t)stream);
  } else {
    rc = qkv_rope_f32(a, q, k, v, (float*)rest, (hipStream_t)stream);
    rest += 3 * qb;
  }
  if (rc) return rc;
  aki_mma_attn_core_args c = {};
  c.q = q; c.k = k; c.v = v; c.o = a->o; c.lse = a->lse; c.rects = a->rects; c.col_valid_bits = a->col_valid_bits;
  c.seq_lens = a->seq_lens; c.max_rects = a->max_rects; c.B = a->B; c.H = a->H; c.L = a->L; c.Dh = a->Dh;
  c.scale = a->scale; c.dtype = cdt; c.dead_rows = a->dead_rows; c.kv_capacity = 0;
  return aki_mma_attn_core_fwd(&c, rest, aki_mma_attn_core_workspace_bytes(a->B, a->H, a->L, a->Dh, cdt), stream);
}

// ---- linear ------------------------------------------------------------------------------------------
size_t aki_linear_stats_counter_bytes(int32_t M) { return M > 0 ? linear_stats_cnt_bytes(M) : 0; }
size_t aki_linear_stats_workspace_bytes(int32_t M, int32_t N_out) { return (M > 0 && N_out > 0) ? aki_align_up(linear_stats_ws_bytes(M, N_out), 256) : 0; }
size_t aki_linear_splitk_workspace_bytes(int32_t M, int32_t N, int32_t K) { return (M > 0 && N > 0 && K > 0) ? aki_align_up(linear_splitk_plan_ws_bytes(M, N, K), 256) : 0; }

int aki_row_stats(const void* x, int32_t rows, int32_t cols, int32_t ldx, float eps, float* rstd, float* mean, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && rstd && rows > 0 && cols > 0 && ldx >= cols && eps > 0.f);
  if (dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
  return row_stats_launch(x, rows, cols, ldx, eps, rstd, mean, (hipStream_t)stream);
}

int aki_linear_fwd(const aki_linear_args* a, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->x && a->w && a->y);
  AKI_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0);
  AKI_CHECK_ARG(dtype_ok(a->dtype) || (a->dtype == AKI_DT_FP8_E4M3 && a->x_scale && a->w_scale) || (a->dtype == AKI_DT_W8A16 && a->w_scale));
  AKI_CHECK_ARG(a->act >= AKI_ACT_NONE && a->act <= AKI_ACT_SWIGLU);
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  AKI_CHECK_ARG(a->ldx >= a->K && a->ldw >= a->K && a->ldy >= n_out && (!a->residual || a->ldr >= n_out));
  if (a->row_scale || a->row_shift || a->stats_rstd) {   // folded normalisation: the bf16 MFMA GEMM only
    if (a->dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
    return linear_bf16(a, (hipStream_t)stream);
  }
  if (a->preact_out) {   // training forward of the gated MLP: the bf16 MFMA GEMM only (whatever M is)
    if (a->dtype != AKI_DT_BF16 || a->act != AKI_ACT_SWIGLU) return AKI_ERR_UNSUPPORTED;
    return linear_bf16(a, (hipStream_t)stream);
  }
  if (a->w2) {   // two-segment weight: the bf16 MFMA GEMM only
    AKI_CHECK_ARG(a->w2_row0 > 0 && a->w2_rows > 0 && a->w2_row0 < a->N);
    if (a->dtype != AKI_DT_BF16 || a->act != AKI_ACT_NONE) return AKI_ERR_UNSUPPORTED;
    return linear_bf16(a, (hipStream_t)stream);
  }
  if (a->dtype == AKI_DT_FP8_E4M3) return linear_fp8(a, (hipStream_t)stream);
  if (a->dtype == AKI_DT_W8A16) {
    if (a->M >= 2 && a->M <= 16) {   // batched decode in the fp8 configuration: the skinny MFMA GEMM on e4m3 weights
      const int rc = skinny_gemm_w8(a, nullptr, 0.f, (hipStream_t)stream);
      if (rc != AKI_ERR_UNSUPPORTED) return rc;
    }
    return gemv_bf16(a, nullptr, 0.f, (hipStream_t)stream);
  }
  if (a->dtype == AKI_DT_BF16) {
    if (a->M >= 2 && a->M <= 16) {  // batched decode: weight-streaming skinny MFMA GEMM
      const int rc = skinny_gemm_bf16(a, nullptr, 0.f, (hipStream_t)stream);
      if (rc != AKI_ERR_UNSUPPORTED) return rc;
    }
    if (a->M <= 8) {  // decode regime: weight-streaming GEMV (falls through when the shape does not qualify)
      const int rc = gemv_bf16(a, nullptr, 0.f, (hipStream_t)stream);
      if (rc != AKI_ERR_UNSUPPORTED) return rc;
    }
    return linear_bf16(a, (hipStream_t)stream);
  }
  return linear_f32(a, (hipStream_t)stream);
}

// ---- fp8 quantisation --------------------------------------------------------------------------------------
int aki_quant_rows_fp8(const void* x, const void* rms_weight, float rms_eps, void* q, float* scale, int32_t rows, int32_t cols,
                       int32_t ldx, int32_t ldq, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && q && scale && rows > 0 && cols > 0 && ldx >= cols && ldq >= cols && (!rms_weight || rms_eps > 0.f));
  return quant_rows_fp8_launch(x, rms_weight, rms_eps, q, scale, rows, cols, ldx, ldq, (hipStream_t)stream);
}

// ---- norms -------------------------------------------------------------------------------------------
int aki_rmsnorm_fwd(const void* x, const void* w, void* y, int32_t rows, int32_t cols, int32_t ldx, int32_t ldy, float eps,
                    int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && w && y && dtype_ok(dtype) && ldx >= cols && ldy >= cols);
  return norm_launch(true, x, w, nullptr, y, rows, cols, ldx, ldy, eps, dtype, (hipStream_t)stream);
}

int aki_layernorm_fwd(const void* x, const void* w, const void* b, void* y, int32_t rows, int32_t cols, int32_t ldx,
                      int32_t ldy, float eps, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && w && y && dtype_ok(dtype) && ldx >= cols && ldy >= cols);
  return norm_launch(false, x, w, b, y, rows, cols, ldx, ldy, eps, dtype, (hipStream_t)stream);
}

// ---- patch embed -------------------------------------------------------------------------------------
size_t aki_patch_embed_workspace_bytes(int32_t N, int32_t S, int32_t P, int32_t dtype) {
  const int G = S / P;
  const size_t Kp = aki_align_up((size_t)3 * P * P, 64);
  return aki_align_up((size_t)N * G * G * Kp * aki_elt_size(dtype), 256);
}

int aki_patch_embed_fwd(const void* pixels, const void* w, const void* bias, const void* pos, void* out, int32_t N, int32_t S,
                        int32_t P, int32_t E, int32_t Kp, int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(pixels && w && out && N > 0 && S > 0 && P > 0 && E > 0 && dtype_ok(dtype));
  AKI_CHECK_ARG(S >= P && Kp == (int)aki_align_up((size_t)3 * P * P, 64));
  if (!ws || ws_bytes < aki_patch_embed_workspace_bytes(N, S, P, dtype)) return AKI_ERR_WORKSPACE;
  const int G = S / P;
  int rc = im2col_launch(pixels, ws, N, S, P, Kp, dtype, (hipStream_t)stream);
  if (rc) return rc;
  aki_linear_args g = {};
  g.x = ws; g.w = w; g.bias = bias; g.residual = pos; g.y = out;
  g.M = N * G * G; g.N = E; g.K = Kp; g.ldx = Kp; g.ldw = Kp; g.ldy = E; g.ldr = E;
  g.res_row_mod = pos ? G * G : 0; g.act = AKI_ACT_NONE; g.dtype = dtype;
  return aki_linear_fwd(&g, stream);
}

// ---- connector ---------------------------------------------------------------------------------------
size_t aki_connector_mlp_workspace_bytes(int32_t rows, int32_t d, int32_t d_inner, int32_t dtype) {
  return aki_align_up((size_t)rows * d * aki_elt_size(dtype), 256) + aki_align_up((size_t)rows * d_inner * aki_elt_size(dtype), 256);
}

int aki_connector_mlp_fwd(const void* x, const void* ln_w, const void* ln_b, const void* w1, const void* w2, void* out,
                          int32_t rows, int32_t d, int32_t d_inner, float eps, int32_t dtype, void* ws, size_t ws_bytes,
                          void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && ln_w && w1 && w2 && out && rows > 0 && d > 0 && d_inner > 0 && dtype_ok(dtype));
  if (!ws || ws_bytes < aki_connector_mlp_workspace_bytes(rows, d, d_inner, dtype)) return AKI_ERR_WORKSPACE;
  char* normed = (char*)ws;
  char* hidden = normed + aki_align_up((size_t)rows * d * aki_elt_size(dtype), 256);
  int rc = aki_layernorm_fwd(x, ln_w, ln_b, normed, rows, d, d, d, eps, dtype, stream);
  if (rc) return rc;
  aki_linear_args g = {};
  g.x = normed; g.w = w1; g.y = hidden; g.M = rows; g.N = d_inner; g.K = d; g.ldx = d; g.ldw = d; g.ldy = d_inner;
  g.act = AKI_ACT_GELU_ERF; g.dtype = dtype;
  rc = aki_linear_fwd(&g, stream);
  if (rc) return rc;
  aki_linear_args g2 = {};
  g2.x = hidden; g2.w = w2; g2.y = out; g2.residual = x; g2.M = rows; g2.N = d; g2.K = d_inner; g2.ldx = d_inner; g2.ldw = d_inner;
  g2.ldy = d; g2.ldr = d; g2.act = AKI_ACT_NONE; g2.dtype = dtype;
  return aki_linear_fwd(&g2, stream);
}

int aki_connector_proj_fwd(const void* x, const void* ln_w, const void* ln_b, const void* w, const void* b, void* out,
                           int32_t rows, int32_t d, int32_t d_out, float eps, int32_t dtype, void* ws, size_t ws_bytes,
                           void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && ln_w && w && out && rows > 0 && d > 0 && d_out > 0 && dtype_ok(dtype));
  if (!ws || ws_bytes < aki_align_up((size_t)rows * d * aki_elt_size(dtype), 256)) return AKI_ERR_WORKSPACE;
  int rc = aki_layernorm_fwd(x, ln_w, ln_b, ws, rows, d, d, d, eps, dtype, stream);
  if (rc) return rc;
  aki_linear_args g = {};
  g.x = ws; g.w = w; g.bias = b; g.y = out; g.M = rows; g.N = d_out; g.K = d; g.ldx = d; g.ldw = d; g.ldy = d_out;
  g.act = AKI_ACT_NONE; g.dtype = dtype;
  return aki_linear_fwd(&g, stream);
}

// ---- decode ------------------------------------------------------------------------------------------
int aki_rope_append_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* pos, const int32_t* cache_len, void* q_out,
                        void* k_cache, void* v_cache, int32_t B, int32_t H, int32_t Dh, int32_t capacity, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(qkv && cos && sin && pos && cache_len && q_out && k_cache && v_cache);
  AKI_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && (Dh % 2) == 0 && capacity > 0 && dtype_ok(dtype));
  return rope_append_launch(qkv, cos, sin, pos, cache_len, q_out, k_cache, v_cache, B, H, Dh, capacity, dtype, (hipStream_t)stream);
}

size_t aki_decode_attn_workspace_bytes(int32_t B, int32_t H, int32_t Dh, int32_t capacity) {
  if (B <= 0 || H <= 0 || Dh <= 0 || capacity <= 0) return 0;
  return decode_attn_ws_bytes(B, H, Dh, capacity);
}

int aki_decode_attn_fwd(const void* q, const void* k_cache, const void* v_cache, void* o, const int32_t* n_keys,
                        const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H, int32_t Dh, int32_t capacity,
                        int32_t max_keys, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(q && k_cache && v_cache && o && n_keys && B > 0 && H > 0 && Dh > 0 && capacity > 0 && scale > 0.f && dtype_ok(dtype));
  AKI_CHECK_ARG(!col_valid_bits || nwords > 0);
  if (dtype == AKI_DT_BF16 && Dh == 96)
    return decode_attn_split_launch(q, nullptr, nullptr, n_keys, (void*)k_cache, (void*)v_cache, o, col_valid_bits, nwords, B, H,
                                    capacity, max_keys, scale, false, ws, ws_bytes, (hipStream_t)stream);
  return decode_attn_launch(q, k_cache, v_cache, o, n_keys, col_valid_bits, nwords, B, H, Dh, capacity, scale, dtype, (hipStream_t)stream);
}

int aki_decode_attn_fused_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, void* k_cache,
                              void* v_cache, void* o, const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H,
                              int32_t Dh, int32_t capacity, int32_t max_keys, float scale, int32_t dtype, void* ws, size_t ws_bytes,
                              void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(qkv && cos && sin && cache_len && k_cache && v_cache && o);
  AKI_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && (Dh % 2) == 0 && capacity > 0 && scale > 0.f && dtype_ok(dtype));
  AKI_CHECK_ARG(!col_valid_bits || nwords > 0);
  if (dtype == AKI_DT_BF16 && Dh == 96)
    return decode_attn_split_launch(qkv, cos, sin, cache_len, k_cache, v_cache, o, col_valid_bits, nwords, B, H, capacity, max_keys,
                                    scale, true, ws, ws_bytes, (hipStream_t)stream);
  return AKI_ERR_UNSUPPORTED;   // f32 / other head sizes: call aki_rope_append_fwd + aki_decode_attn_fwd
}

int aki_kv_cache_quant_fp8(const void* src, int32_t src_capacity, void* dst, float* scale, int32_t dst_capacity, int32_t slabs, int32_t rows,
                           int32_t Dh, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(src && dst && scale);
  AKI_CHECK_ARG(src_capacity > 0 && dst_capacity > 0 && slabs > 0 && rows >= 0 && rows <= src_capacity && rows <= dst_capacity);
  if (Dh != 96 || dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7) || ((uintptr_t)scale & 3)) return AKI_ERR_ALIGNMENT;
  return kv_cache_quant_fp8_launch(src, src_capacity, dst, scale, dst_capacity, slabs, rows, (hipStream_t)stream);
}

int aki_decode_attn_fused_fp8kv_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, void* k_cache,
                                    void* v_cache, float* k_scale, float* v_scale, void* o, const uint64_t* col_valid_bits, int32_t nwords,
                                    int32_t B, int32_t H, int32_t Dh, int32_t capacity, int32_t max_keys, float scale, int32_t dtype, void* ws,
                                    size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(qkv && cos && sin && cache_len && k_cache && v_cache && k_scale && v_scale && o);
  AKI_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && capacity > 0 && scale > 0.f);
  AKI_CHECK_ARG(!col_valid_bits || nwords > 0);
  if (Dh != 96 || dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) || ((uintptr_t)o & 15)) return AKI_ERR_ALIGNMENT;
  return decode_attn_split_fp8kv_launch(qkv, cos, sin, cache_len, k_cache, v_cache, k_scale, v_scale, o, col_valid_bits, nwords, B, H, capacity,
                                        max_keys, scale, ws, ws_bytes, (hipStream_t)stream);
}

size_t aki_decode_attn_group_workspace_bytes(int32_t B0, int32_t N, int32_t H, int32_t Dh, int32_t prefix_capacity, int32_t suffix_capacity) {
  if (B0 <= 0 || N <= 0 || H <= 0 || Dh != 96 || prefix_capacity <= 0 || suffix_capacity <= 0) return 0;
  return decode_attn_group_ws_bytes(B0, N, H, prefix_capacity, suffix_capacity);
}

int aki_decode_attn_group_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, const int32_t* prefix_len,
                              const void* k_prefix, const void* v_prefix, void* k_suffix, void* v_suffix, void* o,
                              const uint64_t* col_valid_bits, int32_t nwords, int32_t B0, int32_t N, int32_t H, int32_t Dh,
                              int32_t prefix_capacity, int32_t suffix_capacity, int32_t max_prefix_keys, int32_t max_suffix_keys, float scale,
                              int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(qkv && cos && sin && cache_len && prefix_len && k_prefix && v_prefix && k_suffix && v_suffix && o);
  AKI_CHECK_ARG(B0 > 0 && N > 0 && H > 0 && Dh > 0 && prefix_capacity > 0 && suffix_capacity > 0 && scale > 0.f);
  AKI_CHECK_ARG(!col_valid_bits || nwords > 0);
  if (Dh != 96 || dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)k_prefix & 15) || ((uintptr_t)v_prefix & 15) || ((uintptr_t)k_suffix & 15) || ((uintptr_t)v_suffix & 15) || ((uintptr_t)o & 15))
    return AKI_ERR_ALIGNMENT;
  return decode_attn_group_launch(qkv, cos, sin, cache_len, prefix_len, k_prefix, v_prefix, k_suffix, v_suffix, o, col_valid_bits, nwords, B0, N,
                                  H, prefix_capacity, suffix_capacity, max_prefix_keys, max_suffix_keys, scale, ws, ws_bytes,
                                  (hipStream_t)stream);
}

size_t aki_chunk_attn_workspace_bytes(int32_t B, int32_t H, int32_t T, int32_t Dh) {
  if (B <= 0 || H <= 0 || T <= 0 || Dh != 96) return 0;
  return chunk_attn_ws_bytes(B, H, T);
}

int aki_chunk_attn_fwd(const void* qkv, const float* cos, const float* sin, const int32_t* cache_len, const int32_t* n_new, void* k_cache,
                       void* v_cache, void* o, const uint64_t* col_valid_bits, int32_t nwords, int32_t B, int32_t H, int32_t Dh, int32_t T,
                       int32_t max_new, int32_t capacity, float scale, int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(qkv && cos && sin && cache_len && k_cache && v_cache && o);
  AKI_CHECK_ARG(B > 0 && H > 0 && Dh > 0 && T > 0 && capacity > 0 && max_new >= 0 && scale > 0.f);
  AKI_CHECK_ARG(!col_valid_bits || nwords > 0);
  if (Dh != 96 || dtype != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) || ((uintptr_t)o & 15) || ((uintptr_t)ws & 15)) return AKI_ERR_ALIGNMENT;
  return chunk_attn_launch(qkv, cos, sin, cache_len, n_new, k_cache, v_cache, o, col_valid_bits, nwords, B, H, T, max_new, capacity, scale, ws,
                           ws_bytes, (hipStream_t)stream);
}

int aki_decode_linear_fwd(const aki_linear_args* a, const void* rms_weight, float rms_eps, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->x && a->w && a->y && rms_weight && rms_eps > 0.f);
  AKI_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0 && (a->dtype == AKI_DT_BF16 || (a->dtype == AKI_DT_W8A16 && a->w_scale)));
  AKI_CHECK_ARG(a->act >= AKI_ACT_NONE && a->act <= AKI_ACT_SWIGLU);
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  AKI_CHECK_ARG(a->ldx >= a->K && a->ldw >= a->K && a->ldy >= n_out && (!a->residual || a->ldr >= n_out));
  if (a->M >= 2 && a->M <= 8) {      // batched decode: the skinny MFMA GEMM with the norm in its prologue
    const int rc = a->dtype == AKI_DT_BF16 ? skinny_gemm_bf16(a, rms_weight, rms_eps, (hipStream_t)stream)
                                           : skinny_gemm_w8(a, rms_weight, rms_eps, (hipStream_t)stream);
    if (rc != AKI_ERR_UNSUPPORTED) return rc;
  }
  return gemv_bf16(a, rms_weight, rms_eps, (hipStream_t)stream);
}

// ---- MXFP4 weight-only decode (mxfp4.hip) ------------------------------------------------------------------
int aki_quant_mxfp4(const void* w, int32_t N, int32_t K, int32_t ldw, uint8_t* wq, uint8_t* ws, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(w && wq && ws && N > 0 && K > 0 && ldw >= K);
  return quant_mxfp4_launch(w, N, K, ldw, wq, ws, (hipStream_t)stream);
}

int aki_linear_w4_fwd(const aki_linear_args* a, const uint8_t* w_scale_e8m0, const void* rms_weight, float rms_eps, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->x && a->w && a->y && w_scale_e8m0 && (!rms_weight || rms_eps > 0.f));
  AKI_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0);
  AKI_CHECK_ARG(a->act >= AKI_ACT_NONE && a->act <= AKI_ACT_SWIGLU);
  if (a->dtype != AKI_DT_BF16 || a->K % 32 || a->M > 16) return AKI_ERR_UNSUPPORTED;
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  AKI_CHECK_ARG(a->ldx >= a->K && a->ldw >= a->K / 2 && a->ldy >= n_out && (!a->residual || a->ldr >= n_out));
  if (a->M == 1) return gemv_w4(a, w_scale_e8m0, rms_weight, rms_eps, (hipStream_t)stream);
  return skinny_gemm_w4(a, w_scale_e8m0, rms_weight, rms_eps, (hipStream_t)stream);
}

size_t aki_decode_chain_workspace_bytes(int32_t n_layers, int32_t d, int32_t H, int32_t F, int32_t capacity) {
  if (n_layers <= 0 || d <= 0 || H <= 0 || F <= 0 || capacity <= 0) return 0;
  return decode_chain_ws_bytes(n_layers, d, H, F, capacity);
}

size_t aki_decode_chain_error_offset(int32_t n_layers, int32_t H) { return (n_layers > 0 && H > 0) ? decode_chain_err_offset(n_layers, H) : 0; }

size_t aki_decode_chain_batch_workspace_bytes(int32_t n_layers, int32_t d, int32_t H, int32_t F, int32_t capacity, int32_t batch) {
  if (batch <= 1) return aki_decode_chain_workspace_bytes(n_layers, d, H, F, capacity);
  if (n_layers <= 0 || d <= 0 || H <= 0 || F <= 0 || capacity <= 0 || batch > 8) return 0;
  return decode_chain_b_ws_bytes(n_layers, d, H, F, capacity, batch);
}

size_t aki_decode_chain_batch_error_offset(int32_t n_layers, int32_t H, int32_t batch) {
  if (batch <= 1) return aki_decode_chain_error_offset(n_layers, H);
  return (n_layers > 0 && H > 0 && batch <= 8) ? decode_chain_b_err_offset(n_layers, H, batch) : 0;
}

int aki_decode_chain_fwd(const aki_decode_chain_args* a, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->layers && a->h_in && a->h_out && a->cos && a->sin && a->cache_len && a->workspace);
  AKI_CHECK_ARG(a->n_layers > 0 && a->d > 0 && a->H > 0 && a->Dh > 0 && a->F > 0 && a->capacity > 0 && a->scale > 0.f && a->rms_eps > 0.f);
  AKI_CHECK_ARG(!a->col_valid_bits || a->nwords > 0);
  return decode_chain_launch(a, (hipStream_t)stream);
}

// ---- training step ---------------------------------------------------------------------------------------
#define AKI_BF16_ONLY(dt) do { if ((dt) != AKI_DT_BF16) return AKI_ERR_UNSUPPORTED; } while (0)

size_t aki_attn_bwd_workspace_bytes(int32_t B, int32_t H, int32_t Lq) { return (B > 0 && H > 0 && Lq > 0) ? attn_bwd_ws_bytes(B, H, Lq) : 0; }

int aki_attn_bwd(const aki_attn_bwd_args* a, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->q && a->k && a->v && a->o && a->d_o && a->lse && a->dq && a->dk && a->dv);
  AKI_CHECK_ARG(a->B > 0 && a->H > 0 && a->Lq > 0 && a->Lk > 0 && a->scale > 0.f);
  AKI_CHECK_ARG(a->max_rects >= 0 && a->max_rects <= AKI_MAX_RECTS);
  AKI_BF16_ONLY(a->dtype);
  return attn_bwd_bf16(a->q, a->k, a->v, a->o, a->d_o, a->lse, a->dq, a->dk, a->dv, a->rects, a->max_rects, a->col_valid_bits,
                       a->seq_lens, a->masked, a->B, a->H, a->Lq, a->Lk, a->Dh, a->scale, ws, ws_bytes, (hipStream_t)stream);
}

int aki_transpose(const void* x, void* y, int32_t R, int32_t C, int32_t ldx, int32_t ldy, int32_t Rpad, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && y && R > 0 && C > 0 && ldx >= C && Rpad >= R && ldy >= Rpad);
  AKI_BF16_ONLY(dtype);
  return transpose_bf16_launch(x, y, R, C, ldx, ldy, Rpad, (hipStream_t)stream);
}

int aki_gemm_tn(const void* a, const void* b, void* c, int32_t Kc, int32_t I, int32_t J, int64_t lda, int64_t ldb, int64_t ldc, int32_t dtype,
                void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && b && c && Kc > 0 && I > 0 && J > 0 && lda >= I && ldb >= J && ldc >= J);
  AKI_BF16_ONLY(dtype);
  return gemm_tn_launch(a, b, c, Kc, I, J, (long)lda, (long)ldb, (long)ldc, (hipStream_t)stream);
}

size_t aki_norm_bwd_workspace_bytes(int32_t cols) { return cols > 0 ? norm_bwd_ws_bytes(cols) : 0; }

int aki_norm_bwd(int32_t rms, const void* x, const void* w, const void* dy, const void* dres, void* dx, void* dw, void* db, int32_t rows,
                 int32_t cols, int32_t ldx, int32_t lddy, int32_t lddr, int32_t lddx, float eps, int32_t accumulate, int32_t dtype,
                 void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && w && dy && dx && dw && rows > 0 && cols > 0 && ldx >= cols && lddy >= cols && lddx >= cols);
  AKI_CHECK_ARG((ldx % 8) == 0 && (lddy % 8) == 0 && (lddx % 8) == 0 && (!dres || (lddr >= cols && (lddr % 8) == 0)));
  AKI_BF16_ONLY(dtype);
  return norm_bwd_launch(rms != 0, x, w, dy, dres, dx, dw, db, rows, cols, ldx, lddy, lddx, lddr, eps, accumulate, ws, ws_bytes,
                         (hipStream_t)stream);
}

size_t aki_colsum_workspace_bytes(int32_t cols) { return cols > 0 ? colsum_ws_bytes(cols) : 0; }

int aki_colsum(const void* x, void* out, int32_t rows, int32_t cols, int32_t ldx, int32_t accumulate, int32_t dtype, void* ws,
               size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && out && rows > 0 && cols > 0 && ldx >= cols);
  AKI_BF16_ONLY(dtype);
  return colsum_launch(x, out, rows, cols, ldx, accumulate, ws, ws_bytes, (hipStream_t)stream);
}

int aki_swiglu_fwd(const void* gate_up, void* a, int32_t rows, int32_t F, int32_t ldg, int32_t lda, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(gate_up && a && rows > 0 && F > 0 && ldg >= 2 * F && lda >= F);
  AKI_BF16_ONLY(dtype);
  return swiglu_launch(0, gate_up, nullptr, a, rows, F, ldg, 0, lda, (hipStream_t)stream);
}

int aki_swiglu_bwd(const void* gate_up, const void* da, void* dgate_up, int32_t rows, int32_t F, int32_t ldg, int32_t ldda, int32_t lddg,
                   int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(gate_up && da && dgate_up && rows > 0 && F > 0 && ldg >= 2 * F && ldda >= F && lddg >= 2 * F);
  AKI_BF16_ONLY(dtype);
  return swiglu_launch(1, gate_up, da, dgate_up, rows, F, ldg, ldda, lddg, (hipStream_t)stream);
}

int aki_gelu_fwd(const void* x, void* y, size_t n, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && y && n > 0);
  AKI_BF16_ONLY(dtype);
  return gelu_launch(0, x, nullptr, y, n, (hipStream_t)stream);
}

int aki_gelu_bwd(const void* x, const void* dy, void* dx, size_t n, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(x && dy && dx && n > 0);
  AKI_BF16_ONLY(dtype);
  return gelu_launch(1, x, dy, dx, n, (hipStream_t)stream);
}

int aki_rope_bwd_merge(const void* dq, const void* dk, const void* dv, const float* cos, const float* sin, const int32_t* position_ids,
                       void* dqkv, int32_t B, int32_t H, int32_t L, int32_t Dh, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(dq && dk && dv && cos && sin && dqkv && B > 0 && H > 0 && L > 0 && Dh > 0);
  AKI_BF16_ONLY(dtype);
  return rope_bwd_merge_launch(dq, dk, dv, cos, sin, position_ids, dqkv, B, H, L, Dh, (hipStream_t)stream);
}

int aki_ce_loss_fwd_bwd(const void* logits, const int64_t* labels, int32_t* n_valid, float* loss_rows, void* dlogits, int32_t B, int32_t L,
                        int32_t V, int32_t ldl, int32_t lddl, float gscale, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(logits && labels && n_valid && loss_rows && B > 0 && L > 0 && V > 0 && ldl >= V && (!dlogits || lddl >= V));
  AKI_BF16_ONLY(dtype);
  return ce_launch(logits, labels, n_valid, loss_rows, dlogits, B, L, V, ldl, lddl, gscale, (hipStream_t)stream);
}

int aki_ce_rows_fwd_bwd(const void* logits, const int64_t* targets, const int32_t* n_valid, float* loss_rows, void* dlogits, int32_t rows,
                        int32_t V, int32_t ldl, int32_t lddl, float gscale, int32_t dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(logits && targets && n_valid && loss_rows && rows > 0 && V > 0 && ldl >= V && (!dlogits || lddl >= V));
  AKI_BF16_ONLY(dtype);
  return ce_rows_launch(logits, targets, n_valid, loss_rows, dlogits, rows, V, ldl, lddl, gscale, (hipStream_t)stream);
}

size_t aki_grad_sqnorm_workspace_bytes(void) { return grad_sqnorm_ws_bytes(); }

int aki_grad_sqnorm(const void* g, size_t n, float* out, int32_t accumulate, int32_t dtype, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(g && out && n > 0);
  if (dtype != AKI_DT_BF16 && dtype != AKI_DT_F32) return AKI_ERR_UNSUPPORTED;
  return grad_sqnorm_launch(g, n, out, accumulate, ws, ws_bytes, dtype == AKI_DT_F32, (hipStream_t)stream);
}

int aki_adamw_step(float* p, float* m, float* v, const void* g, void* w16, size_t n, const float* sqnorm, float max_norm, float gscale,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(p && m && v && g && w16 && n > 0 && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f);
  return adamw_launch(p, m, v, g, w16, n, sqnorm, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step, false, (hipStream_t)stream);
}

int aki_adamw_step_t(float* p, float* m, float* v, const void* g, void* w16, void* wT, int32_t N, int32_t K, int32_t ldT, const float* sqnorm,
                     float max_norm, float gscale, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                     int32_t grad_dtype, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(p && m && v && g && w16 && wT && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f);
  if (grad_dtype != AKI_DT_BF16 && grad_dtype != AKI_DT_F32) return AKI_ERR_UNSUPPORTED;
  return adamw_t_launch(p, m, v, g, w16, wT, N, K, ldT, sqnorm, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step, grad_dtype == AKI_DT_F32,
                        (hipStream_t)stream);
}

int aki_adamw_step_g32(float* p, float* m, float* v, const float* g, void* w16, size_t n, const float* sqnorm, float max_norm, float gscale,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(p && m && v && g && w16 && n > 0 && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f);
  return adamw_launch(p, m, v, g, w16, n, sqnorm, max_norm, gscale, lr, beta1, beta2, eps, weight_decay, step, true, (hipStream_t)stream);
}

// ---- splice / mask -------------------------------------------------------------------------------------
int aki_splice_plan(const int64_t* lang_x, int32_t B, int32_t T, int64_t media_token_id, int64_t assistant_token_id,
                    int32_t Nv, int32_t* plan, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(lang_x && plan && B > 0 && T > 0 && Nv > 0);
  return splice_plan_launch(lang_x, B, T, media_token_id, assistant_token_id, Nv, plan, (hipStream_t)stream);
}

int aki_splice_fwd(const aki_splice_args* a, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(a && a->lang_x && a->embed_weight && a->plan && a->inputs_embeds);
  AKI_CHECK_ARG(a->B > 0 && a->T > 0 && a->Nv > 0 && a->d > 0 && a->L_out > 0 && dtype_ok(a->dtype));
  AKI_CHECK_ARG(a->T_img == 0 || a->vision_tokens);
  AKI_CHECK_ARG(a->max_rects >= 0 && a->max_rects <= AKI_MAX_RECTS);
  AKI_CHECK_ARG(a->padding_side == 0 || a->padding_side == 1);
  if (((size_t)a->d * aki_elt_size(a->dtype)) % 16) return AKI_ERR_ALIGNMENT;
  AKI_CHECK_ALIGN16(a->embed_weight); AKI_CHECK_ALIGN16(a->embed_additional); AKI_CHECK_ALIGN16(a->vision_tokens);
  AKI_CHECK_ALIGN16(a->inputs_embeds);
  return splice_launch(a, (hipStream_t)stream);
}

int aki_mma_mask_dense(const aki_mma_rect* rects, int32_t max_rects, const uint64_t* col_valid_bits, const int32_t* seq_lens,
                       int32_t B, int32_t L, int64_t* out, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(out && B > 0 && L > 0 && max_rects >= 0 && max_rects <= AKI_MAX_RECTS && (max_rects == 0 || rects));
  return mask_dense_launch(rects, max_rects, col_valid_bits, seq_lens, B, L, out, (hipStream_t)stream);
}

int aki_sft_collate_pad(const int64_t* ids, const int64_t* labels, const int64_t* attention_mask, const int32_t* offsets, int32_t B,
                        int32_t T_out, int64_t pad_token_id, int64_t ignore_index, int32_t padding_side, int64_t* out_ids,
                        int64_t* out_labels, int64_t* out_mask, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(ids && offsets && out_ids && B > 0 && T_out > 0 && (padding_side == 0 || padding_side == 1));
  AKI_CHECK_ARG((!out_labels || labels) && (!out_mask || attention_mask));
  return sft_collate_launch(ids, labels, attention_mask, offsets, B, T_out, pad_token_id, ignore_index, padding_side, out_ids, out_labels,
                            out_mask, (hipStream_t)stream);
}

// ---- the picks and the logits processors (include/aki_mi355x.h) -------------------------------------------------------------------------
// Every entry point fills a PickCall (pick_params.h) from its argument groups, then pick_call_check and pick_call_launch (decode.hip) do
// the rest: each argument rule is written once, below.

// the processor arguments of the call-wide forms
static bool processors_ok(const ProcParams& q) {
  return q.V <= AKI_LOGITS_PROCESS_MAX_V && q.penalty > 0.f && q.penalty <= 3.0e38f && q.ngram >= 0 && q.min_len >= 0 && q.n_suppress >= 0 &&
         (q.n_suppress == 0 || q.suppress) && q.n_begin >= 0 && (q.n_begin == 0 || q.begin_suppress) && q.n_bad >= 0 &&
         q.n_bad_ids >= q.n_bad && (q.n_bad == 0 || (q.bad_ids && q.bad_off));
}

// The per-row processor forms: the pool's arrays and the rows' set indices.  Their VALUES are the caller's: the kernel reads a set index
// outside the pool as the neutral set and cuts every range at the pools' ends.
static bool processor_sets_ok(int32_t V, const ProcSetParams& ps) {
  return V <= AKI_LOGITS_PROCESS_MAX_V && ps.sets && ps.n_sets > 0 && ps.row_set && ps.n_ids >= 0 && (ps.n_ids == 0 || ps.ids) &&
         ps.n_words >= 0 && (ps.n_words == 0 || (ps.bad_off && ps.ids));
}

// The constrained forms: a device table with a row for every state and a state history with at least its start column.  CON_WIDE: one
// automaton, below 32768 states.  The per-row kinds: the table is a pool of n_states rows (any positive count: a row's own automaton stays
// below 32768 states, the pool need not), and every row names its slice; the arrays' values are the caller's: the kernel cuts a slice at
// the pool's end.
static bool constraint_ok(int kind, int32_t V, const ConstraintParams& c, int64_t table_ld) {
  if (kind == CON_NONE || ((kind == CON_ROWS_OR_NONE || kind == CON_WIDE_OR_NONE) && !c.table)) return true;
  if (!(c.table && c.states && c.n_states > 0 && table_ld >= V && table_ld < (1ll << 31) && c.states_ld >= 1)) return false;
  return (kind == CON_WIDE || kind == CON_WIDE_OR_NONE) ? c.n_states <= 32767 : (c.row_base && c.row_states);
}

// the sampler's own arguments (the greedy forms have none: step is 0)
static bool sampler_ok(const PickCall& c) {
  if (c.p.step < 0) return false;
  if (c.sampler == SAMPLER_ROWS) {                // device arrays: their values are the caller's to check
    return c.sr.temperature && c.sr.top_k && c.sr.top_p && c.sr.seed && (!c.sr.probs || (c.ld_probs >= c.p.V && c.ld_probs < (1ll << 31)));
  }
  if (c.sampler == SAMPLER_SCALAR) {
    return c.sp.temperature > 0.f && c.sp.temperature <= 3.0e38f && c.sp.top_p > 0.f && c.sp.top_p <= 1.f && c.sp.top_k >= 0 &&
           (!c.sp.probs || (c.ld_probs >= c.p.V && c.ld_probs < (1ll << 31)));
  }
  return true;
}

static int pick_call_check(const PickCall& c) {
  const PickParams& p = c.p;
  const ProcParams& q = c.q;
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(p.logits && p.ids && p.B > 0 && p.V > 0 && c.ld >= p.V && c.ld < (1ll << 31) && p.n_eos >= 0 && (p.n_eos == 0 || p.eos));
  AKI_CHECK_ARG((!p.tokens || p.tokens_ld > 0) && (!p.advance || p.cache_len) && (p.advance == 0 || p.advance == 1));
  if (c.processed) {
    AKI_CHECK_ARG(q.out && c.ld_scores >= p.V && c.ld_scores < (1ll << 31));
    AKI_CHECK_ARG(c.sets ? processor_sets_ok(p.V, c.ps) : processors_ok(q));
  }
  AKI_CHECK_ARG(constraint_ok(c.constraint, p.V, q.c, c.table_ld));
  // aki_sample_pick_rows_processed has always looked at its sampler arguments last: a misaligned scratch outranks them there, and only there
  if (!c.sets) AKI_CHECK_ARG(sampler_ok(c));
  if (c.processed && ((((uintptr_t)q.out) & 15) != 0 || (c.ld_scores & 3) != 0)) return AKI_ERR_ALIGNMENT;
  if (p.emb_main || c.embed_required) {
    AKI_CHECK_ARG(p.emb_main && p.emb_out && p.d > 0 && p.d % 8 == 0 && p.max_original_id >= 0 && c.num_additional >= 0);
    AKI_CHECK_ARG((((uintptr_t)p.emb_main | (uintptr_t)p.emb_extra | (uintptr_t)p.emb_out) & 15) == 0);
    // every id the pick can produce has a row: V' = original rows + additional rows (DecoupledLinear's output width), pad included
    AKI_CHECK_ARG((int64_t)p.V <= p.max_original_id + 1 + (p.emb_extra ? c.num_additional : 0) && p.pad >= 0 &&
                  p.pad <= p.max_original_id + (p.emb_extra ? c.num_additional : 0));
  } else {
    AKI_CHECK_ARG(!p.emb_extra && !p.emb_out);
  }
  if (c.sets) AKI_CHECK_ARG(sampler_ok(c));
  return AKI_OK;
}

static int pick_call(const PickCall& c, void* stream) {
  const int rc = pick_call_check(c);
  return rc != AKI_OK ? rc : pick_call_launch(c, (hipStream_t)stream);
}

// -- the argument groups, in the order the entry points take them
// the 15 every pick begins with
static PickCall pick_common(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                            uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                            int32_t advance, int32_t* done_at) {
  PickCall c{};
  c.p = PickParams{(const bf16_t*)logits, B, V, (int)ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len,
                   advance, done_at};
  c.ld = ld;
  return c;
}

// the embedding gather's 6
static void pick_embed(PickCall& c, const void* embed_weight, const void* additional_weight, int64_t max_original_id, int64_t num_additional,
                       int32_t d, void* next_embeds) {
  c.p.emb_main = (const bf16_t*)embed_weight; c.p.emb_extra = (const bf16_t*)additional_weight; c.p.max_original_id = max_original_id;
  c.p.d = d; c.p.emb_out = (bf16_t*)next_embeds;
  c.num_additional = num_additional;
}

// what a logits-process launch reads of the call, with neutral processor values
static ProcParams proc_common(const void* in, int in_f32, int64_t ld_in, float* out, int64_t ld_out, int32_t V, const int64_t* tokens,
                              int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step, const uint8_t* done,
                              const int64_t* eos_ids, int32_t n_eos) {
  ProcParams q{};
  q.in = in; q.in_f32 = in_f32; q.ld_in = (int)ld_in; q.out = out; q.ld_out = (int)ld_out; q.V = V; q.tokens = tokens; q.tokens_ld = tokens_ld;
  q.cache_len = cache_len; q.start_len = start_len; q.step = step; q.done = done; q.penalty = 1.f; q.eos = eos_ids; q.n_eos = n_eos;
  return q;
}

// the f32 scratch of the processed picks: the processors read what the pick reads
static void pick_scratch(PickCall& c, float* scores, int64_t ld_scores) {
  const PickParams& p = c.p;
  c.q = proc_common(p.logits, 0, c.ld, scores, ld_scores, p.V, p.tokens, p.tokens_ld, p.cache_len, p.start_len, 0, p.done, p.eos, p.n_eos);
  c.ld_scores = ld_scores;
  c.processed = true;
}

// the call-wide processors' 11
static void proc_values(ProcParams& q, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids,
                        int32_t n_suppress, const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                        const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids) {
  q.penalty = repetition_penalty; q.ngram = no_repeat_ngram_size; q.min_len = min_length;
  q.suppress = suppress_ids; q.n_suppress = n_suppress; q.begin_suppress = begin_suppress_ids; q.n_begin = n_begin_suppress;
  q.bad_ids = bad_ids; q.bad_off = bad_offsets; q.n_bad = n_bad; q.n_bad_ids = n_bad_ids;
}

// the per-row processor sets' 7
static ProcSetParams proc_sets(const int32_t* sets, int32_t n_sets, const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids,
                               const int32_t* bad_offsets, int32_t n_words) {
  return ProcSetParams{sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words};
}

// the constraint's 5 (row_base and row_states null) or 7
static ConstraintParams constraint(const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                                   const int32_t* row_base = nullptr, const int32_t* row_states = nullptr) {
  return ConstraintParams{table, (int)table_ld, n_states, states, states_ld, row_base, row_states};
}

static void pick_constraint(PickCall& c, int kind, const ConstraintParams& con, int64_t table_ld) {
  c.q.c = con; c.constraint = kind; c.table_ld = table_ld;
}

// the scalar sampler's 8
static void pick_sampler(PickCall& c, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed, uint64_t offset,
                         float* probs_out, int64_t ld_probs) {
  c.p.step = step;
  c.sp = SampleParams{temperature, top_k, top_p, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32),
                      probs_out, (int)ld_probs, 0};
  c.sampler = SAMPLER_SCALAR; c.ld_probs = ld_probs;
}

// the per-row sampler's 7: four device arrays of B entries in the scalars' place
static void pick_sampler_rows(PickCall& c, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                              const uint64_t* seed, float* probs_out, int64_t ld_probs) {
  c.p.step = step;
  c.sr = SampleRowParams{temperature, top_k, top_p, (const unsigned long long*)seed, probs_out, (int)ld_probs, 0};
  c.sampler = SAMPLER_ROWS; c.ld_probs = ld_probs;
}

int aki_greedy_pick(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                    uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                    int32_t advance, int32_t* done_at, void* stream) {
  const PickCall c = pick_common(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                                 done_at);
  return pick_call(c, stream);
}

int aki_greedy_pick_embed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                          uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                          int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                          int64_t num_additional, int32_t d, void* next_embeds, void* stream) {
  PickCall c = pick_common(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                           done_at);
  pick_embed(c, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds);
  c.embed_required = true;
  return pick_call(c, stream);
}

// the 15 + 6 + 2 + 11 arguments aki_greedy_pick_processed, its constrained forms and the scalar-processor samplers begin with
static PickCall pick_processed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                               uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                               int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight,
                               int64_t max_original_id, int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores,
                               float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids,
                               int32_t n_suppress, const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                               const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids) {
  PickCall c = pick_common(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                           done_at);
  pick_embed(c, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds);
  pick_scratch(c, scores, ld_scores);
  proc_values(c.q, repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_ids,
              bad_offsets, n_bad, n_bad_ids);
  return c;
}

// the 15 + 6 + 2 + 7 arguments the per-row processor picks begin with; their constraint is per row, and optional
static PickCall pick_processed_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                    int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                    int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                    const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                    void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                    const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                    int32_t n_words) {
  PickCall c = pick_common(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                           done_at);
  pick_embed(c, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds);
  pick_scratch(c, scores, ld_scores);
  c.ps = proc_sets(sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  c.sets = true;
  return c;
}

int aki_greedy_pick_processed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, void* stream) {
  const PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                                    done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                                    repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                                    n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  return pick_call(c, stream);
}

int aki_greedy_pick_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_constraint(c, CON_WIDE, constraint(table, table_ld, n_states, states, states_ld), table_ld);
  return pick_call(c, stream);
}

int aki_greedy_pick_constrained_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                     uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                     int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                     int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                     int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                     const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                     int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                                     int32_t states_ld, const int32_t* row_base, const int32_t* row_states, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_constraint(c, CON_ROWS, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  return pick_call(c, stream);
}

int aki_sample_pick(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                    uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                    int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                    int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                    int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                    const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                    int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                    uint64_t offset, float* probs_out, int64_t ld_probs, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_sampler(c, step, temperature, top_k, top_p, seed, offset, probs_out, ld_probs);
  return pick_call(c, stream);
}

int aki_sample_pick_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                         uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                         int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                         int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                         int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                         const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                         int32_t n_bad, int32_t n_bad_ids, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                         const uint64_t* seed, float* probs_out, int64_t ld_probs, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_sampler_rows(c, step, temperature, top_k, top_p, seed, probs_out, ld_probs);
  return pick_call(c, stream);
}

int aki_sample_pick_rows_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                     uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                     int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                     int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                     int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                     const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                     int32_t n_bad, int32_t n_bad_ids, int32_t step, const float* temperature, const int32_t* top_k,
                                     const float* top_p, const uint64_t* seed, float* probs_out, int64_t ld_probs, const int16_t* table,
                                     int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base,
                                     const int32_t* row_states, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_sampler_rows(c, step, temperature, top_k, top_p, seed, probs_out, ld_probs);
  pick_constraint(c, CON_ROWS, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  return pick_call(c, stream);
}

int aki_sample_pick_constrained(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                                uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                                int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                                int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                                int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                                const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                                int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                                uint64_t offset, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_sampler(c, step, temperature, top_k, top_p, seed, offset, probs_out, ld_probs);
  pick_constraint(c, CON_WIDE, constraint(table, table_ld, n_states, states, states_ld), table_ld);
  return pick_call(c, stream);
}

int aki_greedy_pick_rows(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                         uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                         int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                         int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets,
                         int32_t n_sets, const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                         int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                         const int32_t* row_base, const int32_t* row_states, void* stream) {
  PickCall c = pick_processed_rows(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len,
                                   advance, done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores,
                                   ld_scores, sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  pick_constraint(c, CON_ROWS_OR_NONE, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  return pick_call(c, stream);
}

int aki_sample_pick_rows_processed(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                                   const uint64_t* seed, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                   void* stream) {
  PickCall c = pick_processed_rows(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len,
                                   advance, done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores,
                                   ld_scores, sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  pick_sampler_rows(c, step, temperature, top_k, top_p, seed, probs_out, ld_probs);
  pick_constraint(c, CON_ROWS_OR_NONE, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  return pick_call(c, stream);
}

// ---- the penalised forms: min_p and the frequency / presence penalties as nullable per-row device arrays of B floats, beside the
// arguments of the forms above.  A NULL table is "no constraint", so one entry point serves the constrained and the plain call.
int aki_greedy_pick_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                              int32_t states_ld, const float* frequency_penalty, const float* presence_penalty, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_constraint(c, CON_WIDE_OR_NONE, constraint(table, table_ld, n_states, states, states_ld), table_ld);
  c.q.freq = frequency_penalty; c.q.pres = presence_penalty;
  return pick_call(c, stream);
}

int aki_sample_pick_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                              uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld, int32_t* cache_len, const int32_t* start_len,
                              int32_t advance, int32_t* done_at, const void* embed_weight, const void* additional_weight, int64_t max_original_id,
                              int64_t num_additional, int32_t d, void* next_embeds, float* scores, int64_t ld_scores, float repetition_penalty,
                              int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* suppress_ids, int32_t n_suppress,
                              const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids, const int32_t* bad_offsets,
                              int32_t n_bad, int32_t n_bad_ids, int32_t step, float temperature, int32_t top_k, float top_p, uint64_t seed,
                              uint64_t offset, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld, int32_t n_states,
                              int32_t* states, int32_t states_ld, const float* frequency_penalty, const float* presence_penalty,
                              const float* min_p, void* stream) {
  PickCall c = pick_processed(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len, advance,
                              done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores, ld_scores,
                              repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids,
                              n_begin_suppress, bad_ids, bad_offsets, n_bad, n_bad_ids);
  pick_sampler(c, step, temperature, top_k, top_p, seed, offset, probs_out, ld_probs);
  pick_constraint(c, CON_WIDE_OR_NONE, constraint(table, table_ld, n_states, states, states_ld), table_ld);
  c.q.freq = frequency_penalty; c.q.pres = presence_penalty; c.sp.min_p = min_p;
  return pick_call(c, stream);
}

int aki_greedy_pick_rows_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states,
                                   int32_t states_ld, const int32_t* row_base, const int32_t* row_states, const float* frequency_penalty,
                                   const float* presence_penalty, void* stream) {
  PickCall c = pick_processed_rows(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len,
                                   advance, done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores,
                                   ld_scores, sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  pick_constraint(c, CON_ROWS_OR_NONE, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  c.q.freq = frequency_penalty; c.q.pres = presence_penalty;
  return pick_call(c, stream);
}

int aki_sample_pick_rows_penalized(const void* logits, int32_t B, int32_t V, int64_t ld, const int64_t* eos_ids, int32_t n_eos,
                                   int64_t pad_token_id, uint8_t* done, int64_t* next_ids, int64_t* tokens, int32_t tokens_ld,
                                   int32_t* cache_len, const int32_t* start_len, int32_t advance, int32_t* done_at, const void* embed_weight,
                                   const void* additional_weight, int64_t max_original_id, int64_t num_additional, int32_t d,
                                   void* next_embeds, float* scores, int64_t ld_scores, const int32_t* sets, int32_t n_sets,
                                   const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets,
                                   int32_t n_words, int32_t step, const float* temperature, const int32_t* top_k, const float* top_p,
                                   const uint64_t* seed, float* probs_out, int64_t ld_probs, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                   const float* frequency_penalty, const float* presence_penalty, const float* min_p, void* stream) {
  PickCall c = pick_processed_rows(logits, B, V, ld, eos_ids, n_eos, pad_token_id, done, next_ids, tokens, tokens_ld, cache_len, start_len,
                                   advance, done_at, embed_weight, additional_weight, max_original_id, num_additional, d, next_embeds, scores,
                                   ld_scores, sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  pick_sampler_rows(c, step, temperature, top_k, top_p, seed, probs_out, ld_probs);
  pick_constraint(c, CON_ROWS_OR_NONE, constraint(table, table_ld, n_states, states, states_ld, row_base, row_states), table_ld);
  c.q.freq = frequency_penalty; c.q.pres = presence_penalty; c.sr.min_p = min_p;
  return pick_call(c, stream);
}

// aki_logits_process*: q as proc_common / proc_values filled it, ps the per-row sets or nullptr; ld / ld_out / table_ld as the caller passed them
static int logits_process_call(const ProcParams& q, const ProcSetParams* ps, int32_t B, int64_t ld, int64_t ld_out, int32_t dtype, int kind,
                               int64_t table_ld, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(q.in && q.out && B > 0 && q.V > 0 && ld >= q.V && ld < (1ll << 31) && ld_out >= q.V && ld_out < (1ll << 31) && q.step >= 0);
  AKI_CHECK_ARG((!q.tokens || q.tokens_ld > 0) && q.n_eos >= 0 && (q.n_eos == 0 || q.eos));
  AKI_CHECK_ARG(ps ? processor_sets_ok(q.V, *ps) : processors_ok(q));
  AKI_CHECK_ARG(constraint_ok(kind, q.V, q.c, table_ld));
  if (dtype != AKI_DT_BF16 && dtype != AKI_DT_F32) return AKI_ERR_UNSUPPORTED;
  return logits_process_call_launch(q, ps, B, (hipStream_t)stream);
}

int aki_logits_process(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out, const int64_t* tokens,
                       int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step, const uint8_t* done,
                       float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length, const int64_t* eos_ids, int32_t n_eos,
                       const int64_t* suppress_ids, int32_t n_suppress, const int64_t* begin_suppress_ids, int32_t n_begin_suppress,
                       const int64_t* bad_ids, const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, void* stream) {
  ProcParams q = proc_common(logits, dtype == AKI_DT_F32, ld, out, ld_out, V, tokens, tokens_ld, cache_len, start_len, step, done, eos_ids, n_eos);
  proc_values(q, repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_ids,
              bad_offsets, n_bad, n_bad_ids);
  return logits_process_call(q, nullptr, B, ld, ld_out, dtype, CON_NONE, 0, stream);
}

int aki_logits_process_constrained(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                   const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                                   const uint8_t* done, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length,
                                   const int64_t* eos_ids, int32_t n_eos, const int64_t* suppress_ids, int32_t n_suppress,
                                   const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                   const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld,
                                   int32_t n_states, int32_t* states, int32_t states_ld, void* stream) {
  ProcParams q = proc_common(logits, dtype == AKI_DT_F32, ld, out, ld_out, V, tokens, tokens_ld, cache_len, start_len, step, done, eos_ids, n_eos);
  proc_values(q, repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_ids,
              bad_offsets, n_bad, n_bad_ids);
  q.c = constraint(table, table_ld, n_states, states, states_ld);
  return logits_process_call(q, nullptr, B, ld, ld_out, dtype, CON_WIDE, table_ld, stream);
}

int aki_logits_process_rows(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                            const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                            const uint8_t* done, const int64_t* eos_ids, int32_t n_eos, const int32_t* sets, int32_t n_sets,
                            const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids, const int32_t* bad_offsets, int32_t n_words,
                            const int16_t* table, int64_t table_ld, int32_t n_states, int32_t* states, int32_t states_ld,
                            const int32_t* row_base, const int32_t* row_states, void* stream) {
  ProcParams q = proc_common(logits, dtype == AKI_DT_F32, ld, out, ld_out, V, tokens, tokens_ld, cache_len, start_len, step, done, eos_ids, n_eos);
  q.c = constraint(table, table_ld, n_states, states, states_ld, row_base, row_states);
  const ProcSetParams ps = proc_sets(sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  return logits_process_call(q, &ps, B, ld, ld_out, dtype, CON_ROWS_OR_NONE, table_ld, stream);
}

int aki_logits_process_penalized(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                 const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step,
                                 const uint8_t* done, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length,
                                 const int64_t* eos_ids, int32_t n_eos, const int64_t* suppress_ids, int32_t n_suppress,
                                 const int64_t* begin_suppress_ids, int32_t n_begin_suppress, const int64_t* bad_ids,
                                 const int32_t* bad_offsets, int32_t n_bad, int32_t n_bad_ids, const int16_t* table, int64_t table_ld,
                                 int32_t n_states, int32_t* states, int32_t states_ld, const float* frequency_penalty,
                                 const float* presence_penalty, void* stream) {
  ProcParams q = proc_common(logits, dtype == AKI_DT_F32, ld, out, ld_out, V, tokens, tokens_ld, cache_len, start_len, step, done, eos_ids, n_eos);
  proc_values(q, repetition_penalty, no_repeat_ngram_size, min_length, suppress_ids, n_suppress, begin_suppress_ids, n_begin_suppress, bad_ids,
              bad_offsets, n_bad, n_bad_ids);
  q.c = constraint(table, table_ld, n_states, states, states_ld);
  q.freq = frequency_penalty; q.pres = presence_penalty;
  return logits_process_call(q, nullptr, B, ld, ld_out, dtype, CON_WIDE_OR_NONE, table_ld, stream);
}

int aki_logits_process_rows_penalized(const void* logits, int32_t dtype, int32_t B, int32_t V, int64_t ld, float* out, int64_t ld_out,
                                      const int64_t* tokens, int32_t tokens_ld, const int32_t* cache_len, const int32_t* start_len,
                                      int32_t step, const uint8_t* done, const int64_t* eos_ids, int32_t n_eos, const int32_t* sets,
                                      int32_t n_sets, const int32_t* row_set, const int64_t* set_ids, int32_t n_set_ids,
                                      const int32_t* bad_offsets, int32_t n_words, const int16_t* table, int64_t table_ld, int32_t n_states,
                                      int32_t* states, int32_t states_ld, const int32_t* row_base, const int32_t* row_states,
                                      const float* frequency_penalty, const float* presence_penalty, void* stream) {
  ProcParams q = proc_common(logits, dtype == AKI_DT_F32, ld, out, ld_out, V, tokens, tokens_ld, cache_len, start_len, step, done, eos_ids, n_eos);
  q.c = constraint(table, table_ld, n_states, states, states_ld, row_base, row_states);
  q.freq = frequency_penalty; q.pres = presence_penalty;
  const ProcSetParams ps = proc_sets(sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words);
  return logits_process_call(q, &ps, B, ld, ld_out, dtype, CON_ROWS_OR_NONE, table_ld, stream);
}

int aki_beam_logprob(const void* logits, int32_t dtype, int32_t rows, int32_t V, int64_t ld, float* out, int64_t ld_out, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(logits && out && rows > 0 && V > 0 && ld >= V && ld < (1ll << 31) && ld_out >= V && ld_out < (1ll << 31));
  if (dtype != AKI_DT_BF16 && dtype != AKI_DT_F32) return AKI_ERR_UNSUPPORTED;
  return beam_logprob_launch(logits, dtype == AKI_DT_F32, rows, V, (int)ld, out, (int)ld_out, (hipStream_t)stream);
}

int aki_beam_step(const float* logp, int64_t ld, int32_t B, int32_t K, int32_t V, int32_t t, int32_t max_new, float* beam_scores,
                  const int64_t* seqs_in, int64_t* seqs_out, float* hyp_score, int32_t* hyp_len, int64_t* hyp_tokens, int32_t* hyp_count,
                  uint8_t* done, int64_t* next_ids, int32_t* parent, const int64_t* eos_ids, int32_t n_eos, int64_t pad_token_id,
                  float length_penalty, int32_t early_stopping, int32_t last, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(logp && beam_scores && seqs_out && hyp_score && hyp_len && hyp_tokens && hyp_count && done && next_ids && parent);
  AKI_CHECK_ARG(B > 0 && V >= 2 && ld >= V && ld < (1ll << 31) && t >= 0 && t < max_new && (t == 0 || seqs_in) && seqs_in != seqs_out);
  AKI_CHECK_ARG(n_eos >= 0 && (n_eos == 0 || eos_ids) && length_penalty == length_penalty);
  if (K < 1 || K > AKI_BEAM_MAX_K || n_eos > AKI_BEAM_MAX_EOS || (int64_t)K * V >= (1ll << 31)) return AKI_ERR_UNSUPPORTED;
  return beam_step_launch(logp, (int)ld, B, K, V, t, max_new, beam_scores, seqs_in, seqs_out, hyp_score, hyp_len, hyp_tokens, hyp_count, done,
                          next_ids, parent, eos_ids, n_eos, pad_token_id, length_penalty, early_stopping, last ? 1 : 0, (hipStream_t)stream);
}

int aki_kv_beam_reorder(void* const* table, int32_t n_tensors, const int32_t* parent, const int32_t* start_len, const int32_t* cache_len,
                        int32_t B, int32_t K, int32_t H, int32_t capacity, int32_t row_bytes, int32_t pos_lo, int32_t pos_hi, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(table && parent && start_len && cache_len && n_tensors > 0 && B > 0 && H > 0 && capacity > 0 && row_bytes > 0);
  AKI_CHECK_ARG(pos_lo >= 0 && pos_lo <= pos_hi && pos_hi <= capacity);
  if (K < 1 || K > AKI_BEAM_MAX_K || row_bytes % 4 != 0 || H > 65535 || (int64_t)n_tensors * B > 65535) return AKI_ERR_UNSUPPORTED;
  return kv_beam_reorder_launch(table, n_tensors, parent, start_len, cache_len, B, K, H, capacity, row_bytes, pos_lo, pos_hi,
                                (hipStream_t)stream);
}

int aki_token_logprob(const void* logits, int32_t dtype, int32_t rows, int32_t V, int64_t ld, const int64_t* ids, const int64_t* tokens,
                      int64_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, int32_t step, const uint8_t* skip,
                      const int32_t* done_at, int32_t top_k, float* out_logprob, int64_t* out_top_ids, float* out_top_logprobs,
                      int64_t out_ld, int32_t out_cols, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(logits && out_logprob && (ids || tokens) && (cache_len != nullptr) == (start_len != nullptr));
  AKI_CHECK_ARG(rows > 0 && V > 0 && ld >= V && ld < (1ll << 31) && step >= 0 && out_cols > 0 && out_ld >= out_cols && out_ld < (1ll << 31));
  AKI_CHECK_ARG(!tokens || (tokens_ld > 0 && tokens_ld < (1ll << 31)));
  if ((dtype != AKI_DT_BF16 && dtype != AKI_DT_F32) || top_k < 0 || top_k > AKI_LOGPROB_MAX_TOP || V > AKI_LOGPROB_MAX_V) return AKI_ERR_UNSUPPORTED;
  AKI_CHECK_ARG(top_k == 0 || (out_top_ids && out_top_logprobs));
  return token_logprob_launch(logits, dtype == AKI_DT_F32, rows, V, (int)ld, ids, tokens, tokens ? (int)tokens_ld : 0, cache_len, start_len,
                              step, skip, done_at, top_k, out_logprob, out_top_ids, out_top_logprobs, (int)out_ld, out_cols,
                              (hipStream_t)stream);
}

int aki_kv_slot_admit(void* const* table, int32_t n_tensors, const int32_t* src_len, int32_t H, int32_t cap_src, int32_t cap_dst, int32_t B,
                      int32_t slot, int32_t row_bytes, int32_t vec_bytes, int32_t host_len, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(table && src_len && n_tensors > 0 && H > 0 && cap_src > 0 && cap_dst > 0 && B > 0 && row_bytes > 0);
  AKI_CHECK_ARG(slot >= 0 && slot < B && host_len >= 0 && host_len <= cap_src && host_len <= cap_dst);
  if ((vec_bytes != 4 && vec_bytes != 16) || row_bytes % vec_bytes != 0 || H > 65535 || n_tensors > 65535) return AKI_ERR_UNSUPPORTED;
  if ((int64_t)host_len * (row_bytes / vec_bytes) >= (1ll << 40)) return AKI_ERR_UNSUPPORTED;      // the grid's x extent stays below 2^30
  if (host_len == 0) return AKI_OK;
  return kv_slot_admit_launch(table, n_tensors, src_len, H, cap_src, cap_dst, slot, row_bytes, vec_bytes, host_len, (hipStream_t)stream);
}

int aki_slot_tick(uint8_t* done, int32_t* done_at, int32_t* cache_len, const int32_t* start_len, const int32_t* limit, int32_t B, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(done && done_at && cache_len && start_len && limit && B > 0);
  if (B > AKI_SLOT_MAX_ROWS) return AKI_ERR_UNSUPPORTED;
  return slot_tick_launch(done, done_at, cache_len, start_len, limit, B, (hipStream_t)stream);
}

// the pool of stop sequences: ids may be null only when it is empty; the device checks every offset against these counts
static bool stop_pool_ok(const int32_t* ids, int32_t n_ids, const int32_t* seq_off, int32_t n_seqs, const int32_t* set_first, int32_t n_sets,
                         const int32_t* row_set) {
  return n_ids >= 0 && n_seqs >= 0 && n_sets >= 0 && (ids || n_ids == 0) && seq_off && set_first && row_set;
}

int aki_stop_check(const int64_t* tokens, int64_t tokens_ld, const int32_t* cache_len, const int32_t* start_len, uint8_t* done,
                   int32_t* done_at, int32_t* stop_hit, const int32_t* ids, int32_t n_ids, const int32_t* seq_off, int32_t n_seqs,
                   const int32_t* set_first, int32_t n_sets, const int32_t* row_set, int32_t B, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(tokens && cache_len && start_len && done && done_at && stop_hit && B > 0 && tokens_ld > 0 && tokens_ld < (1ll << 31));
  AKI_CHECK_ARG(stop_pool_ok(ids, n_ids, seq_off, n_seqs, set_first, n_sets, row_set));
  return stop_check_launch(tokens, (int)tokens_ld, cache_len, start_len, done, done_at, stop_hit, ids, n_ids, seq_off, n_seqs, set_first,
                           n_sets, row_set, B, (hipStream_t)stream);
}

int aki_slot_tick_stops(uint8_t* done, int32_t* done_at, int32_t* cache_len, const int32_t* start_len, const int32_t* limit,
                        const int64_t* tokens, int64_t tokens_ld, int32_t* stop_hit, const int32_t* ids, int32_t n_ids,
                        const int32_t* seq_off, int32_t n_seqs, const int32_t* set_first, int32_t n_sets, const int32_t* row_set, int32_t B,
                        void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(done && done_at && cache_len && start_len && limit && tokens && stop_hit && B > 0 && tokens_ld > 0 && tokens_ld < (1ll << 31));
  AKI_CHECK_ARG(stop_pool_ok(ids, n_ids, seq_off, n_seqs, set_first, n_sets, row_set));
  if (B > AKI_SLOT_MAX_ROWS) return AKI_ERR_UNSUPPORTED;
  return slot_tick_stops_launch(done, done_at, cache_len, start_len, limit, tokens, (int)tokens_ld, stop_hit, ids, n_ids, seq_off, n_seqs,
                                set_first, n_sets, row_set, B, (hipStream_t)stream);
}

size_t aki_mma_mask_to_table_workspace_bytes(int32_t B, int32_t L) {
  return (B > 0 && L > 0) ? aki_align_up(mask_to_table_ws_bytes(B, L), 256) : 0;
}

int aki_mma_mask_to_table(const int64_t* mask, int32_t B, int32_t L, int32_t max_rects, aki_mma_rect* rects, uint64_t* col_valid_bits,
                          int32_t* seq_lens, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  AKI_CLEAR_ERR();
  AKI_CHECK_ARG(mask && rects && col_valid_bits && seq_lens && status && B > 0 && L > 0);
  AKI_CHECK_ARG(max_rects >= 1 && max_rects <= AKI_MAX_RECTS);
  if (!ws || ws_bytes < aki_mma_mask_to_table_workspace_bytes(B, L)) return AKI_ERR_WORKSPACE;
  AKI_CHECK_ALIGN16(ws);
  return mask_to_table_launch(mask, B, L, max_rects, rects, col_valid_bits, seq_lens, status, ws, (hipStream_t)stream);
}

}  // extern "C"

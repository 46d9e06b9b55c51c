// decode.hip - the token-by-token decode path after the MMA prefill.
//
// Replaces, for the generate() loop of the reference (src/aki.py:136-209 + src/aki_generation.py:36-86, HF
// GenerationMixin greedy decoding): per new token the 32 decoder layers run with M = batch rows (1..8).  That
// regime is HBM-bound (every weight is read once per token), so the kernels here stream weights at full width
// instead of using MFMA tiles:
//   gemv_bf16_kernel    y = act(x W^T + b) [+ residual] for M <= 8 rows: x lives in LDS, each wave owns 2 output
//                       features and sweeps W rows with coalesced 16-byte loads + v_dot2c_f32_bf16
//   rope_append_kernel  split the fused qkv row, rotate q/k at the token's position, append k/v to the KV cache
//   decode_attn_kernel  one query per (batch, head) against the cache: keys are spread over the 256 lanes, each
//                       lane keeps an online-softmax partial (m, l, acc[Dh]) that is merged through LDS
//   decode_attn_group_kernel  the fused split-KV step for N sampled rows per prompt over one shared copy of the prompt's K/V
//   decode_attn_split_fp8kv_kernel  the fused split-KV step on an opt-in e4m3 KV cache (one f32 scale per cached head row),
//                       with kv_cache_quant_fp8_kernel converting the prefill's bf16 rows into it
// After the prefill the reference switches to an all-ones 2-D mask (src/aki_generation.py:58-62), i.e. plain causal
// attention over everything cached; per-sample cache lengths and the prefill's valid-column bits are honoured here,
// which lifts the reference's batch-1 restriction.
#include <type_traits>

#include "aki_device.h"
#include "decode_attn_common.h"
#include "pick_params.h"

namespace aki {

struct GemvParams {
  const bf16_t* x; const bf16_t* w; const bf16_t* bias; const bf16_t* residual; bf16_t* y;
  const bf16_t* norm_w; float norm_eps;       // optional fused RMSNorm of the x rows (decode: the layer's pre-norm)
  int M, N, K, ldx, ldw, ldy, ldr, res_row_mod, act;
  const float* w_scale;                       // W8: w points at e4m3 bytes (ldw in bytes), one f32 scale per weight row
};

// U chunks (of 8 k) per lane for NR weight rows: every load is issued before the first dot product
template <int M, int NR, int U>
__device__ __forceinline__ void gemv_sweep(const bf16_t* const (&wr)[NR], const char* sx, int nchunk, int c, float (&acc)[NR][M]) {
  u32x4 w[U][NR];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < NR; ++r) w[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)(c + 64 * u) * 8));
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const u32x4 xv = *(const u32x4*)(sx + ((size_t)m * nchunk + c + 64 * u) * 16);
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r][m] = dot8_bf16(w[u][r], xv, acc[r][m]);
    }
}

// The two halves of a sweep, for the FIRST sweep of a single-row launch: its loads go out before x is staged (weights do not depend on
// the activation - the staging's round trips and the fused RMSNorm then run under the first weight round trip instead of in front of it).
template <int NR, int U>
__device__ __forceinline__ void gemv_issue(const bf16_t* const (&wr)[NR], int c, u32x4 (&w)[U][NR]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < NR; ++r) w[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)(c + 64 * u) * 8));
}
template <int NR, int U>
__device__ __forceinline__ void gemv_consume(const u32x4 (&w)[U][NR], const char* sx, int c, float (&acc)[NR][1]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const u32x4 xv = *(const u32x4*)(sx + ((size_t)c + 64 * u) * 16);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r][0] = dot8_bf16(w[u][r], xv, acc[r][0]);
  }
}

// weight-only fp8 (e4m3 weights, bf16 activations); the dot product is dot16_w8 (weight_dot.h)
template <int NR, int U>
__device__ __forceinline__ void gemv_issue_w8(const uint8_t* const (&wr)[NR], int c, u32x4 (&w)[U][NR]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < NR; ++r) w[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)(c + 64 * u) * 16));
}
template <int NR, int U>
__device__ __forceinline__ void gemv_consume_w8(const u32x4 (&w)[U][NR], const char* sx, int c, float (&acc)[NR][1]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const u32x4 x0 = *(const u32x4*)(sx + ((size_t)2 * (c + 64 * u)) * 16);
    const u32x4 x1 = *(const u32x4*)(sx + ((size_t)2 * (c + 64 * u) + 1) * 16);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r][0] = dot16_w8(w[u][r], x0, x1, acc[r][0]);
  }
}

template <int M, int NR, int U>
__device__ __forceinline__ void gemv_sweep_w8(const uint8_t* const (&wr)[NR], const char* sx, int nchunk_x, int c, float (&acc)[NR][M]) {
  u32x4 w[U][NR];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < NR; ++r) w[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)(c + 64 * u) * 16));
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const u32x4 x0 = *(const u32x4*)(sx + ((size_t)m * nchunk_x + 2 * (c + 64 * u)) * 16);
      const u32x4 x1 = *(const u32x4*)(sx + ((size_t)m * nchunk_x + 2 * (c + 64 * u) + 1) * 16);
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r][m] = dot16_w8(w[u][r], x0, x1, acc[r][m]);
    }
}

// FPW output features per wave; SWIGLU: feature f pairs weight rows f (gate) and N/2 + f (up).
// The K sweep is unrolled KU chunks deep with all weight loads issued before the dot products: a wave keeps
// NR*KU 16-byte loads in flight per lane, which is what decides the streaming rate at 4-6 waves per CU.
template <int M, bool SWIGLU, int FPW = 2, bool W8 = false>
__global__ __launch_bounds__(256) void gemv_bf16_kernel(const GemvParams p) {
  constexpr int NR = SWIGLU ? 2 * FPW : FPW;   // weight rows per wave
  constexpr int KU = NR <= 2 ? 8 : 4;          // up to 16 sixteen-byte loads in flight per lane
  extern __shared__ __attribute__((aligned(16))) char sx[];
  __shared__ float s_red[M][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = p.K / 8;
  // ---- single row: the first sweep of this workgroup's first feature group is requested BEFORE x is staged ------------------------
  constexpr int PU = W8 ? 2 : 4;                 // chunks per lane and row of that sweep (the ladder below continues behind it)
  u32x4 wpre[PU][NR];
  bool pre = false;
  if constexpr (M == 1 && !W8) {     // e4m3 weights: measured 2.3 % SLOWER with the early sweep (1.488 vs 1.454 ms per token, one box) - not used there
    const int n_out0 = SWIGLU ? p.N / 2 : p.N;
    const int f00 = (blockIdx.x * 4 + wave) * FPW;
    pre = f00 < n_out0 && (W8 ? p.K / 16 : nchunk) >= 64 * PU;
    if (pre) {
      if constexpr (W8) {
        const uint8_t* wr0[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int f = min(f00 + (r % FPW), n_out0 - 1);
          wr0[r] = (const uint8_t*)p.w + (size_t)((SWIGLU && r >= FPW) ? n_out0 + f : f) * p.ldw;
        }
        gemv_issue_w8<NR, PU>(wr0, lane, wpre);
      } else {
        const bf16_t* wr0[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int f = min(f00 + (r % FPW), n_out0 - 1);
          wr0[r] = p.w + (size_t)((SWIGLU && r >= FPW) ? n_out0 + f : f) * p.ldw;
        }
        gemv_issue<NR, PU>(wr0, lane, wpre);
      }
    }
  }
  if (p.norm_w == nullptr) {
    for (int i = tid; i < M * nchunk; i += 256) {
      const int m = i / nchunk, c = i - m * nchunk;
      *(u32x4*)(sx + (size_t)i * 16) = *(const u32x4*)(p.x + (size_t)m * p.ldx + c * 8);
    }
  } else {
    // y = bf16(x * rsqrt(mean(x^2) + eps) * w): same rounding points as norm_bf16_kernel<true> (aux_kernels.hip)
    float ss[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      ss[m] = 0.f;
      for (int c = tid; c < nchunk; c += 256) {
        const u32x4 v = *(const u32x4*)(p.x + (size_t)m * p.ldx + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
          ss[m] = __builtin_fmaf(lo, lo, ss[m]);
          ss[m] = __builtin_fmaf(hi, hi, ss[m]);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss[m] += __shfl_xor(ss[m], o);
      if (lane == 0) s_red[m][wave] = ss[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float r = rsqrtf((s_red[m][0] + s_red[m][1] + s_red[m][2] + s_red[m][3]) / (float)p.K + p.norm_eps);
      for (int c = tid; c < nchunk; c += 256) {
        const u32x4 v = *(const u32x4*)(p.x + (size_t)m * p.ldx + c * 8);
        const u32x4 g = *(const u32x4*)(p.norm_w + c * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // HF Phi3RMSNorm: weight * (x * rstd).to(bf16)
          o[e] = pack_bf16x2(round_bf16(bf16_lo(v[e]) * r) * bf16_lo(g[e]), round_bf16(bf16_hi(v[e]) * r) * bf16_hi(g[e]));
        }
        *(u32x4*)(sx + ((size_t)m * nchunk + c) * 16) = o;
      }
    }
  }
  __syncthreads();
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  // a workgroup owns feature groups blockIdx.x, blockIdx.x + gridDim.x, ...: the x rows staged above are reused
  for (int grp = blockIdx.x; grp * (4 * FPW) < n_out; grp += gridDim.x) {
    const int f0 = (grp * 4 + wave) * FPW;
    if (f0 >= n_out) break;
    float acc[NR][M];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
    float wsc[NR];
    if constexpr (W8) {
      const uint8_t* wr[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int f = min(f0 + (r % FPW), n_out - 1);
        const int row = (SWIGLU && r >= FPW) ? n_out + f : f;
        wr[r] = (const uint8_t*)p.w + (size_t)row * p.ldw;
        wsc[r] = p.w_scale[row];
      }
      const int nchunk_w = p.K / 16;                         // 16-byte weight chunks = 16 k-values each
      int c = lane;
      if constexpr (M == 1) {
        if (pre) { gemv_consume_w8<NR, PU>(wpre, sx, c, acc); c += 64 * PU; }
      }
      for (; c + 64 * 3 < nchunk_w; c += 64 * 4) gemv_sweep_w8<M, NR, 4>(wr, sx, nchunk, c, acc);
      for (; c + 64 < nchunk_w; c += 128) gemv_sweep_w8<M, NR, 2>(wr, sx, nchunk, c, acc);
      for (; c < nchunk_w; c += 64) gemv_sweep_w8<M, NR, 1>(wr, sx, nchunk, c, acc);
    } else {
      const bf16_t* wr[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int f = min(f0 + (r % FPW), n_out - 1);
        wr[r] = p.w + (size_t)((SWIGLU && r >= FPW) ? n_out + f : f) * p.ldw;
        wsc[r] = 1.f;
      }
      int c = lane;
      if constexpr (M == 1) {
        if (pre) { gemv_consume<NR, PU>(wpre, sx, c, acc); c += 64 * PU; }
      }
      for (; c + 64 * (KU - 1) < nchunk; c += 64 * KU) gemv_sweep<M, NR, KU>(wr, sx, nchunk, c, acc);
      if constexpr (KU > 4) {
        for (; c + 64 * 3 < nchunk; c += 64 * 4) gemv_sweep<M, NR, 4>(wr, sx, nchunk, c, acc);
      }
      for (; c + 64 < nchunk; c += 128) gemv_sweep<M, NR, 2>(wr, sx, nchunk, c, acc);
      for (; c < nchunk; c += 64) gemv_sweep<M, NR, 1>(wr, sx, nchunk, c, acc);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float v = acc[r][m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        acc[r][m] = W8 ? v * wsc[r] : v;
      }
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < FPW; ++f) {
        const int n = f0 + f;
        if (n >= n_out) continue;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          float v;
          if (SWIGLU) {
            v = acc[FPW + f][m] * silu_fast(acc[f][m]);
          } else {
            v = acc[f][m];
            if (p.bias) v += bf16_bits_to_f32(p.bias[n]);
            if (p.act == AKI_ACT_GELU_ERF) v = gelu_erf_fast(v);
            else if (p.act == AKI_ACT_GELU_TANH) v = gelu_tanh_fast(v);
          }
          if (p.residual) v += bf16_bits_to_f32(p.residual[(size_t)(p.res_row_mod > 0 ? m % p.res_row_mod : m) * p.ldr + n]);
          ((__bf16*)p.y)[(size_t)m * p.ldy + n] = (__bf16)v;
        }
      }
    }
    if constexpr (M == 1) break;      // single row: the launcher gives every workgroup exactly one feature group (and the pre-issued sweep is its)
  }
}

#ifdef AKI_LAB_HOOKS
// Route log of the decode linears (tests/decode_linear_cases.py): one record of nine int32 per launch decision, so that a test can see which
// instantiation the planner chose -
//   {0, M, SWIGLU, FPW, W8, norm, grid, feature groups per workgroup, dynamic LDS bytes}      gemv_bf16_kernel
//   {1, KS, SWIGLU, FT, NORM, norm, grid, 0, dynamic LDS bytes}                               skinny_gemm_bf16_kernel
//   {2, KS, SWIGLU, 1, NORM, norm, grid, 0, dynamic LDS bytes}                                skinny_gemm_w8_kernel
// (norm: a gain pointer was handed over).  g_decode_dry_run (aki_lab_set_decode_dry_run): record and return before any HIP call, so that the
// planner runs on a machine without a GPU.  A shape that falls through to the MFMA GEMM shows in that GEMM's own log (gemm_bf16.hip).
constexpr int kDecodeLogFields = 9, kDecodeLogCap = 256;
static int g_decode_log[kDecodeLogCap][kDecodeLogFields];
static int g_decode_log_n = 0;
int g_decode_dry_run = 0;
void decode_log_reset() { g_decode_log_n = 0; }
int decode_log_copy(int* out, int cap) {   // records copied: min(count, cap, kDecodeLogCap); returns the number of launches since the reset
  const int n = g_decode_log_n < kDecodeLogCap ? g_decode_log_n : kDecodeLogCap;
  for (int i = 0; out && i < n && i < cap; ++i)
    for (int j = 0; j < kDecodeLogFields; ++j) out[i * kDecodeLogFields + j] = g_decode_log[i][j];
  return g_decode_log_n;
}
static void decode_log_push(const int (&r)[kDecodeLogFields]) {
  if (g_decode_log_n < kDecodeLogCap)
    for (int j = 0; j < kDecodeLogFields; ++j) g_decode_log[g_decode_log_n][j] = r[j];
  ++g_decode_log_n;
}
#endif

template <int M, bool SWIGLU, int FPW, bool W8 = false>
static int launch_gemv_cfg(const GemvParams& p, int n_out, hipStream_t stream) {
  const size_t smem = (size_t)M * p.K * 2;
  // one group = 4 waves x FPW features.  Staging x costs M*K*2 bytes per workgroup against 4*FPW*K*2 bytes of weights per
  // group, so for M > 1 a workgroup takes several groups (at most ~512 workgroups stay in flight).
  const int groups = (n_out + 4 * FPW - 1) / (4 * FPW);
  const int per = M == 1 ? 1 : (groups + 511) / 512;
  const dim3 grid((groups + per - 1) / per), block(256);
#ifdef AKI_LAB_HOOKS
  decode_log_push({0, M, SWIGLU ? 1 : 0, FPW, W8 ? 1 : 0, p.norm_w ? 1 : 0, (int)grid.x, per, (int)smem});
  if (g_decode_dry_run) return AKI_OK;
#endif
  static bool set = false;
  if (!set) {
    if (hipFuncSetAttribute((const void*)gemv_bf16_kernel<M, SWIGLU, FPW, W8>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 8192 * 2) != hipSuccess)
      return AKI_ERR_LAUNCH;
    set = true;
  }
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL((gemv_bf16_kernel<M, SWIGLU, FPW, W8>), grid, block, smem, stream, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

template <int M>
static int launch_gemv(const GemvParams& p, hipStream_t stream) {
  const int n_out = p.act == AKI_ACT_SWIGLU ? p.N / 2 : p.N;
  if (p.w_scale) {                       // weight-only fp8: single-sequence decode in the fp8 configuration
    if constexpr (M == 1) {
      if (p.act == AKI_ACT_SWIGLU) return launch_gemv_cfg<1, true, 2, true>(p, n_out, stream);
      return launch_gemv_cfg<1, false, 2, true>(p, n_out, stream);
    } else {
      return AKI_ERR_UNSUPPORTED;
    }
  }
  if (p.act == AKI_ACT_SWIGLU) return launch_gemv_cfg<M, true, 2>(p, n_out, stream);
  // wide outputs (qkv, lm_head) have waves to spare: 4 features per wave doubles the loads each wave keeps in flight
  if constexpr (M <= 2) {      // (constexpr: the four-feature kernel is not instantiated for the row counts that never take it)
    if (n_out >= 8192) return launch_gemv_cfg<M, false, 4>(p, n_out, stream);
  }
  return launch_gemv_cfg<M, false, 2>(p, n_out, stream);
}

// ------------------------------------------------------------------------------------------------------------
// Skinny MFMA GEMM for 2 <= M <= 16 rows (batched decode): y[M][N] = act(x W^T + b) [+ residual].
// The dot-product GEMV above spends M FMAs and M LDS reads per weight element and stops being HBM-bound beyond M ~ 2;
// here the tokens ride on the 16 columns of v_mfma_f32_16x16x32_bf16 instead.  One workgroup = one 16-feature tile,
// its KS waves split K; every lane streams 32 contiguous bytes of ITS weight row per step (lane = (row l15, k-group kg):
// the four k-groups of a row read one full 128-byte line) straight from HBM into registers - no LDS staging, 16 loads in
// flight per lane - and the matching 32 bytes of x come from L2 (x is M*K*2 bytes, read by every tile).  The two MFMAs of
// a step take the first / second 16 bytes of both operands (any k order is fine as long as A and B agree).  Partial tiles
// of the KS waves meet in LDS; wave 0 runs the epilogue.  SWIGLU: the wave carries the gate tile and the up tile.
// ------------------------------------------------------------------------------------------------------------
// NORM (M <= 8, the decode step's pre-norms): the x rows are RMS-normalised on their way into LDS - wave w takes rows w, w + KS, ... whole, with
// the rounding points of norm_bf16_kernel<true> (HF Phi3RMSNorm: weight * (x * rstd).to(bf16)) - and the B fragments come from there instead of
// L2; the weight loads of the first steps are requested BEFORE that prologue, so it runs under their round trip.  It replaces a 4.9 us norm launch
// in front of the qkv and gate_up GEMMs of every layer of a batched decode step (65 of 231 launches, 9 % of the step at batch 8).
template <int KS, bool SWIGLU, int FT, bool NORM = false>
__global__ __launch_bounds__(KS * 64) void skinny_gemm_bf16_kernel(const GemvParams p) {
  constexpr int NS = FT * (SWIGLU ? 2 : 1);          // weight streams per wave, all fed by one x fragment
  constexpr int UN = NS >= 4 ? 2 : (NS == 2 ? 4 : 8);   // steps of 64 k whose loads are issued together (<= 20 loads in flight)
  __shared__ float red_st[NORM ? 1 : KS][NS][256];
  extern __shared__ __attribute__((aligned(16))) char s_xn[];      // NORM: the normalised rows, (K * 2 + 16) bytes apart (the pad spreads the 16 rows over the banks)
  // NORM: the partial tiles meet in the rows' LDS once every wave is done with them - 49 KB per workgroup instead of 57: three workgroups per CU,
  // and the 576 of the qkv GEMM are resident at once (at two per CU the last 64 were a second round: + 3 us)
  float (*red)[NS][256] = NORM ? (float (*)[NS][256])s_xn : red_st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kg = lane >> 4;
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  const int f0 = blockIdx.x * 16 * FT;
  const int Kw = p.K / KS, kbeg = wave * Kw;
  const bf16_t* wp[NS];
#pragma unroll
  for (int t = 0; t < FT; ++t) {
    const int frow = min(f0 + 16 * t + l15, n_out - 1);
    wp[t] = p.w + (size_t)frow * p.ldw + kbeg + 16 * kg;
    if (SWIGLU) wp[FT + t] = p.w + (size_t)(n_out + frow) * p.ldw + kbeg + 16 * kg;
  }
  const int xrow = min(l15, p.M - 1);
  const bf16_t* xr = p.x + (size_t)xrow * p.ldx + kbeg + 16 * kg;
  const int xs_pitch = p.K * 2 + 16;
  const char* xs = s_xn + (size_t)xrow * xs_pitch + (size_t)(kbeg + 16 * kg) * 2;
  f32x4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nsteps = Kw / 64;
  int it = 0;
  auto load_w = [&](int step, u32x4 (&w2)[NS][2]) {
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      w2[t][0] = __builtin_nontemporal_load((const u32x4*)(wp[t] + (size_t)step * 64));
      w2[t][1] = __builtin_nontemporal_load((const u32x4*)(wp[t] + (size_t)step * 64 + 8));
    }
  };
  auto load_x = [&](int step, u32x4 (&x2)[2]) {
    if constexpr (NORM) {
      x2[0] = *(const u32x4*)(xs + (size_t)step * 128);
      x2[1] = *(const u32x4*)(xs + (size_t)step * 128 + 16);
    } else {
      x2[0] = *(const u32x4*)(xr + (size_t)step * 64);
      x2[1] = *(const u32x4*)(xr + (size_t)step * 64 + 8);
    }
  };
  auto mma_step = [&](const u32x4 (&w2)[NS][2], const u32x4 (&x2)[2]) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const bf16x8 xb = __builtin_bit_cast(bf16x8, x2[hh]);
#pragma unroll
      for (int t = 0; t < NS; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w2[t][hh]), xb, acc[t], 0, 0, 0);
    }
  };
  if constexpr (NORM) {
    constexpr int UP = NS >= 2 ? 3 : 4;               // steps whose weights are requested before the prologue (more cost registers: the 576 workgroups of qkv want three per CU = 84 VGPRs)
    u32x4 wpre[UP][NS][2];
    const bool pre = nsteps >= UP;
    if (pre) {
#pragma unroll
      for (int u = 0; u < UP; ++u) load_w(u, wpre[u]);
    }
    const int nchunk = p.K / 8;
    for (int m = wave; m < p.M; m += KS) {             // a wave normalises whole rows: no cross-wave reduction
      const bf16_t* xm = p.x + (size_t)m * p.ldx;
      char* dst = s_xn + (size_t)m * xs_pitch;
      float ss = 0.f;
      for (int c = lane; c < nchunk; c += 64) {
        const u32x4 v = *(const u32x4*)(xm + (size_t)c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
          ss = __builtin_fmaf(lo, lo, ss);
          ss = __builtin_fmaf(hi, hi, ss);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
      const float r = rsqrtf(ss / (float)p.K + p.norm_eps);
      for (int c = lane; c < nchunk; c += 64) {
        const u32x4 v = *(const u32x4*)(xm + (size_t)c * 8);            // second read: an L1 / L2 hit
        const u32x4 g = *(const u32x4*)(p.norm_w + (size_t)c * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = pack_bf16x2(round_bf16(bf16_lo(v[e]) * r) * bf16_lo(g[e]), round_bf16(bf16_hi(v[e]) * r) * bf16_hi(g[e]));
        *(u32x4*)(dst + (size_t)c * 16) = o;
      }
    }
    __syncthreads();
    if (pre) {
#pragma unroll
      for (int u = 0; u < UP; ++u) {
        u32x4 x2[2];
        load_x(u, x2);
        mma_step(wpre[u], x2);
      }
      it = UP;
    }
  }
  auto run = [&](auto un_c) {
    constexpr int U = decltype(un_c)::value;
    for (; it + U <= nsteps; it += U) {
      u32x4 wa[U][NS][2], xa[U][2];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        load_w(it + u, wa[u]);
        load_x(it + u, xa[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) mma_step(wa[u], xa[u]);
    }
  };
  run(std::integral_constant<int, UN>{});          // ladder: a wave's K slice can be shorter than the deepest unroll
  if constexpr (UN > 4) run(std::integral_constant<int, 4>{});
  if constexpr (UN > 2) run(std::integral_constant<int, 2>{});
  run(std::integral_constant<int, 1>{});
  // accumulator: lane (token = l15, features 4kg..4kg+3 of each tile); fold the KS partial tiles
  if (KS > 1) {
    if constexpr (NORM) __syncthreads();             // every wave has read its last fragment of the rows
#pragma unroll
    for (int t = 0; t < NS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][t][lane * 4 + r] = acc[t][r];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < KS; ++w)
#pragma unroll
      for (int t = 0; t < NS; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += red[w][t][lane * 4 + r];
  }
  const int tok = l15;
  if (tok >= p.M) return;
#pragma unroll
  for (int t = 0; t < FT; ++t) {
    const int f = f0 + 16 * t + 4 * kg;
    if (f >= n_out) continue;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (SWIGLU) {
        v[r] = acc[FT + t][r] * silu_fast(acc[t][r]);
      } else {
        v[r] = acc[t][r];
        if (p.bias) v[r] += bf16_bits_to_f32(p.bias[f + r]);
        if (p.act == AKI_ACT_GELU_ERF) v[r] = gelu_erf_fast(v[r]);
        else if (p.act == AKI_ACT_GELU_TANH) v[r] = gelu_tanh_fast(v[r]);
      }
      if (p.residual) v[r] += bf16_bits_to_f32(p.residual[(size_t)(p.res_row_mod > 0 ? tok % p.res_row_mod : tok) * p.ldr + f + r]);
    }
    *(u32x2*)(p.y + (size_t)tok * p.ldy + f) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  }
}

template <int KS, int FT, bool NORM = false>
static int launch_skinny(const GemvParams& p, hipStream_t stream) {
  const int n_out = p.act == AKI_ACT_SWIGLU ? p.N / 2 : p.N;
  const dim3 grid((n_out + 16 * FT - 1) / (16 * FT)), block(KS * 64);
  constexpr size_t RED = (size_t)KS * 2 * 1024;      // the partial tiles (two streams with SwiGLU) alias the rows
  const size_t rows = (size_t)p.M * ((size_t)p.K * 2 + 16);
  const size_t smem = NORM ? (rows > RED ? rows : RED) : 0;
#ifdef AKI_LAB_HOOKS
  decode_log_push({1, KS, p.act == AKI_ACT_SWIGLU ? 1 : 0, FT, NORM ? 1 : 0, p.norm_w ? 1 : 0, (int)grid.x, 0, (int)smem});
  if (g_decode_dry_run) return AKI_OK;
#endif
  if constexpr (NORM) {
    static bool set_s = false, set_p = false;
    bool& set = p.act == AKI_ACT_SWIGLU ? set_s : set_p;
    if (!set) {
      const void* fn = p.act == AKI_ACT_SWIGLU ? (const void*)skinny_gemm_bf16_kernel<KS, true, FT, true> : (const void*)skinny_gemm_bf16_kernel<KS, false, FT, true>;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (8192 * 2 + 16)) != hipSuccess) return AKI_ERR_LAUNCH;
      set = true;
    }
  }
  AKI_CLEAR_ERR();
  if (p.act == AKI_ACT_SWIGLU) hipLaunchKernelGGL((skinny_gemm_bf16_kernel<KS, true, FT, NORM>), grid, block, smem, stream, p);
  else hipLaunchKernelGGL((skinny_gemm_bf16_kernel<KS, false, FT, NORM>), grid, block, smem, stream, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// 2 <= M <= 16; n_out, ldy, ldr multiples of 4; K a multiple of 64 (per wave).  AKI_ERR_UNSUPPORTED otherwise.
// rms_w != NULL (M <= 8, K <= 8192): the x rows are RMS-normalised (weight rms_w [K], eps) inside the launch.
int skinny_gemm_bf16(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream) {
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  if (a->M < 2 || a->M > 16 || a->K % 64 || (a->ldx % 8) || (a->ldw % 8) || (n_out % 4) || (a->ldy % 4) || (a->residual && (a->ldr % 4)))
    return AKI_ERR_UNSUPPORTED;
  if (a->act == AKI_ACT_SWIGLU && (a->bias || (a->N & 1))) return AKI_ERR_UNSUPPORTED;
  if (rms_w && (a->M > 8 || a->K > 8192)) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)a->x & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->y & 7) || ((uintptr_t)a->bias & 7) || ((uintptr_t)rms_w & 15)) return AKI_ERR_ALIGNMENT;
  GemvParams p = {(const bf16_t*)a->x, (const bf16_t*)a->w, (const bf16_t*)a->bias, (const bf16_t*)a->residual, (bf16_t*)a->y,
                  (const bf16_t*)rms_w, eps, a->M, a->N, a->K, a->ldx, a->ldw, a->ldy, a->ldr, a->res_row_mod, a->act, nullptr};
  // One 16-feature tile per wave and a K split that keeps >= ~4 waves per CU.  (Two tiles per wave sharing the x fragment
  // were measured: fewer x loads, but the lost wave parallelism cost more - 3.85 vs 3.30 ms per step at batch 8.)
  const int tiles = (n_out + 15) / 16;
  if (rms_w) {
    // every workgroup normalises the M rows for itself: fine for the 512-1024 eight- or four-wave workgroups of qkv / gate_up, not for the 2004
    // two-wave ones of the lm_head (measured + 29 us at M = 8): wide outputs keep the norm launch (AKI_ERR_UNSUPPORTED: the caller's choice)
    if (tiles < 768 && a->K % 512 == 0) return launch_skinny<8, 1, true>(p, stream);
    if (tiles < 1536 && a->K % 256 == 0) return launch_skinny<4, 1, true>(p, stream);
    return AKI_ERR_UNSUPPORTED;
  }
  if (tiles < 768 && a->K % 512 == 0) return launch_skinny<8, 1>(p, stream);
  if (tiles < 1536 && a->K % 256 == 0) return launch_skinny<4, 1>(p, stream);
  if (a->K % 128 == 0) return launch_skinny<2, 1>(p, stream);
  return launch_skinny<1, 1>(p, stream);
}

// ------------------------------------------------------------------------------------------------------------
// The skinny GEMM on e4m3 weights (W8A16: one f32 scale per weight row, bf16 rows) for 2 <= M <= 16 - batched decode in the fp8
// configuration streams half the bytes.  Same tile and K split; a step is 128 k: lane (row l15, k-group kg) loads 32 bytes = 32 k of ITS
// weight row (the four k-groups read one 128-byte line), widens them pairwise to bf16 (v_cvt_scalef32_pk_bf16_fp8, exact) and feeds four
// MFMAs against the 64 bytes of x that carry the same k.  The row scale multiplies the finished sum, as in the one-row GEMV (gemv_bf16_kernel<W8>).
// NORM: as in skinny_gemm_bf16_kernel.
// ------------------------------------------------------------------------------------------------------------
template <int KS, bool SWIGLU, bool NORM>
__global__ __launch_bounds__(KS * 64) void skinny_gemm_w8_kernel(const GemvParams p) {
  constexpr int NS = SWIGLU ? 2 : 1;
  constexpr int UN = SWIGLU ? 2 : 4;                 // steps of 128 k whose loads are issued together
  __shared__ float red_st[NORM ? 1 : KS][NS][256];
  extern __shared__ __attribute__((aligned(16))) char s_xn[];
  float (*red)[NS][256] = NORM ? (float (*)[NS][256])s_xn : red_st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kg = lane >> 4;
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  const int f0 = blockIdx.x * 16;
  const int Kw = p.K / KS, kbeg = wave * Kw;
  const int frow = min(f0 + l15, n_out - 1);
  const uint8_t* wp[NS];
  wp[0] = (const uint8_t*)p.w + (size_t)frow * p.ldw + kbeg + 32 * kg;
  if (SWIGLU) wp[NS - 1] = (const uint8_t*)p.w + (size_t)(n_out + frow) * p.ldw + kbeg + 32 * kg;
  const int xrow = min(l15, p.M - 1);
  const bf16_t* xr = p.x + (size_t)xrow * p.ldx + kbeg + 32 * kg;
  const int xs_pitch = p.K * 2 + 16;
  const char* xs = s_xn + (size_t)xrow * xs_pitch + (size_t)(kbeg + 32 * kg) * 2;
  f32x4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nsteps = Kw / 128;
  if constexpr (NORM) {
    const int nchunk = p.K / 8;
    for (int m = wave; m < p.M; m += KS) {
      const bf16_t* xm = p.x + (size_t)m * p.ldx;
      char* dst = s_xn + (size_t)m * xs_pitch;
      float ss = 0.f;
      for (int c = lane; c < nchunk; c += 64) {
        const u32x4 v = *(const u32x4*)(xm + (size_t)c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
          ss = __builtin_fmaf(lo, lo, ss);
          ss = __builtin_fmaf(hi, hi, ss);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
      const float r = rsqrtf(ss / (float)p.K + p.norm_eps);
      for (int c = lane; c < nchunk; c += 64) {
        const u32x4 v = *(const u32x4*)(xm + (size_t)c * 8);
        const u32x4 g = *(const u32x4*)(p.norm_w + (size_t)c * 8);
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = pack_bf16x2(round_bf16(bf16_lo(v[e]) * r) * bf16_lo(g[e]), round_bf16(bf16_hi(v[e]) * r) * bf16_hi(g[e]));
        *(u32x4*)(dst + (size_t)c * 16) = o;
      }
    }
    __syncthreads();
  }
  int it = 0;
  auto run = [&](auto un_c) {
    constexpr int U = decltype(un_c)::value;
    for (; it + U <= nsteps; it += U) {
      u32x4 wa[U][NS][2], xa[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          wa[u][t][0] = __builtin_nontemporal_load((const u32x4*)(wp[t] + (size_t)(it + u) * 128));
          wa[u][t][1] = __builtin_nontemporal_load((const u32x4*)(wp[t] + (size_t)(it + u) * 128 + 16));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xa[u][j] = NORM ? *(const u32x4*)(xs + (size_t)(it + u) * 256 + 16 * j) : *(const u32x4*)(xr + (size_t)(it + u) * 128 + 8 * j);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // k-values 8j .. 8j+7 of the lane's 32: weight bytes 8j .. 8j+7 = dwords 2j, 2j+1 of the 32 bytes
          const bf16x8 xb = __builtin_bit_cast(bf16x8, xa[u][j]);
#pragma unroll
          for (int t = 0; t < NS; ++t) {
            const unsigned d0 = wa[u][t][j >> 1][(j & 1) * 2], d1 = wa[u][t][j >> 1][(j & 1) * 2 + 1];
            const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
            const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
            const u32x4 wq = u32x4{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2), __builtin_bit_cast(unsigned, p3)};
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq), xb, acc[t], 0, 0, 0);
          }
        }
    }
  };
  run(std::integral_constant<int, UN>{});
  if constexpr (UN > 2) run(std::integral_constant<int, 2>{});
  run(std::integral_constant<int, 1>{});
  if (KS > 1) {
    if constexpr (NORM) __syncthreads();
#pragma unroll
    for (int t = 0; t < NS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][t][lane * 4 + r] = acc[t][r];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < KS; ++w)
#pragma unroll
      for (int t = 0; t < NS; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += red[w][t][lane * 4 + r];
  }
  const int tok = l15, f = f0 + 4 * kg;
  if (tok >= p.M || f >= n_out) return;
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (SWIGLU) {
      v[r] = (acc[NS - 1][r] * p.w_scale[n_out + f + r]) * silu_fast(acc[0][r] * p.w_scale[f + r]);
    } else {
      v[r] = acc[0][r] * p.w_scale[f + r];
      if (p.bias) v[r] += bf16_bits_to_f32(p.bias[f + r]);
      if (p.act == AKI_ACT_GELU_ERF) v[r] = gelu_erf_fast(v[r]);
      else if (p.act == AKI_ACT_GELU_TANH) v[r] = gelu_tanh_fast(v[r]);
    }
    if (p.residual) v[r] += bf16_bits_to_f32(p.residual[(size_t)(p.res_row_mod > 0 ? tok % p.res_row_mod : tok) * p.ldr + f + r]);
  }
  *(u32x2*)(p.y + (size_t)tok * p.ldy + f) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

template <int KS, bool NORM>
static int launch_skinny_w8(const GemvParams& p, hipStream_t stream) {
  const int n_out = p.act == AKI_ACT_SWIGLU ? p.N / 2 : p.N;
  const dim3 grid((n_out + 15) / 16), block(KS * 64);
  constexpr size_t RED = (size_t)KS * 2 * 1024;
  const size_t rows = (size_t)p.M * ((size_t)p.K * 2 + 16);
  const size_t smem = NORM ? (rows > RED ? rows : RED) : 0;
#ifdef AKI_LAB_HOOKS
  decode_log_push({2, KS, p.act == AKI_ACT_SWIGLU ? 1 : 0, 1, NORM ? 1 : 0, p.norm_w ? 1 : 0, (int)grid.x, 0, (int)smem});
  if (g_decode_dry_run) return AKI_OK;
#endif
  if constexpr (NORM) {
    static bool set_s = false, set_p = false;
    bool& set = p.act == AKI_ACT_SWIGLU ? set_s : set_p;
    if (!set) {
      const void* fn = p.act == AKI_ACT_SWIGLU ? (const void*)skinny_gemm_w8_kernel<KS, true, true> : (const void*)skinny_gemm_w8_kernel<KS, false, true>;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (8192 * 2 + 16)) != hipSuccess) return AKI_ERR_LAUNCH;
      set = true;
    }
  }
  AKI_CLEAR_ERR();
  if (p.act == AKI_ACT_SWIGLU) hipLaunchKernelGGL((skinny_gemm_w8_kernel<KS, true, NORM>), grid, block, smem, stream, p);
  else hipLaunchKernelGGL((skinny_gemm_w8_kernel<KS, false, NORM>), grid, block, smem, stream, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// 2 <= M <= 16 rows on e4m3 weights; K a multiple of 128 per wave, rows of w 16-byte aligned.  AKI_ERR_UNSUPPORTED otherwise.
int skinny_gemm_w8(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream) {
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  if (a->M < 2 || a->M > 16 || !a->w_scale || (a->ldx % 8) || (a->ldw % 16) || (n_out % 4) || (a->ldy % 4) || (a->residual && (a->ldr % 4)))
    return AKI_ERR_UNSUPPORTED;
  if (a->act == AKI_ACT_SWIGLU && (a->bias || (a->N & 1))) return AKI_ERR_UNSUPPORTED;
  if (rms_w && (a->M > 8 || a->K > 8192)) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)a->x & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->y & 7) || ((uintptr_t)a->bias & 7) || ((uintptr_t)rms_w & 15)) return AKI_ERR_ALIGNMENT;
  GemvParams p = {(const bf16_t*)a->x, (const bf16_t*)a->w, (const bf16_t*)a->bias, (const bf16_t*)a->residual, (bf16_t*)a->y,
                  (const bf16_t*)rms_w, eps, a->M, a->N, a->K, a->ldx, a->ldw, a->ldy, a->ldr, a->res_row_mod, a->act, a->w_scale};
  const int tiles = (n_out + 15) / 16;
  // waves per tile: at least four steps of 128 k per wave, and enough waves per CU for the narrow outputs
  const bool k8 = a->K % 1024 == 0 && a->K / 8 >= 512, k4 = a->K % 512 == 0;
  if (rms_w) {
    if (tiles >= 1536) return AKI_ERR_UNSUPPORTED;      // lm_head-wide outputs keep the norm launch (see skinny_gemm_bf16)
    if (k8 && tiles < 768) return launch_skinny_w8<8, true>(p, stream);
    if (k4) return launch_skinny_w8<4, true>(p, stream);
    return AKI_ERR_UNSUPPORTED;
  }
  if (k8 && tiles < 768) return launch_skinny_w8<8, false>(p, stream);
  if (k4 && tiles < 1536) return launch_skinny_w8<4, false>(p, stream);
  if (a->K % 256 == 0) return launch_skinny_w8<2, false>(p, stream);
  return AKI_ERR_UNSUPPORTED;
}

// M <= 8 rows and M*K*2 <= 128 KiB of LDS; returns AKI_ERR_UNSUPPORTED otherwise (the caller then uses the MFMA GEMM).
// rms_w != NULL: the x rows are RMS-normalised (weight rms_w [K], eps) on the way into LDS.
int gemv_bf16(const aki_linear_args* a, const void* rms_w, float eps, hipStream_t stream) {
  const bool w8 = a->dtype == AKI_DT_W8A16;
  if (a->M > 8 || a->K % (w8 ? 16 : 8) || (size_t)a->M * a->K * 2 > 8 * 8192 * 2 || (a->ldx % 8) || (a->ldw % (w8 ? 16 : 8))) return AKI_ERR_UNSUPPORTED;
  if (a->act == AKI_ACT_SWIGLU && (a->bias || (a->N & 1))) return AKI_ERR_UNSUPPORTED;
  if (w8 && (!a->w_scale || a->M != 1)) return AKI_ERR_UNSUPPORTED;
  GemvParams p = {(const bf16_t*)a->x, (const bf16_t*)a->w, (const bf16_t*)a->bias, (const bf16_t*)a->residual, (bf16_t*)a->y,
                  (const bf16_t*)rms_w, eps, a->M, a->N, a->K, a->ldx, a->ldw, a->ldy, a->ldr, a->res_row_mod, a->act,
                  w8 ? a->w_scale : nullptr};
  switch (a->M) {
    case 1: return launch_gemv<1>(p, stream);
    case 2: return launch_gemv<2>(p, stream);
    case 3: return launch_gemv<3>(p, stream);
    case 4: return launch_gemv<4>(p, stream);
    case 5: return launch_gemv<5>(p, stream);
    case 6: return launch_gemv<6>(p, stream);
    case 7: return launch_gemv<7>(p, stream);
    default: return launch_gemv<8>(p, stream);
  }
}

// ------------------------------------------------------------------------------------------------------------
// RoPE + cache append for the new token of every sequence.
//   qkv [B, 3*H*Dh] (one row per sequence), cos/sin f32 [pos_rows, Dh], pos[b] = position of the new token,
//   q_out [B,H,Dh]; k/v cache [B,H,cap,Dh], written at index cache_len[b].
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void rope_append_kernel(const T* qkv, const float* cos, const float* sin, const int* pos, const int* cache_len,
                                   T* q_out, T* k_cache, T* v_cache, int H, int Dh, int cap) {
  const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;   // i over H*Dh
  if (i >= H * Dh) return;
  const int head = i / Dh, d = i - head * Dh, half = Dh / 2;
  const T* row = qkv + (size_t)b * 3 * H * Dh;
  const int ps = pos[b];
  const float c = cos[(size_t)ps * Dh + d], s = sin[(size_t)ps * Dh + d];
  const float q = (float)row[i], k = (float)row[H * Dh + i], v = (float)row[2 * H * Dh + i];
  const float qp = d < half ? -(float)row[i + half] : (float)row[i - half];
  const float kp = d < half ? -(float)row[H * Dh + i + half] : (float)row[H * Dh + i - half];
  q_out[(size_t)b * H * Dh + i] = (T)(q * c + qp * s);
  const size_t at = ((size_t)(b * H + head) * cap + cache_len[b]) * Dh + d;
  k_cache[at] = (T)(k * c + kp * s);
  v_cache[at] = (T)v;
}

// ------------------------------------------------------------------------------------------------------------
// Single-query attention over the cache.  One 256-thread block per (batch, head); lane t handles keys t, t+256, ...
// n_keys[b] = number of cached keys to attend to (including the token just appended);
// valid bits (optional, [B][nwords]) mask padded columns of the prefill.
// ------------------------------------------------------------------------------------------------------------
template <typename T, int DH>
__global__ __launch_bounds__(256) void decode_attn_kernel(const T* q, const T* kc, const T* vc, T* o, const int* n_keys,
                                                          const uint64_t* vbits, int nwords, int H, int cap, float scale) {
  __shared__ float s_m[256], s_l[256];
  __shared__ float s_acc[4][DH];
  const int bh = blockIdx.x, b = bh / H, tid = threadIdx.x;
  const int n = n_keys[b];
  float qv[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) qv[d] = (float)q[(size_t)bh * DH + d] * scale;
  float m = -INFINITY, l = 0.f, acc[DH];
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] = 0.f;
  const T* kb = kc + (size_t)bh * cap * DH;
  const T* vb = vc + (size_t)bh * cap * DH;
  for (int t = tid; t < n; t += 256) {
    if (vbits && (t >> 6) < nwords && !((vbits[(size_t)b * nwords + (t >> 6)] >> (t & 63)) & 1ull)) continue;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) s = __builtin_fmaf(qv[d], (float)kb[(size_t)t * DH + d], s);
    const float mn = fmaxf(m, s);
    const float a = __expf(m - mn), pr = __expf(s - mn);
    l = l * a + pr;
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] = __builtin_fmaf(pr, (float)vb[(size_t)t * DH + d], acc[d] * a);
    m = mn;
  }
  // merge the 256 partials: global max, rescale, sum
  s_m[tid] = m;
  __syncthreads();
  float gm = -INFINITY;
  for (int i = 0; i < 256; ++i) gm = fmaxf(gm, s_m[i]);
  const float f = (m == -INFINITY) ? 0.f : __expf(m - gm);
  l *= f;
#pragma unroll
  for (int d = 0; d < DH; ++d) acc[d] *= f;
  // wave-level reduction, then 4 waves through LDS
#pragma unroll
  for (int ofs = 32; ofs > 0; ofs >>= 1) {
    l += __shfl_xor(l, ofs);
#pragma unroll
    for (int d = 0; d < DH; ++d) acc[d] += __shfl_xor(acc[d], ofs);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) {
    s_l[wave] = l;
#pragma unroll
    for (int d = 0; d < DH; ++d) s_acc[wave][d] = acc[d];
  }
  __syncthreads();
  if (tid < DH) {
    float t[8] = {s_l[0], s_l[1], s_l[2], s_l[3], s_acc[0][tid], s_acc[1][tid], s_acc[2][tid], s_acc[3][tid]};
    lds_fold_ready(t);
    const float lt = t[0] + t[1] + t[2] + t[3];
    const float a = t[4] + t[5] + t[6] + t[7];
    o[(size_t)bh * DH + tid] = (T)(lt > 0.f ? a / lt : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------------------
// Split-KV single-query attention (bf16, Dh = 96), optionally fused with RoPE + cache append of the new token.
//
// With one query per (batch, head) there are only B*H independent rows, far too few to pull the cache at HBM rate
// from 256 CUs, so the keys of each row are split over S single-wave workgroups of T 64-key tiles each (split_plan;
// the item, the partial it leaves and the merge by the last arriver are decode_attn_common.h's).  The merger
// re-arms the row's counter, so the workspace needs zeroing only once.
// FUSED: q comes un-rotated inside the fused qkv row; every workgroup rotates q itself (96 values), the workgroup
// whose key range contains the new position also rotates k, appends k/v to the cache and uses them from LDS.
// ------------------------------------------------------------------------------------------------------------
struct DecodeAttnParams {
  const bf16_t* q;            // FUSED: qkv rows [B][3*H*96] (un-rotated); else rotated q [B][H*96]
  const float* cos; const float* sin;   // FUSED: [capacity][96]
  const int* len;             // FUSED: cache_len[b] (= position and append index; n_keys = len + 1); else n_keys[b]
  bf16_t* kc; bf16_t* vc;     // [B][H][cap][96]
  bf16_t* o;                  // [B][H*96]
  const uint64_t* vbits; int nwords;
  unsigned* cnt; float* part; // workspace: arrival counters [B*H], partials [B*H][S][DEC_PSTRIDE]
  int H, cap, S, T; float scale;
};

template <bool FUSED>
__global__ __launch_bounds__(64) void decode_attn_split_kernel(const DecodeAttnParams p) {
  __shared__ __attribute__((aligned(16))) bf16_t s_q[96], s_k[96], s_v[96];
  const int lane = threadIdx.x, split = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int ln = p.len[b];
  const int n = FUSED ? ln + 1 : ln;
  const int k_begin = split * p.T * 64;
  const int k_end = min(n, k_begin + p.T * 64);
  bf16_t* kb = p.kc + (size_t)bh * p.cap * 96;
  bf16_t* vb = p.vc + (size_t)bh * p.cap * 96;
  float* part = p.part + ((size_t)bh * p.S + split) * DEC_PSTRIDE;
  float m, l, acc[8];
  if constexpr (FUSED) {
    split_item_bf16<true, true>(kb, vb, ln, ln, k_begin, k_end, p.T, p.vbits, (size_t)b * p.nwords, p.nwords, p.q + (size_t)b * 3 * p.H * 96 + h * 96,
                                p.H, p.cos, p.sin, p.scale, lane, s_q, s_k, s_v, m, l, acc);
  } else {
    // The item on a rotated q and an appended cache.  Kept as its own text: on top of split_item_bf16 this instance took 226 VGPRs
    // for 224 (EXPERIMENTS.md has how to reproduce that); what it computes per tile is the shared item's loop without the new row.
    // The comments there hold here too: rows clamped to k_end - 1 carry probability 0, q is read from LDS where it is used and V is
    // widened row by row (either one held in registers made the kernel 272 VGPRs = one wave per SIMD).
    const int g = lane >> 4, i16 = lane & 15;
    m = -INFINITY;
    l = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (k_begin < k_end) {
      u32x4 kr[12], vr[16];
      auto issue_tile = [&](int base) {
        const bf16_t* krow = kb + (size_t)min(base + lane, k_end - 1) * 96;
#pragma unroll
        for (int i = 0; i < 12; ++i) kr[i] = *(const u32x4*)(krow + i * 8);
#pragma unroll
        for (int t2 = 0; t2 < 16; ++t2) {
          const int r = min(base + 4 * t2 + g, k_end - 1);
          vr[t2] = *(const u32x4*)(vb + (size_t)r * 96 + min(i16, 11) * 8);
        }
      };
      issue_tile(k_begin);
      if (lane < 12) *(u32x4*)(s_q + lane * 8) = *(const u32x4*)(p.q + (size_t)bh * 96 + lane * 8);
      __syncthreads();
      for (int t = 0; t < p.T; ++t) {
        const int base = k_begin + t * 64;
        if (base >= k_end) break;
        const int j = base + lane;
        if (t > 0) issue_tile(base);
        bool ok = j < k_end;
        if (p.vbits && (base >> 6) < p.nwords) ok = ok && ((p.vbits[(size_t)b * p.nwords + (base >> 6)] >> lane) & 1ull);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) s = dot8_bf16(kr[i], *(const u32x4*)(s_q + i * 8), s);
        s = ok ? s * p.scale : -INFINITY;
        const float mn = fmaxf(m, wave_max(s));
        if (mn == -INFINITY) continue;
        const float a = __expf(m - mn);
        const float pr = ok ? __expf(s - mn) : 0.f;
        l = l * a + wave_sum(pr);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= a;
#pragma unroll
        for (int t2 = 0; t2 < 16; ++t2) {
          const float w = __shfl(pr, 4 * t2 + g);
          u32x4 vt = vr[t2];
          asm volatile("" : "+v"(vt));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[2 * e] = __builtin_fmaf(w, bf16_lo(vt[e]), acc[2 * e]);
            acc[2 * e + 1] = __builtin_fmaf(w, bf16_hi(vt[e]), acc[2 * e + 1]);
          }
        }
        m = mn;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[e] += __shfl_xor(acc[e], 16);
        acc[e] += __shfl_xor(acc[e], 32);
      }
    }
  }
  split_publish(part, m, l, acc, lane);
  if (split_ticket(p.cnt + bh, lane) != (unsigned)(p.S - 1)) return;
  asm volatile("" ::: "memory");
  // ---- last workgroup of this (batch, head) merges the partials
  __shared__ float s_mg[DEC_MERGE_FLOATS];
  split_merge(p.part + (size_t)bh * p.S * DEC_PSTRIDE, p.S, 0, lane, s_mg, p.o + (size_t)bh * 96);
  if (lane == 0) AKI_ST_AGENT(p.cnt + bh, 0u);           // re-armed: the workspace needs zeroing only once
}

static inline size_t dec_cnt_bytes(int B, int H) { return (((size_t)B * H * 4) + 255) / 256 * 256; }

size_t decode_attn_ws_bytes(int B, int H, int Dh, int cap) {
  const size_t tiles = ((size_t)cap + 63) / 64;
  const size_t split = dec_cnt_bytes(B, H) + (size_t)B * H * tiles * DEC_PSTRIDE * 4;
  const size_t f32_q = (size_t)B * H * Dh * 4;      // f32 path: rotated q scratch
  return split > f32_q ? split : f32_q;
}

// max_keys: host-side upper bound of n_keys over the batch (sizes the grid; keys beyond it would be ignored).
int decode_attn_split_launch(const void* q_or_qkv, const float* cos, const float* sin, const int* len, void* kc, void* vc, void* o,
                             const uint64_t* vbits, int nwords, int B, int H, int cap, int max_keys, float scale, bool fused,
                             void* ws, size_t ws_bytes, hipStream_t s) {
  int S, T;
  split_plan((size_t)B * H, cap, max_keys, S, T);
  if (ws == nullptr || ws_bytes < dec_cnt_bytes(B, H) + (size_t)B * H * S * DEC_PSTRIDE * 4) return AKI_ERR_WORKSPACE;
  DecodeAttnParams p = {(const bf16_t*)q_or_qkv, cos, sin, len, (bf16_t*)kc, (bf16_t*)vc, (bf16_t*)o, vbits, nwords,
                        (unsigned*)ws, (float*)((char*)ws + dec_cnt_bytes(B, H)), H, cap, S, T, scale};
  const dim3 grid(S, B * H), block(64);
  AKI_CLEAR_ERR();
  if (fused) hipLaunchKernelGGL(decode_attn_split_kernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(decode_attn_split_kernel<false>, grid, block, 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// ------------------------------------------------------------------------------------------------------------
// fp8 (e4m3) KV cache.  Every cached K / V row (one head, one position: 96 values) is stored as 96 e4m3 bytes with one f32
// dequantisation scale, s = max(amax, 1e-12) / 448 over the row, bytes = e4m3(x / s) rounded to nearest even and saturated at
// +-448 (the rule of quant_rows_fp8_kernel, with true divisions).  The rows are those the bf16 cache would hold: the prefill's bf16
// K / V (kv_cache_quant_fp8_kernel, one launch for all layers) and, per decode step, the bf16-rounded rotated k and the v of the new
// token.  Half the bytes of a bf16 row plus 4 per scale: 0.52x the cache traffic of a batched or long-context decode step.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float kv8_scale(float amax) { return fmaxf(amax, 1e-12f) / 448.0f; }

// two values -> two e4m3 bytes in the low 16 bits
__device__ __forceinline__ unsigned kv8_pack2(float a, float b, float s) {
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a / s, -448.f), 448.f), fminf(fmaxf(b / s, -448.f), 448.f), 0, false) & 0xffffu;
}

// src bf16 [slabs][src_cap][96] -> dst e4m3 [slabs][dst_cap][96] + scale f32 [slabs][dst_cap], rows [0, rows) of every slab.
// Sixteen lanes per row: lane i < 12 holds values 8i .. 8i+7, the row's amax meets within the 16 lanes.
__global__ __launch_bounds__(256) void kv_cache_quant_fp8_kernel(const bf16_t* src, uint8_t* dst, float* scale, int src_cap, int dst_cap,
                                                                 int rows, long long total) {
  const int i = threadIdx.x & 15;
  const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = r < total && i < 12;
  const long long slab = r / rows, j = r - slab * rows;
  float v[8];
  u32x4 x = {0u, 0u, 0u, 0u};
  if (live) x = *(const u32x4*)(src + ((size_t)slab * src_cap + j) * 96 + i * 8);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = bf16_lo(x[e]);
    v[2 * e + 1] = bf16_hi(x[e]);
    amax = fmaxf(amax, fmaxf(fabsf(v[2 * e]), fabsf(v[2 * e + 1])));
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
  const float s = kv8_scale(amax);
  if (!live) return;
  const unsigned b0 = kv8_pack2(v[0], v[1], s), b1 = kv8_pack2(v[2], v[3], s), b2 = kv8_pack2(v[4], v[5], s), b3 = kv8_pack2(v[6], v[7], s);
  const size_t at = (size_t)slab * dst_cap + j;
  *(u32x2*)(dst + at * 96 + i * 8) = u32x2{b0 | (b1 << 16), b2 | (b3 << 16)};
  if (i == 0) scale[at] = s;
}

int kv_cache_quant_fp8_launch(const void* src, int src_cap, void* dst, float* scale, int dst_cap, int slabs, int rows, hipStream_t s) {
  const long long total = (long long)slabs * rows;
  const long long blocks = (total + 15) / 16;
  if (blocks > 0x7fffffffLL) return AKI_ERR_UNSUPPORTED;
  if (blocks == 0) return AKI_OK;
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL(kv_cache_quant_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)src, (uint8_t*)dst, scale, src_cap,
                     dst_cap, rows, total);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// The fused decode step (decode_attn_split_kernel<true>: RoPE, append, split-KV attention, merge) on the e4m3 cache.  Same items,
// workspace, counters and merge; what changes is the row format:
//   append       the owner of the new position rotates k as the bf16 kernel does (bf16-rounded), quantises k and v per head and
//                writes bytes + scales; the new row is attended through its quantised copy, from LDS, like any cached key
//   score phase  lane = key: 6 x 16-byte loads of its K row; pairs of e4m3 widen to bf16 exactly (v_cvt_scalef32_pk_bf16_fp8, as
//                the W8 GEMV) into the bf16 dot2 against q; score = (q . k8) * s_k * scale
//   PV phase     lane = (row group g = lane>>3, 16-byte column chunk i8 = lane&7 < 6): 8 loads cover the tile's 64 V rows; row j
//                carries p_j * s_v[j] while the softmax denominator sums the unscaled p_j
// ------------------------------------------------------------------------------------------------------------
struct DecodeAttn8Params {
  const bf16_t* qkv;          // [B][3*H*96] un-rotated
  const float* cos; const float* sin;   // [capacity][96]
  const int* len;             // cache_len[b]
  uint8_t* kc; uint8_t* vc;   // [B][H][cap][96] e4m3
  float* ks; float* vs;       // [B][H][cap] dequantisation scales
  bf16_t* o;                  // [B][H*96]
  const uint64_t* vbits; int nwords;
  unsigned* cnt; float* part;
  int H, cap, S, T; float scale;
};

__global__ __launch_bounds__(64) void decode_attn_split_fp8kv_kernel(const DecodeAttn8Params p) {
  __shared__ __attribute__((aligned(16))) bf16_t s_q[96];
  __shared__ __attribute__((aligned(16))) uint8_t s_k[96], s_v[96];
  __shared__ float s_sc[2];
  const int lane = threadIdx.x, split = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int ln = p.len[b];
  const int n = ln + 1;
  const int k_begin = split * p.T * 64;
  const int k_end = min(n, k_begin + p.T * 64);
  uint8_t* kb = p.kc + (size_t)bh * p.cap * 96;
  uint8_t* vb = p.vc + (size_t)bh * p.cap * 96;
  float* ksb = p.ks + (size_t)bh * p.cap;
  float* vsb = p.vs + (size_t)bh * p.cap;
  float* part = p.part + ((size_t)bh * p.S + split) * DEC_PSTRIDE;
  const int g = lane >> 3, i8 = lane & 7;
  float m = -INFINITY, l = 0.f, acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  if (k_begin < k_end) {
    const bool owner = ln >= k_begin;                    // ln < k_end holds by construction (k_end <= ln + 1)
    u32x4 kr[6], vr[8];
    float ksc, vsc;
    auto issue_tile = [&](int base) {                    // all 16 loads (+ the lane's two scales) of a tile go out back to back
      const int jr = min(base + lane, k_end - 1);       // clamped rows carry probability 0
      const uint8_t* krow = kb + (size_t)jr * 96;
#pragma unroll
      for (int i = 0; i < 6; ++i) kr[i] = *(const u32x4*)(krow + i * 16);
      ksc = ksb[jr];
      vsc = vsb[jr];
#pragma unroll
      for (int t2 = 0; t2 < 8; ++t2) {
        const int r = min(base + 8 * t2 + g, k_end - 1);
        vr[t2] = *(const u32x4*)(vb + (size_t)r * 96 + min(i8, 5) * 16);
      }
    };
    issue_tile(k_begin);                                 // in flight while q is rotated
    float kn0 = 0.f, kn1 = 0.f, vn0 = 0.f, vn1 = 0.f;
    if (lane < 48) {
      const bf16_t* row = p.qkv + (size_t)b * 3 * p.H * 96 + h * 96;
      const RopeRow rr = rope_row(p.cos, p.sin, ln, lane);
      __bf16 q0, q1;
      rope_rotate_half(rr, bf16_bits_to_f32(row[lane]), bf16_bits_to_f32(row[lane + 48]), q0, q1);
      ((__bf16*)s_q)[lane] = q0;
      ((__bf16*)s_q)[lane + 48] = q1;
      if (owner) {
        const bf16_t* krw = row + p.H * 96;
        const bf16_t* vrw = row + 2 * p.H * 96;
        __bf16 k0, k1;
        rope_rotate_half(rr, bf16_bits_to_f32(krw[lane]), bf16_bits_to_f32(krw[lane + 48]), k0, k1);
        kn0 = (float)k0;                                            // the bf16 row the bf16 cache would hold
        kn1 = (float)k1;
        vn0 = bf16_bits_to_f32(vrw[lane]);
        vn1 = bf16_bits_to_f32(vrw[lane + 48]);
      }
    }
    if (owner) {                                         // workgroup-uniform: the amax reductions run on the whole wave (lanes >= 48 hold 0)
      const float sk = kv8_scale(wave_max(fmaxf(fabsf(kn0), fabsf(kn1))));
      const float sv = kv8_scale(wave_max(fmaxf(fabsf(vn0), fabsf(vn1))));
      if (lane < 48) {
        const unsigned kq = kv8_pack2(kn0, kn1, sk), vq = kv8_pack2(vn0, vn1, sv);
        s_k[lane] = (uint8_t)kq;
        s_k[lane + 48] = (uint8_t)(kq >> 8);
        s_v[lane] = (uint8_t)vq;
        s_v[lane + 48] = (uint8_t)(vq >> 8);
        kb[(size_t)ln * 96 + lane] = (uint8_t)kq;
        kb[(size_t)ln * 96 + lane + 48] = (uint8_t)(kq >> 8);
        vb[(size_t)ln * 96 + lane] = (uint8_t)vq;
        vb[(size_t)ln * 96 + lane + 48] = (uint8_t)(vq >> 8);
      }
      if (lane == 0) {
        s_sc[0] = sk;
        s_sc[1] = sv;
        ksb[ln] = sk;
        vsb[ln] = sv;
      }
    }
    __syncthreads();
    for (int t = 0; t < p.T; ++t) {
      const int base = k_begin + t * 64;
      if (base >= k_end) break;
      const int j = base + lane;
      if (t > 0) issue_tile(base);
      if (owner && base <= ln && ln < base + 64) {
        // the new row lives in LDS (the tile's loads were issued before it was stored): every lane whose clamped row is ln takes it from there
        if (min(j, k_end - 1) == ln) {
#pragma unroll
          for (int i = 0; i < 6; ++i) kr[i] = *(const u32x4*)(s_k + i * 16);
          ksc = s_sc[0];
          vsc = s_sc[1];
        }
#pragma unroll
        for (int t2 = 0; t2 < 8; ++t2)
          if (min(base + 8 * t2 + g, k_end - 1) == ln) vr[t2] = *(const u32x4*)(s_v + min(i8, 5) * 16);
      }
      bool ok = j < k_end;
      if (p.vbits && (base >> 6) < p.nwords) ok = ok && ((p.vbits[(size_t)b * p.nwords + (base >> 6)] >> lane) & 1ull);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 6; ++i) s = dot16_w8(kr[i], *(const u32x4*)(s_q + i * 16), *(const u32x4*)(s_q + i * 16 + 8), s);
      s = ok ? s * ksc * p.scale : -INFINITY;
      const float mn = fmaxf(m, wave_max(s));
      if (mn == -INFINITY) continue;                                   // wave-uniform: nothing visible yet
      const float a = __expf(m - mn);
      const float pr = ok ? __expf(s - mn) : 0.f;
      l = l * a + wave_sum(pr);
      const float pw = ok ? pr * vsc : 0.f;                            // a masked row's scale may be anything: 0 * NaN must not reach acc
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] *= a;
#pragma unroll
      for (int t2 = 0; t2 < 8; ++t2) {
        const float w = __shfl(pw, 8 * t2 + g);
        u32x4 vt = vr[t2];
        asm volatile("" : "+v"(vt));                     // widened here, row by row
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vt[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vt[e], true);
          acc[4 * e] = __builtin_fmaf(w, lo[0], acc[4 * e]);
          acc[4 * e + 1] = __builtin_fmaf(w, lo[1], acc[4 * e + 1]);
          acc[4 * e + 2] = __builtin_fmaf(w, hi[0], acc[4 * e + 2]);
          acc[4 * e + 3] = __builtin_fmaf(w, hi[1], acc[4 * e + 3]);
        }
      }
      m = mn;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      acc[e] += __shfl_xor(acc[e], 8);
      acc[e] += __shfl_xor(acc[e], 16);
      acc[e] += __shfl_xor(acc[e], 32);
    }
  }
  split_publish(part, m, l, acc, lane);                  // lane i8 < 6 of row group 0 holds columns 16 i8 .. 16 i8 + 15
  if (split_ticket(p.cnt + bh, lane) != (unsigned)(p.S - 1)) return;
  asm volatile("" ::: "memory");
  __shared__ float s_mg[DEC_MERGE_FLOATS];
  split_merge(p.part + (size_t)bh * p.S * DEC_PSTRIDE, p.S, 0, lane, s_mg, p.o + (size_t)bh * 96);
  if (lane == 0) AKI_ST_AGENT(p.cnt + bh, 0u);
}

// The grid of decode_attn_split_launch (same T and S, so the same workspace and the same eager / replayed key cuts) on the e4m3 cache.
int decode_attn_split_fp8kv_launch(const void* qkv, const float* cos, const float* sin, const int* len, void* kc, void* vc, float* ks, float* vs,
                                   void* o, const uint64_t* vbits, int nwords, int B, int H, int cap, int max_keys, float scale, void* ws,
                                   size_t ws_bytes, hipStream_t s) {
  int S, T;
  split_plan((size_t)B * H, cap, max_keys, S, T);
  if (ws == nullptr || ws_bytes < dec_cnt_bytes(B, H) + (size_t)B * H * S * DEC_PSTRIDE * 4) return AKI_ERR_WORKSPACE;
  DecodeAttn8Params p = {(const bf16_t*)qkv, cos, sin, len, (uint8_t*)kc, (uint8_t*)vc, ks, vs, (bf16_t*)o, vbits, nwords,
                         (unsigned*)ws, (float*)((char*)ws + dec_cnt_bytes(B, H)), H, cap, S, T, scale};
  const dim3 grid(S, B * H), block(64);
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL(decode_attn_split_fp8kv_kernel, grid, block, 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Grouped split-KV decode attention (bf16, Dh = 96): N returned rows per prompt sample over ONE copy of the prompt's K/V.
//   prefix  kp / vp [B0][H][pcap][96]    the prompt's rows as the prefill wrote them; read-only here
//   suffix  ks / vs [B0*N][H][scap][96]  one slab per returned row: the tokens decoded so far
// Row r belongs to sample b = r / N.  Its keys are prefix rows [0, plen[b]) - filtered by the sample's valid bits - followed by suffix
// rows [0, len[r] - plen[b]]; the last of those is the new token, rotated at position len[r] and appended by the item that owns it
// (decode_attn_split_kernel<true>'s rule, stale-row care included).
// Items (one wave each):
//   prefix item (sample, head, key split, chunk of <= 16 rows): every 64-key K/V tile is loaded ONCE and serves all rows of the chunk -
//               their rotated q's sit in LDS, one (m, l, acc) state per row lives in registers.  The K rows of the next tile are
//               requested once the scores of this one are done, its V rows once the PV products are: the loads of a tile fly under
//               the arithmetic of the one before it (with <= 16 queries per K byte the item is no longer purely HBM-bound).
//   suffix item (row, head, key split): the fused kernel's item on the row's own slab.
// Every item leaves (m, l, acc[96]) per row in the workspace; the counter of a (row, head) expects Sp + Ss arrivals and the last arriver
// merges: prefix splits in order, then suffix splits in order (each segment strided over five lane groups on its own, so trailing
// empty items of either segment - a captured step's larger grid - fold exactly and the bits do not depend on the grid).
// ------------------------------------------------------------------------------------------------------------
struct DecodeGroupParams {
  const bf16_t* qkv;                     // [B0*N][3*H*96], un-rotated
  const float* cos; const float* sin;    // [positions][96]
  const int* len;                        // cache_len[r]: keys before the new token = its RoPE position
  const int* plen;                       // prefix_len[b]
  const bf16_t* kp; const bf16_t* vp;
  bf16_t* ks; bf16_t* vs;
  bf16_t* o;                             // [B0*N][H*96]
  const uint64_t* vbits; int nwords;     // [B0][nwords]
  unsigned* cnt; float* part;            // counters [B0*N*H], partials [B0*N*H][Sp + Ss][DEC_PSTRIDE]
  int N, H, pcap, scap, Sp, Tp, Ss, Ts, NC; float scale;
};

// nothing moves across this point, neither in the optimiser (memory operations) nor in the machine scheduler (anything)
__device__ __forceinline__ void group_order() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// a wave-uniform value moved to a scalar register
__device__ __forceinline__ float uniform_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// The last arriver of (row, head) = rh: all Sp + Ss partials -> o, prefix splits in order, then suffix splits.  The whole wave calls it.
__device__ __forceinline__ void group_merge(const DecodeGroupParams& p, int rh, int lane, float* s_mg) {
  split_merge(p.part + (size_t)rh * (p.Sp + p.Ss) * DEC_PSTRIDE, p.Sp, p.Ss, lane, s_mg, p.o + (size_t)rh * 96);
  __syncthreads();                                     // s_mg is free again: a prefix item may merge several rows
  if (lane == 0) AKI_ST_AGENT(p.cnt + rh, 0u);          // re-armed for the next launch
}

// rows r0 .. r0 + nr - 1 (nr <= NR) of sample b against keys [split * Tp * 64, ...) of the sample's prefix
template <int NR>
__device__ __forceinline__ void group_prefix_item(const DecodeGroupParams& p, int b, int h, int split, int r0, int nr, int lane, bf16_t* s_q,
                                                  float* s_p, float* s_mg) {
  const int g = lane >> 4, i16 = lane & 15, S = p.Sp + p.Ss;
  const int plen = min(p.plen[b], p.pcap);
  const int k_begin = split * p.Tp * 64;
  const int k_end = min(plen, k_begin + p.Tp * 64);
  float m[NR], l[NR], acc[NR][8];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    m[j] = -INFINITY;
    l[j] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
  }
  if (k_begin < k_end) {
    const bf16_t* kb = p.kp + ((size_t)b * p.H + h) * p.pcap * 96;
    const bf16_t* vb = p.vp + ((size_t)b * p.H + h) * p.pcap * 96;
    u32x4 kr[12], vr[16];
    auto issue_k = [&](int base) {
      const bf16_t* krow = kb + (size_t)min(base + lane, k_end - 1) * 96;       // clamped rows carry probability 0
#pragma unroll
      for (int i = 0; i < 12; ++i) kr[i] = *(const u32x4*)(krow + i * 8);
    };
    auto issue_v = [&](int base) {
#pragma unroll
      for (int t2 = 0; t2 < 16; ++t2) {
        const int r = min(base + 4 * t2 + g, k_end - 1);
        vr[t2] = *(const u32x4*)(vb + (size_t)r * 96 + min(i16, 11) * 8);
      }
    };
    issue_k(k_begin);                                    // in flight while the q's are rotated
    issue_v(k_begin);
    if (lane < 48) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        __bf16 q0 = (__bf16)0.f, q1 = (__bf16)0.f;       // rows past the chunk: q = 0, finite scores that nobody stores
        if (j < nr) {
          const bf16_t* row = p.qkv + (size_t)(r0 + j) * 3 * p.H * 96 + h * 96;
          rope_rotate_half(rope_row(p.cos, p.sin, p.len[r0 + j], lane), bf16_bits_to_f32(row[lane]), bf16_bits_to_f32(row[lane + 48]), q0, q1);
        }
        ((__bf16*)s_q)[j * 96 + lane] = q0;
        ((__bf16*)s_q)[j * 96 + lane + 48] = q1;
      }
    }
    __syncthreads();
    for (int t = 0; t < p.Tp; ++t) {
      const int base = k_begin + t * 64;
      if (base >= k_end) break;
      const bool more = base + 64 < k_end;
      bool ok = base + lane < k_end;
      if (p.vbits && (base >> 6) < p.nwords) ok = ok && ((p.vbits[(size_t)b * p.nwords + (base >> 6)] >> lane) & 1ull);
      // scores, row by row.  The compiler barriers keep the LDS reads of a row (q: 48 VGPRs) from being gathered ahead of the rows before
      // it - hoisted, the q's (NR * 48 VGPRs) push the row states into scratch.  m and l are wave-uniform and live in scalar registers.
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        group_order();
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) s = dot8_bf16(kr[i], *(const u32x4*)(s_q + j * 96 + i * 8), s);
        s = ok ? s * p.scale : -INFINITY;
        const float mn = uniform_f32(fmaxf(m[j], wave_max(s)));
        float pj = 0.f;
        if (mn != -INFINITY) {                           // wave-uniform
          const float a = __expf(m[j] - mn);
          pj = ok ? __expf(s - mn) : 0.f;
          l[j] = uniform_f32(l[j] * a + wave_sum(pj));
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][e] *= a;
          m[j] = mn;
        }
        s_p[lane * NR + j] = pj;                         // probabilities meet the PV phase through LDS: [key][row]
      }
      group_order();
      if (more) issue_k(base + 64);                      // the K registers are free: the next tile's rows fly under the PV products
      __syncthreads();
#pragma unroll
      for (int t2 = 0; t2 < 16; ++t2) {
        group_order();
        u32x4 vt = vr[t2];
        asm volatile("" : "+v"(vt));                     // widened row by row, once for all the chunk's rows
        float vf[8], w[NR];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vf[2 * e] = bf16_lo(vt[e]);
          vf[2 * e + 1] = bf16_hi(vt[e]);
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) w[j] = s_p[(4 * t2 + g) * NR + j];        // one key's weights for all rows: NR / 4 16-byte reads
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[j][e] = __builtin_fmaf(w[j], vf[e], acc[j][e]);
      }
      group_order();
      __syncthreads();                                   // s_p is free for the next tile
      if (more) issue_v(base + 64);
    }
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[j][e] += __shfl_xor(acc[j][e], 16);
        acc[j][e] += __shfl_xor(acc[j][e], 32);
      }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j)
    if (j < nr) split_publish(p.part + (((size_t)(r0 + j) * p.H + h) * S + split) * DEC_PSTRIDE, m[j], l[j], acc[j], lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // split_ticket for up to 16 rows at once: lane j arrives at row j's counter
  unsigned prev = 0;
  if (lane < nr) prev = AKI_ADD_AGENT(p.cnt + (size_t)(r0 + lane) * p.H + h, 1u);
  unsigned long long last = __ballot(lane < nr && prev == (unsigned)(S - 1));
  group_order();
  while (last) {                                         // wave-uniform: the rows this item was the last to reach
    const int j = __builtin_ctzll(last);
    last &= last - 1;
    group_merge(p, (r0 + j) * p.H + h, lane, s_mg);
  }
}

// row r of sample b against keys [split * Ts * 64, ...) of its own suffix slab: the fused item.  The slab has no valid bits, and this
// caller has never passed over a tile that leaves the running max at -inf; both stay as they are
__device__ __forceinline__ void group_suffix_item(const DecodeGroupParams& p, int b, int r, int h, int split, int lane, bf16_t* s_q, bf16_t* s_k,
                                                  bf16_t* s_v, float* s_mg) {
  const int S = p.Sp + p.Ss, rh = r * p.H + h;
  const int ln = p.len[r];                               // RoPE position
  const int la = ln - p.plen[b];                         // append row in the suffix slab
  const int n = (la >= 0 && la < p.scap) ? la + 1 : 0;   // a length outside the slab touches no memory: the row sees its prefix only
  const int k_begin = split * p.Ts * 64;
  const int k_end = min(n, k_begin + p.Ts * 64);
  float m, l, acc[8];
  split_item_bf16<false, false>(p.ks + (size_t)rh * p.scap * 96, p.vs + (size_t)rh * p.scap * 96, la, ln, k_begin, k_end, p.Ts, nullptr, 0, 0,
                                      p.qkv + (size_t)r * 3 * p.H * 96 + h * 96, p.H, p.cos, p.sin, p.scale, lane, s_q, s_k, s_v, m, l, acc);
  split_publish(p.part + ((size_t)rh * S + p.Sp + split) * DEC_PSTRIDE, m, l, acc, lane);
  const unsigned prev = split_ticket(p.cnt + rh, lane);
  asm volatile("" ::: "memory");
  if (prev == (unsigned)(S - 1)) group_merge(p, rh, lane, s_mg);
}

// grid (NC * Sp + N * Ss, B0 * H): the prefix items of a (sample, head) come first, they are the long ones.  One instance per chunk
// width NR = 2 / 4 / 8 / 16 rows (the launch picks the smallest that holds min(N, 16)): a kernel's registers are those of its largest
// item, and the 16-row prefix item (160 accumulator registers beside a 112-register tile) must not set them for N = 2 or 4.
template <int NR>
__global__ __launch_bounds__(64) void decode_attn_group_kernel(const DecodeGroupParams p) {
  __shared__ __attribute__((aligned(16))) bf16_t s_q[NR * 96], s_k[96], s_v[96];
  __shared__ __attribute__((aligned(16))) float s_p[64 * NR];
  __shared__ float s_mg[DEC_MERGE_FLOATS];
  const int lane = threadIdx.x, x = blockIdx.x, b = blockIdx.y / p.H, h = blockIdx.y - b * p.H;
  if (x < p.NC * p.Sp) {
    const int c = x / p.Sp, split = x - c * p.Sp;
    group_prefix_item<NR>(p, b, h, split, b * p.N + c * 16, min(min(16, NR), p.N - c * 16), lane, s_q, s_p, s_mg);
  } else {
    const int y = x - p.NC * p.Sp, j = y / p.Ss, split = y - j * p.Ss;
    group_suffix_item(p, b, b * p.N + j, h, split, lane, s_q, s_k, s_v, s_mg);
  }
}

size_t decode_attn_group_ws_bytes(int B0, int N, int H, int pcap, int scap) {
  const size_t tiles = ((size_t)pcap + 63) / 64 + ((size_t)scap + 63) / 64;
  return dec_cnt_bytes(B0 * N, H) + (size_t)B0 * N * H * tiles * DEC_PSTRIDE * 4;
}

// max_pkeys / max_skeys: host upper bounds of prefix_len[b] and of the suffix keys (new token included) - they size the grid.
// Tiles per item from the CAPACITIES, items from the bounds (split_plan, once per segment): eager and captured steps cut alike.
int decode_attn_group_launch(const void* qkv, const float* cos, const float* sin, const int* len, const int* plen, const void* kp,
                             const void* vp, void* ks, void* vs, void* o, const uint64_t* vbits, int nwords, int B0, int N, int H, int pcap,
                             int scap, int max_pkeys, int max_skeys, float scale, void* ws, size_t ws_bytes, hipStream_t s) {
  const int NC = (N + 15) / 16;
  int Sp, Tp, Ss, Ts;
  split_plan((size_t)B0 * NC * H, pcap, max_pkeys, Sp, Tp);
  split_plan((size_t)B0 * N * H, scap, max_skeys, Ss, Ts);
  const size_t cnt_bytes = dec_cnt_bytes(B0 * N, H);
  if (ws == nullptr || ws_bytes < cnt_bytes + (size_t)B0 * N * H * (Sp + Ss) * DEC_PSTRIDE * 4) return AKI_ERR_WORKSPACE;
  if ((size_t)B0 * H > 65535 || (size_t)NC * Sp + (size_t)N * Ss > 0x7fffffffu) return AKI_ERR_UNSUPPORTED;
  DecodeGroupParams p = {(const bf16_t*)qkv, cos, sin, len, plen, (const bf16_t*)kp, (const bf16_t*)vp, (bf16_t*)ks, (bf16_t*)vs, (bf16_t*)o,
                         vbits, nwords, (unsigned*)ws, (float*)((char*)ws + cnt_bytes), N, H, pcap, scap, Sp, Tp, Ss, Ts, NC, scale};
  const dim3 grid(NC * Sp + N * Ss, B0 * H), block(64);
  AKI_CLEAR_ERR();
  const int width = N < 16 ? N : 16;
  if (width <= 2) hipLaunchKernelGGL(decode_attn_group_kernel<2>, grid, block, 0, s, p);
  else if (width <= 4) hipLaunchKernelGGL(decode_attn_group_kernel<4>, grid, block, 0, s, p);
  else if (width <= 8) hipLaunchKernelGGL(decode_attn_group_kernel<8>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(decode_attn_group_kernel<16>, grid, block, 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int rope_append_launch(const void* qkv, const float* cos, const float* sin, const int* pos, const int* cache_len, void* q_out,
                       void* k_cache, void* v_cache, int B, int H, int Dh, int cap, int dtype, hipStream_t s) {
  const dim3 grid(B, (H * Dh + 255) / 256), block(256);
  AKI_CLEAR_ERR();
  if (dtype == AKI_DT_BF16)
    hipLaunchKernelGGL(rope_append_kernel<__bf16>, grid, block, 0, s, (const __bf16*)qkv, cos, sin, pos, cache_len, (__bf16*)q_out,
                       (__bf16*)k_cache, (__bf16*)v_cache, H, Dh, cap);
  else
    hipLaunchKernelGGL(rope_append_kernel<float>, grid, block, 0, s, (const float*)qkv, cos, sin, pos, cache_len, (float*)q_out,
                       (float*)k_cache, (float*)v_cache, H, Dh, cap);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int decode_attn_launch(const void* q, const void* kc, const void* vc, void* o, const int* n_keys, const uint64_t* vbits, int nwords,
                       int B, int H, int Dh, int cap, float scale, int dtype, hipStream_t s) {
  if (Dh != 96) return AKI_ERR_UNSUPPORTED;
  const dim3 grid(B * H), block(256);
  AKI_CLEAR_ERR();
  if (dtype == AKI_DT_BF16)
    hipLaunchKernelGGL((decode_attn_kernel<__bf16, 96>), grid, block, 0, s, (const __bf16*)q, (const __bf16*)kc, (const __bf16*)vc,
                       (__bf16*)o, n_keys, vbits, nwords, H, cap, scale);
  else
    hipLaunchKernelGGL((decode_attn_kernel<float, 96>), grid, block, 0, s, (const float*)q, (const float*)kc, (const float*)vc,
                       (float*)o, n_keys, vbits, nwords, H, cap, scale);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}


// ---- greedy token pick: what the reference's generate loop does between two decode steps (HF GenerationMixin greedy branch:
// argmax over the vocabulary, finished rows take pad_token_id, append, eos check; src/aki.py:136-209 hands its kwargs to it) as
// ONE launch that can sit inside the replayed step - the loop's five small launches and its per-token host sync were 4 % of a token.
// Ties go to the lower index and a NaN outranks every number (torch.argmax's ordering).  PickParams and the other parameter structs of
// this section: pick_params.h.
__device__ __forceinline__ bool pick_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na != nb) return na;
  if (na) return ia < ib;
  return a > b || (a == b && ia < ib);
}

// Constrained decoding (ConstraintParams, pick_params.h).  The table rows row b's states index: [base, base + count).  Without the per-row arrays that is the whole table; with them the row's own
// slice, cut at the pool's end (a negative base: no rows at all, the row is left untouched).
struct ConstraintRow { int base, count; };
__device__ __forceinline__ ConstraintRow constraint_row(const ConstraintParams* c, int b) {
  if (c == nullptr || c->table == nullptr) return ConstraintRow{0, 0};
  if (c->row_base == nullptr || c->row_states == nullptr) return ConstraintRow{0, c->n_states};
  const int base = c->row_base[b], count = c->row_states[b];
  if (base < 0 || base >= c->n_states) return ConstraintRow{0, 0};
  return ConstraintRow{base, min(count, c->n_states - base)};
}

// states[b, n], or -1 where there is nothing to read (no constraint, n outside the history)
__device__ __forceinline__ int constraint_state(const ConstraintParams* c, int b, int n) {
  if (c == nullptr || c->table == nullptr || n < 0 || n >= c->states_ld) return -1;
  return c->states[(size_t)b * c->states_ld + n];
}

constexpr int PICK_THREADS = 1024;
// The pick's bookkeeping tail, shared by the greedy and the sampling kernels: thread 0 holds the picked id `bi` and what it requested before
// the scan (was_done, len0, start0, eos4; cs: the row's state under a constraint `c`, cr: its table rows); pad for finished rows, append,
// the next state, eos check, cache_len advance, then every thread gathers the next step's embedding row.
__device__ __forceinline__ void pick_finish(const PickParams& p, int b, bool was_done, int len0, int start0, const int64_t (&eos4)[4], int bi,
                                            const ConstraintParams* c = nullptr, int cs = -1, ConstraintRow cr = ConstraintRow{0, 0}) {
  __shared__ int64_t s_next;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int64_t nxt = was_done ? p.pad : (int64_t)bi;
    int t = p.step;
    if (p.cache_len != nullptr) {
      t += len0 + p.advance - start0;
      if (p.advance) p.cache_len[b] = len0 + 1;
    }
    if (p.tokens != nullptr && t >= 0 && t < p.tokens_ld) p.tokens[(size_t)b * p.tokens_ld + t] = nxt;
    if (c != nullptr && c->table != nullptr && t >= 0 && t + 1 < c->states_ld) {
      // a finished row keeps its state; a state or a token outside the table gives -1, which the mask reads as "row untouched".  The entry
      // is stored as it stands: under the per-row form a number local to the row's automaton
      int ns = cs;
      if (!was_done) ns = (cs >= 0 && cs < cr.count && bi >= 0 && bi < p.V) ? (int)c->table[(size_t)(cr.base + cs) * c->table_ld + bi] : -1;
      c->states[(size_t)b * c->states_ld + t + 1] = ns;
    }
    p.ids[b] = nxt;
    s_next = nxt;
    if (p.done != nullptr && !was_done) {
      bool hit = eos4[0] == nxt || eos4[1] == nxt || eos4[2] == nxt || eos4[3] == nxt;
      for (int i = 4; i < p.n_eos; ++i) hit = hit || p.eos[i] == nxt;
      if (hit) {
        p.done[b] = 1;
        if (p.done_at) p.done_at[b] = t;
      }
    }
  }
  if (p.emb_out != nullptr) {
    __syncthreads();
    const int64_t nxt = s_next;
    const bool extra = p.emb_extra != nullptr && nxt > p.max_original_id;
    const bf16_t* src = extra ? p.emb_extra + (size_t)(nxt - p.max_original_id - 1) * p.d : p.emb_main + (size_t)nxt * p.d;
    bf16_t* dst = p.emb_out + (size_t)b * p.d;
    for (int c = tid; c < p.d / 8; c += PICK_THREADS) *(u32x4*)(dst + (size_t)c * 8) = *(const u32x4*)(src + (size_t)c * 8);
  }
}

// One workgroup of 16 waves per row: the scan of 32 064 logits is a latency chain (load, eight compares, next load); 1024 threads walk it in 4 trips of two
// loads each instead of 16 trips of one (19.4 -> measured in profiles/r05_decode_token_trace.txt).
// F32: the row to scan is `rowf` (an f32 row of processed scores, see logits processors below), not p.logits
template <bool F32>
__device__ __forceinline__ void greedy_pick_row(const PickParams& p, const float* rowf, const ConstraintParams* c = nullptr) {
  __shared__ float s_v[PICK_THREADS / 64];
  __shared__ int s_i[PICK_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // What the bookkeeping needs does not depend on the argmax: thread 0 requests it BEFORE the scan, so that behind the scan only stores are
  // left (it used to be a chain of five dependent round trips behind the reduction, about a third of the launch).
  bool was_done = false;
  int len0 = 0, start0 = 0;
  int64_t eos4[4] = {-1, -1, -1, -1};                        // token ids are >= 0: -1 matches nothing
  int cs = -1;
  ConstraintRow cr = {0, 0};
  if (tid == 0) {
    was_done = p.done != nullptr && p.done[b] != 0;
    if (p.cache_len != nullptr) {
      len0 = p.cache_len[b];
      if (p.start_len) start0 = p.start_len[b];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < p.n_eos) eos4[i] = p.eos[i];
    if (c != nullptr) {
      cr = constraint_row(c, b);                             // two loads that depend on nothing: out with the others, ahead of the scan
      cs = constraint_state(c, b, p.step + (p.cache_len != nullptr ? len0 + p.advance - start0 : 0));
    }
  }
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if constexpr (F32) {
    // rowf is 16-byte aligned (checked on the host); two float4 loads per trip, as the bf16 scan below
    const int nvec = p.V / 4;
    for (int c0 = tid; c0 < nvec; c0 += 2 * PICK_THREADS) {
      const int c1 = c0 + PICK_THREADS;
      const float4 v0 = *(const float4*)(rowf + (size_t)c0 * 4);
      const float4 v1 = c1 < nvec ? *(const float4*)(rowf + (size_t)c1 * 4) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 v = h ? v1 : v0;
        const int c = (h ? c1 : c0) * 4;
        if (h && c1 >= nvec) break;
        if (pick_better(v.x, c, best, bi)) { best = v.x; bi = c; }
        if (pick_better(v.y, c + 1, best, bi)) { best = v.y; bi = c + 1; }
        if (pick_better(v.z, c + 2, best, bi)) { best = v.z; bi = c + 2; }
        if (pick_better(v.w, c + 3, best, bi)) { best = v.w; bi = c + 3; }
      }
    }
    for (int i = nvec * 4 + tid; i < p.V; i += PICK_THREADS)
      if (pick_better(rowf[i], i, best, bi)) { best = rowf[i]; bi = i; }
  } else {
  const bf16_t* row = p.logits + (size_t)b * p.ld;
  const bool vec = ((p.ld & 7) == 0) && ((((uintptr_t)p.logits) & 15) == 0);
  const int nvec = vec ? p.V / 8 : 0;
  for (int c0 = tid; c0 < nvec; c0 += 2 * PICK_THREADS) {
    const int c1 = c0 + PICK_THREADS;                        // both loads go out before the first compare
    const u32x4 v0 = *(const u32x4*)(row + (size_t)c0 * 8);
    const u32x4 v1 = c1 < nvec ? *(const u32x4*)(row + (size_t)c1 * 8) : u32x4{0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};   // -inf: never picked
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 v = h ? v1 : v0;
      const int c = h ? c1 : c0;
      if (h && c1 >= nvec) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
        if (pick_better(lo, c * 8 + 2 * e, best, bi)) { best = lo; bi = c * 8 + 2 * e; }
        if (pick_better(hi, c * 8 + 2 * e + 1, best, bi)) { best = hi; bi = c * 8 + 2 * e + 1; }
      }
    }
  }
  for (int i = nvec * 8 + tid; i < p.V; i += PICK_THREADS) {
    const float x = bf16_bits_to_f32(row[i]);
    if (pick_better(x, i, best, bi)) { best = x; bi = i; }
  }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (pick_better(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { s_v[wave] = best; s_i[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PICK_THREADS / 64; ++w)
      if (pick_better(s_v[w], s_i[w], best, bi)) { best = s_v[w]; bi = s_i[w]; }
  }
  pick_finish(p, b, was_done, len0, start0, eos4, bi, c, cs, cr);
}

__global__ __launch_bounds__(PICK_THREADS) void greedy_pick_kernel(const PickParams p) { greedy_pick_row<false>(p, nullptr); }


// ---- logits processors: what HF `generate` applies to a step's f32 scores before it picks (GenerationMixin._get_logits_processor, in its
// order), for the case the reference runs - a decoder-only model called with inputs_embeds only, so the processors' input_ids are the row's
// GENERATED tokens h[0, n) and never the prompt:
//   1 repetition penalty  s = s < 0 ? s * penalty : s / penalty for every distinct token of h (RepetitionPenaltyLogitsProcessor)
//   1b frequency / presence penalty  (not HF's: the OpenAI definition, in vLLM's place) for every distinct token of h with c occurrences:
//                         s = s - fl(frequency * c) when frequency != 0, then s = s - presence when presence != 0; one value of each per row
//   2 no-repeat n-gram    -inf for every token that would complete an n-gram already in h (NoRepeatNGramLogitsProcessor)
//   3 bad words           -inf for a one-token word; for a longer word, -inf for its last token when h ends with the rest of it and h holds
//                         at least the whole word's length (SequenceBiasLogitsProcessor's rule)
//   4 minimum length      -inf for every eos id while n < min_length (MinLength / MinNewTokensLength: the prompt length is 0 here)
//   5 suppress tokens     -inf always; begin-suppress tokens -inf at n == 0
//   6 token constraint    (not HF's: ConstraintParams above) -inf for every token the row's state states[b, n] does not allow, n unclamped
// n = step + (cache_len ? cache_len[b] - start_len[b] : 0), so that one captured graph serves every replay.  Rows with done[b] set get the
// plain f32 copy.  One workgroup per row, O(V + n * ngram + bad-word ids); ids outside [0, V) are skipped.  (ProcParams: pick_params.h)
constexpr int PROC_MAX_V = 131072;   // the repetition penalty's LDS bitmap: 16 KB

__device__ __forceinline__ void ban(float* out, int V, int64_t g) {
  if (g >= 0 && g < V) out[g] = -INFINITY;
}

constexpr int PROC_HIST_LDS = 4096;  // 1b counts from an LDS copy of a history up to this length (16 KB), from global memory above it

// arr[b] of a nullable per-row float array, in a scalar register; nullptr and a value that is not finite read as 0
__device__ __forceinline__ float row_penalty(const float* arr, int b) {
  if (arr == nullptr) return 0.f;
  const float v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(arr[b])));
  return (v >= -3.0e38f && v <= 3.0e38f) ? v : 0.f;
}

__device__ void process_row(const ProcParams& q, int b, float* out, unsigned* s_bits) {
  __shared__ __attribute__((aligned(16))) int s_hist_ids[PROC_HIST_LDS];
  const int tid = threadIdx.x, nt = blockDim.x, V = q.V;
  int n = q.step;
  if (q.cache_len != nullptr) n += q.cache_len[b] - (q.start_len != nullptr ? q.start_len[b] : 0);
  const int n_state = n;                                     // the state history has its own width: indexed before the clamp
  n = q.tokens == nullptr ? 0 : min(max(n, 0), q.tokens_ld);
  const bool skip = q.done != nullptr && q.done[b] != 0;
  // 0: the row in f32
  if (q.in_f32) {
    const float* in = (const float*)q.in + (size_t)b * q.ld_in;
    for (int i = tid; i < V; i += nt) out[i] = in[i];
  } else {
    const bf16_t* in = (const bf16_t*)q.in + (size_t)b * q.ld_in;
    const bool vec = ((q.ld_in & 7) == 0) && ((((uintptr_t)q.in) & 15) == 0) && ((q.ld_out & 3) == 0) && ((((uintptr_t)q.out) & 15) == 0);
    const int nvec = vec ? V / 8 : 0;
    for (int c = tid; c < nvec; c += nt) {
      const u32x4 v = *(const u32x4*)(in + (size_t)c * 8);
      *(float4*)(out + (size_t)c * 8) = make_float4(bf16_lo(v[0]), bf16_hi(v[0]), bf16_lo(v[1]), bf16_hi(v[1]));
      *(float4*)(out + (size_t)c * 8 + 4) = make_float4(bf16_lo(v[2]), bf16_hi(v[2]), bf16_lo(v[3]), bf16_hi(v[3]));
    }
    for (int i = nvec * 8 + tid; i < V; i += nt) out[i] = bf16_bits_to_f32(in[i]);
  }
  if (skip) {
    __syncthreads();
    return;
  }
  const int64_t* h = q.tokens + (size_t)b * q.tokens_ld;
  // 1b's two values: one float per row, the same address for every thread of the row, so what they decide below is workgroup-uniform
  // (moved to a scalar register to say so).  A value that is not finite reads as 0.
  const float fq = row_penalty(q.freq, b), pr = row_penalty(q.pres, b);
  const bool rep = q.penalty != 1.f;
  const bool pen = (rep || fq != 0.f || pr != 0.f) && n > 0;
  const bool hist_lds = pen && fq != 0.f && n <= PROC_HIST_LDS;
  if (pen)
    for (int i = tid; i < (V + 31) / 32; i += nt) s_bits[i] = 0u;
  if (hist_lds)                                              // the history as 32-bit ids (V < 2^31), what is outside [0, V) as -1
    for (int i = tid; i < n; i += nt) {
      const int64_t g = h[i];
      s_hist_ids[i] = (g >= 0 && g < V) ? (int)g : -1;
    }
  __syncthreads();                                           // the copy (and the bitmap, the staged history) before any scattered write
  if (pen) {
    // every distinct token once: the occurrence that sets its bit owns it, reads the copied score and writes the penalised one.
    // 1 the repetition penalty; 1b then x - fl(frequency * count) and x - presence, each ONE rounded f32 operation (never an FMA).
    // The owner counts its token's occurrences itself, over the whole history: no counter lives between steps and no atomic adds up.
    for (int i = tid; i < n; i += nt) {
      const int64_t g = h[i];
      if (g < 0 || g >= V) continue;
      const unsigned m = 1u << (g & 31);
      if (atomicOr(&s_bits[g >> 5], m) & m) continue;
      float x = out[g];
      if (rep) x = x < 0.f ? x * q.penalty : x / q.penalty;
      if (fq != 0.f) {
        int c = 0;
        if (hist_lds) {
          const int gi = (int)g;
          int j = 0;
          for (; j + 4 <= n; j += 4) {                       // every lane reads the same words: one broadcast read per four tokens
            const int4 v = *(const int4*)(s_hist_ids + j);
            c += (v.x == gi) + (v.y == gi) + (v.z == gi) + (v.w == gi);
          }
          for (; j < n; ++j) c += s_hist_ids[j] == gi;
        } else {
          for (int j = 0; j < n; ++j) c += h[j] == g;
        }
        x = __fsub_rn(x, __fmul_rn(fq, (float)c));
      }
      if (pr != 0.f) x = __fsub_rn(x, pr);
      out[g] = x;
    }
    __syncthreads();                                         // penalties before the bans: a banned token ends at -inf
  }
  const int ng = q.ngram;
  if (ng > 0 && n + 1 >= ng) {
    for (int i = tid; i <= n - ng; i += nt) {
      bool match = true;
      for (int j = 0; j < ng - 1 && match; ++j) match = h[i + j] == h[n - ng + 1 + j];
      if (match) ban(out, V, h[i + ng - 1]);
    }
  }
  for (int s = tid; s < q.n_bad; s += nt) {
    const int o0 = min(max(q.bad_off[s], 0), q.n_bad_ids), o1 = min(max(q.bad_off[s + 1], o0), q.n_bad_ids), L = o1 - o0;
    if (L <= 0) continue;
    bool hit = L == 1 || L <= n;
    for (int j = 0; j < L - 1 && hit; ++j) hit = h[n - (L - 1) + j] == q.bad_ids[o0 + j];
    if (hit) ban(out, V, q.bad_ids[o1 - 1]);
  }
  if (n < q.min_len)
    for (int i = tid; i < q.n_eos; i += nt) ban(out, V, q.eos[i]);
  for (int i = tid; i < q.n_suppress; i += nt) ban(out, V, q.suppress[i]);
  if (n == 0)
    for (int i = tid; i < q.n_begin; i += nt) ban(out, V, q.begin_suppress[i]);
  // 6: the constraint.  Like the bans it only ever writes -inf, so it shares their side of the barrier behind the penalties.  Eight int16
  // entries per 16-byte load (a negative entry = its sign bit); a state outside the table leaves the row as it is.
  if (q.c.table != nullptr) {
    const ConstraintRow cr = constraint_row(&q.c, b);
    const int s = constraint_state(&q.c, b, n_state);
    if (s >= 0 && s < cr.count) {
      const int16_t* row = q.c.table + (size_t)(cr.base + s) * q.c.table_ld;
      const bool vec = ((q.c.table_ld & 7) == 0) && ((((uintptr_t)q.c.table) & 15) == 0);
      const bool vec_out = (((uintptr_t)out) & 15) == 0;
      const int nvec = vec ? V / 8 : 0;
      for (int c = tid; c < nvec; c += nt) {
        const u32x4 w = *(const u32x4*)(row + (size_t)c * 8);
        if (((w[0] | w[1] | w[2] | w[3]) & 0x80008000u) == 0u) continue;            // all eight allowed
        float* o = out + (size_t)c * 8;
        if (vec_out && ((w[0] & w[1] & w[2] & w[3]) & 0x80008000u) == 0x80008000u) {  // none allowed: the common chunk of a sparse state
          *(float4*)o = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
          *(float4*)(o + 4) = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (w[e] & 0x8000u) o[2 * e] = -INFINITY;
            if (w[e] & 0x80000000u) o[2 * e + 1] = -INFINITY;
          }
        }
      }
      for (int i = nvec * 8 + tid; i < V; i += nt)
        if (row[i] < 0) out[i] = -INFINITY;
    }
  }
  __syncthreads();
}

constexpr int PROC_THREADS = 1024;
__global__ __launch_bounds__(PROC_THREADS) void logits_process_kernel(const ProcParams q) {
  __shared__ unsigned s_bits[PROC_MAX_V / 32];
  process_row(q, blockIdx.x, q.out + (size_t)blockIdx.x * q.ld_out, s_bits);
}

// the greedy pick over the processed row: one launch, the processed scores land in q.out (a [B, ld_out] f32 scratch) and are scanned from there
__global__ __launch_bounds__(PICK_THREADS) void greedy_pick_processed_kernel(const PickParams p, const ProcParams q) {
  __shared__ unsigned s_bits[PROC_MAX_V / 32];
  float* rowf = q.out + (size_t)blockIdx.x * q.ld_out;
  process_row(q, blockIdx.x, rowf, s_bits);
  greedy_pick_row<true>(p, rowf, &q.c);
}

// ---- sampling pick: HF's `do_sample` step (processors -> temperature -> top-k -> top-p -> softmax -> multinomial) with the greedy pick's
// bookkeeping and embedding gather, as ONE launch, one workgroup per row.  No sort: both filters are thresholds on the order-preserving
// 32-bit key of y = x / T, "keep i iff the weight of the strictly larger keys is below P" - weight 1 and P = k for top-k, weight
// exp(y - max) and P = top_p * (mass top-k kept) for top-p - found by a three-digit (11 + 11 + 10 bit) radix select over LDS histograms.
// The histograms are 64-bit INTEGERS (the mass as 2^-40 fixed point) filled with integer atomics, so the result does not depend on the
// order the atomics land in: run-to-run deterministic without a float atomic.  The draw is a counter-based Philox4x32-10 word per
// (token index, row, call), inverted through the cumulative sum in index order: per-thread chunk sums and a fixed-order block scan.
// SampleParams and SampleRowParams (the per-row form, aki_sample_pick_rows): pick_params.h.
template <bool ROWS> struct SampleArgs { using type = SampleParams; };
template <> struct SampleArgs<true> { using type = SampleRowParams; };

__device__ __forceinline__ unsigned sample_key(float y) {   // larger y <=> larger key; -0 and +0 share one
  unsigned u = __float_as_uint(y);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long m0 = 0xD2511F53ull * c0, m1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(m1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(m0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)m1; c3 = (unsigned)m0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// exclusive scan in thread order over the workgroup, one fixed association: 6 shuffle levels in a wave, 4 over the 16 wave totals, 1 add
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_w, T* incl, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_up(inc, o);
    if (lane >= o) inc += n;
  }
  T exl = __shfl_up(inc, 1);
  if (lane == 0) exl = T(0);
  __syncthreads();                                          // s_w may still be read from the scan before
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  T wt = lane < PICK_THREADS / 64 ? s_w[lane] : T(0);
#pragma unroll
  for (int o = 1; o < PICK_THREADS / 64; o <<= 1) {
    const T n = __shfl_up(wt, o);
    if (lane >= o) wt += n;
  }
  *total = __shfl(wt, PICK_THREADS / 64 - 1);
  const T pre = __shfl(wt, wave > 0 ? wave - 1 : 0);
  if (wave > 0) { exl = pre + exl; inc = pre + inc; }
  *incl = inc;
  return exl;
}

constexpr int SEL_BINS = 2048;                              // 16 KB of 64-bit bins: the processors' bitmap, free once they have run
constexpr float SEL_FIX = 1099511627776.f;                  // 2^40: exp(y - max) in (0, 1] as fixed point; V * 2^40 < 2^57

// The smallest key tau such that the weight of the keys above it (among keys >= lo_key) is below P: kept <=> key >= tau.
// MASS: weight exp(y - ymax) and P = ceil(top_p * total weight); else weight 1 and P = P_count.
template <bool MASS>
__device__ unsigned select_threshold(const float* rowf, int V, unsigned lo_key, float ymax, unsigned long long P_count, float top_p,
                                     unsigned long long* hist, unsigned long long* s_w, unsigned long long* s_pick) {
  const int tid = threadIdx.x, ngroups = (V + 3) / 4;
  unsigned pre = 0;
  unsigned long long P = P_count;
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, bits = pass == 2 ? 10 : 11;
    for (int i = tid; i < SEL_BINS; i += PICK_THREADS) hist[i] = 0ull;
    if (tid == 0) { s_pick[0] = 0ull; s_pick[1] = 1ull; }
    __syncthreads();
    for (int g = tid; g < ngroups; g += PICK_THREADS) {
      const float4 v = *(const float4*)(rowf + (size_t)g * 4);
      const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (g * 4 + e >= V) continue;
        const unsigned key = sample_key(ve[e]);
        if (key < lo_key || (pass > 0 && (key >> (shift + bits)) != pre)) continue;
        const unsigned long long w = MASS ? (unsigned long long)(expf(ve[e] - ymax) * SEL_FIX) : 1ull;
        if (w) atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], w);
      }
    }
    __syncthreads();
    // bins from the top: thread t owns bins 2047 - 2t and 2046 - 2t; `above` = the weight of the bins above its first one
    const int d = SEL_BINS - 1 - 2 * tid;
    const unsigned long long a = hist[d], b = hist[d - 1];
    unsigned long long incl, total;
    const unsigned long long above = block_excl_scan<unsigned long long>(a + b, s_w, &incl, &total);
    if (MASS && pass == 0) {
      P = (unsigned long long)ceil((double)top_p * (double)total);
      if (P < 1ull) P = 1ull;
    }
    // exactly one bin holds the threshold: above(d) < P <= above(d) + hist[d]
    if (above < P && P <= above + a) { s_pick[0] = (unsigned long long)d; s_pick[1] = P - above; }
    else if (above + a < P && P <= above + a + b) { s_pick[0] = (unsigned long long)(d - 1); s_pick[1] = P - above - a; }
    __syncthreads();
    pre = (pre << bits) | (unsigned)s_pick[0];
    P = s_pick[1];
    __syncthreads();
  }
  return pre;
}

template <bool ROWS>
__device__ __forceinline__ void sample_pick_body(const PickParams& p, const ProcParams& q, const typename SampleArgs<ROWS>::type& sp) {
  __shared__ unsigned long long s_hist[SEL_BINS];           // first the processors' bitmap (PROC_MAX_V / 32 words), then the select's bins
  __shared__ unsigned long long s_w64[PICK_THREADS / 64], s_pick[2];
  __shared__ float s_wf[PICK_THREADS / 64];
  __shared__ float s_v[PICK_THREADS / 64];
  __shared__ int s_i[PICK_THREADS / 64];
  __shared__ int s_owner, s_last, s_tok;
  static_assert(sizeof(s_hist) >= PROC_MAX_V / 8, "the bitmap has to fit the bins");
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = p.V;
  float* rowf = q.out + (size_t)b * q.ld_out;
  if (sp.processed) process_row(q, b, rowf, (unsigned*)s_hist);
  bool was_done = false;
  int len0 = 0, start0 = 0;
  int64_t eos4[4] = {-1, -1, -1, -1};
  int cs = -1;
  ConstraintRow cr = {0, 0};
  if (tid == 0) {
    was_done = p.done != nullptr && p.done[b] != 0;
    if (p.cache_len != nullptr) {
      len0 = p.cache_len[b];
      if (p.start_len) start0 = p.start_len[b];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < p.n_eos) eos4[i] = p.eos[i];
    cr = constraint_row(&q.c, b);
    cs = constraint_state(&q.c, b, p.step + (p.cache_len != nullptr ? len0 + p.advance - start0 : 0));
    s_owner = 0x7fffffff; s_last = -1; s_tok = -1;
  }
  const bool row_done = p.done != nullptr && p.done[b] != 0;   // uniform: every thread reads the same byte, before thread 0 can set it
  float* probs = sp.probs ? sp.probs + (size_t)b * sp.ld_probs : nullptr;
  float T, top_p;
  int top_k;
  unsigned seed_lo, seed_hi, ctr1, off_lo, off_hi;
  if constexpr (ROWS) {
    T = sp.temperature[b]; top_k = sp.top_k[b]; top_p = sp.top_p[b];
    const unsigned long long key = sp.seed[b];
    seed_lo = (unsigned)key; seed_hi = (unsigned)(key >> 32);
    ctr1 = 0u; off_lo = 0u; off_hi = 0u;
  } else {
    T = sp.temperature; top_k = sp.top_k; top_p = sp.top_p;
    seed_lo = sp.seed_lo; seed_hi = sp.seed_hi;
    ctr1 = (unsigned)b; off_lo = sp.off_lo; off_hi = sp.off_hi;
  }
  // min_p (HF MinPLogitsWarper, behind top-k and top-p): a kept token stays iff exp(y - ymax) >= min_p - the weight the draw computes
  // anyway.  One float per row, every thread reads the same entry; a value outside (0, 1] (0, NaN, no array) is no filter: w >= 0 holds.
  float min_p = sp.min_p != nullptr ? sp.min_p[b] : 0.f;
  if (!(min_p > 0.f && min_p <= 1.f)) min_p = 0.f;
  // pass 0: argmax of x in the greedy pick's ordering, y = x / T (correctly rounded) into the scratch row
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (sp.processed) {
    for (int g = tid; g < V / 4; g += PICK_THREADS) {
      float4 v = *(const float4*)(rowf + (size_t)g * 4);
      const int c = g * 4;
      if (pick_better(v.x, c, best, bi)) { best = v.x; bi = c; }
      if (pick_better(v.y, c + 1, best, bi)) { best = v.y; bi = c + 1; }
      if (pick_better(v.z, c + 2, best, bi)) { best = v.z; bi = c + 2; }
      if (pick_better(v.w, c + 3, best, bi)) { best = v.w; bi = c + 3; }
      v.x = __fdiv_rn(v.x, T); v.y = __fdiv_rn(v.y, T); v.z = __fdiv_rn(v.z, T); v.w = __fdiv_rn(v.w, T);
      *(float4*)(rowf + (size_t)g * 4) = v;
    }
    for (int i = V / 4 * 4 + tid; i < V; i += PICK_THREADS) {
      const float x = rowf[i];
      if (pick_better(x, i, best, bi)) { best = x; bi = i; }
      rowf[i] = __fdiv_rn(x, T);
    }
  } else {
    const bf16_t* row = p.logits + (size_t)b * p.ld;
    const bool vec = ((p.ld & 7) == 0) && ((((uintptr_t)p.logits) & 15) == 0);
    const int nvec = vec ? V / 8 : 0;
    for (int c = tid; c < nvec; c += PICK_THREADS) {
      const u32x4 v = *(const u32x4*)(row + (size_t)c * 8);
      float y[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
        if (pick_better(lo, c * 8 + 2 * e, best, bi)) { best = lo; bi = c * 8 + 2 * e; }
        if (pick_better(hi, c * 8 + 2 * e + 1, best, bi)) { best = hi; bi = c * 8 + 2 * e + 1; }
        y[2 * e] = __fdiv_rn(lo, T); y[2 * e + 1] = __fdiv_rn(hi, T);
      }
      *(float4*)(rowf + (size_t)c * 8) = make_float4(y[0], y[1], y[2], y[3]);
      *(float4*)(rowf + (size_t)c * 8 + 4) = make_float4(y[4], y[5], y[6], y[7]);
    }
    for (int i = nvec * 8 + tid; i < V; i += PICK_THREADS) {
      const float x = bf16_bits_to_f32(row[i]);
      if (pick_better(x, i, best, bi)) { best = x; bi = i; }
      rowf[i] = __fdiv_rn(x, T);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (pick_better(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { s_v[wave] = best; s_i[wave] = bi; }
  __syncthreads();                                          // also: the scratch row is written
  best = s_v[0]; bi = s_i[0];
#pragma unroll
  for (int w = 1; w < PICK_THREADS / 64; ++w)
    if (pick_better(s_v[w], s_i[w], best, bi)) { best = s_v[w]; bi = s_i[w]; }
  const float ymax = __fdiv_rn(best, T);
  // rows the draw has nothing to say about take the greedy pick: finished (pad), a NaN / +inf / -inf maximum, top_k == 1
  // (the per-row form also for a temperature that is not > 0: the host validates what it writes, the kernel keeps bad bits in the row)
  const bool greedy = row_done || !(ymax == ymax) || ymax == INFINITY || ymax == -INFINITY || top_k == 1 || (ROWS && !(T > 0.f));
  int tok = bi;
  if (greedy) {
    if (probs)
      for (int i = tid; i < V; i += PICK_THREADS) probs[i] = (!row_done && i == bi) ? 1.f : 0.f;
  } else {
    unsigned tau = 0u;
    if (top_k > 0 && top_k < V)
      tau = select_threshold<false>(rowf, V, 0u, ymax, (unsigned long long)top_k, 1.f, s_hist, s_w64, s_pick);
    if (top_p < 1.f) {
      const unsigned tp = select_threshold<true>(rowf, V, tau, ymax, 0ull, top_p, s_hist, s_w64, s_pick);
      tau = tp > tau ? tp : tau;
    }
    // the draw: thread t owns the groups of four [t * gpt, (t + 1) * gpt); group sums pairwise, chunk sums in order, then the block scan
    const int ngroups = (V + 3) / 4, gpt = (ngroups + PICK_THREADS - 1) / PICK_THREADS;
    const int g0 = tid * gpt, g1 = min(g0 + gpt, ngroups);
    float csum = 0.f;
    int last = -1;
    for (int g = g0; g < g1; ++g) {
      const float4 v = *(const float4*)(rowf + (size_t)g * 4);
      const float ve[4] = {v.x, v.y, v.z, v.w};
      float w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool keep = g * 4 + e < V && sample_key(ve[e]) >= tau;
        w[e] = keep ? expf(ve[e] - ymax) : 0.f;
        if (w[e] < min_p) { keep = false; w[e] = 0.f; }
        if (keep) last = g * 4 + e;
      }
      csum += (w[0] + w[1]) + (w[2] + w[3]);
    }
    float incl, total;
    const float excl = block_excl_scan<float>(csum, s_wf, &incl, &total);
    const int n = p.step + (p.cache_len != nullptr ? p.cache_len[b] + p.advance - (p.start_len ? p.start_len[b] : 0) : 0);
    const unsigned x0 = philox4x32_10_word0((unsigned)n, ctr1, off_lo, off_hi, seed_lo, seed_hi);
    const float target = (float)((((double)(x0 >> 8)) + 0.5) * (1.0 / 16777216.0) * (double)total);
    if (csum > 0.f && incl > target) atomicMin(&s_owner, tid);
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    if (tid == s_owner) {
      float run = 0.f;
      int pick = -1, lastpos = -1;
      for (int g = g0; g < g1 && pick < 0; ++g) {
        const float4 v = *(const float4*)(rowf + (size_t)g * 4);
        const float ve[4] = {v.x, v.y, v.z, v.w};
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          w[e] = (g * 4 + e < V && sample_key(ve[e]) >= tau) ? expf(ve[e] - ymax) : 0.f;
          if (w[e] < min_p) w[e] = 0.f;
        }
        const float c[4] = {w[0], w[0] + w[1], (w[0] + w[1]) + w[2], (w[0] + w[1]) + (w[2] + w[3])};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!(w[e] > 0.f)) continue;
          lastpos = g * 4 + e;
          if (pick < 0 && excl + (run + c[e]) > target) pick = g * 4 + e;
        }
        run += c[3];
      }
      s_tok = pick >= 0 ? pick : lastpos;
    }
    __syncthreads();
    tok = s_owner == 0x7fffffff ? s_last : s_tok;
    if (probs) {
      for (int i = tid; i < V; i += PICK_THREADS) {
        const float y = rowf[i];
        const float w = sample_key(y) >= tau ? expf(y - ymax) : 0.f;
        probs[i] = (w > 0.f && w >= min_p) ? w / total : 0.f;
      }
    }
  }
  pick_finish(p, b, was_done, len0, start0, eos4, tok, &q.c, cs, cr);
}

template <bool ROWS>
__global__ __launch_bounds__(PICK_THREADS) void sample_pick_kernel(const PickParams p, const ProcParams q, const typename SampleArgs<ROWS>::type sp) {
  sample_pick_body<ROWS>(p, q, sp);
}

// ---- per-row logits processors (generate_many: every slot serves a request with settings of its own).  The distinct settings of a call
// are a small pool of fixed-size records; row b names its record in row_set[b], a device int the launch reads, so a captured step serves
// a row whose settings are replaced in place between replays.  A record is PROC_SET_WORDS 32-bit words:
//   0 penalty (the float's bits)  1 ngram  2 min_len  3..4 suppress ids [sup0, sup1)  5..6 begin-suppress ids [bsup0, bsup1)
//   7..8 bad words [word0, word1)
// The id ranges index `ids` (n_ids entries: every set's lists one behind the other); a word w is ids[bad_off[w], bad_off[w + 1]), bad_off
// holding n_words + 1 ascending offsets.  Nothing validates the arrays on the device, so bad bits stay inside their row: a set index
// outside [0, n_sets) is the neutral set, ranges are cut at the pools' ends, a penalty that is not finite and positive is 1, and
// process_row skips ids outside [0, V) and cuts bad_off itself.  One workgroup serves one row and every thread reads the same words, so
// what process_row branches on around its barriers stays workgroup-uniform; the words are moved to scalar registers to say so.
// (PROC_SET_WORDS and ProcSetParams: pick_params.h)

// q with row b's record in the place of the call-wide processor values (q's own are ignored)
__device__ __forceinline__ ProcParams proc_row_params(const ProcParams& q, const ProcSetParams& ps, int b) {
  ProcParams r = q;
  r.penalty = 1.f; r.ngram = 0; r.min_len = 0;
  r.suppress = nullptr; r.n_suppress = 0; r.begin_suppress = nullptr; r.n_begin = 0;
  r.bad_ids = ps.ids; r.bad_off = ps.bad_off; r.n_bad = 0; r.n_bad_ids = ps.n_ids;
  const int si = __builtin_amdgcn_readfirstlane(ps.row_set[b]);
  if (si < 0 || si >= ps.n_sets) return r;
  const int* rec = ps.sets + (size_t)si * PROC_SET_WORDS;
  int w[PROC_SET_WORDS];
#pragma unroll
  for (int i = 0; i < PROC_SET_WORDS; ++i) w[i] = __builtin_amdgcn_readfirstlane(rec[i]);
  const float pen = __int_as_float(w[0]);
  r.penalty = (pen > 0.f && pen <= 3.0e38f) ? pen : 1.f;   // what the scalar entry points accept; NaN fails both
  r.ngram = max(w[1], 0);
  r.min_len = w[2];
  const int s0 = min(max(w[3], 0), ps.n_ids), s1 = min(max(w[4], s0), ps.n_ids);
  const int b0 = min(max(w[5], 0), ps.n_ids), b1 = min(max(w[6], b0), ps.n_ids);
  const int w0 = min(max(w[7], 0), ps.n_words), w1 = min(max(w[8], w0), ps.n_words);
  r.suppress = ps.ids + s0; r.n_suppress = s1 - s0;
  r.begin_suppress = ps.ids + b0; r.n_begin = b1 - b0;
  r.bad_off = ps.bad_off + w0; r.n_bad = w1 - w0;          // bad_off[w1] exists: n_words + 1 offsets
  return r;
}

__global__ __launch_bounds__(PROC_THREADS) void logits_process_rows_kernel(const ProcParams q, const ProcSetParams ps) {
  __shared__ unsigned s_bits[PROC_MAX_V / 32];
  const ProcParams r = proc_row_params(q, ps, blockIdx.x);
  process_row(r, blockIdx.x, r.out + (size_t)blockIdx.x * r.ld_out, s_bits);
}

__global__ __launch_bounds__(PICK_THREADS) void greedy_pick_rows_kernel(const PickParams p, const ProcParams q, const ProcSetParams ps) {
  __shared__ unsigned s_bits[PROC_MAX_V / 32];
  const ProcParams r = proc_row_params(q, ps, blockIdx.x);
  float* rowf = r.out + (size_t)blockIdx.x * r.ld_out;
  process_row(r, blockIdx.x, rowf, s_bits);
  greedy_pick_row<true>(p, rowf, &r.c);
}

__global__ __launch_bounds__(PICK_THREADS) void sample_pick_rows_processed_kernel(const PickParams p, const ProcParams q, const ProcSetParams ps,
                                                                                  const SampleRowParams sp) {
  const ProcParams r = proc_row_params(q, ps, blockIdx.x);
  sample_pick_body<true>(p, r, sp);
}


// ---- the two launchers (api.hip has checked the arguments) ----------------------------------------------------------------------------
// aki_logits_process*: ps == nullptr is the call-wide form; with ps the processor values of q are placeholders, proc_row_params fills them
// per row, and a NULL table is "no constraint"
int logits_process_call_launch(const ProcParams& q_in, const ProcSetParams* ps, int B, hipStream_t s) {
  ProcParams q = q_in;
  if (q.c.table == nullptr) q.c = ConstraintParams{};
  AKI_CLEAR_ERR();
  if (ps != nullptr) hipLaunchKernelGGL(logits_process_rows_kernel, dim3(B), dim3(PROC_THREADS), 0, s, q, *ps);
  else hipLaunchKernelGGL(logits_process_kernel, dim3(B), dim3(PROC_THREADS), 0, s, q);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// every aki_greedy_pick* / aki_sample_pick*: one of the six pick kernels, chosen by what the descriptor holds
int pick_call_launch(const PickCall& c, hipStream_t s) {
  const PickParams& p = c.p;
  ProcParams q = c.q;
  // the processors see the tokens generated BEFORE this pick: n = step + cache_len + advance - start_len, the index the pick writes
  q.step = p.step + (p.cache_len ? p.advance : 0);
  if (q.c.table == nullptr) q.c = ConstraintParams{};     // the "or none" kinds: a NULL table is no constraint, whatever stands behind it
  const dim3 grid(p.B), block(PICK_THREADS);
  AKI_CLEAR_ERR();
  if (!c.processed) {
    hipLaunchKernelGGL(greedy_pick_kernel, grid, block, 0, s, p);
  } else if (c.sampler == SAMPLER_NONE) {
    if (c.sets) hipLaunchKernelGGL(greedy_pick_rows_kernel, grid, block, 0, s, p, q, c.ps);
    else hipLaunchKernelGGL(greedy_pick_processed_kernel, grid, block, 0, s, p, q);
  } else if (c.sets) {
    // processed = 1: which rows have something to process is the device's to know; the neutral set's row is the plain f32 copy
    SampleRowParams sr = c.sr;
    sr.processed = 1;
    hipLaunchKernelGGL(sample_pick_rows_processed_kernel, grid, block, 0, s, p, q, c.ps, sr);
  } else {
    const bool processed = q.penalty != 1.f || q.ngram > 0 || q.n_bad > 0 || (q.min_len > 0 && q.n_eos > 0) || q.n_suppress > 0 ||
                           q.n_begin > 0 || q.c.table != nullptr || q.freq != nullptr || q.pres != nullptr;
    if (c.sampler == SAMPLER_ROWS) {                        // the per-row form: the four arrays stand in for the scalars
      SampleRowParams sr = c.sr;
      sr.processed = processed ? 1 : 0;
      hipLaunchKernelGGL(sample_pick_kernel<true>, grid, block, 0, s, p, q, sr);
    } else {
      SampleParams sp = c.sp;
      sp.processed = processed ? 1 : 0;
      hipLaunchKernelGGL(sample_pick_kernel<false>, grid, block, 0, s, p, q, sp);
    }
  }
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

}  // namespace aki



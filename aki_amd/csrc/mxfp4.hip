// mxfp4.hip - opt-in MXFP4 weight-only decode (OCP microscaling: e2m1 elements, one e8m0 scale byte per block of 32 k).
//
// Decode is bound by weight bytes; e4m3 weights (decode.hip, W8) stop at 8 bits per weight, this format takes 4.25:
//   wq [N, K/2] bytes   byte j of a row = k 2j in the low nibble, k 2j+1 in the high nibble; a nibble = sign (bit 3) + e2m1 code
//                       (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6)
//   ws [N, K/32] bytes  e8m0: the block's values are nibble * 2^(byte - 127)
//   mxfp4_quant_kernel      bf16 [N, K] -> wq, ws (once per weight): e = floor(log2(amax)) - 2, byte = clamp(e + 127, 0, 254),
//                           v / 2^e rounded to the nearest e2m1 value, ties to the even code, saturating at +-6; a zero block = byte 127
//   gemv_w4_kernel          one row (M = 1): gemv_bf16_kernel<W8>'s structure - x in LDS, a wave owns FPW features, a lane's 16-byte weight
//                           chunk is 32 k = exactly one block = one scale byte, and meets four 16-byte x chunks
//   skinny_gemm_w4_kernel   2 <= M <= 16: skinny_gemm_w8_kernel's tile, K split and v_mfma_f32_16x16x32_bf16
// v_cvt_scalef32_pk_bf16_fp4 turns two nibbles into a bf16 pair in one instruction; the block scale rides in its scale operand (an exact
// power of two: e2m1 x 2^e has two significant bits, so the bf16 pair IS the dequantised weight) - one convert and one dot2 (or a quarter of
// an MFMA operand) per two weights, the VALU work per weight of the W8 kernels over half the bytes.
// Activations, accumulation (f32) and the epilogues (bias, GELU, SwiGLU, residual) are those of the bf16 / W8 kernels.
#include <type_traits>

#include "aki_device.h"
#include "weight_dot.h"

namespace aki {

struct W4Params {
  const bf16_t* x; const uint8_t* w; const uint8_t* ws; const bf16_t* bias; const bf16_t* residual; bf16_t* y;
  const bf16_t* norm_w; float norm_eps;       // optional fused RMSNorm of the x rows
  int M, N, K, ldx, ldw, ldy, ldr, res_row_mod, act;      // ldw in bytes; ws rows are K / 32 bytes, dense
};

// ---- quantiser ---------------------------------------------------------------------------------------------------------------------
// One thread = one block of 32 k: 64 bytes of bf16 in, 16 bytes of nibbles + one scale byte out.  Integer arithmetic on the bf16 bits for the
// exponent (no log2), exact power-of-two scaling (v_ldexp_f32) and exact comparisons against the e2m1 midpoints for the elements: bit-exact
// against the f64 reference whatever the values.
__global__ __launch_bounds__(256) void mxfp4_quant_kernel(const bf16_t* w, uint8_t* wq, uint8_t* ws, int N, int K, int ld) {
  const int nblk = K / 32;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (size_t)N * nblk) return;
  const int row = (int)(gid / nblk), blk = (int)(gid - (size_t)row * nblk);
  const bf16_t* src = w + (size_t)row * ld + (size_t)blk * 32;
  u32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = *(const u32x4*)(src + 8 * i);
  unsigned amax = 0;                                       // largest magnitude as bf16 bits (monotonic in the value for finite inputs)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) amax = max(amax, max(v[i][e] & 0x7fffu, (v[i][e] >> 16) & 0x7fffu));
  u32x4 out = {0u, 0u, 0u, 0u};
  int byte = 127;
  if (amax != 0) {
    const int ef = (int)(amax >> 7), man = (int)(amax & 0x7f);
    const int fl = ef > 0 ? ef - 127 : (31 - __builtin_clz((unsigned)man)) - 133;      // floor(log2(amax)); bf16 subnormals: man * 2^-133
    byte = min(max(fl - 2 + 127, 0), 254);
    const int sh = 127 - byte;                             // v * 2^sh = v / 2^e
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned word = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned bits = (e & 1) ? (v[i][e >> 1] >> 16) : (v[i][e >> 1] & 0xffffu);
        const float a = __builtin_ldexpf(__builtin_bit_cast(float, (bits & 0x7fffu) << 16), sh);
        // midpoints between neighbouring e2m1 magnitudes; a tie goes to the even code (0, 1, 2, 4 and 4 of the pairs below)
        const unsigned code = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) +
                              (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
        word |= (code | ((bits >> 15) << 3)) << (4 * e);
      }
      out[i] = word;
    }
  }
  *(u32x4*)(wq + (size_t)row * (K / 2) + (size_t)blk * 16) = out;
  ws[(size_t)row * nblk + blk] = (uint8_t)byte;
}

int quant_mxfp4_launch(const void* w, int N, int K, int ldw, uint8_t* wq, uint8_t* ws, hipStream_t s) {
  if (K % 32 || (ldw % 8)) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)w & 15) || ((uintptr_t)wq & 15)) return AKI_ERR_ALIGNMENT;
  const size_t blocks = ((size_t)N * (K / 32) + 255) / 256;
  if (blocks > 0x7fffffffu) return AKI_ERR_UNSUPPORTED;
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL(mxfp4_quant_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)w, wq, ws, N, K, ldw);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// U chunks (of 32 k) per lane for NR weight rows: every weight load and scale byte is requested before the first dot product
template <int NR, int U>
__device__ __forceinline__ void gemv_sweep_w4(const uint8_t* const (&wr)[NR], const uint8_t* const (&sr)[NR], const char* sx, int c, float (&acc)[NR]) {
  u32x4 w[U][NR];
  unsigned sc[U][NR];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      w[u][r] = __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)(c + 64 * u) * 16));
      sc[u][r] = sr[r][c + 64 * u];
    }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    u32x4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = *(const u32x4*)(sx + ((size_t)4 * (c + 64 * u) + i) * 16);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = dot32_w4(w[u][r], w4_scale(sc[u][r]), x, acc[r]);
  }
}

// FPW output features per wave; SWIGLU: feature f pairs weight rows f (gate) and N/2 + f (up).  One workgroup = one group of 4 x FPW features.
template <bool SWIGLU, int FPW = 2>
__global__ __launch_bounds__(256) void gemv_w4_kernel(const W4Params p) {
  constexpr int NR = SWIGLU ? 2 * FPW : FPW;   // weight rows per wave
  extern __shared__ __attribute__((aligned(16))) char sx[];
  __shared__ float s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunk = p.K / 8;
  if (p.norm_w == nullptr) {
    for (int c = tid; c < nchunk; c += 256) *(u32x4*)(sx + (size_t)c * 16) = *(const u32x4*)(p.x + (size_t)c * 8);
  } else {
    // y = bf16(x * rsqrt(mean(x^2) + eps) * w): same rounding points as norm_bf16_kernel<true> (aux_kernels.hip)
    float ss = 0.f;
    for (int c = tid; c < nchunk; c += 256) {
      const u32x4 v = *(const u32x4*)(p.x + (size_t)c * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = bf16_lo(v[e]), hi = bf16_hi(v[e]);
        ss = __builtin_fmaf(lo, lo, ss);
        ss = __builtin_fmaf(hi, hi, ss);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == 0) s_red[wave] = ss;
    __syncthreads();
    const float r = rsqrtf((s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (float)p.K + p.norm_eps);
    for (int c = tid; c < nchunk; c += 256) {
      const u32x4 v = *(const u32x4*)(p.x + (size_t)c * 8);
      const u32x4 g = *(const u32x4*)(p.norm_w + c * 8);
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e)      // HF Phi3RMSNorm: weight * (x * rstd).to(bf16)
        o[e] = pack_bf16x2(round_bf16(bf16_lo(v[e]) * r) * bf16_lo(g[e]), round_bf16(bf16_hi(v[e]) * r) * bf16_hi(g[e]));
      *(u32x4*)(sx + (size_t)c * 16) = o;
    }
  }
  __syncthreads();
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  const int f0 = (blockIdx.x * 4 + wave) * FPW;
  if (f0 >= n_out) return;
  const int nblk = p.K / 32;                               // 16-byte weight chunks = blocks of 32 k
  float acc[NR];
  const uint8_t* wr[NR];
  const uint8_t* sr[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    acc[r] = 0.f;
    const int f = min(f0 + (r % FPW), n_out - 1);
    const int row = (SWIGLU && r >= FPW) ? n_out + f : f;
    wr[r] = p.w + (size_t)row * p.ldw;
    sr[r] = p.ws + (size_t)row * nblk;
  }
  int c = lane;
  for (; c + 64 * 3 < nblk; c += 64 * 4) gemv_sweep_w4<NR, 4>(wr, sr, sx, c, acc);
  for (; c + 64 < nblk; c += 128) gemv_sweep_w4<NR, 2>(wr, sr, sx, c, acc);
  for (; c < nblk; c += 64) gemv_sweep_w4<NR, 1>(wr, sr, sx, c, acc);
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o);
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
      const int n = f0 + f;
      if (n >= n_out) continue;
      float v;
      if (SWIGLU) {
        v = acc[FPW + f] * silu_fast(acc[f]);
      } else {
        v = acc[f];
        if (p.bias) v += bf16_bits_to_f32(p.bias[n]);
        if (p.act == AKI_ACT_GELU_ERF) v = gelu_erf_fast(v);
        else if (p.act == AKI_ACT_GELU_TANH) v = gelu_tanh_fast(v);
      }
      if (p.residual) v += bf16_bits_to_f32(p.residual[n]);     // one row: res_row_mod selects row 0 whatever its value
      ((__bf16*)p.y)[n] = (__bf16)v;
    }
  }
}

template <bool SWIGLU>
static int launch_gemv_w4(const W4Params& p, hipStream_t stream) {
  constexpr int FPW = 2;
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  const dim3 grid((n_out + 4 * FPW - 1) / (4 * FPW)), block(256);
  static bool set = false;
  if (!set) {
    if (hipFuncSetAttribute((const void*)gemv_w4_kernel<SWIGLU, FPW>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 8192 * 2) != hipSuccess)
      return AKI_ERR_LAUNCH;
    set = true;
  }
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL((gemv_w4_kernel<SWIGLU, FPW>), grid, block, (size_t)p.K * 2, stream, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

static W4Params w4_params(const aki_linear_args* a, const uint8_t* ws, const void* rms_w, float eps) {
  return W4Params{(const bf16_t*)a->x, (const uint8_t*)a->w, ws, (const bf16_t*)a->bias, (const bf16_t*)a->residual, (bf16_t*)a->y,
                  (const bf16_t*)rms_w, eps, a->M, a->N, a->K, a->ldx, a->ldw, a->ldy, a->ldr, a->res_row_mod, a->act};
}

// M = 1 on MXFP4 weights: K a multiple of 32 with the row in 128 KiB of LDS, rows of w 16-byte aligned.  AKI_ERR_UNSUPPORTED otherwise.
int gemv_w4(const aki_linear_args* a, const uint8_t* ws, const void* rms_w, float eps, hipStream_t stream) {
  if (a->M != 1 || a->K % 32 || (size_t)a->K * 2 > 8 * 8192 * 2 || (a->ldx % 8) || (a->ldw % 16)) return AKI_ERR_UNSUPPORTED;
  if (a->act == AKI_ACT_SWIGLU && (a->bias || (a->N & 1))) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)a->x & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)rms_w & 15)) return AKI_ERR_ALIGNMENT;
  const W4Params p = w4_params(a, ws, rms_w, eps);
  return a->act == AKI_ACT_SWIGLU ? launch_gemv_w4<true>(p, stream) : launch_gemv_w4<false>(p, stream);
}

// ------------------------------------------------------------------------------------------------------------
// The skinny GEMM on MXFP4 weights for 2 <= M <= 16.  skinny_gemm_w8_kernel's tile (one workgroup = 16 features, KS waves split K, lane =
// (row l15, k-group kg)) and its step of 128 k, so the same K gates hold.  A lane streams 16 BYTES of its weight row per step = 32 k = ONE whole
// block with one scale byte: the four k-groups of a row then read 64 contiguous bytes, so each load instruction of a wave covers sixteen
// 64-byte segments with every byte used, and the two steps that share a 128-byte line are requested back to back in one unrolled group.  32 bytes
// per step (two blocks, a whole line per row and step) was the alternative: it doubles the step to 256 k, which K / KS of the model's shapes
// (3072 / 4 = 768 fits, 5120 / 8 = 640 does not) would need a half step for, and buys nothing per instruction (a lane's load is 16 bytes
// either way).  The bytes in flight match the W8 kernel's instead through the unroll: 8 (4 with SwiGLU's two streams) steps per group.
// The nibbles widen to bf16 pairs in registers (v_cvt_scalef32_pk_bf16_fp4 with the block's scale: exact); dword j of the 16 bytes = k 8j .. 8j+7
// of the lane's 32 feeds MFMA j against the x bytes that carry the same k.  NORM: as in skinny_gemm_bf16_kernel.
// ------------------------------------------------------------------------------------------------------------
template <int KS, bool SWIGLU, bool NORM>
__global__ __launch_bounds__(KS * 64) void skinny_gemm_w4_kernel(const W4Params p) {
  constexpr int NS = SWIGLU ? 2 : 1;
  constexpr int UN = SWIGLU ? 4 : 8;                 // steps of 128 k whose weight loads are issued together
  __shared__ float red_st[NORM ? 1 : KS][NS][256];
  extern __shared__ __attribute__((aligned(16))) char s_xn[];
  float (*red)[NS][256] = NORM ? (float (*)[NS][256])s_xn : red_st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kg = lane >> 4;
  const int n_out = SWIGLU ? p.N / 2 : p.N;
  const int f0 = blockIdx.x * 16;
  const int Kw = p.K / KS, kbeg = wave * Kw, nblk = p.K / 32;
  const int frow = min(f0 + l15, n_out - 1);
  const uint8_t* wp[NS];
  const uint8_t* sp[NS];
  wp[0] = p.w + (size_t)frow * p.ldw + (kbeg + 32 * kg) / 2;
  sp[0] = p.ws + (size_t)frow * nblk + kbeg / 32 + kg;
  if (SWIGLU) {
    wp[NS - 1] = p.w + (size_t)(n_out + frow) * p.ldw + (kbeg + 32 * kg) / 2;
    sp[NS - 1] = p.ws + (size_t)(n_out + frow) * nblk + kbeg / 32 + kg;
  }
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
      u32x4 wa[U][NS];
      unsigned sc[U][NS];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < NS; ++t) {
          wa[u][t] = __builtin_nontemporal_load((const u32x4*)(wp[t] + (size_t)(it + u) * 64));
          sc[u][t] = sp[t][(it + u) * 4];
        }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 xa[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xa[j] = NORM ? *(const u32x4*)(xs + (size_t)(it + u) * 256 + 16 * j) : *(const u32x4*)(xr + (size_t)(it + u) * 128 + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // k-values 8j .. 8j+7 of the lane's 32: nibble dword j of the 16 bytes
          const bf16x8 xb = __builtin_bit_cast(bf16x8, xa[j]);
#pragma unroll
          for (int t = 0; t < NS; ++t) {
            const unsigned d = wa[u][t][j];
            const float s = w4_scale(sc[u][t]);
            const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
            const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
            const u32x4 wq = u32x4{__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1), __builtin_bit_cast(unsigned, p2), __builtin_bit_cast(unsigned, p3)};
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq), xb, acc[t], 0, 0, 0);
          }
        }
      }
    }
  };
  run(std::integral_constant<int, UN>{});
  if constexpr (UN > 4) run(std::integral_constant<int, 4>{});
  run(std::integral_constant<int, 2>{});
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
      v[r] = acc[NS - 1][r] * silu_fast(acc[0][r]);
    } else {
      v[r] = acc[0][r];
      if (p.bias) v[r] += bf16_bits_to_f32(p.bias[f + r]);
      if (p.act == AKI_ACT_GELU_ERF) v[r] = gelu_erf_fast(v[r]);
      else if (p.act == AKI_ACT_GELU_TANH) v[r] = gelu_tanh_fast(v[r]);
    }
    if (p.residual) v[r] += bf16_bits_to_f32(p.residual[(size_t)(p.res_row_mod > 0 ? tok % p.res_row_mod : tok) * p.ldr + f + r]);
  }
  *(u32x2*)(p.y + (size_t)tok * p.ldy + f) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

template <int KS, bool NORM>
static int launch_skinny_w4(const W4Params& p, hipStream_t stream) {
  const int n_out = p.act == AKI_ACT_SWIGLU ? p.N / 2 : p.N;
  const dim3 grid((n_out + 15) / 16), block(KS * 64);
  constexpr size_t RED = (size_t)KS * 2 * 1024;
  const size_t rows = (size_t)p.M * ((size_t)p.K * 2 + 16);
  const size_t smem = NORM ? (rows > RED ? rows : RED) : 0;
  if constexpr (NORM) {
    static bool set_s = false, set_p = false;
    bool& set = p.act == AKI_ACT_SWIGLU ? set_s : set_p;
    if (!set) {
      const void* fn = p.act == AKI_ACT_SWIGLU ? (const void*)skinny_gemm_w4_kernel<KS, true, true> : (const void*)skinny_gemm_w4_kernel<KS, false, true>;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * (8192 * 2 + 16)) != hipSuccess) return AKI_ERR_LAUNCH;
      set = true;
    }
  }
  AKI_CLEAR_ERR();
  if (p.act == AKI_ACT_SWIGLU) hipLaunchKernelGGL((skinny_gemm_w4_kernel<KS, true, NORM>), grid, block, smem, stream, p);
  else hipLaunchKernelGGL((skinny_gemm_w4_kernel<KS, false, NORM>), grid, block, smem, stream, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

// 2 <= M <= 16 rows on MXFP4 weights; the gates of skinny_gemm_w8: K a multiple of 128 per wave, rows of w 16-byte aligned, N_out % 4 == 0.
int skinny_gemm_w4(const aki_linear_args* a, const uint8_t* ws, const void* rms_w, float eps, hipStream_t stream) {
  const int n_out = a->act == AKI_ACT_SWIGLU ? a->N / 2 : a->N;
  if (a->M < 2 || a->M > 16 || (a->ldx % 8) || (a->ldw % 16) || (n_out % 4) || (a->ldy % 4) || (a->residual && (a->ldr % 4)))
    return AKI_ERR_UNSUPPORTED;
  if (a->act == AKI_ACT_SWIGLU && (a->bias || (a->N & 1))) return AKI_ERR_UNSUPPORTED;
  if (rms_w && (a->M > 8 || a->K > 8192)) return AKI_ERR_UNSUPPORTED;
  if (((uintptr_t)a->x & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->y & 7) || ((uintptr_t)a->bias & 7) || ((uintptr_t)rms_w & 15)) return AKI_ERR_ALIGNMENT;
  const W4Params p = w4_params(a, ws, rms_w, eps);
  const int tiles = (n_out + 15) / 16;
  const bool k8 = a->K % 1024 == 0 && a->K / 8 >= 512, k4 = a->K % 512 == 0;
  if (rms_w) {
    if (tiles >= 1536) return AKI_ERR_UNSUPPORTED;      // lm_head-wide outputs keep the norm launch (see skinny_gemm_bf16)
    if (k8 && tiles < 768) return launch_skinny_w4<8, true>(p, stream);
    if (k4) return launch_skinny_w4<4, true>(p, stream);
    return AKI_ERR_UNSUPPORTED;
  }
  if (k8 && tiles < 768) return launch_skinny_w4<8, false>(p, stream);
  if (k4 && tiles < 1536) return launch_skinny_w4<4, false>(p, stream);
  if (a->K % 256 == 0) return launch_skinny_w4<2, false>(p, stream);
  return AKI_ERR_UNSUPPORTED;
}

}  // namespace aki

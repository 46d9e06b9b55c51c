// weight_dot.h - the per-lane dot products of the decode path: one 16-byte chunk of a bf16 / e4m3 / MXFP4 row against bf16 activations, into one
// f32.  Shared by decode.hip, mxfp4.hip, the split-KV attention core (decode_attn_common.h) and the one-launch chain (decode_chain.hip), whose
// outputs are compared bit for bit: the pairing and the order of the dot2 instructions they share is this text.
#pragma once
#include "aki_device.h"

namespace aki {

// NB: indexing the u32x4 and bit-casting each dword (bit_cast<bf16x2>(a[i])) is folded by hipcc 7.2 into four uses of
// dword 0; viewing the whole 16 bytes as bf16x8 and slicing pairs with shufflevector selects the right operands.
__device__ __forceinline__ float dot8_bf16(const u32x4 a, const u32x4 b, float acc) {
  const bf16x8 a8 = __builtin_bit_cast(bf16x8, a), b8 = __builtin_bit_cast(bf16x8, b);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a8, a8, 0, 1), __builtin_shufflevector(b8, b8, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a8, a8, 2, 3), __builtin_shufflevector(b8, b8, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a8, a8, 4, 5), __builtin_shufflevector(b8, b8, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(a8, a8, 6, 7), __builtin_shufflevector(b8, b8, 6, 7), acc, false);
  return acc;
}

// weight-only fp8 (e4m3 weights, bf16 activations): a 16-byte weight chunk holds 16 k-values and meets two 16-byte x chunks;
// v_cvt_scalef32_pk_bf16_fp8 (scale 1) turns two weights into a bf16 pair in one instruction (exact: e4m3 fits bf16) for the same dot2:
// 16 VALU operations per 16 weights (until round 5: v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 + dot2 = 24, and the e4m3 decode was VALU-bound).
__device__ __forceinline__ float dot16_w8(const u32x4 w, const u32x4 x0, const u32x4 x1, float acc) {
  const bf16x8 xa = __builtin_bit_cast(bf16x8, x0), xb = __builtin_bit_cast(bf16x8, x1);
#define AKI_W8_PAIR(word, hi, xv, i0)                                                                               \
  {                                                                                                                 \
    const bf16x2 wb = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((unsigned)(word), 1.0f, hi);   /* two e4m3 -> a bf16 pair in ONE instruction, exact */ \
    acc = __builtin_amdgcn_fdot2_f32_bf16(wb, __builtin_shufflevector(xv, xv, i0, i0 + 1), acc, false);             \
  }
  AKI_W8_PAIR(w[0], false, xa, 0) AKI_W8_PAIR(w[0], true, xa, 2) AKI_W8_PAIR(w[1], false, xa, 4) AKI_W8_PAIR(w[1], true, xa, 6)
  AKI_W8_PAIR(w[2], false, xb, 0) AKI_W8_PAIR(w[2], true, xb, 2) AKI_W8_PAIR(w[3], false, xb, 4) AKI_W8_PAIR(w[3], true, xb, 6)
#undef AKI_W8_PAIR
  return acc;
}

// MXFP4: the scale operand of the convert - an f32 whose exponent field is the e8m0 byte, i.e. 2^(byte - 127)
__device__ __forceinline__ float w4_scale(unsigned byte) { return __builtin_bit_cast(float, byte << 23); }

// one block: 16 bytes of nibbles (32 k) against four 16-byte x chunks; dword i of w carries k 8i .. 8i+7 = x chunk i
__device__ __forceinline__ float dot32_w4(const u32x4 w, const float scale, const u32x4 (&x)[4], float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x8 xv = __builtin_bit_cast(bf16x8, x[i]);
#define AKI_W4_PAIR(sel, i0)                                                                                      \
  {                                                                                                               \
    const bf16x2 wb = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[i], scale, sel);   /* byte sel: low nibble -> element 0, high -> 1 */ \
    acc = __builtin_amdgcn_fdot2_f32_bf16(wb, __builtin_shufflevector(xv, xv, i0, i0 + 1), acc, false);           \
  }
    AKI_W4_PAIR(0, 0) AKI_W4_PAIR(1, 2) AKI_W4_PAIR(2, 4) AKI_W4_PAIR(3, 6)
#undef AKI_W4_PAIR
  }
  return acc;
}

}  // namespace aki

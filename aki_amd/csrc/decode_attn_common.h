// decode_attn_common.h - the split-KV decode attention core (bf16 queries, Dh = 96) shared by decode.hip (the split, fp8-cache and
// grouped kernels) and decode_chain.hip (the attention phase of the one-launch chain): the host rule that cuts a cache into items,
// the partial an item leaves in the workspace, the ticket that elects the merger, the merge arithmetic, rotate-half RoPE and the bf16
// fused item.  The outputs of these kernels are compared bit for bit (aki_device.h); the order of operations they share is this text.
#pragma once
#include "aki_device.h"
#include "weight_dot.h"      // dot8_bf16: the score of one key

namespace aki {

// ---- host: how a cache is cut into items ---------------------------------------------------------------------------------------
// Every row (one query against one K/V slab of `cap` keys, `rows` of them in the launch) is cut into S items of T 64-key tiles.
// Tiles per item from the cache CAPACITY, items per row from max_keys (a host-side upper bound of the keys any row holds; <= 0 or
// > cap means cap): a launch sized for the keys cached so far (eager steps) and one sized for the whole cache (a captured step)
// then cut the keys at the same places and differ only by trailing empty items, whose partials (m = -inf, l = 0) fold exactly -
// eager and replayed steps give the same bits at any cache size.
static inline void split_plan(size_t rows, int cap, int max_keys, int& S, int& T) {
  if (max_keys <= 0 || max_keys > cap) max_keys = cap;
  const int tiles = (max_keys + 63) / 64, tiles_cap = (cap + 63) / 64;
  T = (int)((rows * tiles_cap + AKI_DEC_ITEMS - 1) / AKI_DEC_ITEMS);
  if (T < 1) T = 1;
  S = (tiles + T - 1) / T;
}

// ---- the partial of one item: m, l, 6 pad, acc[96] -----------------------------------------------------------------------------
constexpr int DEC_PSTRIDE = 104;

// Partials travel between workgroups (possibly on different XCDs, i.e. different L2s) as agent-scope relaxed atomic
// stores / loads: those carry sc1 and are written through / read past the non-coherent levels.  A __threadfence()
// here would instead make every workgroup write back and invalidate its whole L2 (buffer_wbl2 + buffer_inv).
#define AKI_ST_AGENT(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AKI_LD_AGENT(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AKI_ADD_AGENT(ptr, v) __hip_atomic_fetch_add((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// lane < 96 / CPL holds columns CPL * lane .. CPL * lane + CPL - 1 of acc (bf16 cache: 12 lanes x 8, e4m3 cache: 6 lanes x 16)
template <int CPL>
__device__ __forceinline__ void split_publish(float* part, float m, float l, const float (&acc)[CPL], int lane) {
  if (lane == 0) { AKI_ST_AGENT(part, m); AKI_ST_AGENT(part + 1, l); }
  if (lane < 96 / CPL) {
#pragma unroll
    for (int e = 0; e < CPL; ++e) AKI_ST_AGENT(part + 8 + lane * CPL + e, acc[e]);
  }
}

// one arrival at the row's counter once the wave's published stores have reached the coherence point; the arrivals before it, in every lane
__device__ __forceinline__ unsigned split_ticket(unsigned* cnt, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned prev = 0;
  if (lane == 0) prev = AKI_ADD_AGENT(cnt, 1u);
  return __shfl(prev, 0);
}

// ---- the merge by the last arriver ----------------------------------------------------------------------------------------------
// lane = (split slot sl = lane / 12 in 0..4, column chunk ch = lane % 12): slot sl folds partials sl, sl + 5, ... in order into a running
// (gm, lt, o8), five partials in flight per pass (each is a round trip to memory); the five slots then meet through 5 x 12 x 10 floats
// of LDS, where lanes 0..11 combine them in slot order.  A trailing empty partial (m = -inf, l = 0) changes nothing in either step.
constexpr int DEC_MERGE_FLOATS = 5 * 12 * 10;

__device__ __forceinline__ void split_fold(float& gm, float& lt, float (&o8)[8], float ms, float ls, const float (&a)[8]) {
  const float mn = fmaxf(gm, ms);
  const float f0 = gm == -INFINITY ? 0.f : __expf(gm - mn), f1 = ms == -INFINITY ? 0.f : __expf(ms - mn);
  lt = lt * f0 + ls * f1;
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = o8[e] * f0 + a[e] * f1;
  gm = mn;
}

__device__ __forceinline__ void split_slot_store(float* s_mg, int sl, int ch, float gm, float lt, const float (&o8)[8]) {
  float* sm = s_mg + (sl * 12 + ch) * 10;
  sm[0] = gm;
  sm[1] = lt;
#pragma unroll
  for (int e = 0; e < 8; ++e) sm[2 + e] = o8[e];
}

// lane < 12, after the barrier that follows split_slot_store: the lane's eight output columns, normalised and packed to bf16
__device__ __forceinline__ u32x4 split_finish(const float* s_mg, int lane) {
  float sv[50];
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int e = 0; e < 10; ++e) sv[q * 10 + e] = s_mg[(q * 12 + lane) * 10 + e];
  lds_fold_ready(sv);
  float M5 = -INFINITY;
#pragma unroll
  for (int q = 0; q < 5; ++q) M5 = fmaxf(M5, sv[q * 10]);
  float lt = 0.f, o8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = 0.f;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const float mq = sv[q * 10];
    const float f = mq == -INFINITY ? 0.f : __expf(mq - M5);
    lt += sv[q * 10 + 1] * f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] += sv[q * 10 + 2 + e] * f;
  }
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  u32x4 ov;
#pragma unroll
  for (int e = 0; e < 4; ++e) ov[e] = pack_bf16x2(o8[2 * e] * inv, o8[2 * e + 1] * inv);
  return ov;
}

// The whole (single-wave) workgroup calls it: partials [0, n0) and then [n0, n0 + n1) of pp -> the 96 bf16 outputs at o.  Each segment is
// strided over the five slots on its own, so trailing empty items of either fold exactly (n1 = 0: one segment).
__device__ __forceinline__ void split_merge(const float* pp, int n0, int n1, int lane, float* s_mg, bf16_t* o) {
  const int sl = lane / 12, ch = lane - sl * 12;
  float gm = -INFINITY, lt = 0.f, o8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = 0.f;
  if (sl < 5) {
    auto fold = [&](const float* ps) {
      const float ms = AKI_LD_AGENT(ps), ls = AKI_LD_AGENT(ps + 1);
      float a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = AKI_LD_AGENT(ps + 8 + ch * 8 + e);
      split_fold(gm, lt, o8, ms, ls, a);
    };
    for (int s2 = sl; s2 < n0; s2 += 5) fold(pp + (size_t)s2 * DEC_PSTRIDE);
    for (int s2 = sl; s2 < n1; s2 += 5) fold(pp + (size_t)(n0 + s2) * DEC_PSTRIDE);
    split_slot_store(s_mg, sl, ch, gm, lt, o8);
  }
  __syncthreads();
  if (lane < 12) *(u32x4*)(o + lane * 8) = split_finish(s_mg, lane);
}

// ---- rotate-half RoPE of a 96-wide head: lane < 48 handles dims lane and lane + 48 ---------------------------------------------
struct RopeRow { float c0, c1, s0, s1; };

__device__ __forceinline__ RopeRow rope_row(const float* cos, const float* sin, int pos, int lane) {
  return {cos[(size_t)pos * 96 + lane], cos[(size_t)pos * 96 + lane + 48], sin[(size_t)pos * 96 + lane], sin[(size_t)pos * 96 + lane + 48]};
}
// d < 48 pairs with -x[d + 48]
__device__ __forceinline__ void rope_rotate_half(const RopeRow& t, float x0, float x1, __bf16& r0, __bf16& r1) {
  r0 = (__bf16)(x0 * t.c0 - x1 * t.s0);
  r1 = (__bf16)(x1 * t.c1 + x0 * t.s1);
}

// ---- the bf16 item: keys [k_begin, k_end) of one K/V slab ([cap][96] rows at kb / vb) against one query, one wave ----------------
//   score phase  lane = key: the lane loads its whole 192-byte K row (12 x 16 B, all in flight) and dots it with q
//   PV phase     lane = (row group g = lane>>4, 16-byte column chunk i = lane&15 < 12): 16 loads cover the tile's
//                64 V rows; the probability of row 4*t+g comes from its owner lane through a wave shuffle
// Leaves (m, l) in every lane and, in lane < 12, columns 8 * lane .. of acc: what split_publish<8> takes.
// x is the head's un-rotated q inside a fused qkv row of 3 * H * 96 (k at + H * 96, v at + 2 * H * 96); every item rotates q itself
// at table row `pos`, the item whose range holds the append row `la` (la = k_end - 1 then) also rotates k, appends k / v to the slab
// and uses them from LDS.
// vbits (with VBITS; may be null): the valid bits of the slab's keys are the nwords words from vbits[vword0].  SKIP_EMPTY: a tile that
// leaves the running max at -inf is passed over.  Both are what each caller computed before it shared this text: the grouped suffix
// item runs with neither.
template <bool VBITS, bool SKIP_EMPTY>
__device__ __forceinline__ void split_item_bf16(bf16_t* kb, bf16_t* vb, int la, int pos, int k_begin, int k_end, int T, const uint64_t* vbits,
                                                size_t vword0, int nwords, const bf16_t* x, int H, const float* cos, const float* sin, float scale, int lane,
                                                bf16_t* s_q, bf16_t* s_k, bf16_t* s_v, float& m, float& l, float (&acc)[8]) {
  const int g = lane >> 4, i16 = lane & 15;
  m = -INFINITY;
  l = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (k_begin >= k_end) return;
  const bool owner = la >= k_begin;                      // la < k_end holds by construction (k_end <= la + 1)
  u32x4 kr[12], vr[16];
  auto issue_tile = [&](int base) {                      // all 28 loads of a tile go out back to back
    const bf16_t* krow = kb + (size_t)min(base + lane, k_end - 1) * 96;         // clamped rows carry probability 0
#pragma unroll
    for (int i = 0; i < 12; ++i) kr[i] = *(const u32x4*)(krow + i * 8);
#pragma unroll
    for (int t2 = 0; t2 < 16; ++t2) {
      const int r = min(base + 4 * t2 + g, k_end - 1);
      vr[t2] = *(const u32x4*)(vb + (size_t)r * 96 + min(i16, 11) * 8);
    }
  };
  issue_tile(k_begin);                                   // in flight while q is rotated
  if (lane < 48) {
    const RopeRow rr = rope_row(cos, sin, pos, lane);
    __bf16 q0, q1;
    rope_rotate_half(rr, bf16_bits_to_f32(x[lane]), bf16_bits_to_f32(x[lane + 48]), q0, q1);
    ((__bf16*)s_q)[lane] = q0;
    ((__bf16*)s_q)[lane + 48] = q1;
    if (owner) {
      const bf16_t* kx = x + H * 96;
      const bf16_t* vx = x + 2 * H * 96;
      __bf16 kn0, kn1;
      rope_rotate_half(rr, bf16_bits_to_f32(kx[lane]), bf16_bits_to_f32(kx[lane + 48]), kn0, kn1);
      ((__bf16*)s_k)[lane] = kn0;
      ((__bf16*)s_k)[lane + 48] = kn1;
      ((__bf16*)kb)[(size_t)la * 96 + lane] = kn0;
      ((__bf16*)kb)[(size_t)la * 96 + lane + 48] = kn1;
      s_v[lane] = vx[lane];
      s_v[lane + 48] = vx[lane + 48];
      vb[(size_t)la * 96 + lane] = vx[lane];
      vb[(size_t)la * 96 + lane + 48] = vx[lane + 48];
    }
  }
  __syncthreads();
  // q is read from LDS where it is used (a broadcast): holding it (48 VGPRs) next to the K and V tiles put the kernel at 272 VGPRs = ONE wave
  // per SIMD, 1024 single-wave items in flight for the 1536 of a batch of eight; without it two fit
  for (int t = 0; t < T; ++t) {
    const int base = k_begin + t * 64;
    if (base >= k_end) break;
    const int j = base + lane;
    if (t > 0) issue_tile(base);
    if (owner && base <= la && la < base + 64) {
      // The new token's row lives in LDS: the tile loads were issued before it was stored, so every lane whose (clamped)
      // row index is la - the row itself and all rows past k_end - 1 = la, which carry probability 0 - holds stale
      // cache contents (0 * NaN would poison the sum) and takes the row from LDS instead.
      if (min(j, k_end - 1) == la) {
#pragma unroll
        for (int i = 0; i < 12; ++i) kr[i] = *(const u32x4*)(s_k + i * 8);
      }
#pragma unroll
      for (int t2 = 0; t2 < 16; ++t2)
        if (min(base + 4 * t2 + g, k_end - 1) == la) vr[t2] = *(const u32x4*)(s_v + min(i16, 11) * 8);
    }
    bool ok = j < k_end;
    if (VBITS && vbits && (base >> 6) < nwords) ok = ok && ((vbits[vword0 + (base >> 6)] >> lane) & 1ull);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s = dot8_bf16(kr[i], *(const u32x4*)(s_q + i * 8), s);
    s = ok ? s * scale : -INFINITY;
    const float mn = fmaxf(m, wave_max(s));
    if (SKIP_EMPTY && mn == -INFINITY) continue;         // wave-uniform: nothing visible yet
    const float a = __expf(m - mn);
    const float pr = ok ? __expf(s - mn) : 0.f;
    l = l * a + wave_sum(pr);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= a;
#pragma unroll
    for (int t2 = 0; t2 < 16; ++t2) {
      const float w = __shfl(pr, 4 * t2 + g);
      u32x4 vt = vr[t2];
      asm volatile("" : "+v"(vt));                       // widened here, row by row - not all 128 values ahead of the loop (that made it 272 VGPRs: one wave per SIMD)
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

}  // namespace aki

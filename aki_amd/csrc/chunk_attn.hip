// chunk_attn.hip - T new tokens per sample appended to a KV cache and attended in one pass (bf16, head_dim 96, MHA), CDNA4 MFMA.
//
// The continuation of a cached sequence by more than one token (Phi3ForCausalLM._continue with chunked_continue): query t of sample b
// sits at position cache_len[b] + t and sees
//   key j < cache_len[b]        iff its bit in col_valid_bits[b] is set (columns past nwords * 64 are valid)
//   key cache_len[b] + u        iff u <= t                       (the chunk's own causal prefix; a token always sees itself)
// Neither the single-query decode kernels (one query per row) nor the prefill cores (square: query row i is key row i) cover it.
//
// Two launches on the caller's stream, and stream order is the only dependency between them - no workgroup waits for another, there
// are no counters, tickets or polling:
//   chunk_rope_append_kernel   one wave per (row b*T + t, head): rotate-half RoPE of q and k at position cache_len[b] + t with the arithmetic
//                              of rope_rotate_half; q -> q_rot [B, H, T, 96] (the workspace), k / v -> cache row cache_len[b] + t.  Rows
//                              t >= n_new[b] write nothing.
//   chunk_attn_kernel          one workgroup of four waves per (b, head, 32-query block); layouts of the 32-row prefill core
//                              (mma_attn_bf16.hip): S^T = K Q^T with the query on the lane, online softmax in the log2 domain, O^T += V^T P
//                              with P taken from the score accumulators.  Wave w walks the 64-key tiles j = w, w + 4, ... of
//                              [0, cache_len[b] + last row of the block] and keeps one partial (m, l, acc); the four partials meet
//                              in LDS and are combined in wave order 0, 1, 2, 3 - the same inputs give the same bits on every run.
// Why two launches: a query block needs the rotated keys of every earlier block of its chunk, written by other workgroups; the launch
// boundary is the one hand-off that needs no cross-workgroup protocol.
//
// K fragments (A operand, 16 contiguous bytes of one key row per lane) come straight from global memory; a V tile goes through the
// wave's own 12 KiB of LDS ([key][96] rows, as the prefill core's image) and is read transposed with ds_read_b64_tr_b16.  Each wave
// touches only its own LDS until the merge, so the tile loop has no barrier.  Key rows are clamped to the block's last visible row and
// every clamped or masked column gets the score -inf, i.e. probability exactly 0: unused cache rows (NaN in the tests) are never read.
#include "attn_mma_common.h"
#include "decode_attn_common.h"

namespace aki {

struct ChunkParams {
  const bf16_t* qkv;       // [B*T, 3*H*96] un-rotated
  const float* cos;
  const float* sin;
  const int* cache_len;    // [B]
  const int* n_new;        // [B] or null (every sample brings T tokens)
  bf16_t* q_rot;           // [B, H, T, 96]
  bf16_t* k;               // [B, H, cap, 96]
  bf16_t* v;
  bf16_t* o;               // [B*T, H*96]
  const uint64_t* vbits;   // [B, nwords] or null
  int nwords;
  int B, H, T, cap;
  int Tm;                  // host bound of n_new (<= T): rows and query blocks past it are not launched
  float scale_log2;
};

__device__ __forceinline__ int chunk_rows(const ChunkParams& p, int b) {
  const int nn = p.n_new ? p.n_new[b] : p.T;
  return max(0, min(nn, p.T));
}

__global__ __launch_bounds__(64) void chunk_rope_append_kernel(const ChunkParams p) {
  const int head = blockIdx.y, lane = threadIdx.x;
  const int b = blockIdx.x / p.Tm, t = blockIdx.x - b * p.Tm;
  const int row = b * p.T + t;
  const int pos = p.cache_len[b] + t;
  if (t >= chunk_rows(p, b) || pos < 0 || pos >= p.cap || lane >= 48) return;
  const bf16_t* x = p.qkv + (size_t)row * 3 * p.H * 96 + head * 96;
  const bf16_t* kx = x + p.H * 96;
  const bf16_t* vx = x + 2 * p.H * 96;
  const RopeRow rr = rope_row(p.cos, p.sin, pos, lane);
  __bf16 q0, q1, k0, k1;
  rope_rotate_half(rr, bf16_bits_to_f32(x[lane]), bf16_bits_to_f32(x[lane + 48]), q0, q1);
  rope_rotate_half(rr, bf16_bits_to_f32(kx[lane]), bf16_bits_to_f32(kx[lane + 48]), k0, k1);
  __bf16* qo = (__bf16*)p.q_rot + (((size_t)b * p.H + head) * p.T + t) * 96;
  qo[lane] = q0;
  qo[lane + 48] = q1;
  const size_t crow = (((size_t)b * p.H + head) * p.cap + pos) * 96;
  ((__bf16*)p.k)[crow + lane] = k0;
  ((__bf16*)p.k)[crow + lane + 48] = k1;
  p.v[crow + lane] = vx[lane];
  p.v[crow + lane + 48] = vx[lane + 48];
}

// transposed LDS read with a memory clobber: it must stay behind the (compiler-visible) stores that fill the tile
template <int OFF>
__device__ __forceinline__ u32x2 chunk_read_tr(unsigned lds_addr) {
  u32x2 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lds_addr), "n"(OFF) : "memory");
  return r;
}

constexpr int CHUNK_NW = 4;
constexpr int CHUNK_OROW = 208;                       // staged output rows: 192 B + 16 (mma_attn_bf16.hip's epilogue)
constexpr int CHUNK_ML = CHUNK_NW * VTILE;            // (m, l) of every wave and lane: 2 * 4 * 64 floats
constexpr int CHUNK_SO = CHUNK_ML + 2 * CHUNK_NW * 64 * 4;
constexpr int CHUNK_LDS = CHUNK_SO + 32 * CHUNK_OROW; // 57,856 B: two workgroups per CU keep 113 KiB of the 160

__global__ __launch_bounds__(CHUNK_NW * 64, 2) void chunk_attn_kernel(const ChunkParams p) {
  __shared__ __attribute__((aligned(16))) char smem[CHUNK_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int nqb = (p.Tm + 31) >> 5;
  const int qblk = blockIdx.x % nqb;
  const int bh = blockIdx.x / nqb;
  const int b = bh / p.H, head = bh - b * p.H;
  const int q0 = qblk * 32;
  const int nn = chunk_rows(p, b);
  bf16_t* const obase = p.o + ((size_t)b * p.T * p.H + head) * 96;

  if (q0 >= nn) {   // a block past the sample's tokens: zeros, and nothing is read
    for (int ch = tid; ch < 32 * 12; ch += CHUNK_NW * 64) {
      const int r = ch / 12, c = ch - r * 12;
      if (q0 + r < p.T) *(u32x4*)((char*)(obase + (size_t)(q0 + r) * p.H * 96) + c * 16) = u32x4{0u, 0u, 0u, 0u};
    }
    return;
  }
  const int clen = max(0, p.cache_len[b]);
  const int t = q0 + l31;
  const int te = min(t, nn - 1);                       // rows past n_new run as the last real row and are written as zeros
  const int last = min(clen + min(q0 + 31, nn - 1), p.cap - 1);   // the block's last visible key row
  const int ntiles = (last >> 6) + 1;
  const char* kb = (const char*)(p.k + ((size_t)bh * p.cap) * 96);
  const char* vb_ = (const char*)(p.v + ((size_t)bh * p.cap) * 96);
  char* const sV = smem + wave * VTILE;                // this wave's V tile, later its partial accumulators

  bf16x8 qf[6];   // B operand of S^T = K Q^T: lane (q = l31, h) holds Q[q][16 ks + 8 h .. + 7]
  {
    const bf16_t* qrow = p.q_rot + ((size_t)bh * p.T + te) * 96 + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) qf[ks] = *(const bf16x8*)(qrow + 16 * ks);
  }
  const int voff = (4 * h + ((lane & 15) >> 2)) * VROW + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
  const unsigned vaddr = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)sV) + voff;

  f32x16 o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_run = -1e30f, l_part = 0.f;

  for (int j = wave; j < ntiles; j += CHUNK_NW) {      // wave-uniform: EXEC is all ones at the transposed reads
    const int c0 = j * 64;
    unsigned long long vb = ~0ull;
    if (p.vbits && j < p.nwords) vb = p.vbits[(size_t)b * p.nwords + j];
    {
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)vb), hi = __builtin_amdgcn_readfirstlane((unsigned)(vb >> 32));
      vb = ((unsigned long long)hi << 32) | lo;
    }
    const bool below = c0 + 63 < clen;                 // the whole tile lies in the cached prefix
    if (below && vb == 0ull) continue;                 // nothing of it is visible to any row
    // V tile: 64 rows x 192 B, global -> registers -> this wave's LDS image; K fragments straight from global
    u32x4 vst[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int ch = i * 64 + lane;
      const int kr = ch / 12, pos = ch - kr * 12;
      vst[i] = *(const u32x4*)(vb_ + (size_t)min(c0 + kr, last) * 192 + pos * 16);
    }
    bf16x8 ka[6], kc[6];
    {
      const char* k0 = kb + (size_t)min(c0 + l31, last) * 192 + h * 16;
      const char* k1 = kb + (size_t)min(c0 + 32 + l31, last) * 192 + h * 16;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        ka[ks] = *(const bf16x8*)(k0 + ks * 32);
        kc[ks] = *(const bf16x8*)(k1 + ks * 32);
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) *(u32x4*)(sV + (i * 64 + lane) * 16) = vst[i];
    asm volatile("" ::: "memory");

    f32x16 s0 = {}, s1 = {};
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ks], qf[ks], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kc[ks], qf[ks], s1, 0, 0, 0);
    }
    // the V^T fragments do not depend on the softmax: their reads land under it (same wave, LDS operations execute in order behind the stores)
    u32x2 vlo[4][3], vhi[4][3];
    static_for<4>([&](auto ks4) {
      static_for<3>([&](auto dt) {
        constexpr int off = ks4 * 16 * VROW + dt * 64;
        vlo[ks4][dt] = chunk_read_tr<off>(vaddr);
        vhi[ks4][dt] = chunk_read_tr<off + 8 * VROW>(vaddr);
      });
    });
    if (!(below && vb == ~0ull)) {
      // register i of s0:s1 is key c0 + 4h + (i&3) + 8*((i&15)>>2) + 32*(i>>4) (attn_mma_common.h, count_le)
      const unsigned long long vbh = vb >> (4 * h);
      const int kbase = c0 + 4 * h;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const int bit = (i & 3) + 8 * ((i & 15) >> 2) + 32 * (i >> 4);
        const int key = kbase + bit;
        const bool vis = key < clen ? (((vbh >> bit) & 1ull) != 0ull) : (key - clen <= te);
        if (i < 16) s0[i] = vis ? s0[i] : -INFINITY;
        else s1[i - 16] = vis ? s1[i - 16] : -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fmaxf(s0[r], s1[r]));
    mx = halves_max(mx) * p.scale_log2;
    const float m_new = fmaxf(m_run, mx);              // finite: m_run starts at -1e30, so a hidden column's exp2(-inf - m) is exactly 0
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[r], p.scale_log2, -m_new));
      s1[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[r], p.scale_log2, -m_new));
      ps += s0[r] + s1[r];
    }
    l_part = l_part * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;

    // every transposed read has to be back before its registers are touched: one wait naming all destinations
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(vlo[0][0]), "+v"(vhi[0][0]), "+v"(vlo[0][1]), "+v"(vhi[0][1]), "+v"(vlo[0][2]), "+v"(vhi[0][2]),
                   "+v"(vlo[1][0]), "+v"(vhi[1][0]), "+v"(vlo[1][1]), "+v"(vhi[1][1]), "+v"(vlo[1][2]), "+v"(vhi[1][2]),
                   "+v"(vlo[2][0]), "+v"(vhi[2][0]), "+v"(vlo[2][1]), "+v"(vhi[2][1]), "+v"(vlo[2][2]), "+v"(vhi[2][2]),
                   "+v"(vlo[3][0]), "+v"(vhi[3][0]), "+v"(vlo[3][1]), "+v"(vhi[3][1]), "+v"(vlo[3][2]), "+v"(vhi[3][2])
                 :
                 : "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks4 = 0; ks4 < 4; ++ks4) {
      bf16x8 pf;
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[e] = (__bf16)((ks4 < 2) ? s0[8 * (ks4 & 1) + e] : s1[8 * (ks4 & 1) + e]);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) {
        const u32x4 vv = {vlo[ks4][dt][0], vlo[ks4][dt][1], vhi[ks4][dt][0], vhi[ks4][dt][1]};
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vv), pf, o[dt], 0, 0, 0);
      }
    }
  }

  // ---- the four partials meet in LDS: [wave][register f = 16 dt + r][lane] floats in the wave's (now idle) V tile ----
  const float l_tot = halves_sum(l_part);
  float* const sP = (float*)sV;
  float* const sML = (float*)(smem + CHUNK_ML);
#pragma unroll
  for (int dt = 0; dt < 3; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sP[(dt * 16 + r) * 64 + lane] = o[dt][r];
  sML[wave * 64 + lane] = m_run;
  sML[(CHUNK_NW + wave) * 64 + lane] = l_tot;
  __syncthreads();
  // wave w finishes accumulator registers 12 w .. 12 w + 11 of every lane; wave order 0, 1, 2, 3 in every sum
  float pv[CHUNK_NW * 14];
#pragma unroll
  for (int w = 0; w < CHUNK_NW; ++w) {
    pv[w * 14] = sML[w * 64 + lane];
    pv[w * 14 + 1] = sML[(CHUNK_NW + w) * 64 + lane];
#pragma unroll
    for (int e = 0; e < 12; ++e) pv[w * 14 + 2 + e] = ((const float*)(smem + w * VTILE))[(12 * wave + e) * 64 + lane];
  }
  lds_fold_ready(pv);
  float M = pv[0];
#pragma unroll
  for (int w = 1; w < CHUNK_NW; ++w) M = fmaxf(M, pv[w * 14]);
  float lt = 0.f, acc[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) acc[e] = 0.f;
#pragma unroll
  for (int w = 0; w < CHUNK_NW; ++w) {
    const float f = __builtin_amdgcn_exp2f(pv[w * 14] - M);
    lt += pv[w * 14 + 1] * f;
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] += pv[w * 14 + 2 + e] * f;
  }
  const bool live = t < nn && lt > 0.f;
  const float inv = live ? 1.0f / lt : 0.f;
  if (!live) {                                         // a row past n_new is +0.0 bit for bit: acc * 0.f would keep acc's sign
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
  }
  char* const sO = smem + CHUNK_SO;
#pragma unroll
  for (int qq = 0; qq < 3; ++qq) {
    const int quad = 3 * wave + qq, dt = quad >> 2, q4 = quad & 3;   // registers 4 quad .. + 3 = features 32 dt + 8 q4 + 4 h + e
    const u32x2 pk = {pack_bf16x2(acc[4 * qq] * inv, acc[4 * qq + 1] * inv), pack_bf16x2(acc[4 * qq + 2] * inv, acc[4 * qq + 3] * inv)};
    *(u32x2*)(sO + l31 * CHUNK_OROW + (dt * 32 + q4 * 8 + 4 * h) * 2) = pk;
  }
  __syncthreads();
  for (int ch = tid; ch < 32 * 12; ch += CHUNK_NW * 64) {           // whole 192-B rows, 16 B per lane
    const int r = ch / 12, c = ch - r * 12;
    const u32x4 w4 = *(const u32x4*)(sO + r * CHUNK_OROW + c * 16);
    if (q0 + r < p.T) *(u32x4*)((char*)(obase + (size_t)(q0 + r) * p.H * 96) + c * 16) = w4;
  }
}

size_t chunk_attn_ws_bytes(int B, int H, int T) { return (size_t)B * H * T * 96 * sizeof(bf16_t); }

int chunk_attn_launch(const void* qkv, const float* cos, const float* sin, const int* cache_len, const int* n_new, void* k_cache, void* v_cache,
                      void* o, const uint64_t* vbits, int nwords, int B, int H, int T, int max_new, int cap, float scale, void* ws,
                      size_t ws_bytes, hipStream_t s) {
  if (!ws || ws_bytes < chunk_attn_ws_bytes(B, H, T)) return AKI_ERR_WORKSPACE;
  ChunkParams p = {};
  p.qkv = (const bf16_t*)qkv; p.cos = cos; p.sin = sin; p.cache_len = cache_len; p.n_new = n_new;
  p.q_rot = (bf16_t*)ws; p.k = (bf16_t*)k_cache; p.v = (bf16_t*)v_cache; p.o = (bf16_t*)o;
  p.vbits = vbits; p.nwords = vbits ? nwords : 0;
  p.B = B; p.H = H; p.T = T; p.cap = cap;
  p.Tm = (max_new <= 0 || max_new > T) ? T : max_new;
  p.scale_log2 = scale * 1.44269504088896340736f;
  AKI_CLEAR_ERR();
  hipLaunchKernelGGL(chunk_rope_append_kernel, dim3(B * p.Tm, H), dim3(64), 0, s, p);
  AKI_LAUNCH_CHECK();
  hipLaunchKernelGGL(chunk_attn_kernel, dim3(B * H * ((p.Tm + 31) / 32)), dim3(CHUNK_NW * 64), 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

}  // namespace aki

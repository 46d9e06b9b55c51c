// logprob.hip - the log-probability of one token per row, with up to 8 alternatives (include/aki_mi355x.h: aki_token_logprob).
// What `generate(output_logprobs=True)` and `score` launch behind every pick: HF's compute_transition_scores(normalize_logits=True) for the
// step's raw logits, one number per row instead of beam_logprob_kernel's whole f32 row.
#include "aki_device.h"

namespace aki {

constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_MAX_TOP = AKI_LOGPROB_MAX_TOP;
// Survivors of the threshold held in LDS.  At most top_k - 1 <= 7 threads hold values above the threshold and a thread owns at most
// 8 * ceil(V / 8192) + 1 <= 257 columns for V <= AKI_LOGPROB_MAX_V = 2^18 (lp_row), so at most 7 * 257 + 1 = 1800 words arrive: no overflow path.
constexpr int LP_LIST = 2048;
static_assert(AKI_LOGPROB_MAX_V <= (1 << 18) && (LP_MAX_TOP - 1) * (AKI_LOGPROB_MAX_V / 1024 + 1) + 1 <= LP_LIST, "the LDS list holds every survivor");

struct LogprobParams {
  const void* logits;
  int V, ld;
  const int64_t* ids;
  const int64_t* tokens;
  int tokens_ld;
  const int* cache_len;
  const int* start_len;
  int step;
  const unsigned char* skip;
  const int* done_at;
  int top_k;
  float* out_logprob;
  int64_t* out_top_ids;
  float* out_top_logprobs;
  int out_ld, out_cols;
};

// A column as one word: the value above (larger value <=> larger word; -0 and +0 share one), the complement of the column below - beam.hip's
// beam_word.  The columns of a row have distinct words and "larger word" is "larger value, or the same value and the lower column": the
// top_k largest words in descending order ARE the ranking.  0 is no column's word.
__device__ __forceinline__ unsigned long long lp_word(float x, int v) {
  if (x == 0.f) x = 0.f;
  const unsigned u = __builtin_bit_cast(unsigned, x);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)o << 32) | (unsigned long long)(0xffffffffu - (unsigned)v);
}
__device__ __forceinline__ float lp_word_value(unsigned long long w) {
  const unsigned k = (unsigned)(w >> 32);
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// f(column, value) for every column this thread owns, in a fixed order.  VEC (16-byte aligned rows): thread tid owns the 16-byte vectors
// tid, tid + 1024, ... (8 bf16 or 4 f32 columns each, ascending) and then the column (V rounded down to whole vectors) + tid of the tail.
// Otherwise the columns tid, tid + 1024, ...  Nothing outside the row's V columns is read.
template <bool F32, bool VEC, typename F>
__device__ __forceinline__ void lp_row(const void* row, int V, F&& f) {
  const int tid = threadIdx.x;
  const float* xf = (const float*)row;
  const bf16_t* xb = (const bf16_t*)row;
  if constexpr (!VEC) {
    for (int v = tid; v < V; v += LP_THREADS) f(v, F32 ? xf[v] : bf16_bits_to_f32(xb[v]));
  } else {
    constexpr int W = F32 ? 4 : 8;
    const int nv = V / W;
    for (int i = tid; i < nv; i += LP_THREADS) {
      if constexpr (F32) {
        const f32x4 q = ((const f32x4*)row)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) f(i * 4 + j, q[j]);
      } else {
        const u32x4 q = ((const u32x4*)row)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned w = q[j];
          f(i * 8 + 2 * j, bf16_lo(w));
          f(i * 8 + 2 * j + 1, bf16_hi(w));
        }
      }
    }
    const int v = nv * W + tid;
    if (v < V) f(v, F32 ? xf[v] : bf16_bits_to_f32(xb[v]));
  }
}

// One workgroup per row.
//   1. m = max x (exact) and every thread's best word; each wave's top_k best thread words; the threshold tau = the top_k-th largest of
//      those 16 * top_k.  top_k distinct columns are >= tau, so the top_k best are all >= tau.  (Fewer than top_k threads with a column: tau = 0.)
//   2. s = sum exp(x - m): a thread adds its columns in lp_row's order, the 64 lanes of a wave fold by xor butterfly (every lane holds the
//      same bits), the 16 wave sums are added in wave order.  The same pass puts every word >= tau on an LDS list (in any order: the ranking
//      below counts, it does not depend on it).  lse = m + log s.  No float atomics: the same inputs give the same bits on every run.
//   3. the list is ranked by counting; thread j < top_k writes rank j, one thread the chosen token's x - lse.
template <bool F32, bool VEC>
__global__ __launch_bounds__(LP_THREADS) void token_logprob_kernel(const LogprobParams p) {
  __shared__ float s_red[LP_WAVES];
  __shared__ unsigned long long s_cand[LP_WAVES * LP_MAX_TOP];
  __shared__ unsigned long long s_list[LP_LIST];
  __shared__ unsigned long long s_top[LP_MAX_TOP];
  __shared__ unsigned long long s_tau;
  __shared__ int s_n;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = p.top_k, V = p.V;

  // the position the pick just wrote; everything up to the first barrier is workgroup-uniform
  int t = p.step;
  if (p.cache_len != nullptr) t += p.cache_len[r] - p.start_len[r];
  if (t < 0 || t >= p.out_cols) return;
  const size_t o = (size_t)r * p.out_ld + t;
  bool skipped = p.skip != nullptr && p.skip[r] != 0;
  if (p.done_at != nullptr) {
    const int d = p.done_at[r];
    skipped = skipped || (d >= 0 && d < t);
  }
  if (skipped) {
    if (tid == 0) p.out_logprob[o] = 0.f;
    if (tid < K) {
      p.out_top_ids[o * K + tid] = -1;
      p.out_top_logprobs[o * K + tid] = 0.f;
    }
    return;
  }

  const void* row = (const char*)p.logits + (size_t)r * p.ld * (F32 ? 4 : 2);
  float m = -INFINITY;
  unsigned long long best = 0ull;
  lp_row<F32, VEC>(row, V, [&](int v, float x) {
    m = fmaxf(m, x);
    const unsigned long long w = lp_word(x, v);
    best = w > best ? w : best;
  });
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  if (tid == 0) { s_n = 0; s_tau = K > 0 ? 0ull : ~0ull; }
  unsigned long long prev = ~0ull;
  for (int j = 0; j < K; ++j) {                          // the wave's j-th best thread word (0: it has fewer)
    unsigned long long w = best < prev ? best : 0ull;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      const unsigned long long y = __shfl_xor(w, sh);
      w = y > w ? y : w;
    }
    if (lane == 0) s_cand[wave * LP_MAX_TOP + j] = w;
    prev = w;
  }
  __syncthreads();
  m = s_red[0];
#pragma unroll
  for (int i = 1; i < LP_WAVES; ++i) m = fmaxf(m, s_red[i]);
  if (tid < LP_WAVES * LP_MAX_TOP && tid % LP_MAX_TOP < K) {
    const unsigned long long c = s_cand[tid];
    if (c != 0ull) {
      int above = 0;
      for (int w2 = 0; w2 < LP_WAVES; ++w2)
        for (int j = 0; j < K; ++j) above += s_cand[w2 * LP_MAX_TOP + j] > c ? 1 : 0;
      if (above == K - 1) s_tau = c;                     // the candidates are distinct words: at most one thread
    }
  }
  __syncthreads();
  const unsigned long long tau = s_tau;

  float s = 0.f;
  lp_row<F32, VEC>(row, V, [&](int v, float x) {
    s += expf(x - m);
    const unsigned long long w = lp_word(x, v);
    if (w >= tau) {
      const int at = atomicAdd(&s_n, 1);
      if (at < LP_LIST) s_list[at] = w;
    }
  });
  s = wave_sum(s);
  if (lane == 0) s_red[wave] = s;
  __syncthreads();
  s = s_red[0];
#pragma unroll
  for (int i = 1; i < LP_WAVES; ++i) s += s_red[i];
  const float lse = m + logf(s);

  const int n = min(s_n, LP_LIST);
  if (K > 0) {
    for (int i = tid; i < n; i += LP_THREADS) {
      const unsigned long long w = s_list[i];
      int above = 0;
      for (int j = 0; j < n; ++j) above += s_list[j] > w ? 1 : 0;
      if (above < K) s_top[above] = w;
    }
    __syncthreads();
    if (tid < K) {                                       // a row with fewer than top_k columns: id -1, logprob -inf behind them
      const unsigned long long w = tid < n ? s_top[tid] : 0ull;
      p.out_top_ids[o * K + tid] = tid < n ? (int64_t)(0xffffffffu - (unsigned)(w & 0xffffffffull)) : (int64_t)-1;
      p.out_top_logprobs[o * K + tid] = tid < n ? lp_word_value(w) - lse : -INFINITY;
    }
  }
  if (tid == LP_THREADS - 1) {
    int64_t id = -1;
    if (p.ids != nullptr) id = p.ids[r];
    else if (t < p.tokens_ld) id = p.tokens[(size_t)r * p.tokens_ld + t];
    float lp = __builtin_nanf("");
    if (id >= 0 && id < (int64_t)V) {
      const float x = F32 ? ((const float*)row)[id] : bf16_bits_to_f32(((const bf16_t*)row)[id]);
      lp = x - lse;
    }
    p.out_logprob[o] = lp;
  }
}

int token_logprob_launch(const void* logits, int in_f32, int rows, int V, int ld, const int64_t* ids, const int64_t* tokens, int tokens_ld,
                         const int* cache_len, const int* start_len, int step, const unsigned char* skip, const int* done_at, int top_k,
                         float* out_logprob, int64_t* out_top_ids, float* out_top_logprobs, int out_ld, int out_cols, hipStream_t s) {
  const LogprobParams p = {logits, V, ld, ids, tokens, tokens_ld, cache_len, start_len, step, skip, done_at, top_k,
                           out_logprob, out_top_ids, out_top_logprobs, out_ld, out_cols};
  const bool vec = (((uintptr_t)logits) & 15) == 0 && ((size_t)ld * (in_f32 ? 4 : 2)) % 16 == 0;      // every row starts on 16 bytes
  const dim3 grid(rows), block(LP_THREADS);
  if (in_f32 && vec) hipLaunchKernelGGL((token_logprob_kernel<true, true>), grid, block, 0, s, p);
  else if (in_f32) hipLaunchKernelGGL((token_logprob_kernel<true, false>), grid, block, 0, s, p);
  else if (vec) hipLaunchKernelGGL((token_logprob_kernel<false, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((token_logprob_kernel<false, false>), grid, block, 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

}  // namespace aki

// beam.hip - beam search on the device (include/aki_mi355x.h: aki_beam_logprob, aki_beam_step, aki_kv_beam_reorder).
// The algorithm is HF `GenerationMixin` beam search with a `BeamSearchScorer`, as AKI._beam_search (aki_amd/aki.py) states it on the host:
// 2K candidates per step, EOS candidates among the K best become hypotheses, at most K hypotheses per sample, one `done` flag per sample.
#include "aki_device.h"

namespace aki {

constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_MAX_K = AKI_BEAM_MAX_K;
constexpr int BEAM_LIST = 1024;        // survivors of the threshold pass held in LDS; more than that takes the pass-per-rank path
constexpr int BEAM_GROUPS = 256;       // the threshold is the 2K-th largest of this many group maxima

// ---- log-softmax of a row, f32, fixed reduction order -------------------------------------------------------------------------------
// One workgroup per row.  m = max x (exact); s = sum exp(x - m): every thread adds its columns tid, tid + 1024, ... in that order, the 64
// lanes of a wave fold by xor butterfly (both partners of an exchange add the same two numbers, so every lane holds the same bits), the
// 16 wave sums are added in wave order; out = x - (m + log s).  No atomics: the same inputs give the same bits on every run.
template <bool F32>
__global__ __launch_bounds__(BEAM_THREADS) void beam_logprob_kernel(const void* logits, int V, int ld, float* out, int ld_out) {
  __shared__ float s_red[BEAM_THREADS / 64];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xf = (const float*)logits + (size_t)row * ld;
  const bf16_t* xb = (const bf16_t*)logits + (size_t)row * ld;
  auto at = [&](int v) -> float { return F32 ? xf[v] : bf16_bits_to_f32(xb[v]); };
  float m = -INFINITY;
  for (int v = tid; v < V; v += BEAM_THREADS) m = fmaxf(m, at(v));
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  m = s_red[0];
#pragma unroll
  for (int i = 1; i < BEAM_THREADS / 64; ++i) m = fmaxf(m, s_red[i]);
  __syncthreads();
  float s = 0.f;
  for (int v = tid; v < V; v += BEAM_THREADS) s += expf(at(v) - m);
  s = wave_sum(s);
  if (lane == 0) s_red[wave] = s;
  __syncthreads();
  s = s_red[0];
#pragma unroll
  for (int i = 1; i < BEAM_THREADS / 64; ++i) s += s_red[i];
  const float lse = m + logf(s);
  float* o = out + (size_t)row * ld_out;
  for (int v = tid; v < V; v += BEAM_THREADS) o[v] = at(v) - lse;
}

// ---- one beam step ------------------------------------------------------------------------------------------------------------------
struct BeamParams {
  const float* logp;
  int ld, K, V, t, max_new;
  float* beam_scores;
  const int64_t* seqs_in;
  int64_t* seqs_out;
  float* hyp_score;
  int* hyp_len;
  int64_t* hyp_tokens;
  int* hyp_count;
  unsigned char* done;
  int64_t* next_ids;
  int* parent;
  const int64_t* eos;
  int n_eos;
  int64_t pad;
  float length_penalty;
  int early, last;
};

// larger score <=> larger word; -0 and +0 share one (they are equal scores: the index decides)
__device__ __forceinline__ unsigned beam_ord(float x) {
  if (x == 0.f) x = 0.f;
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float beam_ord_inv(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// A candidate as one word: the score above, the complement of the flat index k * V + v below.  Candidates of one sample have distinct
// words, "larger word" is "better score, or the same score and the lower flat index": the 2K largest words in descending order ARE the
// ranking, whatever order the threads met them in.  0 is no candidate's word (flat < 2^31).
__device__ __forceinline__ unsigned long long beam_word(float score, unsigned flat) {
  return ((unsigned long long)beam_ord(score) << 32) | (unsigned long long)(0xffffffffu - flat);
}

__device__ __forceinline__ unsigned long long beam_block_max(unsigned long long x, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y > x ? y : x;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                   // the previous round's readers are through with red
  if (lane == 0) red[wave] = x;
  __syncthreads();
  x = red[0];
#pragma unroll
  for (int i = 1; i < BEAM_THREADS / 64; ++i) x = red[i] > x ? red[i] : x;
  return x;
}

// One workgroup per sample.  Thread tid owns the columns v = tid, tid + 1024, ... of all K beams of the sample.
//   1. every thread's best word; the threshold tau = the 2K-th largest of the 256 maxima over the thread groups {g, g + 256, g + 512,
//      g + 768}.  2K distinct candidates are >= tau, so the 2K best are all >= tau.  (Fewer than 2K groups with a candidate: tau = 0.)
//   2. every word >= tau goes to an LDS list (in any order: the ranking below does not depend on it) - for scores without structure that
//      is 2K plus a few.  A list of at most 1024 is ranked by counting; a longer one (many large scores in one thread's columns) is
//      dropped and the 2K best are found one rank per pass over the candidates.  Both give the same 2K words.
//   3. thread 0 walks the ranking as the host loop does; then all threads move the token rows.
__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(const BeamParams p) {
  __shared__ unsigned long long s_tm[BEAM_THREADS];
  __shared__ unsigned long long s_list[BEAM_LIST];
  __shared__ unsigned long long s_top[2 * BEAM_MAX_K];
  __shared__ unsigned long long s_red[BEAM_THREADS / 64];
  __shared__ unsigned long long s_tau;
  __shared__ float s_score[BEAM_MAX_K];
  __shared__ int s_n;
  __shared__ int s_nbeam[BEAM_MAX_K];                // running beams chosen at this step: the local parent beam
  __shared__ int64_t s_ntok[BEAM_MAX_K];
  __shared__ float s_nscore[BEAM_MAX_K];
  __shared__ float s_hs[BEAM_MAX_K];                 // hypothesis slots: score, and what this step put there (beam < 0: nothing)
  __shared__ int s_hbeam[BEAM_MAX_K];
  __shared__ int64_t s_htok[BEAM_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x, K = p.K, V = p.V, t = p.t;
  const size_t row0 = (size_t)b * K;

  if (p.done[b] != 0) {                              // a frozen sample: state untouched, pad tokens, identity parents (workgroup-uniform)
    for (int i = tid; i < K * (t + 1); i += BEAM_THREADS) {
      const int n = i / (t + 1), j = i % (t + 1);
      p.seqs_out[(row0 + n) * p.max_new + j] = j < t ? p.seqs_in[(row0 + n) * p.max_new + j] : p.pad;
    }
    if (tid < K) {
      p.next_ids[row0 + tid] = p.pad;
      p.parent[row0 + tid] = (int)row0 + tid;
    }
    return;
  }

  if (tid < K) s_score[tid] = p.beam_scores[row0 + tid];
  if (tid == 0) { s_n = 0; s_tau = 0ull; }
  __syncthreads();

  unsigned long long best = 0ull;
  for (int k = 0; k < K; ++k) {
    const float* row = p.logp + (row0 + k) * p.ld;
    const float sc = s_score[k];
    for (int v = tid; v < V; v += BEAM_THREADS) {
      const unsigned long long w = beam_word(row[v] + sc, (unsigned)(k * V + v));
      best = w > best ? w : best;
    }
  }
  s_tm[tid] = best;
  __syncthreads();
  unsigned long long g = 0ull;
  if (tid < BEAM_GROUPS) {
#pragma unroll
    for (int i = 0; i < BEAM_THREADS / BEAM_GROUPS; ++i) {
      const unsigned long long w = s_tm[tid + i * BEAM_GROUPS];
      g = w > g ? w : g;
    }
  }
  __syncthreads();
  if (tid < BEAM_GROUPS) s_tm[tid] = g;
  __syncthreads();
  if (tid < BEAM_GROUPS && g != 0ull) {
    int above = 0;
    for (int j = 0; j < BEAM_GROUPS; ++j) above += s_tm[j] > g ? 1 : 0;
    if (above == 2 * K - 1) s_tau = g;               // the group maxima are distinct words: at most one thread
  }
  __syncthreads();
  const unsigned long long tau = s_tau;

  for (int k = 0; k < K; ++k) {
    const float* row = p.logp + (row0 + k) * p.ld;
    const float sc = s_score[k];
    for (int v = tid; v < V; v += BEAM_THREADS) {
      const unsigned long long w = beam_word(row[v] + sc, (unsigned)(k * V + v));
      if (w >= tau) {
        const int at = atomicAdd(&s_n, 1);
        if (at < BEAM_LIST) s_list[at] = w;
      }
    }
  }
  __syncthreads();
  const int n_list = s_n;
  if (n_list <= BEAM_LIST) {
    for (int i = tid; i < n_list; i += BEAM_THREADS) {
      const unsigned long long w = s_list[i];
      int above = 0;
      for (int j = 0; j < n_list; ++j) above += s_list[j] > w ? 1 : 0;
      if (above < 2 * K) s_top[above] = w;
    }
  } else {
    unsigned long long prev = ~0ull;
    for (int r = 0; r < 2 * K; ++r) {                // workgroup-uniform loop: n_list and K are
      unsigned long long mx = 0ull;
      for (int k = 0; k < K; ++k) {
        const float* row = p.logp + (row0 + k) * p.ld;
        const float sc = s_score[k];
        for (int v = tid; v < V; v += BEAM_THREADS) {
          const unsigned long long w = beam_word(row[v] + sc, (unsigned)(k * V + v));
          mx = (w < prev && w > mx) ? w : mx;
        }
      }
      prev = beam_block_max(mx, s_red);
      if (tid == 0) s_top[r] = prev;
    }
  }
  __syncthreads();

  if (tid == 0) {
    int count = p.hyp_count[b];
    for (int i = 0; i < K; ++i) {
      s_hs[i] = i < count ? p.hyp_score[row0 + i] : 0.f;
      s_hbeam[i] = -1;
    }
    const float norm = powf((float)(t + 1), p.length_penalty);
    auto worst_slot = [&]() -> int {                 // the minimum; among equal minima the lowest slot
      int w = 0;
      for (int i = 1; i < K; ++i) w = s_hs[i] < s_hs[w] ? i : w;
      return w;
    };
    auto add = [&](float sum, int beam, int64_t tok) {
      const float sc = sum / norm;
      int slot = -1;
      if (count < K) slot = count++;
      else {
        const int w = worst_slot();
        if (sc > s_hs[w]) slot = w;
      }
      if (slot >= 0) { s_hs[slot] = sc; s_hbeam[slot] = beam; s_htok[slot] = tok; }
    };
    int64_t eos[AKI_BEAM_MAX_EOS];
    for (int i = 0; i < AKI_BEAM_MAX_EOS; ++i) eos[i] = i < p.n_eos ? p.eos[i] : (int64_t)-1;
    int n = 0;
    for (int r = 0; r < 2 * K && n < K; ++r) {
      const unsigned long long w = s_top[r];
      const unsigned flat = 0xffffffffu - (unsigned)(w & 0xffffffffull);
      const int beam = min((int)(flat / (unsigned)V), K - 1);    // a candidate's word always decodes to a beam < K; never index past the sample
      const int64_t tok = (int64_t)(flat % (unsigned)V);
      const float sc = beam_ord_inv((unsigned)(w >> 32));
      bool is_eos = false;
      for (int i = 0; i < AKI_BEAM_MAX_EOS; ++i) is_eos = is_eos || eos[i] == tok;
      if (is_eos) {
        if (r < K) add(sc, beam, tok);               // HF: an EOS beyond the K best is ignored
        continue;
      }
      s_nbeam[n] = beam; s_ntok[n] = tok; s_nscore[n] = sc;
      ++n;
    }
    for (; n < K; ++n) { s_nbeam[n] = 0; s_ntok[n] = p.pad; s_nscore[n] = -1e9f; }
    bool done = false;
    if (count >= K) {
      float best_running = s_nscore[0];
      for (int i = 1; i < K; ++i) best_running = fmaxf(best_running, s_nscore[i]);
      best_running = best_running / norm;
      done = p.early == 1 || (p.early == 0 && s_hs[worst_slot()] >= best_running);
    }
    if (p.last && !done)                             // the closing step: the running beams become hypotheses, with this step's token
      for (int i = 0; i < K; ++i)
        if (s_nscore[i] > -1e8f) add(s_nscore[i], s_nbeam[i], s_ntok[i]);
    for (int i = 0; i < K; ++i) {
      p.beam_scores[row0 + i] = s_nscore[i];
      p.next_ids[row0 + i] = s_ntok[i];
      p.parent[row0 + i] = (int)row0 + s_nbeam[i];
      if (s_hbeam[i] >= 0) { p.hyp_score[row0 + i] = s_hs[i]; p.hyp_len[row0 + i] = t + 1; }
    }
    p.hyp_count[b] = count;
    if (done) p.done[b] = 1;
  }
  __syncthreads();
  // the token rows: seqs_out[n] = seqs_in[parent n] + [token n]; a slot filled at this step = seqs_in[its beam] + [its token]
  for (int i = tid; i < K * (t + 1); i += BEAM_THREADS) {
    const int n = i / (t + 1), j = i % (t + 1);
    p.seqs_out[(row0 + n) * p.max_new + j] = j < t ? p.seqs_in[(row0 + s_nbeam[n]) * p.max_new + j] : s_ntok[n];
    if (s_hbeam[n] >= 0)
      p.hyp_tokens[(row0 + n) * p.max_new + j] = j < t ? p.seqs_in[(row0 + s_hbeam[n]) * p.max_new + j] : s_htok[n];
  }
}

// ---- in-place re-ordering of the rows written since the prefill ----------------------------------------------------------------------
// dst[b*K + n, h, pos, :] = src[parent[b*K + n], h, pos, :] for start_len <= pos < cache_len, for every tensor of the table.  Parents repeat, so a
// row is source and destination at once; the hazard is removed by ownership: a workgroup owns one (tensor, sample, head, chunk of
// REORDER_CHUNK positions) across all K beams, and inside it ONE thread owns a vector of the chunk across all K beams - it loads the K sources into
// registers and only then stores the K destinations, and no other thread of the launch touches those bytes.  (A thread's own program
// order is the synchronisation: no barrier is needed between its loads and its stores.)
constexpr int REORDER_THREADS = 256;
constexpr int REORDER_CHUNK = AKI_KV_BEAM_REORDER_CHUNK;

template <typename VT>
__global__ __launch_bounds__(REORDER_THREADS) void kv_beam_reorder_kernel(void* const* table, const int* parent, const int* start_len,
                                                                          const int* cache_len, int B, int K, int H, int cap, int row_vecs,
                                                                          int pos_lo) {
  __shared__ int s_par[BEAM_MAX_K], s_lo[BEAM_MAX_K], s_hi[BEAM_MAX_K];
  const int tid = threadIdx.x, h = blockIdx.y;
  const int b = blockIdx.z % B, tensor = blockIdx.z / B;
  const int row0 = b * K;
  if (tid < K) {
    int par = parent[row0 + tid];
    if (par < row0 || par >= row0 + K) par = row0 + tid;      // a parent outside the sample is never followed
    s_par[tid] = par - row0;
    s_lo[tid] = max(start_len[row0 + tid], 0);
    s_hi[tid] = min(cache_len[row0 + tid], cap);
  }
  __syncthreads();
  bool identity = true;
  for (int n = 0; n < K; ++n) identity = identity && s_par[n] == n;
  if (identity) return;                                        // workgroup-uniform: nothing moves in this sample
  VT* base = (VT*)table[tensor];
  const size_t row_stride = (size_t)H * cap * row_vecs;
  const int pos0 = pos_lo + blockIdx.x * REORDER_CHUNK;
  const size_t off0 = ((size_t)h * cap + pos0) * row_vecs;
  for (int i = tid; i < REORDER_CHUNK * row_vecs; i += REORDER_THREADS) {
    const int pos = pos0 + i / row_vecs;
    VT buf[BEAM_MAX_K];
    bool move[BEAM_MAX_K];
#pragma unroll
    for (int n = 0; n < BEAM_MAX_K; ++n) {
      move[n] = false;
      if (n < K) {
        const int src = s_par[n];
        move[n] = src != n && pos >= s_lo[n] && pos < s_hi[n] && pos >= s_lo[src] && pos < s_hi[src];
        if (move[n]) buf[n] = base[(size_t)(row0 + src) * row_stride + off0 + i];
      }
    }
#pragma unroll
    for (int n = 0; n < BEAM_MAX_K; ++n)
      if (move[n]) base[(size_t)(row0 + n) * row_stride + off0 + i] = buf[n];
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
int beam_logprob_launch(const void* logits, int in_f32, int rows, int V, int ld, float* out, int ld_out, hipStream_t s) {
  if (in_f32) hipLaunchKernelGGL(beam_logprob_kernel<true>, dim3(rows), dim3(BEAM_THREADS), 0, s, logits, V, ld, out, ld_out);
  else hipLaunchKernelGGL(beam_logprob_kernel<false>, dim3(rows), dim3(BEAM_THREADS), 0, s, logits, V, ld, out, ld_out);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int beam_step_launch(const float* logp, int ld, int B, int K, int V, int t, int max_new, float* beam_scores, const int64_t* seqs_in,
                     int64_t* seqs_out, float* hyp_score, int* hyp_len, int64_t* hyp_tokens, int* hyp_count, unsigned char* done,
                     int64_t* next_ids, int* parent, const int64_t* eos, int n_eos, int64_t pad, float length_penalty, int early, int last,
                     hipStream_t s) {
  BeamParams p;
  p.logp = logp; p.ld = ld; p.K = K; p.V = V; p.t = t; p.max_new = max_new;
  p.beam_scores = beam_scores; p.seqs_in = seqs_in; p.seqs_out = seqs_out;
  p.hyp_score = hyp_score; p.hyp_len = hyp_len; p.hyp_tokens = hyp_tokens; p.hyp_count = hyp_count; p.done = done;
  p.next_ids = next_ids; p.parent = parent; p.eos = eos; p.n_eos = n_eos; p.pad = pad; p.length_penalty = length_penalty;
  p.early = early; p.last = last;
  hipLaunchKernelGGL(beam_step_kernel, dim3(B), dim3(BEAM_THREADS), 0, s, p);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int kv_beam_reorder_launch(void* const* table, int n_tensors, const int* parent, const int* start_len, const int* cache_len, int B, int K,
                           int H, int cap, int row_bytes, int pos_lo, int pos_hi, hipStream_t s) {
  const int lo = pos_lo / REORDER_CHUNK * REORDER_CHUNK;
  if (pos_hi <= lo) return AKI_OK;
  const dim3 grid((pos_hi - lo + REORDER_CHUNK - 1) / REORDER_CHUNK, H, n_tensors * B);
  if (row_bytes % 16 == 0)
    hipLaunchKernelGGL(kv_beam_reorder_kernel<u32x4>, grid, dim3(REORDER_THREADS), 0, s, table, parent, start_len, cache_len, B, K, H, cap,
                       row_bytes / 16, lo);
  else
    hipLaunchKernelGGL(kv_beam_reorder_kernel<unsigned>, grid, dim3(REORDER_THREADS), 0, s, table, parent, start_len, cache_len, B, K, H, cap,
                       row_bytes / 4, lo);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

}  // namespace aki

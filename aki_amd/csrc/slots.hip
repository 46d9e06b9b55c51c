// slots.hip - in-flight batching for generate (include/aki_mi355x.h: aki_kv_slot_admit, aki_slot_tick): a prefilled request is copied into
// one row ("slot") of a larger KV cache, and a per-row token budget retires a row on the device.  aki_amd/slots.py and
// AkiMethods.generate_many (aki_amd/aki.py) are the host side.  Stop sequences (aki_stop_check, aki_slot_tick_stops; aki_amd/stops.py): a
// row also ends when its generated tokens end with one of its set's token sequences.
#include "aki_device.h"

namespace aki {

// ---- admit: one prefilled sequence into row `slot` of the slot cache -------------------------------------------------------------------
// table holds 2 * n_tensors base addresses: the sources [1, H, cap_src, row] first, then the destinations [B, H, cap_dst, row] (every layer's K
// and V).  For one (tensor, head) the rows 0 <= pos < len are ONE contiguous run of len * row bytes on both sides, so the copy is a flat
// stream of vectors: a workgroup owns ADMIT_THREADS * ADMIT_UNROLL consecutive vectors of it, a thread issues its ADMIT_UNROLL loads (lane i
// at base + i vectors: 1 KiB per wave and instruction at 16 bytes per lane) before its first store.  len is read on the device and clamped to
// both capacities: nothing outside [slot, h, 0 .. len) of a destination is written, nothing outside [0, h, 0 .. len) of a source is read.
constexpr int ADMIT_THREADS = 256;
constexpr int ADMIT_UNROLL = 4;

template <typename VT>
__global__ __launch_bounds__(ADMIT_THREADS) void kv_slot_admit_kernel(void* const* table, int n_tensors, const int* src_len, int H, int cap_src,
                                                                      int cap_dst, int slot, int row_vecs) {
  const int tensor = blockIdx.z, h = blockIdx.y;
  const int len = min(min(src_len[0], cap_src), cap_dst);
  if (len <= 0) return;
  const size_t n = (size_t)len * row_vecs;
  const size_t i0 = (size_t)blockIdx.x * (ADMIT_THREADS * ADMIT_UNROLL) + threadIdx.x;
  if (i0 >= n) return;
  const VT* src = (const VT*)table[tensor] + (size_t)h * cap_src * row_vecs;
  VT* dst = (VT*)table[n_tensors + tensor] + ((size_t)slot * H + h) * cap_dst * row_vecs;
  VT buf[ADMIT_UNROLL];
#pragma unroll
  for (int u = 0; u < ADMIT_UNROLL; ++u) {
    const size_t i = i0 + (size_t)u * ADMIT_THREADS;
    if (i < n) buf[u] = src[i];
  }
#pragma unroll
  for (int u = 0; u < ADMIT_UNROLL; ++u) {
    const size_t i = i0 + (size_t)u * ADMIT_THREADS;
    if (i < n) dst[i] = buf[u];
  }
}

// ---- tick: the per-row token budget, right behind the pick -------------------------------------------------------------------------------
// One thread per row.  generated = cache_len - start_len + 1 is the number of tokens the row has picked (token 0 comes from the prefill, with
// cache_len == start_len).  A live row at or over its budget becomes done at its last token; a done row - by this kernel or by the pick's
// eos check - is parked at cache_len = start_len + done_at, the cache row of the token it never feeds: the pad-token steps the loop still
// gives it overwrite that one dead row.  A done row without an index (done_at < 0) is left where it is.
__global__ __launch_bounds__(64) void slot_tick_kernel(unsigned char* done, int* done_at, int* cache_len, const int* start_len, const int* limit,
                                                       int B) {
  const int b = threadIdx.x;
  if (b >= B) return;
  const int start = start_len[b];
  bool d = done[b] != 0;
  int at = done_at[b];
  if (!d) {
    const int generated = cache_len[b] - start + 1;
    if (generated >= limit[b]) {
      at = generated - 1;
      done[b] = 1;
      done_at[b] = at;
      d = true;
    }
  }
  if (d && at >= 0) cache_len[b] = start + at;
}

// ---- stop sequences: a row ends when its generated tokens end with one of its set's sequences ---------------------------------------------
// The pool: ids holds every sequence one behind the other, sequence s is ids[seq_off[s] .. seq_off[s + 1]), set k is the sequences
// set_first[k] .. set_first[k + 1], row b is checked against set row_set[b].  One wave per row, lane l owns sequence l of the row's set
// (a set holds at most 64).  Every index read from the pool is range-checked against the pool's counts before it is used, so a bad pool
// or a row_set outside it reads nothing: such a row has no stops.
struct StopPool {
  const int* ids;
  const int* seq_off;
  const int* set_first;
  const int* row_set;
  int n_ids, n_seqs, n_sets;
};

// The index within row b's set of the lowest-numbered sequence that ends at row[t], or -1.  The whole wave calls it with the same b and t
// (0 <= t < the row's length); the result is the same in every lane.  A lane walks backwards from row[t] and leaves at the first mismatch;
// n <= t + 1 keeps the walk inside the row: only generated tokens count.
__device__ __forceinline__ int stop_match(const long long* row, int t, const StopPool& p, int b, int lane) {
  bool hit = false;
  const int set = p.row_set[b];
  if (set >= 0 && set < p.n_sets) {
    const int first = p.set_first[set], last = p.set_first[set + 1];
    if (first >= 0 && first <= last && last <= p.n_seqs && lane < last - first) {
      const int s = first + lane;
      const int o0 = p.seq_off[s], o1 = p.seq_off[s + 1];
      const int n = o1 - o0;
      if (o0 >= 0 && o1 <= p.n_ids && n >= 1 && n <= AKI_STOP_MAX_LEN && n <= t + 1) {
        hit = true;
        for (int i = 0; i < n; ++i) {
          if (row[t - i] != (long long)p.ids[o1 - 1 - i]) {
            hit = false;
            break;
          }
        }
      }
    }
  }
  const unsigned long long lanes = __ballot(hit);
  return lanes ? __ffsll(lanes) - 1 : -1;
}

// One wave per row, right behind the pick (and the log-probability): t = cache_len - start_len is the index the pick just wrote.  A done row
// and a row whose t is outside the token buffer are skipped.  Lane 0 alone writes.
__global__ __launch_bounds__(64) void stop_check_kernel(const long long* tokens, int tokens_ld, const int* cache_len, const int* start_len,
                                                        unsigned char* done, int* done_at, int* stop_hit, const StopPool p, int B) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B || done[b] != 0) return;
  const int t = cache_len[b] - start_len[b];
  if (t < 0 || t >= tokens_ld) return;
  const int hit = stop_match(tokens + (size_t)b * tokens_ld, t, p, b, lane);
  if (hit >= 0 && lane == 0) {
    done[b] = 1;
    done_at[b] = t;
    stop_hit[b] = hit;
  }
}

// stop_check_kernel followed by slot_tick_kernel for row b = blockIdx.x, in one launch: the wave checks the row's stops, lane 0 then runs the
// tick on the state it holds in registers (a stop and the budget at one token is a stop).
__global__ __launch_bounds__(64) void slot_tick_stops_kernel(unsigned char* done, int* done_at, int* cache_len, const int* start_len,
                                                             const int* limit, const long long* tokens, int tokens_ld, int* stop_hit,
                                                             const StopPool p, int B) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const int start = start_len[b], len = cache_len[b];
  bool d = done[b] != 0;
  int at = done_at[b];
  const int t = len - start;
  int hit = -1;
  if (!d && t >= 0 && t < tokens_ld) hit = stop_match(tokens + (size_t)b * tokens_ld, t, p, b, lane);
  if (lane != 0) return;
  if (hit >= 0) {
    at = t;
    done[b] = 1;
    done_at[b] = at;
    stop_hit[b] = hit;
    d = true;
  }
  if (!d) {
    const int generated = t + 1;
    if (generated >= limit[b]) {
      at = generated - 1;
      done[b] = 1;
      done_at[b] = at;
      d = true;
    }
  }
  if (d && at >= 0) cache_len[b] = start + at;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------------
int kv_slot_admit_launch(void* const* table, int n_tensors, const int* src_len, int H, int cap_src, int cap_dst, int slot, int row_bytes,
                         int vec_bytes, int host_len, hipStream_t s) {
  const int row_vecs = row_bytes / vec_bytes;
  const size_t n = (size_t)host_len * row_vecs;
  const size_t per_block = (size_t)ADMIT_THREADS * ADMIT_UNROLL;
  const dim3 grid((unsigned)((n + per_block - 1) / per_block), H, n_tensors);
  if (vec_bytes == 16)
    hipLaunchKernelGGL(kv_slot_admit_kernel<u32x4>, grid, dim3(ADMIT_THREADS), 0, s, table, n_tensors, src_len, H, cap_src, cap_dst, slot, row_vecs);
  else
    hipLaunchKernelGGL(kv_slot_admit_kernel<unsigned>, grid, dim3(ADMIT_THREADS), 0, s, table, n_tensors, src_len, H, cap_src, cap_dst, slot,
                       row_vecs);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int slot_tick_launch(unsigned char* done, int* done_at, int* cache_len, const int* start_len, const int* limit, int B, hipStream_t s) {
  hipLaunchKernelGGL(slot_tick_kernel, dim3(1), dim3(64), 0, s, done, done_at, cache_len, start_len, limit, B);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int stop_check_launch(const int64_t* tokens, int tokens_ld, const int* cache_len, const int* start_len, unsigned char* done, int* done_at,
                      int* stop_hit, const int* ids, int n_ids, const int* seq_off, int n_seqs, const int* set_first, int n_sets,
                      const int* row_set, int B, hipStream_t s) {
  const StopPool p{ids, seq_off, set_first, row_set, n_ids, n_seqs, n_sets};
  hipLaunchKernelGGL(stop_check_kernel, dim3(B), dim3(64), 0, s, (const long long*)tokens, tokens_ld, cache_len, start_len, done, done_at,
                     stop_hit, p, B);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

int slot_tick_stops_launch(unsigned char* done, int* done_at, int* cache_len, const int* start_len, const int* limit, const int64_t* tokens,
                           int tokens_ld, int* stop_hit, const int* ids, int n_ids, const int* seq_off, int n_seqs, const int* set_first,
                           int n_sets, const int* row_set, int B, hipStream_t s) {
  const StopPool p{ids, seq_off, set_first, row_set, n_ids, n_seqs, n_sets};
  hipLaunchKernelGGL(slot_tick_stops_kernel, dim3(B), dim3(64), 0, s, done, done_at, cache_len, start_len, limit, (const long long*)tokens,
                     tokens_ld, stop_hit, p, B);
  AKI_LAUNCH_CHECK();
  return AKI_OK;
}

}  // namespace aki

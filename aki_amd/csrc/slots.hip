// slots.hip - in-flight batching for generate (include/aki_mi355x.h: aki_kv_slot_admit, aki_slot_tick): a prefilled request is copied into
// one row ("slot") of a larger KV cache, and a per-row token budget retires a row on the device.  aki_amd/slots.py and
// AkiMethods.generate_many (aki_amd/aki.py) are the host side.
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

}  // namespace aki

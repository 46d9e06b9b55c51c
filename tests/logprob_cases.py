"""Data and float64 reference for ops.token_logprob (logprob.hip): the log-probability of one chosen column per row under the row's
log-softmax, with the top_k columns ranked on the input values (equal values: the lower column first).

The rows are bf16-exact f32 values, so the bf16 and the f32 kernels see the same numbers and the ranking on the inputs is exact.

THE ERROR BOUND of the kernel's f32 arithmetic, derived as beam_cases.logprob_bound is (first order, u = 2^-24, M = max |finite logit|):
the kernel's reduction differs from beam_logprob_kernel's only in which columns a thread owns.  With 16-byte loads a thread adds the 8 (bf16)
or 4 (f32) columns of each of its vectors in turn, then one tail column: at most 8 * ceil(V / 8192) + 1 <= ceil(V / 1024) + 8 terms, against
ceil(V / 1024) on the column-by-column path (which unaligned rows take) and in beam.hip.  Everything else is the same arithmetic:
  d = x - m: u * 2M.  expf(d): relative 2M u + 4u.  The sum of the V non-negative terms: (ceil(V / 1024) + 8) + 6 butterfly levels + 15 wave
  sums: relative (ceil(V / 1024) + 29) u.  logf: the sum's relative error + 4u ln V.  m + log s: u (M + ln V).  x - lse: u (2M + ln V).
    E(M, V) = u * (5 M + 6 ln V + ceil(V / 1024) + 34)        = beam_cases.logprob_bound(M, V) + 8 u
-inf columns add exact zeros to the sum and take no part in M; a chosen or ranked -inf column has logprob -inf exactly."""
import math

import numpy as np

U = 2.0 ** -24
KERNEL_THREADS = 1024          # logprob.hip: LP_THREADS
TOP_KS = (0, 1, 8)             # every case is run at each; 8 = ops.LOGPROB_MAX_TOP


def logprob_bound(M, V):
    return U * (5.0 * M + 6.0 * math.log(V) + math.ceil(V / KERNEL_THREADS) + 34.0)


def bf16_exact(x):
    """f32 array -> the nearest bf16 value (ties to even) as f32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# name -> (V, rows, M, kind)
CASES = {
    "v2_m1": (2, 3, 1.0, "plain"),
    "v1023_m30": (1023, 1, 30.0, "plain"),
    "v1024_m1": (1024, 3, 1.0, "plain"),
    "v1025_m80": (1025, 33, 80.0, "plain"),
    "v32013_m30": (32013, 3, 30.0, "plain"),
    "v32013_m1_rows33": (32013, 33, 1.0, "plain"),
    "ties_v1025": (1025, 3, 30.0, "ties"),
    "neginf_v1024": (1024, 3, 30.0, "neginf"),
    "neginf_v32013": (32013, 3, 80.0, "neginf"),
}
TIE_COLUMNS = (1000, 5, 77, 512, 513, 900, 64, 63, 1024, 300)      # row 0 of a "ties" case: ten columns share the largest value
NEGINF_FINITE = (3, 700, 701, 1023, 40)                             # row 1 of a "neginf" case: the only finite columns (fewer than 8)


def make(name):
    """-> (x f32 [rows, V] of bf16-exact values, ids int64 [rows])."""
    V, rows, M, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1234)
    x = rng.standard_normal((rows, V)).astype(np.float32)
    x = bf16_exact(x * (M / np.abs(x).max(axis=1, keepdims=True)))           # every row reaches |x| = M
    ids = np.array([0 if r % 3 == 0 else V - 1 if r % 3 == 1 else int(rng.integers(0, V)) for r in range(rows)], dtype=np.int64)
    if kind == "ties":
        top = np.float32(M)
        x[0] = np.minimum(x[0], np.float32(M / 2))
        x[0, list(TIE_COLUMNS)] = top                  # ten equal maxima: a tie inside the top 8, across rank 8 | 9 and across rank 1 | 2
        x[1] = np.minimum(x[1], np.float32(M / 2))
        for col, below in zip((9, 800, 21, 20, 400, 1001, 1002, 1024, 33, 2), (0, 1, 2, 2, 4, 5, 6, 7, 7, 9)):
            x[1, col] = np.float32(M - below)          # small integers: the 3rd = 4th and the 8th = 9th largest tie, the rest are distinct
        x[2] = np.float32(-M)                          # a constant row: every rank is a tie
        ids[:] = (TIE_COLUMNS[0], 21, V - 1)
    if kind == "neginf":
        holes = rng.choice(V, size=V // 10, replace=False)
        x[0, holes] = -np.inf
        x[0, 17] = np.float32(M)                       # the row keeps a finite maximum
        keep = x[1, list(NEGINF_FINITE)].copy()
        x[1] = -np.inf
        x[1, list(NEGINF_FINITE)] = keep
        x[2, 0] = x[2, V - 1] = -np.inf
        ids[:] = (int(holes[0]) if holes[0] != 17 else int(holes[1]), NEGINF_FINITE[1], 0)      # a -inf column, a finite one, -inf at column 0
    return x, ids


def reference(x, ids, k):
    """float64: (logprob [rows], top ids int64 [rows, k] (-1 behind the row's V columns), top logprobs [rows, k] (-inf there), the kernel's
    bound per row [rows])."""
    x64 = np.asarray(x, dtype=np.float64)
    rows, V = x64.shape
    m = x64.max(axis=1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(axis=1))
    lp = x64[np.arange(rows), ids] - lse
    top_ids = np.full((rows, k), -1, dtype=np.int64)
    top_lp = np.full((rows, k), -np.inf)
    for r in range(rows):
        order = np.lexsort((np.arange(V), -x64[r]))[:k]          # descending value, then ascending column
        top_ids[r, :order.size] = order
        top_lp[r, :order.size] = x64[r, order] - lse[r]
    finite = np.where(np.isfinite(x64), np.abs(x64), 0.0).max(axis=1)
    bound = np.array([logprob_bound(float(M), V) for M in finite])
    return lp, top_ids, top_lp, bound

"""Row table, draws and float64 references of the per-row device sampler (aki_amd/csrc/decode.hip: sample_pick_kernel<true>, C entry
aki_sample_pick_rows, ops.sample_pick_rows) - the sampler of generate_many, where every row has its own temperature, top_k, top_p
and Philox key.  numpy only; everything is built from tests/sampling_cases.py (its Case, reference, uniform, accepted and DELTA, unchanged).

Six rows at V = V_SMALL (1003: the scalar tails of every loop), each passed through find_salt:
  row  sigma  T    k     p
  0    2      0.7  0     1.0
  1    2      1.0  1     1.0    the greedy row (top_k == 1 takes the greedy pick)
  2    2      1.3  50    0.9
  3    4      0.7  1000  0.5
  4    2      1.0  0     0.9
  5    the same Case as row 0 - the same logits and parameters - with row 0's seed: equal tokens in different rows
One distinct 64-bit seed per row (row 5 excepted): SEED ^ (0x9E3779B97F4A7C15 * (r + 1) mod 2^64).

The draw of row b at generated-token index n is u = sampling_cases.uniform(n, 0, 0, seed=seed_b): key = the row's seed, counter
(n, 0, 0, 0) - the row index is NOT in the counter.  n = 0..255.

The cap (a condition on the inputs, asserted by tests/test_many_sampling_cases_cpu.py): per row, the share of draws with more than one
acceptable token (accept_set_sizes > 1) is at most 0.02, so `accepted` decides almost every draw to a single token.

V_MAIN_ROWS: three rows at V = 32064 for one pass of 64 steps; the unfiltered row keeps sampling_cases' limit of 0.15."""
import numpy as np

import sampling_cases as S

MASK64 = (1 << 64) - 1
STEPS = 256
MULTI_CAP = 0.02
MAIN_STEPS, MAIN_UNFILTERED_CAP = 64, 0.15


def row_seed(r: int) -> int:
    return S.SEED ^ ((0x9E3779B97F4A7C15 * (r + 1)) & MASK64)


_ROWS = None
_MAIN = None


def rows():
    """[(Case, seed)] of the six rows, built once."""
    global _ROWS
    if _ROWS is None:
        table = [S.Case("rows-0", S.V_SMALL, 2.0, 0.7, 0, 1.0), S.Case("rows-1", S.V_SMALL, 2.0, 1.0, 1, 1.0),
                 S.Case("rows-2", S.V_SMALL, 2.0, 1.3, 50, 0.9), S.Case("rows-3", S.V_SMALL, 4.0, 0.7, 1000, 0.5),
                 S.Case("rows-4", S.V_SMALL, 2.0, 1.0, 0, 0.9)]
        cases = [S.find_salt(c) for c in table]
        cases.append(cases[0])
        _ROWS = [(c, row_seed(0 if r == 5 else r)) for r, c in enumerate(cases)]
    return _ROWS


def main_rows():
    """[(Case, seed)] of the three V_MAIN rows."""
    global _MAIN
    if _MAIN is None:
        table = [S.Case("rows-main-0", S.V_MAIN, 2.0, 0.7, 0, 1.0), S.Case("rows-main-1", S.V_MAIN, 2.0, 1.3, 50, 0.9),
                 S.Case("rows-main-2", S.V_MAIN, 2.0, 1.0, 1000, 0.5)]
        _MAIN = [(S.find_salt(c), row_seed(8 + r)) for r, c in enumerate(table)]
    return _MAIN


def draws(seed: int, steps: int = STEPS, row: int = 0) -> np.ndarray:
    """u of a row with key `seed` for n = 0..steps-1.  row: counter word 1 - 0 is the rule; anything else is the mutation "the row index
    is in the counter"."""
    return S.uniform(np.arange(steps), row, 0, seed=seed)


_REFS = {}


def reference(c: S.Case) -> S.Ref:
    """sampling_cases.reference, computed once per case and shared."""
    if c.name not in _REFS:
        _REFS[c.name] = S.reference(c)
    return _REFS[c.name]


def multi_share(c: S.Case, u: np.ndarray) -> float:
    return float((S.accept_set_sizes(reference(c), u) > 1).mean())


def param_arrays(table):
    """(temperature f32, top_k int32, top_p f32, seed int64 with the key's bits) of a row table, as numpy arrays."""
    T = np.array([c.T for c, _ in table], np.float32)
    k = np.array([c.k for c, _ in table], np.int32)
    p = np.array([c.p for c, _ in table], np.float32)
    seed = np.array([s for _, s in table], np.uint64).view(np.int64)
    return T, k, p, seed

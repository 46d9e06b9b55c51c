"""Case table, inputs, float64 reference and reference mutations of the device sampler (aki_amd/csrc/decode.hip: sample_pick_kernel,
C entry aki_sample_pick, ops.sample_pick).

numpy only (tests/test_sampling_cases_cpu.py adds CPU torch and the installed transformers for the comparison with HF's warpers).
tests/test_sampling_cases_cpu.py checks the table itself - the Philox restatement against its known answers, the conditions on the
inputs, the f32 restatement of the kernel's summation order against float64, and that every mutation of the reference is caught -
and tests/test_sampling_gpu.py runs every case on the device.

The reference, per row, in HF's order (processors -> temperature -> top-k -> top-p -> softmax -> multinomial):
  x      the bf16 logits as f32; with processors, the f32 arithmetic of aki_logits_process (repetition penalty, then bans to -inf)
  y      f32(x / T), one correctly rounded division
  top-k  0 < k < V: keep y >= the k-th largest y (ties at the threshold all kept)
  top-p  p < 1: among those, keep i iff the softmax mass of the tokens with strictly larger y is < p (equal values stay together)
  draw   w = exp(y - max) over the kept set in float64, C = inclusive cumulative sum in index order, C / C_total compared with
         u = ((x0 >> 8) + 0.5) 2^-24, x0 = Philox4x32-10(key = seed, counter = (n, b, offset, 0))[0]; the token is the smallest kept i
         with C_i / C_total > u.

Accepting a device token.  The device sums in f32, so a token t is accepted for a draw u iff t is kept and
  C64_{t-1} / S - DELTA <= u <= C64_t / S + DELTA.

DELTA = 2e-6, from f32 arithmetic in the kernel's summation order (unit roundoff eps = 2^-24 = 5.96e-8, first order).  A term w_j of
C_i passes through at most
   9 additions inside its thread's chunk at V = 32064 (groups of four summed pairwise: 2, then up to 7 sequential group additions;
     the owner's running sum has the same depth),
   6 + 4 + 1 additions of the block scan (shuffle scan over 64 lanes, shuffle scan over the 16 wave totals, prefix + lane value),
   1 addition of the chunk's prefix to the running sum,
and carries 2 eps of expf (1 ulp) and |y_j - max| eps from the rounding of the exponent's argument; the comparison adds 1 eps for the
product u * C_total.  The mass-weighted mean of |y_j - max| is asserted to stay below MAX_MEAN_GAP = 8 on every case (it is 1 - 5 on
N(0, sigma) rows: the mass sits near the maximum).  Sum: (9 + 11 + 1 + 2 + 8 + 1) eps = 32 eps = 1.9e-6 <= DELTA.  The bound is on
|C_i / C_total - C64_i / S| because the same w_j errors enter numerator and denominator with the same sign.  The CPU test asserts that
an f32 numpy restatement in that order stays within DELTA / 2 of float64 on every case.
"""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

DELTA = 2e-6
MAX_MEAN_GAP = 8.0
THREADS = 1024                       # PICK_THREADS
V_MAIN, V_SMALL = 32064, 1003        # 1003 % 8 == 3: the scalar tails of every loop
SEED = 0x1234_5678_9ABC_DEF1
ROWS, STEPS, OFFSETS = 8, 25, (0, 1, 2, 3, 5, 8, 13, 21, 34, 1 << 20)     # 8 * 25 * 10 = 2000 draws per case
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)
MUTATIONS = ("exclusive_cdf", "index_plus_one", "temperature_ignored", "topk_strict", "topp_own_mass", "counter_swapped",
             "offset_ignored")


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers: counter (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(c) & 0xFFFFFFFF for c in ctr)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        m0, m1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (m1 >> 32) ^ c1 ^ k0, m1 & 0xFFFFFFFF, (m0 >> 32) ^ c3 ^ k1, m0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_word0(n, b, offset, seed):
    """Vectorised first word for arrays n, b, offset (uint64 arithmetic on numpy arrays) - checked against philox4x32_10."""
    n, b, offset = np.broadcast_arrays(np.asarray(n, np.uint64), np.asarray(b, np.uint64), np.asarray(offset, np.uint64))
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = n & M, b & M, offset & M, offset >> np.uint64(32)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        m0, m1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (m1 >> np.uint64(32)) ^ c1 ^ k0, m1 & M, (m0 >> np.uint64(32)) ^ c3 ^ k1, m0 & M
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c0


def uniform(n, b, offset, seed=SEED, swap=False, no_offset=False):
    """u = ((x0 >> 8) + 0.5) 2^-24 in float64 (exact)."""
    if swap:
        n, b = b, n
    if no_offset:
        offset = np.zeros_like(np.asarray(offset))
    return ((philox_word0(n, b, offset, seed) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def bf16_round(x: np.ndarray) -> np.ndarray:
    """f32 -> the nearest bf16 (ties to even), as f32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


@dataclass
class Case:
    name: str
    V: int
    sigma: float
    T: float
    k: int
    p: float
    kind: str = "normal"              # normal | neg_inf | ties
    penalty: float = 1.0              # repetition penalty over `history`
    history: Tuple[int, ...] = ()
    suppress: Tuple[int, ...] = ()
    salt: int = 0                     # bumped by find_salt until the conditions on the inputs hold

    @property
    def processed(self) -> bool:
        return self.penalty != 1.0 or bool(self.suppress)

    @property
    def filtered(self) -> bool:
        return 0 < self.k < self.V or self.p < 1.0


def logits(c: Case) -> np.ndarray:
    """The case's bf16 logits row, as f32."""
    g = np.random.default_rng([zlib.crc32(c.name.encode()), c.salt])
    x = g.standard_normal(c.V).astype(np.float32) * np.float32(c.sigma)
    if c.kind == "neg_inf":           # all but 37 columns are -inf
        live = g.choice(c.V, 37, replace=False)
        keep = x[live]
        x[:] = -np.inf
        x[live] = keep
    if c.kind == "ties":              # 40 distinct leaders in [5, 6.25), then 30 columns tied at 4.75: the top-50 threshold sits in the tie
        x = np.minimum(x, np.float32(3.0))
        idx = g.choice(c.V, 70, replace=False)
        x[idx[:40]] = np.float32(5.0) + np.arange(40, dtype=np.float32) * np.float32(0.03125)
        x[idx[40:]] = np.float32(4.75)
    return bf16_round(x)


def processed_scores(c: Case, x: np.ndarray) -> np.ndarray:
    """aki_logits_process's f32 arithmetic for the two processors the cases use: repetition penalty over the distinct history tokens,
    then the suppressed ids to -inf."""
    x = x.copy()
    if c.penalty != 1.0:
        h = np.unique(np.asarray(c.history, np.int64))
        pen = np.float32(c.penalty)
        x[h] = np.where(x[h] < 0, x[h] * pen, x[h] / pen).astype(np.float32)
    if c.suppress:
        x[list(c.suppress)] = -np.inf
    return x


@dataclass
class Ref:
    y: np.ndarray                     # f32 [V]
    kept: np.ndarray                  # bool [V]
    probs: np.ndarray                 # f64 [V], 0 outside kept
    cdf: np.ndarray                   # f64 [V] inclusive cumulative sum of probs in index order
    boundary_gap: float               # top-p: the smallest |mass above a class / S - p| over the classes (inf when p == 1)
    boundary_multiplicity: int        # top-p: the number of tokens in the last kept class (1: HF's set is the same set)
    mean_gap: float                   # mass-weighted mean of max - y


def reference(c: Case, x: Optional[np.ndarray] = None, mutation: Optional[str] = None) -> Ref:
    x = processed_scores(c, logits(c)) if x is None else x
    T = np.float32(1.0 if mutation == "temperature_ignored" else c.T)
    y = (x.astype(np.float32) / T).astype(np.float32)
    kept = np.ones(c.V, bool)
    if 0 < c.k < c.V:
        kth = np.partition(y, c.V - c.k)[c.V - c.k]
        kept = y > kth if mutation == "topk_strict" else y >= kth
    y64 = y.astype(np.float64)
    ymax = y64.max()
    gap, mult = float("inf"), 1
    if c.p < 1.0:
        w = np.where(kept, np.exp(y64 - ymax), 0.0)
        vals, inv = np.unique(y64[kept], return_inverse=True)                  # ascending classes of equal value
        mass = np.bincount(inv, weights=w[kept], minlength=len(vals))
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]]) / w.sum()      # mass of the strictly larger classes
        crit = above + mass / w.sum() if mutation == "topp_own_mass" else above
        keep_class = crit < c.p
        keep_class[-1] = True                                                  # at least the maximum
        gap = float(np.abs(above[:-1] - c.p).min()) if len(vals) > 1 else float("inf")
        mult = int(np.bincount(inv)[np.flatnonzero(keep_class)[0]])
        k2 = np.zeros(c.V, bool)
        k2[np.flatnonzero(kept)] = keep_class[inv]
        kept = k2
    w = np.where(kept, np.exp(y64 - ymax), 0.0)
    S = w.sum()
    probs = w / S
    return Ref(y, kept, probs, np.cumsum(w) / S, gap, mult, float((probs * np.where(probs > 0, ymax - y64, 0.0)).sum()))


def draws(c: Optional[Case] = None):
    """(n, b, offset) of the 2000 draws of a case, each an int64 array [len(OFFSETS), STEPS, ROWS].  The token index n starts at the
    length of the case's history: it is also the number of generated tokens the processors see."""
    o, n, b = np.meshgrid(np.asarray(OFFSETS, np.int64), np.arange(STEPS), np.arange(ROWS), indexing="ij")
    return n + (len(c.history) if c is not None else 0), b, o


def reference_tokens(r: Ref, u: np.ndarray, mutation: Optional[str] = None) -> np.ndarray:
    """The smallest kept i with C_i > u (the last kept index when there is none)."""
    idx = np.flatnonzero(r.kept & (r.probs > 0))
    c = r.cdf[idx]
    if mutation == "exclusive_cdf":
        c = c - r.probs[idx]
    j = np.minimum(np.searchsorted(c, u, side="right"), len(idx) - 1)
    t = idx[j]
    return np.minimum(t + 1, len(r.cdf) - 1) if mutation == "index_plus_one" else t


def accepted(r: Ref, tok: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Per draw: is the token kept, with u inside [C_{t-1} - DELTA, C_t + DELTA]?"""
    tok = np.asarray(tok, np.int64)
    ok = (tok >= 0) & (tok < len(r.cdf))
    t = np.where(ok, tok, 0)
    hi = r.cdf[t]
    lo = hi - r.probs[t]
    return ok & r.kept[t] & (u >= lo - DELTA) & (u <= hi + DELTA)


def accept_set_sizes(r: Ref, u: np.ndarray) -> np.ndarray:
    """How many tokens `accepted` would take for each draw."""
    idx = np.flatnonzero(r.kept)
    hi = r.cdf[idx]
    lo = np.concatenate([[0.0], hi[:-1]])
    shape, u = np.shape(u), np.asarray(u).reshape(-1)
    first = np.searchsorted(hi + DELTA, u, side="left")        # hi is non-decreasing: tokens with hi + DELTA >= u
    last = np.searchsorted(lo - DELTA, u, side="right")        # tokens with lo - DELTA <= u
    return (last - first).reshape(shape)


def mutated_tokens(c: Case, mutation: str) -> np.ndarray:
    """What a reference with one defect would draw, for the case's 2000 draws."""
    n, b, o = draws(c)
    r = reference(c, mutation=mutation if mutation in ("temperature_ignored", "topk_strict", "topp_own_mass") else None)
    u = uniform(n, b, o, swap=mutation == "counter_swapped", no_offset=mutation == "offset_ignored")
    return reference_tokens(r, u, mutation if mutation in ("exclusive_cdf", "index_plus_one") else None)


def f32_cdf_in_kernel_order(r: Ref) -> np.ndarray:
    """C_i / C_total as the kernel sums it, in f32: thread t owns `gpt` consecutive groups of four; a group is (w0 + w1) + (w2 + w3); the
    chunk sum adds the groups in order; the chunk sums go through a shuffle scan per 64 lanes and one over the 16 wave totals; the
    owner's running value is prefix + (run + partial group)."""
    f = np.float32
    V = len(r.y)
    ngroups = (V + 3) // 4
    gpt = (ngroups + THREADS - 1) // THREADS
    ymax = r.y.max()
    w = np.zeros(THREADS * gpt * 4, f)
    w[:V] = np.where(r.kept, np.exp((r.y - ymax).astype(f)).astype(f), f(0))
    w = w.reshape(THREADS, gpt, 4)
    part = np.stack([w[..., 0], w[..., 0] + w[..., 1], (w[..., 0] + w[..., 1]) + w[..., 2],
                     (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])], -1).astype(f)          # the running value inside a group
    run = np.zeros((THREADS, gpt), f)                                                           # the chunk's running sum before group g
    for g in range(1, gpt):
        run[:, g] = run[:, g - 1] + part[:, g - 1, 3]
    csum = (run[:, -1] + part[:, -1, 3]).astype(f)

    def shuffle_scan(v):              # inclusive, along the last axis
        v = v.copy()
        o = 1
        while o < v.shape[-1]:
            nxt = v.copy()
            nxt[..., o:] = v[..., o:] + v[..., :-o]
            v, o = nxt, o * 2
        return v

    inc = shuffle_scan(csum.reshape(THREADS // 64, 64))
    wt = shuffle_scan(inc[:, -1])
    exl = np.concatenate([np.zeros((THREADS // 64, 1), f), inc[:, :-1]], 1)
    pre = np.concatenate([[f(0)], wt[:-1]]).astype(f)[:, None]
    excl = np.where(np.arange(THREADS // 64)[:, None] > 0, pre + exl, exl).astype(f).reshape(THREADS)
    C = (excl[:, None, None] + (run[:, :, None] + part)).astype(f).reshape(-1)[:V]
    return C.astype(np.float64) / np.float64(wt[-1])


def find_salt(c: Case) -> Case:
    """The first salt whose row meets the conditions on the inputs that depend on chance (see conditions_hold)."""
    for salt in range(64):
        c.salt = salt
        if conditions_hold(c)[0]:
            return c
    raise AssertionError(f"no salt below 64 gives {c.name} a row that meets the conditions")


def conditions_hold(c: Case):
    """(ok, facts): the top-p boundary is further than DELTA (x8: room for the f32 mass sums) from top_p, the maximum is unique where
    the case is compared with the greedy pick (top_k == 1 IS the greedy pick, lowest index among equal maxima, while the filter's own
    rule would keep every one of them; top_p = 1e-6 keeps the maximum's class), and the share of draws with more than one acceptable token is within the limit."""
    r = reference(c)
    n, b, o = draws(c)
    multi = float((accept_set_sizes(r, uniform(n, b, o)) > 1).mean())
    kept = int(r.kept.sum())
    limit = 0.02 if kept <= 1000 else 0.15 if not c.filtered else 1.0
    y = r.y
    unique_max = int((y == y.max()).sum()) == 1
    ok = r.boundary_gap > 8 * DELTA and multi <= limit and r.mean_gap <= MAX_MEAN_GAP and (unique_max or (c.p > 1e-5 and c.k != 1))
    return ok, dict(kept=kept, multi=multi, limit=limit, gap=r.boundary_gap, mult=r.boundary_multiplicity, mean_gap=r.mean_gap)


def _table():
    out = []
    for sigma in (2.0, 4.0):
        for T in (0.7, 1.0, 1.3):
            for k in (0, 1, 50, 1000):
                for p in (1.0, 0.9, 0.5, 1e-6):
                    out.append(Case(f"main-s{sigma:g}-T{T:g}-k{k}-p{p:g}", V_MAIN, sigma, T, k, p))
    hist = tuple(range(5, 3000, 7))
    for T in (0.7, 1.3):
        for k in (0, 50):
            for p in (1.0, 0.9):
                out.append(Case(f"proc-T{T:g}-k{k}-p{p:g}", V_MAIN, 2.0, T, k, p, penalty=1.3, history=hist,
                                suppress=tuple(range(100, 4000, 3))))
    for k in (0, 1, 50, 1000):
        for p in (1.0, 0.9, 0.5):
            out.append(Case(f"small-k{k}-p{p:g}", V_SMALL, 2.0, 0.7, k, p))
    out.append(Case("small-proc", V_SMALL, 2.0, 1.3, 50, 0.9, penalty=1.5, history=tuple(range(0, 1003, 5)), suppress=(1, 2, 1002)))
    for k, p in ((0, 1.0), (10, 1.0), (50, 0.9), (0, 0.5)):
        out.append(Case(f"neginf-k{k}-p{p:g}", V_MAIN, 2.0, 1.0, k, p, kind="neg_inf"))
    for k, p in ((50, 1.0), (50, 0.9), (0, 0.8), (45, 1.0)):
        out.append(Case(f"ties-k{k}-p{p:g}", V_MAIN, 2.0, 1.0, k, p, kind="ties"))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = [find_salt(c) for c in _table()]
    return _CASES

"""Case table, inputs, float64 reference, componentwise tolerance and reference mutations of the training attention path
(aki_amd/csrc/attn_bwd_bf16.hip: attn_delta_kernel, attn_bwd_dkv_kernel, attn_bwd_dq_kernel, masked or plain, head_dim 96 or 64, fed
with the o / lse of ops.mma_attn_core or ops.attention).

numpy and CPU torch only.  tests/test_attn_bwd_cases_cpu.py checks the table itself - the reference against float64 autograd, every
named corner reached, every mutation visible - and tests/test_attn_bwd_gpu.py runs every case on the device.

Why a componentwise bar.  dk[0] and dv[0] collect from every query, late keys from a handful: a bar relative to the tensor's maximum
lets a wrong small row through.  Here every output element x = sum_i t_i is held to

    tol(x) = KAPPA * 2^-9 * M(x) + 2^-8 * |x|,        M(x) = sum_i |t_i|   (computed from the float64 reference)

Derivation of KAPPA (first order; unit 2^-9; u = 2^-8 = 2 units is the unit roundoff of bf16, round to nearest even).
  e_P   relative error of a recomputed P = exp2(s scale log2e - lse log2e): the f32 dot product of 96 exact bf16 products
        (<= 96 * 2^-24 * sum_d |q_d k_d| * scale, below 2^-11.4 while sum_d |q_d k_d| scale <= 64, which the CPU test asserts of the
        inputs), exp2 / log of the hardware (a few 2^-23) and the f32 lse of the 32-row forward (which sums the UNROUNDED p): together
        below 2^-10 = 0.5 units.  f32 accumulation over n <= 1792 terms adds n * 2^-24 M < 0.06 units and rides in the same half unit.
  o     = sum_k bf16(p_k) v_k / l: one cast per term, u * M_o, and e_P:                                     KAPPA = 2 + 0.5 = 2.5
  dv    = sum_q bf16(P) dO: the same:                                                                      KAPPA = 2.5
  delta = sum_d dO_d bf16(o_d) = sum_k w_k dP_k with w_k = bf16(p_k) / l the weights the forward really used.  Two sources:
        the forward's casts, |w_k - P_k| <= u P_k, give u * sum_k P_k |dP_k|; the cast of o gives sum_d |dO_d| * 2^-8 * hb(o_d),
        hb(x) = 2^floor(log2 |x|) <= |x| (half an ulp of the binade o_d lies in).  Both are 2 units of
            E[q] = sum_k P_k |dP_k| + sum_d |dO_d| hb(o_d).
  dS    = bf16(P' (dP' - delta')): the cast and e_P act on |dS| (2 + 0.5 units), the error of delta on P * E (2 units), the f32 error of
        dP (96 * 2^-24 * A, A = sum_d |dO_d| |v_d|) on P * A, which enters M with the weight 2^-8.  So with
            W[q, k] = |dS| + P (E[q] + 2^-8 A[q, k]),    M_dq = scale sum_k W |K|,    M_dk = scale sum_q W |Q|:     KAPPA = 2.5
  lse   32-row forward and ops.attention: f32 arithmetic on m + log2 l, |m| < 64: 2^-16 absolute + 2^-20 |lse|.
The 64-row forward core (mma_attn64_bf16.hip) sums the bf16-ROUNDED p on the matrix pipe: l' = sum_k p_k (1 + e_k), |e_k| <= u, so
|lse' - lse| <= log(1 + u) < 2^-8 (all casts the same way; typically far less), and 2^-16 + 2^-20 |lse| of f32 as before.  Every P the
backward recomputes from it is off by that factor, 2 more units on |dS| and on dv's terms; its o divides by the rounded sum (2 more
units on M_o) and its weights w_k are off by 2u, 2 more units on delta.  With the 64-row forward KAPPA = 4.5 for every output.
These are worst-case bounds: rounding errors of different terms do not line up, a kernel normally sits several times below them
(the GPU test records the largest err / tol per kernel), and a case above them is a finding.

Two of the issue's mutations perturb every term of an element by a fixed relative amount and are capped by this bar whatever
the inputs: "lse off by 2^-6" scales every term of x by e^(2^-6) - 1 = 8.06 units, a ratio of 8.06 |x| / (2.5 M + 2 |x|) <= 1.79;
"delta scaled by 1 - 2^-4" moves dS by 32 units of P |delta|, and P E >= P |delta| (1 + hb / |o|) holds the ratio below 32 / (2.5 * 1.5)
= 8.5 - reached only where a row sees a single key, dO is aligned with that key's v and |v_d| sits just below a power of two (hb = |v| /
1.99), which the sentinel family builds on row 0.  CAPPED lists the first with the ratio it must reach.

Two input families, everything rounded to bf16 first.
  diffuse   q, k ~ N(0, 1); v and dO are |N(0, 1)| with a random sign per (head, feature) column, so that the terms of dv do not
            cancel (M ~ |dv|) and a missing 32-row tile is a fixed share of the element whatever the length.
  sentinel  a short list of (query, key) pairs per sample at the structural edges (sentinel_pairs).  Sentinel keys are random
            directions of norm sqrt(Dh); each sentinel row's q is the minimum-norm vector whose scores against its own sentinel
            keys are LEVEL = ln(100 Lk), so these hold most of the row's mass about equally, and dO on sentinel rows is SENT_DO times
            larger than elsewhere, which makes the pair a large share of M in dv[k], dk[k] and dq[q].  Forbidden pairs just outside
            each edge (the column at col_hi, the row at row_hi, the column after the diagonal, a masked column, row seq_len) get
            the score LEVEL + LIFT and, for the key, v = 50: one leaked pair dominates.
"""
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

FAMILIES = ("diffuse", "sentinel")
CORES = ("32", "64")                         # which forward produced o and lse: the 32-row core / ops.attention, or the 64-row core
KAPPA = {"32": 2.5, "64": 4.5}
LSE_ABS = {"32": 2.0 ** -16, "64": 2.0 ** -8 + 2.0 ** -16}
LSE_REL = 2.0 ** -20
MIN_RATIO = 8.0
CAPPED = {"lse+2^-6": 1.75}                  # see the module docstring: the bar itself caps this one at 1.79
FORBIDDEN_V = 50.0
LIFT = 2.0
SENT_DO = 16.0
TQ, BLK = 32, 128                            # rows / keys per streamed tile and per workgroup of attn_bwd_dkv / attn_bwd_dq
MAX_SCORE_TERMS = 64.0                       # sum_d |q_d k_d| scale allowed by the e_P term of the derivation


@dataclass(frozen=True)
class Case:
    id: str
    masked: bool
    B: int
    H: int
    Dh: int
    Lq: int
    Lk: int
    rects: Optional[tuple] = None            # per sample: ((row_lo, row_hi, col_lo, col_hi), ...), all-zero entries included; None: no table
    holes: Optional[tuple] = None            # per sample: masked column ranges [lo, hi); None: col_valid_bits absent
    seq_lens: Optional[tuple] = None
    why: str = ""

    @property
    def scale(self):
        return self.Dh ** -0.5

    def seq_len(self, b):
        return self.Lq if self.seq_lens is None else min(self.seq_lens[b], self.Lq)

    def valid(self, b):
        v = np.ones(self.Lk, dtype=bool)
        if self.holes is not None:
            for lo, hi in self.holes[b]:
                v[lo:hi] = False
        return v

    def live_rects(self, b, table=None):
        rects = self.rects if table is None else table
        return [] if rects is None else [r for r in rects[b] if r[1] > r[0] and r[3] > r[2]]

    def visible(self, b, rects_of=None, valid_of=None, seq_of=None) -> np.ndarray:
        """[Lq, Lk] bool by the rule of include/aki_mi355x.h: valid(c) && r < seq_len && (c <= r || (r, c) inside a rectangle).
        rects_of / valid_of / seq_of: take that part of the table from another sample (a mutation)."""
        if not self.masked:
            return np.ones((self.Lq, self.Lk), dtype=bool)
        r, c = np.arange(self.Lq)[:, None], np.arange(self.Lk)[None, :]
        vis = c <= r
        for rlo, rhi, clo, chi in self.live_rects(b if rects_of is None else rects_of):
            vis = vis | ((r >= rlo) & (r < rhi) & (c >= clo) & (c < chi))
        return vis & self.valid(b if valid_of is None else valid_of)[None, :] & (r < self.seq_len(b if seq_of is None else seq_of))

    def mask_1d(self):
        return np.stack([self.valid(b) for b in range(self.B)])

    def rect_table(self):
        """What MaskTable.from_host takes, or None."""
        return None if self.rects is None else [list(rs) for rs in self.rects]


Z = (0, 0, 0, 0)


def _m(id, B, H, L, rects=None, holes=None, seq_lens=None, why=""):
    if rects is not None:
        rects = tuple(tuple(tuple(r) for r in rs) for rs in rects)
        assert len(rects) == B and all(0 < len(rs) <= 8 for rs in rects), id
        for rs in rects:                      # inside the matrix, row ranges disjoint (the ABI's condition)
            live = sorted(r for r in rs if r[1] > r[0] and r[3] > r[2])
            assert all(0 <= r[0] < r[1] <= L and 0 <= r[2] < r[3] <= L for r in live), id
            assert all(a[1] <= b_[0] for a, b_ in zip(live, live[1:])), f"{id}: overlapping row ranges"
    if holes is not None:
        holes = tuple(tuple(tuple(h) for h in hs) for hs in holes)
        assert len(holes) == B and all(0 <= lo < hi <= L for hs in holes for lo, hi in hs), id
    if seq_lens is not None:
        assert len(seq_lens) == B and all(0 < s <= L for s in seq_lens), id
        seq_lens = tuple(seq_lens)
    return Case(id, True, B, H, 96, L, L, rects, holes, seq_lens, why)


def _p(Dh, B, H, Lq, Lk, why=""):
    return Case(f"plain-d{Dh}-b{B}-h{H}-{Lq}x{Lk}", False, B, H, Dh, Lq, Lk, why=why)


N = ()
CASES = (
    _m("L1-b1-h2-causal-no-table", 1, 2, 1, why="one row, one key; no rectangles, no bits, no seq_lens"),
    _m("L31-b2-h1-rect-mid-tile", 2, 1, 31, [[(2, 20, 20, 29)], [Z]], [N, N], why="everything inside one partial 32-row tile; a sample with an all-zero table"),
    _m("L32-b1-h3-rect-to-L", 1, 3, 32, [[(4, 16, 16, 32)]], [N], why="exactly one tile; col_hi = L on the tile edge"),
    _m("L33-b3-h2-ragged-17-32-33", 3, 2, 33, [[(3, 10, 10, 33)], [(3, 10, 10, 30)], [Z]], [N, N, [(5, 7)]], [33, 32, 17],
       why="one row past a tile; seq_len on the tile edge and mid-tile; a hole inside a word"),
    _m("L127-b2-h3-leftpad5-rect-one-short", 2, 3, 127, [[Z], [(10, 31, 31, 127)]], [[(0, 5)], N],
       why="left padding: rows 0..4 see nothing; row_hi and col_hi one short of 32 / 128"),
    _m("L128-b1-h2-rect-on-edges", 1, 2, 128, [[(10, 32, 32, 128)]], [N], why="one full workgroup; row_hi and col_lo on 32, col_hi on 128"),
    _m("L129-b2-h1-rect-one-past", 2, 1, 129, [[(10, 33, 33, 129)], [Z]], [N, N],
       why="a second workgroup of one row / one key; row_hi and col_hi one past 32 / 128: the rectangle touches the block by one column"),
    _m("L257-b2-h3-causal-no-table", 2, 3, 257, why="pure causal over three workgroups, no table at all: col_valid_bits absent"),
    _m("L257-b3-h2-two-rects-above-diagonal-empty-blocks", 3, 2, 257,
       [[(4, 40, 40, 100), (50, 120, 130, 257)], [(8, 24, 200, 230), Z], [(3, 10, 10, 100)]], [N, N, [(60, 70)]], [257, 257, 120],
       why="two rectangles; one wholly above the diagonal (rows 8..23 x keys 200..229: Q tile 0 is needed by key block 1 and key tiles "
           "6, 7 by query block 0 only through it); seq_len 120 leaves two trailing 128-blocks without work; a hole across a 64-bit word"),
    _m("L333-b2-h3-four-and-eight-rects-ragged", 2, 3, 333,
       [[(3, 30, 30, 64), Z, (33, 95, 96, 129), (100, 128, 128, 300), (129, 160, 161, 333), Z, Z, Z],
        [(2, 10, 20, 40), (12, 20, 40, 65), (22, 31, 63, 100), (32, 40, 127, 130), (64, 70, 128, 200), (96, 100, 100, 260), (128, 129, 255, 257), (130, 200, 200, 256)]],
       [N, [(0, 1)]], [333, 260],
       why="four live rectangles with all-zero entries between them, eight in the other sample; edges one short of, at and one past 32 / 64 / "
           "128; a one-row rectangle on a block edge; seq_len 260 inside a tile of the last block; left padding of one"),
    _m("L655-b1-h2-one-rect-hole", 1, 2, 655, [[(6, 150, 150, 600)]], [[(100, 170)]], why="the headline length, the reference's single rectangle, a hole across words"),
) + tuple(_p(Dh, B, H, Lq, Lk, why) for Dh in (64, 96) for B, H, Lq, Lk, why in (
    (2, 1, 1, 1, "one row, one key"),
    (1, 3, 33, 31, "tails on both sides, Lq > Lk"),
    (3, 2, 128, 128, "exactly one workgroup each way"),
    (2, 3, 129, 257, "one row / one key past a workgroup: clamped loads on both sides"),
    (1, 2, 144, 873, "the Perceiver shape"),
))
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# what the GPU test sends through the product library without the lab switch: the rule's own boundary, one head pair
PRODUCT_CASE = _m("L1792-b1-h1-product-rule-boundary", 1, 1, 1792, [[(6, 150, 150, 1700)]], [N], why="AKI_ATTN64_MIN_L: the 64-row core by the product rule")


def properties(case: Case) -> set:
    """The corners of the issue's case list that this case reaches, from the table and the tile sizes TQ / BLK."""
    P = {f"L={case.Lq}" if case.masked else f"plain-d{case.Dh}:{case.Lq}x{case.Lk}"}
    if not case.masked:
        return P
    L = case.Lq
    if case.rects is None:
        P.add("no-table")
    if case.holes is None:
        P.add("no-bits")
    if case.B != case.H:
        P.add("B!=H")
    for b in range(case.B):
        live, Ls, valid = case.live_rects(b), case.seq_len(b), case.valid(b)
        vis = case.visible(b)
        P.add(f"rects={len(live)}")
        if case.rects is not None:
            idx = [i for i, r in enumerate(case.rects[b]) if r[1] > r[0]]
            if idx and any(i not in idx for i in range(idx[0], idx[-1])):
                P.add("zero-entry-between-live")
        for rlo, rhi, clo, chi in live:
            for name, e in (("row_hi", rhi), ("col_hi", chi)):
                for base in (TQ, BLK):
                    P.update(f"{name}%{base}={d:+d}" for d in (-1, 0, 1) if (e - d) % base == 0)
            if clo > rhi - 1:                                                   # wholly above the diagonal
                for kb in range(clo // BLK, (chi - 1) // BLK + 1):             # a key block that needs a Q tile only through it
                    if any(t * TQ + TQ - 1 < kb * BLK for t in range(rlo // TQ, (rhi - 1) // TQ + 1)):
                        P.add("q-tile-needed-only-through-rect")
                for t in range(clo // TQ, (chi - 1) // TQ + 1):                 # a key tile that a query block needs only through it
                    if t * TQ > (rlo // BLK) * BLK + BLK - 1:
                        P.add("k-tile-needed-only-through-rect")
            for e, lo in ((chi, clo), (rhi, rlo)):
                if e % BLK == 1 or (e - 1) // BLK != (lo // BLK) and (e - 1) % BLK == 0:
                    P.add("rect-touches-block-by-one")
        if Ls < L:
            P.add("seq:mid-tile" if Ls % TQ else "seq:tile-edge")
            if (Ls + BLK - 1) // BLK < (L + BLK - 1) // BLK:
                P.add("seq:trailing-block-without-work")
        if not valid[0]:
            P.add("leftpad")
        for lo, hi in (case.holes[b] if case.holes else ()):
            if lo > 0 and lo // 64 != (hi - 1) // 64:
                P.add("hole-across-word")
            elif lo > 0:
                P.add("hole-in-word")
        if (~vis[:Ls].any(1)).any():
            P.add("row-sees-nothing")
    return P


REQUIRED = tuple(f"L={L}" for L in (1, 31, 32, 33, 127, 128, 129, 257, 333, 655)) + tuple(
    f"plain-d{d}:{a}x{b}" for d in (64, 96) for a, b in ((1, 1), (33, 31), (128, 128), (129, 257), (144, 873))) + (
    "no-table", "no-bits", "B!=H", "rects=0", "rects=1", "rects=2", "rects=4", "rects=8", "zero-entry-between-live",
    "row_hi%32=-1", "row_hi%32=+0", "row_hi%32=+1", "col_hi%128=-1", "col_hi%128=+0", "col_hi%128=+1", "col_hi%32=+0", "row_hi%128=+0", "row_hi%128=+1",
    "q-tile-needed-only-through-rect", "k-tile-needed-only-through-rect", "rect-touches-block-by-one",
    "seq:mid-tile", "seq:tile-edge", "seq:trailing-block-without-work", "leftpad", "hole-across-word", "hole-in-word", "row-sees-nothing")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def bf16(x) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def sentinel_pairs(case: Case, b: int):
    """(pairs, forbidden): visible (row, key) pairs at the structural edges of sample b, and invisible ones just outside them."""
    Lq, Lk, Ls = case.Lq, case.Lk, case.seq_len(b)
    vis, valid = case.visible(b), case.valid(b)
    want, forb = set(), set()
    k0 = int(np.argmax(valid)) if valid.any() else 0                           # the first valid key
    edges_q = sorted({e for base in (TQ, BLK) for e in range(base, Lq, base)})
    edges_k128 = list(range(BLK, Lk, BLK))
    last = Ls - 1
    for r in sorted({0, last, Lq - 1} | {e - 1 for e in edges_q} | set(edges_q)):
        if case.masked:
            want |= {(r, r), (r, k0)}
            forb.add((r, r + 1))
        else:
            want |= {(r, 0), (r, Lk - 1), (r, min(r, Lk - 1))}
    for e in edges_k128:                                                        # both sides of every 128-key block, seen from the last row
        want |= {(last, e - 1), (last, e)}
    want |= {(last, Lk - 1), (Lq - 1, Lk - 1)}
    if case.masked:
        for rlo, rhi, clo, chi in case.live_rects(b):
            for r in (rlo, rhi - 1):
                want |= {(r, clo), (r, chi - 1)}
                forb |= {(r, chi), (r, clo - 1)}
            want |= {(rlo + 1, clo + 1), (rhi - 2, chi - 2)}
            forb |= {(rhi, chi - 1), (rhi, clo), (rlo - 1, clo), (rlo - 1, chi - 1)}
        for lo, hi in (case.holes[b] if case.holes else ()):
            rows = [r for r in (last, min(hi, last)) if r >= 0]
            for r in rows:
                want |= {(r, lo - 1), (r, hi)}
                forb |= {(r, lo), (r, hi - 1)}
        if Ls < Lq:
            forb |= {(Ls, Ls), (Ls, k0), (Ls, max(Ls - 1, 0))}
    ok = lambda r, c: 0 <= r < Lq and 0 <= c < Lk
    pairs = sorted((r, c) for r, c in want if ok(r, c) and vis[r, c])
    forbidden = sorted((r, c) for r, c in forb if ok(r, c) and not vis[r, c])
    return pairs, forbidden


@dataclass
class Inputs:
    case: Case
    family: str
    q: torch.Tensor                # bf16 [B, H, Lq, Dh]
    k: torch.Tensor                # bf16 [B, H, Lk, Dh]
    v: torch.Tensor
    d_o: torch.Tensor              # bf16 [B, Lq, H * Dh]
    pairs: list                    # per sample: sentinel pairs (listed in both families)
    forbidden: list


def make_inputs(case: Case, family: str) -> Inputs:
    assert family in FAMILIES
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.Dh
    rng = np.random.default_rng(zlib.crc32(f"{case.id}/{family}".encode()))
    q = rng.standard_normal((B, H, Lq, D))
    k = rng.standard_normal((B, H, Lk, D))
    pairs, forbidden = zip(*(sentinel_pairs(case, b) for b in range(B)))
    if family == "diffuse":
        v = np.abs(rng.standard_normal((B, H, Lk, D))) * rng.choice([-1.0, 1.0], (B, H, 1, D))
        d_o = np.abs(rng.standard_normal((B, H, Lq, D))) * rng.choice([-1.0, 1.0], (B, H, 1, D))
    else:
        v = rng.standard_normal((B, H, Lk, D))
        d_o = rng.standard_normal((B, H, Lq, D))
        level = np.log(100.0 * Lk)
        for b in range(B):
            targets = {}
            for r, c in pairs[b]:
                targets.setdefault(r, {})[c] = level
            for r, c in forbidden[b]:
                targets.setdefault(r, {})[c] = level + LIFT
            keys = sorted({c for t in targets.values() for c in t})
            u = rng.standard_normal((H, len(keys), D))
            k[b][:, keys] = u / np.linalg.norm(u, axis=-1, keepdims=True) * np.sqrt(D)
            fk = sorted({c for _, c in forbidden[b]})
            v[b][:, fk] = FORBIDDEN_V
            kb = bf16(k[b]).astype(np.float64)
            for r, t in targets.items():
                cols = sorted(t)
                want = np.array([t[c] for c in cols]) / case.scale
                for h in range(H):                                              # minimum-norm q with the wanted scores against these keys
                    q[b, h, r] = np.linalg.lstsq(kb[h][cols], want, rcond=None)[0]
                d_o[b, :, r] *= SENT_DO
            # delta-sensitive row: where row 0 sees key 0 alone, v[0] sits just below a power of two and dO[0] is aligned with it
            vis = case.visible(b)
            if vis[0].sum() == 1 and vis[0, 0]:
                sgn = rng.choice([-1.0, 1.0], (H, D))
                v[b][:, 0] = sgn * (2.0 - 2.0 ** -7)
                d_o[b, :, 0] = sgn * SENT_DO * np.abs(d_o[b, :, 0] / SENT_DO if 0 in targets else d_o[b, :, 0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return Inputs(case, family, t(q), t(k), t(v), t(d_o.transpose(0, 2, 1, 3).reshape(B, Lq, H * D)), list(pairs), list(forbidden))


# ---- reference ------------------------------------------------------------------------------------------------------------------
def hb(x):
    """2^floor(log2 |x|): the binade floor of |x| (0 for 0)."""
    ax = np.abs(x)
    return np.where(ax > 0, 2.0 ** np.floor(np.log2(np.where(ax > 0, ax, 1.0))), 0.0)


class Sample:
    """One sample in float64: the closed-form forward and backward, the magnitudes M of every output, and what a mutation needs."""

    def __init__(self, inp: Inputs, b: int, d_o=None):
        c = self.case = inp.case
        self.b, self.scale = b, c.scale
        H, D = c.H, c.Dh
        self.q, self.k, self.v = (a[b].double().numpy() for a in (inp.q, inp.k, inp.v))
        self.d_o = inp.d_o[b].double().numpy().reshape(c.Lq, H, D).transpose(1, 0, 2) if d_o is None else d_o       # [H, Lq, D]
        self.vis = c.visible(b)
        self.s = np.einsum("hqd,hkd->hqk", self.q, self.k) * self.scale
        live = self.vis.any(1)
        m = np.where(live, np.where(self.vis, self.s, -np.inf).max(-1), 0.0)
        e = np.where(self.vis, np.exp(np.minimum(self.s - m[..., None], 0.0)), 0.0)
        l = e.sum(-1)
        with np.errstate(divide="ignore"):
            self.lse = np.where(live, m + np.log(np.where(l > 0, l, 1.0)), -np.inf)
        self.P = e / np.where(l > 0, l, 1.0)[..., None]
        self.live = live
        self.o = self.P @ self.v
        self.dP = np.einsum("hqd,hkd->hqk", self.d_o, self.v)
        self.delta = (self.d_o * self.o).sum(-1)
        self.dq, self.dk, self.dv = self.backward()
        # magnitudes
        self.M_o = self.P @ np.abs(self.v)
        self.M_dv = self.P.transpose(0, 2, 1) @ np.abs(self.d_o)
        A = np.einsum("hqd,hkd->hqk", np.abs(self.d_o), np.abs(self.v))
        self.E = (self.P * np.abs(self.dP)).sum(-1) + (np.abs(self.d_o) * hb(self.o)).sum(-1)
        W = np.abs(self.P * (self.dP - self.delta[..., None])) + self.P * (self.E[..., None] + 2.0 ** -8 * A)
        self.M_dq = self.scale * (W @ np.abs(self.k))
        self.M_dk = self.scale * (W.transpose(0, 2, 1) @ np.abs(self.q))

    def backward(self, P=None, delta=None, d_o=None, dP=None):
        P = self.P if P is None else P
        delta = self.delta if delta is None else delta
        d_o = self.d_o if d_o is None else d_o
        dP = self.dP if dP is None else dP
        with np.errstate(invalid="ignore", over="ignore"):
            dS = P * (dP - delta[..., None])
            return self.scale * (dS @ self.k), self.scale * (dS.transpose(0, 2, 1) @ self.q), P.transpose(0, 2, 1) @ d_o

    def P_of(self, vis, lse=None):
        """What a backward kernel recomputes: exp(s - lse) on the pairs it takes for visible (never renormalised)."""
        lse = self.lse if lse is None else lse
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(vis, np.exp(self.s - lse[..., None]), 0.0)

    def tol(self, name, core="32"):
        ref, M = getattr(self, name), getattr(self, "M_" + name)
        return KAPPA[core] * 2.0 ** -9 * M + 2.0 ** -8 * np.abs(ref)

    def lse_tol(self, core="32"):
        return LSE_ABS[core] + LSE_REL * np.abs(np.where(self.live, self.lse, 0.0))

    def score_terms(self):
        return float((np.einsum("hqd,hkd->hqk", np.abs(self.q), np.abs(self.k)) * self.scale)[:, self.vis].max()) if self.vis.any() else 0.0


def reference(inp: Inputs):
    return [Sample(inp, b) for b in range(inp.case.B)]


def autograd_f64(inp: Inputs, b: int):
    """The independent anchor: torch autograd in float64 over a dense masked softmax (rows that see nothing give zeros)."""
    c = inp.case
    q, k, v = (a[b].double().requires_grad_() for a in (inp.q, inp.k, inp.v))
    mask = torch.from_numpy(c.visible(b))
    s = (q @ k.transpose(-1, -2)) * c.scale
    s = s.masked_fill(~mask, float("-inf"))
    dead = ~mask.any(-1, keepdim=True)
    p = torch.where(dead, torch.zeros_like(s), torch.softmax(s.masked_fill(dead, 0.0), -1))
    o = p @ v
    o.backward(inp.d_o[b].double().reshape(c.Lq, c.H, c.Dh).permute(1, 0, 2))
    return o.detach().numpy(), q.grad.numpy(), k.grad.numpy(), v.grad.numpy()


# ---- mutations of the reference -------------------------------------------------------------------------------------------------
# name -> f(S: Sample, inp) -> [(label, outputs compared, (dq, dk, dv))].  A visibility mutation changes the pairs a backward kernel
# takes for visible while o, lse and delta stay the forward's; one that lives in a single kernel is compared on that kernel's outputs.
ALL, DKV, DQ = ("dq", "dk", "dv"), ("dk", "dv"), ("dq",)


def _with_vis(S, vis, out=ALL, label=""):
    return (label, out, S.backward(P=S.P_of(vis)))


def _rect_mut(S, which, d):
    c, res = S.case, []
    if not c.masked or c.rects is None:
        return res
    for i, r in enumerate(c.rects[S.b]):
        if r[1] > r[0] and r[3] > r[2]:
            r2 = list(r)
            r2[which] += d
            if r2[1] <= r2[0] or r2[3] <= r2[2] or r2[1] > c.Lq or r2[3] > c.Lk:
                continue
            table = [list(rs) for rs in c.rects]
            table[S.b][i] = tuple(r2)
            r_, c_ = np.arange(c.Lq)[:, None], np.arange(c.Lk)[None, :]
            vis = c_ <= r_
            for rlo, rhi, clo, chi in c.live_rects(S.b, table):
                vis = vis | ((r_ >= rlo) & (r_ < rhi) & (c_ >= clo) & (c_ < chi))
            vis = vis & c.valid(S.b)[None] & (r_ < c.seq_len(S.b))
            if (vis != S.vis).any():
                res.append(_with_vis(S, vis, label=f"rect {i} -> {tuple(r2)}"))
    return res


def m_diagonal_excluded(S, inp):
    if not S.case.masked:
        return []
    vis = S.vis & ~np.eye(S.case.Lq, S.case.Lk, dtype=bool)
    return [_with_vis(S, vis, label="c < r")]


def m_seq_last_row_skipped(S, inp):
    Ls = S.case.seq_len(S.b)
    vis = S.vis.copy()
    vis[Ls - 1] = False
    return [_with_vis(S, vis, label=f"row {Ls - 1} skipped")] if S.vis[Ls - 1].any() else []


def m_seq_row_included(S, inp):
    c, Ls = S.case, S.case.seq_len(S.b)
    if not c.masked or Ls >= c.Lq:
        return []
    vis = S.vis.copy()
    vis[Ls] = (np.arange(c.Lk) <= Ls) & c.valid(S.b)
    return [_with_vis(S, vis, label=f"row {Ls} included")]


def _holes(S):
    return list(S.case.holes[S.b]) if S.case.masked and S.case.holes else []


def m_hole_edge_visible(S, inp):
    res = []
    for lo, hi in _holes(S):
        for col in sorted({lo, hi - 1}):
            vis = S.vis.copy()
            r = np.arange(S.case.Lq)
            seen = (r >= col) & (r < S.case.seq_len(S.b))                       # at least the causal rows would see it
            vis[:, col] = seen
            res.append(_with_vis(S, vis, label=f"masked column {col} visible"))
    return res


def m_column_after_hole_hidden(S, inp):
    res = []
    for lo, hi in _holes(S):
        if hi < S.case.Lk and S.vis[:, hi].any():
            vis = S.vis.copy()
            vis[:, hi] = False
            res.append(_with_vis(S, vis, label=f"column {hi} hidden"))
    return res


def _needed_q_tiles(S, kb):
    return [t for t in range((S.case.Lq + TQ - 1) // TQ) if S.vis[t * TQ:(t + 1) * TQ, kb * BLK:(kb + 1) * BLK].any()]


def _needed_k_tiles(S, qb):
    return [t for t in range((S.case.Lk + TQ - 1) // TQ) if S.vis[qb * BLK:(qb + 1) * BLK, t * TQ:(t + 1) * TQ].any()]


def _drop(S, rows, cols, out, label):
    vis = S.vis.copy()
    vis[rows[0]:rows[1], cols[0]:cols[1]] = False
    return _with_vis(S, vis, out, label)


def m_drop_q_tile(S, inp, which):
    """One 32-row Q tile dropped for one 128-key block (attn_bwd_dkv_kernel): first needed, last needed, needed only through a rectangle."""
    res, c = [], S.case
    for kb in range((c.Lk + BLK - 1) // BLK):
        need = _needed_q_tiles(S, kb)
        if not need:
            continue
        if which == "rect":
            ts = [t for t in need if c.masked and t * TQ + TQ - 1 < kb * BLK]
        else:
            ts = [need[0] if which == "first" else need[-1]]
        res += [_drop(S, (t * TQ, t * TQ + TQ), (kb * BLK, kb * BLK + BLK), DKV, f"Q tile {t} dropped for key block {kb}") for t in ts]
    return res


def m_drop_k_tile(S, inp, which):
    """One 32-key tile dropped for one 128-query block (attn_bwd_dq_kernel): the diagonal tile, a rectangle's last tile, only-through-rectangle."""
    res, c = [], S.case
    for qb in range((c.Lq + BLK - 1) // BLK):
        need = _needed_k_tiles(S, qb)
        if not need:
            continue
        if which == "diagonal":
            ts = [t for t in need if t * TQ <= qb * BLK + BLK - 1][-1:] if c.masked else need[-1:]
        else:
            ts = [t for t in need if c.masked and t * TQ > qb * BLK + BLK - 1]
            ts = ts[-1:] if which == "rect-last" else ts[:1]
        res += [_drop(S, (qb * BLK, qb * BLK + BLK), (t * TQ, t * TQ + TQ), DQ, f"key tile {t} dropped for query block {qb}") for t in ts]
    return res


def m_drop_trailing_slice(S, inp):
    """The trailing 32-key wave slice of a partial key block, and the trailing 32 rows of a partial query block."""
    c, res = S.case, []
    if c.Lk % BLK and S.vis[:, (c.Lk - 1) // TQ * TQ:].any():
        res.append(_drop(S, (0, c.Lq), ((c.Lk - 1) // TQ * TQ, c.Lk), DKV, "last wave slice of keys dropped"))
    if c.Lq % BLK and S.vis[(c.Lq - 1) // TQ * TQ:].any():
        res.append(_drop(S, ((c.Lq - 1) // TQ * TQ, c.Lq), (0, c.Lk), DQ, "last wave slice of rows dropped"))
    return res


def m_last_key_twice(S, inp):
    """Key Lk - 1 counted twice in dq (a clamped load taken for data)."""
    c = S.case
    if not S.vis[:, c.Lk - 1].any():
        return []
    dq, dk, dv = S.dq.copy(), S.dk, S.dv
    dS = S.P[:, :, -1] * (S.dP[:, :, -1] - S.delta)
    dq += S.scale * dS[..., None] * S.k[:, None, -1]
    return [("key Lk-1 twice", DQ, (dq, dk, dv))]


def m_last_row_twice(S, inp):
    """Row Lq - 1 counted twice in dk / dv."""
    c = S.case
    r = c.Lq - 1
    if not S.vis[r].any():
        return []
    dS = S.P[:, r] * (S.dP[:, r] - S.delta[:, r, None])
    return [("row Lq-1 twice", DKV, (S.dq, S.dk + S.scale * dS[..., None] * S.q[:, r][:, None], S.dv + S.P[:, r][..., None] * S.d_o[:, r][:, None]))]


def m_delta_omitted(S, inp):
    return [("delta = 0", ALL, S.backward(delta=0 * S.delta))]


def m_delta_scaled(S, inp):
    return [("delta (1 - 2^-4)", ALL, S.backward(delta=S.delta * (1 - 2.0 ** -4)))]


def m_scale_dropped_dq(S, inp):
    return [("dq without scale", DQ, (S.dq / S.scale, S.dk, S.dv))]


def m_scale_dropped_dk(S, inp):
    return [("dk without scale", DKV, (S.dq, S.dk / S.scale, S.dv))]


def m_do_next_head(S, inp):
    if S.case.H < 2:
        return []
    d_o = np.roll(S.d_o, -1, axis=0)
    dP = np.einsum("hqd,hkd->hqk", d_o, S.v)
    return [("dO of head h+1", ALL, S.backward(d_o=d_o, dP=dP))]


def _other_sample(S, part):
    c = S.case
    if not c.masked or c.B < 2:
        return []
    o = (S.b + 1) % c.B
    vis = c.visible(S.b, **{part: o})
    return [_with_vis(S, vis, label=f"{part[:-3]} of sample {o}")] if (vis != S.vis).any() else []


def m_lse_off(S, inp):
    return [("lse + 2^-6", ALL, S.backward(P=S.P_of(S.vis, S.lse + 2.0 ** -6)))]


MUTATIONS = {
    "diagonal-excluded": m_diagonal_excluded,
    "row_lo+1": lambda S, i: _rect_mut(S, 0, +1), "row_hi-1": lambda S, i: _rect_mut(S, 1, -1),
    "col_lo+1": lambda S, i: _rect_mut(S, 2, +1), "col_hi-1": lambda S, i: _rect_mut(S, 3, -1),
    "col_hi+1": lambda S, i: _rect_mut(S, 3, +1), "row_hi+1": lambda S, i: _rect_mut(S, 1, +1),
    "row-seq_len-1-skipped": m_seq_last_row_skipped, "row-seq_len-included": m_seq_row_included,
    "hole-edge-visible": m_hole_edge_visible, "column-after-hole-hidden": m_column_after_hole_hidden,
    "q-tile-dropped-first-needed": lambda S, i: m_drop_q_tile(S, i, "first"),
    "q-tile-dropped-last-needed": lambda S, i: m_drop_q_tile(S, i, "last"),
    "q-tile-dropped-only-through-rect": lambda S, i: m_drop_q_tile(S, i, "rect"),
    "k-tile-dropped-diagonal": lambda S, i: m_drop_k_tile(S, i, "diagonal"),
    "k-tile-dropped-rect-last": lambda S, i: m_drop_k_tile(S, i, "rect-last"),
    "k-tile-dropped-only-through-rect": lambda S, i: m_drop_k_tile(S, i, "rect-first"),
    "trailing-wave-slice-dropped": m_drop_trailing_slice,
    "key-Lk-1-twice": m_last_key_twice, "row-Lq-1-twice": m_last_row_twice,
    "delta-omitted": m_delta_omitted, "delta(1-2^-4)": m_delta_scaled,
    "scale-dropped-dq": m_scale_dropped_dq, "scale-dropped-dk": m_scale_dropped_dk,
    "dO-of-head-h+1": m_do_next_head,
    "rects-of-sample-b+1": lambda S, i: _other_sample(S, "rects_of"),
    "bits-of-sample-b+1": lambda S, i: _other_sample(S, "valid_of"),
    "seq_len-of-sample-b+1": lambda S, i: _other_sample(S, "seq_of"),
    "lse+2^-6": m_lse_off,
}


def ratio(S: Sample, out, got) -> float:
    """Worst |mutated - reference| / tolerance over the compared outputs (inf where the mutant is not finite: exp(s - lse) of a dead row)."""
    worst = 0.0
    for name, g in zip(ALL, got):
        if name in out:
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.abs(g - getattr(S, name))
                if not np.isfinite(d).all():
                    return float("inf")
                tol = S.tol(name)
                r = np.where(d > 0, d / np.where(tol > 0, tol, 1e-300), 0.0)
            worst = max(worst, float(r.max()))
    return worst


def mutation_ratios(S: Sample, inp: Inputs, names=None) -> dict:
    """{mutation: {label: ratio}} of one sample."""
    return {n: {label: ratio(S, out, got) for label, out, got in f(S, inp)} for n, f in MUTATIONS.items() if names is None or n in names}

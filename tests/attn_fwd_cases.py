"""Case table, inputs, float64 reference, componentwise tolerance and reference mutations of the attention FORWARD at the lengths the
64-row core exists for (aki_amd/csrc/mma_attn64_bf16.hip, routed to at L >= AKI_ATTN64_MIN_L; mma_attn_bf16.hip below it), of its dead
rows under both conventions, and of the vision attention (attn_nc_bf16.hip, ops.attention) at every head_dim it exports - 72 (SigLIP), 64
(the Perceiver), 96 and 32 - in the memory layouts the product hands it ("layouts of the plain route" at the end of this file).

numpy and CPU torch only.  tests/test_attn_fwd_cases_cpu.py checks the table itself and tests/test_attn_fwd_gpu.py runs it on the device.
Case, visible(), bf16, hb, sentinel_pairs, FORBIDDEN_V, LIFT and MIN_RATIO are those of attn_bwd_cases.py; the reference is not: Sample
there holds dense [H, L, L] arrays many times over.  Here a sample is walked in blocks of ROWS_PER_BLOCK rows (a few arrays of
[H, 256, L] float64: ~40 MB each at L = 5000, H = 2), forward only, and cached per (case, family) so that every route shares it.

Why a bar of its own.  With N(0, 1) inputs a row that sees n keys has |o| ~ (e / n)^1/2; the suite's bf16 bar has an absolute term of
4e-3, so at n = 4096 a dropped 64-key tile (13 / n) and a dropped or leaked key (1 / n) pass.  Here every element o = sum_k P_k v_k is held to

    tol(o)   = (KAPPA + ACC n 2^-15) 2^-9 M_o + 2^-8 |o| + S_o,         M_o = sum_k P_k |v_k|   (float64 reference)
    tol(lse) = LSE_ABS + 2^-20 |lse| + n 2^-24 + S_lse

Derivation, term by term (unit 2^-9; u = 2^-8 = 2 units is the unit roundoff of bf16).
  KAPPA   attn_bwd_cases.py derives it: one cast of p per term (u M_o = 2 units) and e_P = 0.5 units for the error of a recomputed p (f32
          dot product of 96 exact bf16 products while sum_d |q_d k_d| scale <= MAX_SCORE_TERMS = 64, exp2 / log of the hardware): 2.5 for
          the 32-row core and ops.attention (attn_nc_bf16 at every head_dim: it adds the unrounded f32 p into l_part on the VALU, casts
          p to bf16 once as the PV operand and divides by the unrounded sum - head_dim changes KS, DT and the LDS pitches, not this).  The 64-row core sums the bf16-ROUNDED p on the matrix pipe and divides by that sum: 2 more
          units, 4.5 - in its shipped build (blind softmax), in its every-tile-exact build and through the product rule alike.  Against
          the reference maximum of a rank's first tile p = exp2(s c - m_ref) may be as large as 2^64: bf16 has f32's exponent, the cast
          stays a RELATIVE error u, and the bound does not move.
  ACC n   f32 accumulation.  attn_bwd_cases.py folds n 2^-24 M into e_P's half unit for n <= 1792 (0.06 units).  Here n reaches 5000 and
          the term is carried: the numerator sum_k p_k v_k and the denominator sum_k p_k are both n-term f32 sums (on the matrix pipe or
          the VALU), each off by at most n 2^-24 of its sum of magnitudes, so ACC = 2 and the term is 2 n 2^-24 M_o = 2 n 2^-15 units (0.31
          units at n = 5000).  n is the number of keys the row SEES (a hidden key adds an exact zero); for a dead row under the uniform
          convention n = L.  The log of the denominator moves by n 2^-24.
  2^-8|o| the cast of the output (half an ulp <= 2^-9 |o|) and the division by l, with room.
  S_o     rising family only.  The score error 96 * 2^-24 * sum_d |q_d k_d| * scale =: e_k of a key (the f32 dot product; it also covers the
          one rounding of the fma s c - m, 2^-24 |s c|) is a relative error of p_k.  With scores lifted by 50 nats it passes the 64 that
          e_P's half unit assumes, so it is computed from the inputs: d o = sum_k P_k e_k v_k - o sum_k P_k e_k, bounded by
          S_o = sum_k P_k e_k |v_k| + |o| sum_k P_k e_k, and S_lse = sum_k P_k e_k.  For every other family the CPU test asserts
          sum_d |q_d k_d| scale <= 64 on all visible pairs, and S = 0.
  lse     as in attn_bwd_cases.py: 2^-16 + 2^-20 |lse| for f32 arithmetic on m + log2 l (the relative part also covers |m| > 64 of the
          rising family: m carries 2^-24 |m|), 2^-8 more for the 64-row core's sum of rounded p.
  dead    rows >= seq_len, and rows inside seq_len that see no valid column.  AKI_DEAD_ROWS_UNIFORM: o = mean of v over ALL L columns
          (the reference's finfo.min mask: a uniform softmax), the same bar with P = 1 / L and n = L; AKI_DEAD_ROWS_ZERO: exact zeros.
          lse of a dead row is not specified by include/aki_mi355x.h beyond "[B,H,L] f32"; the 32-row kernel writes -inf wherever its row
          sum is zero (rows inside seq_len that see nothing, and rows >= seq_len under the zero convention) and a finite number for the
          rows it runs as a uniform softmax (rows >= seq_len under the uniform convention).  lse_pattern() is that pattern; no value is asserted.
These are worst-case first-order bounds: a kernel should sit several times below 1, and a case above it is a finding.

Input families, everything rounded to bf16 first.
  diffuse   q, k ~ N(0, 1); v = |N(0, 1)| with one random sign per (head, feature) column: M_o ~ |o|, and a missing tile is 64 / n of the
            element - 1.2 x the bar at n = 4096, so tiles are caught through the sentinel rows, the other sample's table through this one.
  sentinel  visible pairs at the structural edges share a common score ln(100 Lk) and so most of their row's mass about equally (at
            most MAX_TARGETS = 6 per row: a minimum-norm q against more keys is so long that ordinary keys outweigh them at L = 5000);
            forbidden pairs just outside each edge get that score + LIFT and v = FORBIDDEN_V, and so does every invalid column, which
            only a dead row's uniform mean may touch.  The pairs are those of attn_bwd_cases.sentinel_pairs (thinned to the cap) plus,
            seen from the last live row and from one row inside each rectangle: both sides of the 64-key tile edges 64 | 128 (a rank's
            first / second tile), of the tile edge below each rectangle's col_hi, of key 4096 (tile 63 | 64: the seam of the 64-row core's
            64-tile mask windows), the last key Lk - 1; and rows r and r + 32 (a wave's two blocks) on one key.
  rising    (64-row core) diffuse, plus a feature that lifts the score of every key >= RISE_KEY by 2^40 (the rank stays blind: row sums
            <= 2^60 against the first tile's maximum) or 2^72 (row sums >= 2^68: the verification fails and the rank is walked again through
            the exact path).  Three keys of the first tile carry v = +-2^x, x chosen so that they hold about half of M_o on the lifted
            rows: the CPU test asserts a median share in [0.3, 0.7] and a 5th percentile >= 0.1 - the first tile's loss is 8 bars or more.

A persistent workgroup that snakes over several ranks of its pair is the subject of tests/attn_walk_cases.py (the same bar, heads that
share data so that B * H of a few hundred stays affordable in float64), not of this table: a rank of the 64-row core is 256 rows
(attn_core64_bf16_launch: nqt = ceil(L / 256), splits = min(ceil(CUs / (B H)), nqt)), so a workgroup walks a second rank only where
ceil(CUs / (B H)) < ceil(L / 256), and the 32-row core (ranks of 128 rows, splits >= L / 256) needs B * H >= 35 at L = 2048.
ranks_per_workgroup() states the rule; the CPU test asserts that no case of THIS table passes 1.
"""
import os
import re
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import attn_bwd_cases as A
from attn_bwd_cases import Case, bf16, hb, sentinel_pairs, FORBIDDEN_V, LIFT, MIN_RATIO, Z, N   # noqa: F401 (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA = {"32": 2.5, "64": 4.5}                # "64": shipped, every-tile-exact and product-rule launches of the 64-row core
ACC = 2.0
LSE_ABS, LSE_REL = A.LSE_ABS, A.LSE_REL
MAX_SCORE_TERMS = A.MAX_SCORE_TERMS
MAX_TARGETS = 6
ROWS_PER_BLOCK = 256
TILE = 64
SEAM = 4096                                    # key 4096 = tile 64: the first tile of the 64-row core's second mask window
RISE_KEY, RISE_Q = 1024, 16.0
RISE_SENT = (3, 33, 60)
CAPPED = {}                                    # no mutation is capped by this bar


def kernel_constants() -> dict:
    """AKI_ATTN64_MIN_L, kSchedMax and the 64-row core's ranked-block limit as the library is compiled: a retune re-aims properties()."""
    src32 = open(os.path.join(ROOT, "aki_amd", "csrc", "mma_attn_bf16.hip")).read()
    src64 = open(os.path.join(ROOT, "aki_amd", "csrc", "mma_attn64_bf16.hip")).read()
    m1 = re.search(r"^#define\s+AKI_ATTN64_MIN_L\s+(\d+)", src32, re.M)
    m2 = re.search(r"constexpr int kSchedMax = (\d+);", src32)
    m3 = re.search(r"const bool sched = nblk <= (\d+);", src64)
    m4 = re.search(r"!\(lA < 0x1p(\d+)f\)", src64)
    assert m1 and m2 and m3 and m4, "attention-core constants not found in the sources"
    assert "t != 63 &&" in src64 and "(j & 63) != 0" in src64 and "(j & 63) == 0" in src64, "the 64-tile mask window of the 64-row core moved"
    return dict(MIN_L=int(m1.group(1)), SCHED32=int(m2.group(1)), SCHED64=int(m3.group(1)), SUM_LOG2=int(m4.group(1)))


KC = kernel_constants()
CUS = 256                                      # compute units of an MI355X: what ranks_per_workgroup() assumes


def ranks_per_workgroup(B: int, H: int, L: int, core: str, cus: int = CUS) -> int:
    """The most ranks one persistent workgroup walks (the host side of both cores: nqt ranks per pair over `splits` workgroups)."""
    nbh = B * H
    if core == "64":
        nqt = (L + 255) // 256
        splits = max(1, min((cus + nbh - 1) // nbh, nqt))
    else:
        nqt = (L + 127) // 128
        splits = max(1, min(max((2 * cus + nbh - 1) // nbh, L // 256), nqt))
    return (nqt + splits - 1) // splits


# ---- cases ----------------------------------------------------------------------------------------------------------------------
_m, _p = A._m, A._p


def _boundary(L):
    return _m(f"L{L}-b2-h1-product-rule-ragged", 2, 1, L, [[(6, 150, 150, L - 64)], [(6, 150, 150, L - 400)]], [N, [(L - 321, L)]], [L, L - 321],
              why="AKI_ATTN64_MIN_L - 1 / + 0 / + 1 through the product rule: a ragged two-sample batch, one rectangle each")


PLAIN_DH = (72, 32, 64, 96)                    # every head_dim attn_nc_bf16 exports: SigLIP 72, the Perceiver 64
_S32 = 32 * KC["SCHED32"]                      # the lengths aimed at a constant of the kernels move with it
CASES = (
    _boundary(KC["MIN_L"] - 1), _boundary(KC["MIN_L"]), _boundary(KC["MIN_L"] + 1),
    _m(f"L{_S32}-b1-h2-sched32-ranked", 1, 2, _S32, [[(6, 150, 150, _S32 - 48)]], [N], why="32-row core: kSchedMax blocks, ranked by extent"),
    _m(f"L{_S32 + 1}-b1-h2-sched32-position", 1, 2, _S32 + 1, [[(6, 150, 150, _S32 - 48)]], [N], why="32-row core: kSchedMax + 1 blocks, position order; a last block of one row"),
    _m("L4096-b1-h2-four-rects-col_hi-around-tile-edge", 1, 2, 4096,
       [[(6, 150, 150, 4031), (900, 1044, 1044, 4032), (1800, 1944, 1944, 4033), (2700, 2844, 2844, 4096)]], [N],
       why="128 ranked blocks (the limit); four image rectangles, col_hi one short of, on and one past a tile edge and at L; rectangle rows walk ~60 fast tiles"),
    _m("L4097-b1-h2-position-order-tile64-one-key", 1, 2, 4097, [[(6, 150, 150, 4097), (3000, 3144, 3144, 4096)]], [N],
       why="129 blocks: position order; tile 64 holds the single key 4096; a rectangle to L and one to the seam"),
    _m("L4160-b1-h1-rect-across-seam-col_hi-in-tile-64", 1, 1, 4160, [[(6, 150, 150, 4096), (1000, 1144, 1144, 4150)]], [N],
       why="a rectangle whose columns cross key 4096 with col_hi inside tile 64; another ends exactly at 4096"),
    _m("L4161-b1-h1-rect-across-seam-col_hi-in-tile-65", 1, 1, 4161, [[(6, 150, 150, 4096), (1000, 1144, 1144, 4161)]], [N],
       why="the same with col_hi in tile 65 (= L: a tile of one key)"),
    _m("L5000-b1-h2-two-windows-hole-at-seam", 1, 2, 5000, [[(6, 150, 150, 4900), (4200, 4344, 4344, 4990)]], [[(4090, 4100)]],
       why="two mask windows: early image rows whose rectangle reaches past 4096, a rectangle wholly in the second window, a hole across the 64-bit word at the seam"),
    _m("L2300-b2-h2-ragged-mid-tile-and-tile-edge", 2, 2, 2300, [[(6, 150, 150, 2100)], [(6, 150, 150, 1900)]], [[(2117, 2300)], N], [2117, 1984],
       why="seq_len mid-tile (2117) and on a tile edge (1984); run under both dead-row conventions"),
    _m("L1856-b2-h1-leftpad-137-and-195-hole-later", 2, 1, 1856, [[(150, 294, 294, 1800)], [(200, 344, 344, 1700)]], [[(0, 137), (900, 920)], [(0, 195)]],
       why="left padding of more than 64 (137) and of 64 k + 3 (195) keys: rows that see nothing through the first tile(s); a hole later on"),
    _m("L2304-b1-h2-rising-blind", 1, 2, 2304, [[(6, 150, 150, 2200)]], [N], why="later tiles beat the first tile's maximum by 2^40: inside the 2^64 bound, the rank stays blind"),
    _m("L2304-b1-h2-rising-redo", 1, 2, 2304, [[(6, 150, 150, 2200)]], [N], why="later tiles beat it by 2^72: the row sums pass 2^64 and the rank is walked again"),
) + tuple(_p(Dh, B, H, Lq, Lk, why) for Dh in PLAIN_DH for B, H, Lq, Lk, why in (
    (2, 1, 1, 1, "one row, one key"),
    (1, 3, 33, 31, "tails on both sides, Lq > Lk"),
    (2, 3, 129, 257, "one row / one key past a workgroup"),
    (1, 2, 576, 576, "SigLIP's token count"),
    (1, 2, 144, 873, "the Perceiver shape"),
    (1, 2, 729, 729, "SigLIP at 384 px: 5 workgroups + 89 rows, 11 tiles + 25 keys"),
    (1, 2, 144, 720, "the Perceiver at 336 px: 11 tiles + 16 keys"),
))
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
RISING = {"L2304-b1-h2-rising-blind": 40.0, "L2304-b1-h2-rising-redo": 72.0}       # lift of the late keys, log2 units
# aki_dead_rows values a case runs under (default: uniform); the boundary case below MIN_L also takes the 32-row route
DEAD_ROWS = {"L2300-b2-h2-ragged-mid-tile-and-tile-edge": (1, 0), CASES[0].id: (1, 0)}
# The sentinel keys are random directions.  With the plain seed the six keys of row 143, head 0 of this case lie so close to a common
# subspace that the minimum-norm q is long and ordinary keys take 86 % of the row (share 0.137 against the 0.2 the CPU test asks for):
# another draw, not another condition.  No other (case, family) is salted, so no other input moves.
SEED_SALT = {("plain-d64-b1-h2-144x873", "sentinel"): "/draw-1"}
KV_CACHE_CASE = "L4097-b1-h2-position-order-tile64-one-key"                         # two heads; the last tile holds one key


def families(case: Case) -> tuple:
    return ("rising",) if case.id in RISING else ("diffuse", "sentinel")


def dead_conventions(case: Case) -> tuple:
    return DEAD_ROWS.get(case.id, (1,))


def routes(case: Case) -> tuple:
    """Which launches the GPU test sends a case through: '32' / '64' / '164' = lab variants 1 / 9 / 164, 'product' = no lab switch."""
    if not case.masked:
        return ("plain",)
    kc, L = kernel_constants(), case.Lq
    r = []
    if L <= 2100 and case.id not in RISING:
        r.append("32")
    r.append("64")
    if L > SEAM or case.id in RISING:
        r.append("164")
    if L >= kc["MIN_L"] - 1:
        r.append("product")
    return tuple(r)


def product_core(case: Case) -> str:
    return "64" if case.Lq >= kernel_constants()["MIN_L"] else "32"


def properties(case: Case) -> set:
    """The corners of the case list that this case reaches, from the case and the kernels' own constants."""
    if not case.masked:
        return {f"plain-d{case.Dh}:{case.Lq}x{case.Lk}"}
    kc, L = kernel_constants(), case.Lq
    P = {f"L={L}"}
    for d in (-1, 0, 1):
        if L == kc["MIN_L"] + d:
            P.add(f"min_l{d:+d}")
    nblk, ntile = (L + 31) // 32, (L + 63) // 64
    if "32" in routes(case):
        P.update({"sched32:ranked-at-limit"} if nblk == kc["SCHED32"] else {"sched32:position-order-first"} if nblk == kc["SCHED32"] + 1 else ())
    P.update({"sched64:ranked-at-limit"} if nblk == kc["SCHED64"] else {"sched64:position-order-first"} if nblk == kc["SCHED64"] + 1 else ())
    if ntile > 64:
        P.add("two-mask-windows")
        if L - 64 * 64 == 1:
            P.add("tile-64-holds-one-key")
    if case.B != case.H:
        P.add("B!=H")
    if case.id in RISING:
        P.add("rising:blind" if RISING[case.id] + 20 < kc["SUM_LOG2"] else "rising:redo" if RISING[case.id] > kc["SUM_LOG2"] + 4 else "rising:?")
    for dr in dead_conventions(case):
        if any(case.seq_len(b) < L or not case.visible(b)[:case.seq_len(b)].any(1).all() for b in range(case.B)):
            P.add("dead-rows:uniform" if dr else "dead-rows:zero")
    for b in range(case.B):
        live, Ls, valid = case.live_rects(b), case.seq_len(b), case.valid(b)
        P.add(f"rects={len(live)}")
        for rlo, rhi, clo, chi in live:
            P.update(f"col_hi%64={d:+d}" for d in (-1, 0, 1) if (chi - d) % 64 == 0)
            if clo < SEAM < chi:
                P.add(f"rect-across-seam:col_hi-in-tile-{(chi - 1) // 64}")
                if rhi <= SEAM // 2:
                    P.add("early-rows-reach-past-seam")
            if chi == SEAM:
                P.add("rect-ends-at-seam")
            if clo >= SEAM:
                P.add("rect-in-second-window")
            if chi // 64 - (rhi + 63) // 64 >= 60:
                P.add("rect-rows-walk-60-fast-tiles")
        if Ls < L:
            P.add("seq:mid-tile" if Ls % 64 else "seq:tile-edge")
        k0 = int(np.argmax(valid))
        if k0 > 64:
            P.add("leftpad>64")
        if k0 > 64 and k0 % 64 == 3:
            P.add("leftpad=64k+3")
        if k0 >= 64 and L >= kc["MIN_L"]:
            P.add("rows-see-nothing-through-first-tile")
        for lo, hi in (case.holes[b] if case.holes else ()):
            if lo > k0 and hi < L:
                P.add("hole-across-word-at-seam" if lo < SEAM < hi and lo // 64 != (hi - 1) // 64 else "hole-later")
    return P


REQUIRED = tuple(f"L={L}" for L in (KC["MIN_L"] - 1, KC["MIN_L"], KC["MIN_L"] + 1, _S32, _S32 + 1, 4096, 4097, 4160, 4161, 5000, 2300, 1856, 2304)) + tuple(
    f"plain-d{d}:{a}x{b}" for d in PLAIN_DH for a, b in ((1, 1), (33, 31), (129, 257), (576, 576), (144, 873), (729, 729), (144, 720))) + (
    "min_l-1", "min_l+0", "min_l+1", "sched32:ranked-at-limit", "sched32:position-order-first", "sched64:ranked-at-limit",
    "sched64:position-order-first", "two-mask-windows", "tile-64-holds-one-key", "B!=H", "rects=1", "rects=2", "rects=4",
    "col_hi%64=-1", "col_hi%64=+0", "col_hi%64=+1", "rect-across-seam:col_hi-in-tile-64", "rect-across-seam:col_hi-in-tile-65",
    "rect-ends-at-seam", "rect-in-second-window", "early-rows-reach-past-seam", "rect-rows-walk-60-fast-tiles", "hole-across-word-at-seam",
    "seq:mid-tile", "seq:tile-edge", "dead-rows:uniform", "dead-rows:zero", "leftpad>64", "leftpad=64k+3",
    "rows-see-nothing-through-first-tile", "hole-later", "rising:blind", "rising:redo")


_VIS = {}


def vis_of(case: Case, b: int) -> np.ndarray:
    """case.visible(b), made once and shared: read-only."""
    key = (case.id, b)
    if key not in _VIS:
        if len(_VIS) > 8:
            _VIS.clear()
        v = case.visible(b)
        v.setflags(write=False)
        _VIS[key] = v
    return _VIS[key]


def max_targets(case: Case) -> int:
    """Sentinel keys per row: a minimum-norm q against more keys is so long that ordinary keys outweigh them (one key at head_dim 32)."""
    return MAX_TARGETS if case.Dh >= 64 else 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def fwd_pairs(case: Case, b: int):
    """(pairs, forbidden) of sample b: attn_bwd_cases.sentinel_pairs plus the long-context edges (module docstring), at most
    MAX_TARGETS per row - forbidden pairs first, then the edges added here, then the rest by column distance from the row's ends."""
    Lq, Lk, Ls = case.Lq, case.Lk, case.seq_len(b)
    vis, valid = vis_of(case, b), case.valid(b)
    base_pairs, base_forb = sentinel_pairs(case, b)
    want = {}
    for r, c in base_forb:
        want.setdefault(r, {})[c] = 0
    extra = {}

    def place(viewer, cols, step, stop):
        for c in cols:
            if not 0 <= c < Lk:
                continue
            r = viewer
            while r != stop and 0 <= r < Lq:
                if vis[r, c] and len(extra.get(r, ())) < min(3, max_targets(case)) and c not in want.get(r, {}):
                    extra.setdefault(r, []).append(c)
                    break
                r += step
    last = Ls - 1
    live = vis.any(1)
    while last > 0 and not live[last]:
        last -= 1
    edge_cols = [Lk - 1, SEAM - 1, SEAM, 63, 64, 127, 128]                    # (only the last row sees the last key: first)
    place(last, edge_cols, -1, max(last - 12, -1))
    if case.masked:
        for rlo, rhi, clo, chi in case.live_rects(b):
            te = (chi - 1) // 64 * 64
            place(rlo + 2, [c for c in edge_cols if c >= clo] + [te - 1, te], +1, rhi - 1)
        r0 = (Ls // 128) * 64 + 5                                                # rows r and r + 32 of a wave's two blocks on one key
        for r in (r0, r0 + 32):
            if r < Ls and vis[r, r0 - 3]:
                extra.setdefault(r, []).append(r0 - 3)
                extra[r].append(r)
    for r, cols in extra.items():
        for c in cols:
            if vis[r, c]:
                want.setdefault(r, {}).setdefault(c, 1)
    for r, c in base_pairs:
        want.setdefault(r, {}).setdefault(c, 2)
    pairs, forbidden = [], []
    for r, t in want.items():
        order = sorted(t, key=lambda c: (t[c], min(c, Lk - 1 - c)))[:max_targets(case)]
        for c in order:
            (forbidden if t[c] == 0 else pairs).append((r, c))
    ok = lambda r, c: 0 <= r < Lq and 0 <= c < Lk
    return sorted(p for p in pairs if ok(*p) and vis[p]), sorted(p for p in forbidden if ok(*p) and not vis[p])


@dataclass
class Inputs:
    case: Case
    family: str
    q: torch.Tensor                # bf16 [B, H, Lq, Dh]
    k: torch.Tensor                # bf16 [B, H, Lk, Dh]
    v: torch.Tensor
    pairs: list                    # per sample (empty lists in the rising family)
    forbidden: list


def make_inputs(case: Case, family: str) -> Inputs:
    assert family in families(case)
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.Dh
    rng = np.random.default_rng(zlib.crc32(f"fwd/{case.id}/{family}{SEED_SALT.get((case.id, family), '')}".encode()))
    q = rng.standard_normal((B, H, Lq, D))
    k = rng.standard_normal((B, H, Lk, D))
    pairs, forbidden = [[] for _ in range(B)], [[] for _ in range(B)]
    if family in ("diffuse", "rising"):
        v = np.abs(rng.standard_normal((B, H, Lk, D))) * rng.choice([-1.0, 1.0], (B, H, 1, D))
    if family == "rising":
        lift = RISING[case.id] * np.log(2.0)
        q[..., D - 1] = RISE_Q
        k[..., :RISE_KEY, D - 1] = 0.0
        k[..., RISE_KEY:, D - 1] = float(bf16(np.array([lift / (RISE_Q * case.scale)]))[0])
        # the first tile's sentinels: v = +-2^x with x such that they hold about half of M_o on the lifted rows (probe: 64 rows, float64)
        qb, kb = bf16(q).astype(np.float64), bf16(k).astype(np.float64)
        rows = np.arange(RISE_KEY + 64, Lq, max(1, (Lq - RISE_KEY - 64) // 64))[:64]
        share = []
        for b in range(B):
            vis = vis_of(case, b)[rows]
            s = np.einsum("hqd,hkd->hqk", qb[b][:, rows], kb[b]) * case.scale
            s = np.where(vis, s, -np.inf)
            P = np.exp(s - s.max(-1, keepdims=True))
            P /= P.sum(-1, keepdims=True)
            share.append(P[..., list(RISE_SENT)].sum(-1))
        x = np.round(np.log2(np.sqrt(2 / np.pi) / np.median(np.concatenate(share))))
        v[:, :, list(RISE_SENT)] = 2.0 ** x * np.sign(v[:, :, list(RISE_SENT)])
    if family == "sentinel":
        v = rng.standard_normal((B, H, Lk, D))
        level = np.log(100.0 * Lk)
        for b in range(B):
            pairs[b], forbidden[b] = fwd_pairs(case, b)
            targets = {}
            for r, c in pairs[b]:
                targets.setdefault(r, {})[c] = level
            for r, c in forbidden[b]:
                targets.setdefault(r, {})[c] = level + LIFT
            keys = sorted({c for t in targets.values() for c in t})
            u = rng.standard_normal((H, len(keys), D))
            k[b][:, keys] = u / np.linalg.norm(u, axis=-1, keepdims=True) * np.sqrt(D)
            v[b][:, sorted({c for _, c in forbidden[b]})] = FORBIDDEN_V
            v[b][:, ~case.valid(b)] = FORBIDDEN_V
            kb = bf16(k[b]).astype(np.float64)
            for r, t in targets.items():
                cols = sorted(t)
                want = np.array([t[c] for c in cols]) / case.scale
                for h in range(H):                                              # minimum-norm q with the wanted scores against these keys
                    q[b, h, r] = np.linalg.lstsq(kb[h][cols], want, rcond=None)[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    return Inputs(case, family, t(q), t(k), t(v), pairs, forbidden)


# ---- reference ------------------------------------------------------------------------------------------------------------------
@dataclass
class Rows:
    """Float64 forward of some rows of one sample (all [H, rows, ...]); a row that sees nothing has o = M = 0, lse = -inf, n = 0."""
    rows: np.ndarray
    o: np.ndarray
    lse: np.ndarray
    M: np.ndarray
    n: np.ndarray                  # [rows] keys seen
    S_o: np.ndarray                # the score-error terms of the derivation (used by the rising family)
    S_lse: np.ndarray
    m0: np.ndarray                 # maximum over the visible keys of the first 64-key tile (-inf: none)
    terms: float                   # max sum_d |q_d k_d| scale over the visible pairs


def forward_rows(inp, b: int, rows=None, vis=None) -> Rows:
    """Rows `rows` (default: all) of sample b under visibility `vis` ([rows, Lk] bool; default: the case's own), walked in blocks."""
    c = inp.case
    rows = np.arange(c.Lq) if rows is None else np.asarray(rows, dtype=np.int64)
    vis = vis_of(c, b)[rows] if vis is None else vis
    q, k, v = (a[b].double() for a in (inp.q, inp.k, inp.v))
    aq, ak, av = q.abs(), k.abs(), v.abs()
    H, D, nr = c.H, c.Dh, len(rows)
    out = Rows(rows, np.zeros((H, nr, D)), np.zeros((H, nr)), np.zeros((H, nr, D)), vis.sum(1), np.zeros((H, nr, D)), np.zeros((H, nr)), np.zeros((H, nr)), 0.0)
    unit = 96.0 * 2.0 ** -24 * c.scale
    for i in range(0, nr, ROWS_PER_BLOCK):
        sl = slice(i, i + ROWS_PER_BLOCK)
        r = torch.from_numpy(rows[sl])
        m = torch.from_numpy(np.ascontiguousarray(vis[sl]))[None]                # [1, r, Lk]
        s = (q[:, r] @ k.transpose(1, 2)) * c.scale
        s = torch.where(m, s, torch.full_like(s, -np.inf))
        live = m.any(-1)                                                          # [1, r]
        mx = torch.where(live, s.max(-1).values, torch.zeros(()).double())
        e = torch.exp(s - mx[..., None])                                          # 0 on hidden pairs
        l = e.sum(-1)
        P = e / torch.where(l > 0, l, torch.ones(()).double())[..., None]
        o, M = P @ v, P @ av
        T = (aq[:, r] @ ak.transpose(1, 2)) * c.scale
        out.terms = max(out.terms, float(torch.where(m, T, torch.zeros(()).double()).max()))
        PE = P * (T * (unit / c.scale))
        pe = PE.sum(-1)
        out.o[:, sl], out.M[:, sl] = o.numpy(), M.numpy()
        out.lse[:, sl] = torch.where(live, mx + torch.log(torch.where(l > 0, l, torch.ones(()).double())), torch.full_like(l, -np.inf)).numpy()
        out.S_o[:, sl], out.S_lse[:, sl] = (PE @ av + o.abs() * pe[..., None]).numpy(), pe.numpy()
        out.m0[:, sl] = s[..., :TILE].max(-1).values.numpy()
    return out


def lse_pattern(case: Case, b: int, dead_rows: int) -> np.ndarray:
    """[Lq] bool: True where lse must be finite, False where it must be -inf (module docstring, "dead")."""
    live = vis_of(case, b).any(1)
    if dead_rows and case.masked:
        live = live | (np.arange(case.Lq) >= case.seq_len(b))
    return live


class Reference:
    """One (case, family) in float64, every row of every sample; expected() adds a dead-row convention."""

    def __init__(self, inp: Inputs):
        self.inp, self.case = inp, inp.case
        self.S = [forward_rows(inp, b) for b in range(inp.case.B)]
        self.v_mean = [inp.v[b].double().mean(1).numpy() for b in range(inp.case.B)]               # [H, D] over all Lk columns
        self.av_mean = [inp.v[b].double().abs().mean(1).numpy() for b in range(inp.case.B)]

    def expected(self, b: int, dead_rows: int = 1):
        """(o, M, n, live) of sample b with its dead rows filled in under the convention."""
        s = self.S[b]
        live = s.n > 0
        o, M, n = s.o.copy(), s.M.copy(), s.n.astype(np.float64)
        if dead_rows:
            o[:, ~live], M[:, ~live], n[~live] = self.v_mean[b][:, None], self.av_mean[b][:, None], self.case.Lk
        return o, M, n, live

    def tol(self, b: int, core: str, dead_rows: int = 1):
        """(tol_o [H, L, D], tol_lse [H, L]) of the module docstring."""
        s = self.S[b]
        o, M, n, _ = self.expected(b, dead_rows)
        return tol_of(self.case, core, o, M, n, s.lse, s.S_o, s.S_lse)


def tol_of(case, core, o, M, n, lse, S_o, S_lse):
    rising = case.id in RISING
    t_o = (KAPPA[core] * 2.0 ** -9 + ACC * n[None, :, None] * 2.0 ** -24) * M + 2.0 ** -8 * np.abs(o) + (S_o if rising else 0.0)
    t_l = LSE_ABS[core] + LSE_REL * np.abs(np.where(np.isfinite(lse), lse, 0.0)) + n[None] * 2.0 ** -24 + (S_lse if rising else 0.0)
    return t_o, t_l


_REFS = {}


def reference(case: Case, family: str) -> Reference:
    """Cached per (case, family): every route and convention of the GPU test shares one reference, and nobody writes to it."""
    key = (case.id, family)
    if key not in _REFS:
        _REFS[key] = Reference(make_inputs(case, family))
    return _REFS[key]


def dense_f64(inp, b: int):
    """The independent anchor for short cases: a dense float64 torch softmax (rows that see nothing give zeros and -inf)."""
    c = inp.case
    q, k, v = (a[b].double() for a in (inp.q, inp.k, inp.v))
    mask = torch.from_numpy(c.visible(b))
    s = ((q @ k.transpose(-1, -2)) * c.scale).masked_fill(~mask, float("-inf"))
    dead = ~mask.any(-1, keepdim=True)
    p = torch.where(dead, torch.zeros_like(s), torch.softmax(s.masked_fill(dead, 0.0), -1))
    return (p @ v).numpy(), torch.logsumexp(s, -1).numpy()


# ---- mutations of the reference -------------------------------------------------------------------------------------------------
# name -> f(inp, b) -> [(label, rows, what)]: what a subtly wrong kernel would return on those rows.  `what` is a visibility
# [rows, Lk] the rows are recomputed under, or a callable (Rows of the true reference, expected o) -> (o', lse').
def _tile_of(c):
    return c // TILE


def _pick(items, n=2):
    items = sorted(set(items))
    return items[:1] + items[-1:] if len(items) > n else items


def _drop_key(inp, b, sel, label):
    c, res = inp.case, []
    for r, col in _pick([p for p in inp.pairs[b] if sel(*p)]):
        vis = vis_of(c, b)[[r]].copy()
        vis[0, col] = False
        res.append((f"{label}: key {col} hidden from row {r}", [r], vis))
    return res


def _leak_key(inp, b, sel, label):
    c, res = inp.case, []
    for r, col in _pick([p for p in inp.forbidden[b] if sel(*p)]):
        vis = vis_of(c, b)[[r]].copy()
        vis[0, col] = True
        res.append((f"{label}: key {col} shown to row {r}", [r], vis))
    return res


def _in_rect(case, b, r, col=None, edge=None):
    for rlo, rhi, clo, chi in case.live_rects(b):
        if rlo <= r < rhi and (edge is None or col == chi + edge):
            return True
    return False


def _drop_tile(inp, b, tile_sel, label):
    """One 64-key tile hidden from one 32-row block: a block that holds a sentinel row with a sentinel key in that tile."""
    c, res, seen = inp.case, [], set()
    k0 = int(np.argmax(c.valid(b)))
    for r, col in inp.pairs[b]:
        t, blk = _tile_of(col), r // 32
        if tile_sel(t, k0) and (t, blk) not in seen and len(seen) < 2:
            seen.add((t, blk))
            rows = np.arange(blk * 32, min(blk * 32 + 32, c.Lq))
            vis = vis_of(c, b)[rows].copy()
            vis[:, t * TILE:(t + 1) * TILE] = False
            res.append((f"{label}: tile {t} hidden from rows {rows[0]}..{rows[-1]}", rows, vis))
    return res


def m_rows_swapped(inp, b):
    if not inp.case.masked:
        return []
    rows = {r for r, _ in inp.pairs[b]}
    for r in sorted(rows):
        if r + 32 in rows and r % 64 < 32:
            return [(f"rows {r} and {r + 32} swapped", [r, r + 32], lambda R, o: (o[:, ::-1], R.lse[:, ::-1]))]
    return []


def _other_sample(inp, b, part):
    c = inp.case
    if not c.masked or c.B < 2:
        return []
    other = (b + 1) % c.B
    vis0, vis1 = vis_of(c, b), c.visible(b, **{part: other})
    rows = np.flatnonzero((vis0 != vis1).any(1))
    if not len(rows):
        return []
    rows = rows[np.linspace(0, len(rows) - 1, min(len(rows), 8)).astype(int)]
    return [(f"{part[:-3]} of sample {other}", rows, vis1[rows])]


def m_dead_mean_over_valid(inp, b):
    c = inp.case
    if not c.masked or c.valid(b).all():
        return []
    rows = np.flatnonzero(~vis_of(c, b).any(1))[:2]
    if not len(rows):
        return []
    valid = c.valid(b)
    mean = inp.v[b].double().numpy()[:, valid].mean(1)                           # [H, D]
    return [("dead rows averaged over the valid columns only", rows, lambda R, o: (np.broadcast_to(mean[:, None], o.shape), R.lse))]


def m_lse_first_tile(inp, b):
    """lse = m_ref + log l with the first tile's maximum where l was taken against the row's true maximum."""
    c = inp.case
    if not c.masked or int(np.argmax(c.valid(b))) >= TILE:                      # (a first tile nobody sees leaves no maximum)
        return []
    rows = np.arange(max(c.seq_len(b) - 8, 0), c.seq_len(b))

    def f(R, o):
        s = forward_rows(inp, b, rows)                                           # true maximum from the scores: lse - log l
        q, k = inp.q[b].double(), inp.k[b].double()
        sc = ((q[:, rows] @ k.transpose(1, 2)) * c.scale).numpy()
        mt = np.where(vis_of(c, b)[rows][None], sc, -np.inf).max(-1)
        with np.errstate(invalid="ignore"):
            return o, np.where(np.isfinite(s.m0), R.lse - (mt - s.m0), R.lse)
    return [("lse against the first tile's maximum", rows, f)]


_edge_lo = lambda r, c: c % TILE == TILE - 1 and c != SEAM - 1
_edge_hi = lambda r, c: c % TILE == 0 and c not in (0, SEAM)
MUTATIONS = {
    "key-dropped:below-tile-edge": lambda i, b: _drop_key(i, b, lambda r, c: _edge_lo(r, c) and c + 1 < i.case.Lk, "below a tile edge"),
    "key-dropped:above-tile-edge": lambda i, b: _drop_key(i, b, lambda r, c: _edge_hi(r, c), "above a tile edge"),
    "key-dropped:4095": lambda i, b: _drop_key(i, b, lambda r, c: c == SEAM - 1, "seam"),
    "key-dropped:4096": lambda i, b: _drop_key(i, b, lambda r, c: c == SEAM, "seam"),
    "key-dropped:last-key": lambda i, b: _drop_key(i, b, lambda r, c: c == i.case.Lk - 1, "last key"),
    "key-dropped:rect-last-column": lambda i, b: _drop_key(i, b, lambda r, c: i.case.masked and c > r and _in_rect(i.case, b, r, c, -1), "col_hi - 1"),
    "key-leaked:col_hi": lambda i, b: _leak_key(i, b, lambda r, c: i.case.masked and c > r and _in_rect(i.case, b, r, c, 0), "col_hi"),
    "key-leaked:after-diagonal": lambda i, b: _leak_key(i, b, lambda r, c: c == r + 1 and r < i.case.seq_len(b) and i.case.valid(b)[c], "diagonal + 1"),
    "key-leaked:in-hole": lambda i, b: _leak_key(i, b, lambda r, c: not i.case.valid(b)[c] and r < i.case.seq_len(b) and vis_of(i.case, b)[r].any(), "hole"),
    "key-leaked:row-seq_len": lambda i, b: _leak_key(i, b, lambda r, c: r == i.case.seq_len(b) and i.case.valid(b)[c], "row seq_len"),
    "tile-dropped:first-of-rank": lambda i, b: _drop_tile(i, b, lambda t, k0: t == _tile_of(k0), "first tile"),
    "tile-dropped:tile-64": lambda i, b: _drop_tile(i, b, lambda t, k0: t == SEAM // TILE, "tile 64"),
    "rows-r-and-r+32-swapped": m_rows_swapped,
    "rects-of-other-sample": lambda i, b: _other_sample(i, b, "rects_of"),
    "bits-of-other-sample": lambda i, b: _other_sample(i, b, "valid_of"),
    "seq_len-of-other-sample": lambda i, b: _other_sample(i, b, "seq_of"),
    "dead-rows-mean-over-valid-only": m_dead_mean_over_valid,
    "lse-against-first-tile": m_lse_first_tile,
}
PER_KEY = tuple(n_ for n_ in MUTATIONS if n_.startswith("key-"))
RISING_MUTATIONS = ("tile-dropped:first-of-rank", "lse-against-first-tile")      # what applies to the rising family (it lists no pairs)


def _rising_first_tile(inp, b):
    c = inp.case
    rows = np.arange(c.Lq - 32, c.Lq)
    vis = vis_of(c, b)[rows].copy()
    vis[:, :TILE] = False
    return [(f"first tile hidden from rows {rows[0]}..{rows[-1]}", rows, vis)]


def mutation_ratios(inp, b: int, names=None, dead_rows: int = 1, core: str = "64") -> dict:
    """{mutation: {label: worst |mutated - reference| / tolerance over o and lse}} of sample b, under the widest bar (the 64-row core's)."""
    c, res = inp.case, {}
    uni = (inp.v[b].double().mean(1).numpy(), inp.v[b].double().abs().mean(1).numpy())
    for name, f in MUTATIONS.items():
        if names is not None and name not in names:
            continue
        if inp.family == "rising":
            if name not in RISING_MUTATIONS:
                continue
            if name.startswith("tile-"):
                f = _rising_first_tile
        res[name] = {}
        for label, rows, what in f(inp, b):
            rows = np.asarray(rows)
            R = forward_rows(inp, b, rows)
            live = R.n > 0
            o, M, n = R.o.copy(), R.M.copy(), R.n.astype(np.float64)
            if dead_rows:
                o[:, ~live], M[:, ~live], n[~live] = uni[0][:, None], uni[1][:, None], c.Lk
            t_o, t_l = tol_of(c, core, o, M, n, R.lse, R.S_o, R.S_lse)
            if callable(what):
                o2, l2 = what(R, o)
            else:
                R2 = forward_rows(inp, b, rows, what)
                o2, l2 = R2.o.copy(), R2.lse
                if dead_rows:
                    o2[:, R2.n == 0] = uni[0][:, None]
            # what the GPU test compares: o on every row, lse on live rows, and the -inf / finite pattern of lse (lse_pattern)
            past = (rows >= c.seq_len(b)) & bool(dead_rows) & c.masked
            with np.errstate(invalid="ignore", divide="ignore"):
                ro = np.abs(o2 - o) / np.where(t_o > 0, t_o, 1e-300)
                pattern = (np.isfinite(l2) | past[None]) != (np.isfinite(R.lse) | past[None])
                rl = np.where(pattern, np.inf, np.where(live[None] & np.isfinite(l2), np.abs(l2 - R.lse) / t_l, 0.0))
            res[name][label] = float(max(np.where(o2 == o, 0.0, ro).max(), rl.max()))
    return res


# ---- layouts of the plain route ---------------------------------------------------------------------------------------------------
# The same values and the same float64 result; only where the device finds them differs.  ops.attention reads q, k, v in place through a
# batch, a head and a token stride each, and the product never hands it head-major tensors:
#   heads        permuted contiguous [B, H, L, Dh] tensors (token stride Dh, head stride L Dh)
#   heads+spare  the same with SPARE more key rows per head in the k and the v buffer that the call does not name
#   qkv          one buffer [B, L + SPARE, 3, H, Dh], q / k / v = buf[:, :L, i]: SigLIP's call (token stride 3 H Dh, head stride Dh)
#   q+kv         q [B, Lq, H, Dh] and one buffer [B, Lk + SPARE, 2, H, Dh], k / v = kv[:, :Lk, i]: the Perceiver's call (v sits H Dh behind k)
# Every layout but "heads" takes its views from buffers with one more LEADING sample when B > 1 (the base is not the allocation's and,
# with the spare rows, the batch stride is not the product of the view's sizes).  What the call does not name is adversarial, as the table
# treats forbidden pairs: a spare key row scores LEVEL + LIFT against a sentinel row's q (row Lk against the last row's, the others in turn
# against every row that has pairs; N(0, 1) in the diffuse family, where the value alone is enough) and carries v = FORBIDDEN_V; the
# leading sample is sample 0 with v = FORBIDDEN_V throughout.  Spare rows of a q slot are zero: the kernel guards its stores by row < Lq.
# attn_nc_bf16 loads the rows min(c, Lk - 1) and masks the last tile by a count: a kernel that keeps to that never touches a spare row;
# one that rounds Lk up to a tile, or miscounts by one, reads row Lk.  Every stride is a multiple of 8 elements and every base of 16 bytes.
LAYOUTS = ("heads", "heads+spare", "qkv", "q+kv")
SPARE = 70                                     # more than one 64-key tile and no multiple of it


def layouts(case: Case) -> tuple:
    if case.masked:
        return ()
    return LAYOUTS if case.Lq == case.Lk else tuple(l for l in LAYOUTS if l != "qkv")


@dataclass
class Placed:
    """The buffers of one (case, family, layout) on the host; views() cuts q, k, v out of them (or out of copies on a device)."""
    case: Case
    layout: str
    bufs: dict                     # name -> bf16 tensor
    lead: int                      # leading samples the views skip

    def views(self, bufs=None):
        """q [B, Lq, H, Dh], k, v [B, Lk, H, Dh] as ops.attention takes them."""
        b_, c, s = self.bufs if bufs is None else bufs, self.case, self.lead
        if self.layout in ("heads", "heads+spare"):
            return tuple(b_[n_][s:, :, :L_].permute(0, 2, 1, 3) for n_, L_ in (("q", c.Lq), ("k", c.Lk), ("v", c.Lk)))
        if self.layout == "qkv":
            return tuple(b_["qkv"][s:, :c.Lq, i] for i in range(3))
        return b_["q"][s:], b_["kv"][s:, :c.Lk, 0], b_["kv"][s:, :c.Lk, 1]


def spare_rows(inp, b: int):
    """(k, v) [H, SPARE, Dh] float64 of the rows behind key Lk - 1 of sample b (the comment above)."""
    c = inp.case
    rng = np.random.default_rng(zlib.crc32(f"fwd/{c.id}/{inp.family}/spare/{b}".encode()))
    k = rng.standard_normal((c.H, SPARE, c.Dh))
    if inp.family == "sentinel":
        rows = sorted({r for r, _ in inp.pairs[b]}, reverse=True)              # the last row first: it is on every case's list
        assert rows and rows[0] == c.Lq - 1
        q = inp.q[b].double().numpy()
        for j in range(SPARE):
            qr = q[:, rows[j % len(rows)]]                                       # [H, Dh]
            k[:, j] = qr * ((np.log(100.0 * c.Lk) + LIFT) / (c.scale * (qr * qr).sum(-1, keepdims=True)))
    return k, np.full((c.H, SPARE, c.Dh), FORBIDDEN_V)


def place(inp, layout: str) -> Placed:
    c = inp.case
    assert layout in layouts(c)
    B, H, Lq, Lk, D = c.B, c.H, c.Lq, c.Lk, c.Dh
    if layout == "heads":
        return Placed(c, layout, dict(q=inp.q.contiguous(), k=inp.k.contiguous(), v=inp.v.contiguous()), 0)
    lead = 1 if B > 1 else 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)
    q = torch.cat([inp.q[:lead], inp.q])                                         # [lead + B, H, L, D]: the leading sample is sample 0 ...
    k = torch.cat([inp.k[:lead], inp.k])
    v = torch.cat([torch.full_like(inp.v[:lead], FORBIDDEN_V), inp.v])           # ... with the forbidden value on every key
    sp = [spare_rows(inp, max(i - lead, 0)) for i in range(lead + B)]
    k = torch.cat([k, t(np.stack([s[0] for s in sp]))], 2)                       # [lead + B, H, Lk + SPARE, D]
    v = torch.cat([v, t(np.stack([s[1] for s in sp]))], 2)
    if layout == "heads+spare":
        bufs = dict(q=q.contiguous(), k=k.contiguous(), v=v.contiguous())
    elif layout == "qkv":
        qs = torch.cat([q, torch.zeros_like(k[:, :, Lk:])], 2)
        bufs = dict(qkv=torch.stack([a.permute(0, 2, 1, 3) for a in (qs, k, v)], 2).contiguous())                   # [., L + SPARE, 3, H, D]
    else:
        bufs = dict(q=q.permute(0, 2, 1, 3).contiguous(), kv=torch.stack([a.permute(0, 2, 1, 3) for a in (k, v)], 2).contiguous())
    return Placed(c, layout, bufs, lead)


def check_views(placed: Placed, views):
    """What attn_nc_bf16 refuses, asserted before a launch: channel stride 1, the other strides multiples of 8 elements, bases of 16 bytes;
    and every element the strides can reach lies inside its buffer."""
    for x in views:
        assert x.stride(3) == 1 and all(x.stride(i) % 8 == 0 for i in range(3)) and x.data_ptr() % 16 == 0, (placed.layout, x.stride())
        last = x.storage_offset() + sum((n_ - 1) * s for n_, s in zip(x.shape, x.stride()))
        assert last < x.untyped_storage().nbytes() // 2


def gather(placed: Placed, mutation: str = None):
    """q, k, v [B, H, L, Dh] bf16 read back out of the buffers by the kernel's own address rule - element = base + b s_b + h s_h + t s_t + d
    with the base and the strides of the views - or by a subtly wrong one: the layout mutations."""
    c = placed.case
    views = placed.views()
    check_views(placed, views)
    out = []
    for name, x in zip("qkv", views):
        flat = torch.as_strided(x, (x.untyped_storage().nbytes() // 2,), (1,), 0)                                  # the whole allocation
        base, (sb, st, sh, _) = x.storage_offset(), x.stride()
        L_ = x.shape[1]
        if name != "q" and mutation == "keys-past-Lk-visible":
            L_ += SPARE
        if name != "q" and mutation == "one-key-past-Lk-visible":
            L_ += 1
        if name == "v" and mutation == "v-read-from-k-slot":
            base = views[1].storage_offset()
        bi = torch.arange(c.B)[:, None, None, None] * (0 if mutation == "batch-stride-ignored" else sb)
        hi = torch.arange(c.H)[None, :, None, None]
        if name == "v" and mutation == "head-h-reads-head-h+1":
            hi = (hi + 1) % c.H
        idx = base + bi + hi * sh + torch.arange(L_)[None, None, :, None] * st + torch.arange(c.Dh)[None, None, None, :]
        out.append(flat[idx])
    return tuple(out)


def _fused(placed):
    return placed.layout in ("qkv", "q+kv")


def _spare(placed):
    return placed.layout != "heads"


# name -> (applies(placed), samples that show it)
LAYOUT_MUTATIONS = {
    "v-read-from-k-slot": (_fused, lambda c: range(c.B)),                        # the fused offset: v = k
    "head-h-reads-head-h+1": (lambda p: p.case.H > 1, lambda c: range(c.B)),     # v of the next head (the last head reads the first)
    "batch-stride-ignored": (lambda p: p.case.B > 1, lambda c: range(1, c.B)),   # every sample reads the first one the call names
    "keys-past-Lk-visible": (_spare, lambda c: range(c.B)),                      # the whole spare region counted
    "one-key-past-Lk-visible": (_spare, lambda c: range(c.B)),                   # a last-tile count that is one too large
}


def layout_mutation_ratios(inp, layout: str, core: str = "64") -> dict:
    """{mutation: {sample: worst |mutated - reference| / tolerance over o and lse}} of the layout mutations that apply, under the widest
    bar as in mutation_ratios().  The unmutated gather must give back the inputs bit for bit."""
    c = inp.case
    placed = place(inp, layout)
    assert all(torch.equal(a, b_) for a, b_ in zip(gather(placed), (inp.q, inp.k, inp.v))), f"{c.id} [{layout}]: the gather does not return the inputs"
    res = {}
    for name, (applies, samples) in LAYOUT_MUTATIONS.items():
        if not applies(placed):
            continue
        q, k, v = gather(placed, name)
        got = Inputs(c, inp.family, q, k, v, inp.pairs, inp.forbidden)
        res[name] = {}
        for b in samples(c):
            R = forward_rows(inp, b)
            R2 = forward_rows(got, b, vis=np.ones((c.Lq, k.shape[2]), dtype=bool))
            t_o, t_l = tol_of(c, core, R.o, R.M, R.n.astype(np.float64), R.lse, R.S_o, R.S_lse)
            res[name][b] = float(max((np.abs(R2.o - R.o) / t_o).max(), (np.abs(R2.lse - R.lse) / t_l).max()))
    return res

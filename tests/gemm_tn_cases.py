"""Case table, input families, float64 reference, bars and reference mutations of the weight-gradient GEMM aki_gemm_tn
(aki_amd/csrc/gemm_tn_bf16.hip):  c[i][j] = sum_r a[r][i] b[r][j]  over the Kc rows of two row-major operands, bf16 in, f32 accumulate, bf16 out.

numpy and CPU torch only.  tests/test_gemm_tn_cases_cpu.py checks the table itself - every structural edge of the kernel reached (from the
constants parsed out of gemm_tn_bf16.hip), every mutation visible, a plain float32 product inside both bars - and tests/test_gemm_tn_gpu.py
runs every case on the device.

Cases.  A case is (Kc, I, J) and three layouts.  nk = ceil(Kc / TN_BK) K-steps: the hot loop takes six at a time while seven lie ahead, a
run-time loop the steps that still have two behind them, a last loop the final two; A sits on a three-deep ring, B on a two-deep one.
  operand layouts (OPERANDS)   the view is rows row0.. and columns col0.. of a [row0 + Kc + below, ld] buffer filled with NaN: one row or more above,
      64 rows or more below, and - where ld > cols - columns on both sides.  'whole' and 'rows' (a row slice of a taller tensor) have ld = cols:
      what lies beside a row there is the neighbouring rows.  'cols' / 'cols16' are column slices of wider tensors.  col0 is a multiple of 8.
      The kernel zeroes rows Kc.. of the last step through the buffer descriptor only; a NaN that leaks in is 0 * NaN = NaN in every output.
  output layouts (OUTPUTS)     the view starts `ldc + off` elements into a flat buffer of (I + 2) * ldc + 16 elements filled with GUARD.
      wide (16-byte stores): ldc % 8 == 0 and the view 16-byte aligned.  narrow (8-byte stores): ldc % 4 == 0 only, or the view 8-byte aligned.
  near-4g   both operands are views (columns 8..15 and 24..31) of ONE [1 + 64 nk, LD_BIG] buffer, LD_BIG = 2^20 + 1024, Kc = 2047:
      ((Kc - 1) * ld + 8) * 2 = 2^32 - 4080, and row 2047, the one padding row of the last step, lies at byte 2^32 + 2^21 - 2048: a 32-bit
      voffset + soffset wraps to row 0, column 2^20 - 1024 + col0.  The buffer spans all 64 nk rows, so no read leaves the allocation whatever
      the range check does.  Rows Kc.. hold P_TAIL, everything else outside the two views P_WRAP, both finite: a leak of the padding row adds
      P_TAIL^2 = 9 to every output, a wrapped read P_WRAP^2 = 4, zeros nothing.  b shares a's buffer because the two operands' padding rows
      meet in a product: a finite leak into one operand alone is multiplied by the other's zeros and cannot be seen.
  near-4g-twin   one row further (Kc = 2048): the span reaches 2^32 bytes; aki_gemm_tn and _tn_ok refuse it.

Input families (rounded to bf16 first).
  exact     a, b = +-1 with probability 1/4 each, else 0; a row that came out all zero gets one +-1, so every contraction row has a non-zero
            outer product.  Every partial sum is a small integer: the f32 accumulation is exact in any order and the bf16 cast is exact
            while |x| <= 256 (the CPU test asserts it of every case).  The bar is zero.  A dropped, doubled, stale or mis-ordered
            contraction row changes about a quarter of the elements it touches by +-1.
  diffuse   a, b ~ N(0, 1);  one-sign: |N(0, 1)| with one sign per column, so that M = |x|.  The bar is the one of tests/train_kernel_cases.py
            (Out, imported): tol = half_ulp_bf16(|x| + alpha) + alpha + floor, alpha = KAPPA 2^-24 M, M = sum_r |a_ri b_rj|, KAPPA = 64 nk:
            a product of two bf16 values is exact in f32, so one f32 rounding per accumulated term, padding rows included, whatever the order.
Nothing is tuned on the kernel's output.
"""
import os
import re
from types import SimpleNamespace as NS

import numpy as np

from train_kernel_cases import BF, MIN_RATIO, ROOT, Out, bf, f64, rng_of      # the bar is imported, not copied

FAMILIES = ("exact", "diffuse", "one-sign")
GUARD = 0x5A5A
P_TAIL, P_WRAP = 3.0, 2.0
LD_BIG = (1 << 20) + 1024
EXACT_MAX = 256.0


def kernel_constants():
    """Tile sizes, the i-tile group, the loop bounds and the ring depths as gemm_tn_bf16.hip is compiled: a changed constant moves an
    edge, and the CPU test then fails the table instead of silently testing beside it."""
    with open(os.path.join(ROOT, "aki_amd", "csrc", "gemm_tn_bf16.hip")) as f:
        src = f.read()
    out = {}
    for name in ("TN_BI", "TN_BJ", "TN_BK", "GM"):
        m = re.search(r"constexpr\s+int\b[^;]*\b%s\s*=\s*(\d+)" % name, src)
        assert m, f"{name} not found in gemm_tn_bf16.hip"
        out[name] = int(m.group(1))
    m = re.search(r"for\s*\(;\s*kt\s*\+\s*(\d+)\s*<\s*nk;\s*kt\s*\+=\s*(\d+)\)\s*static_for<(\d+)>", src)
    assert m and m.group(2) == m.group(3), "the unrolled loop not found in gemm_tn_bf16.hip"
    out["UNROLL_AHEAD"], out["UNROLL"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"for\s*\(;\s*kt\s*\+\s*(\d+)\s*<\s*nk;\s*\+\+kt\)\s*kstep\(std::true_type", src)
    assert m, "the FULL run-time loop not found in gemm_tn_bf16.hip"
    out["FULL_AHEAD"] = int(m.group(1))
    m, n = re.search(r"\((\d+)\s*\+\s*slot\)\s*\*\s*TN_OP_BYTES", src), re.search(r"SMEM\s*=\s*(\d+)\s*\*\s*TN_OP_BYTES", src)
    assert m and n, "the ring depths not found in gemm_tn_bf16.hip"
    out["A_RING"], out["B_RING"] = int(m.group(1)), int(n.group(1)) - int(m.group(1))
    return out


def loops(nk, K=None):
    """The loop that runs K-step kt, for kt = 0..nk-1: 'unrolled' | 'full' | 'last'."""
    K = K or kernel_constants()
    out, kt = [], 0
    while kt + K["UNROLL_AHEAD"] < nk:
        out += ["unrolled"] * K["UNROLL"]
        kt += K["UNROLL"]
    while kt + K["FULL_AHEAD"] < nk:
        out.append("full")
        kt += 1
    return out + ["last"] * (nk - kt)


def xcd_remap(bid, nwg):
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


def tile_of(t, tiles_i, tiles_j, GM, short_groups=True):
    """(ti, tj) of logical tile id t; short_groups=False decodes the last group of i-tiles as if it were full."""
    per = GM * tiles_j
    first = t // per * GM
    gsz = min(tiles_i - first, GM) if short_groups else GM
    return first + (t % per) % gsz, (t % per) // gsz


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
OPERANDS = {                                  # ld = cols + pad
    "whole": dict(pad=0, col0=0, row0=1, below=64),
    "rows": dict(pad=0, col0=0, row0=70, below=96),
    "cols": dict(pad=64, col0=8, row0=1, below=64),
    "cols16": dict(pad=24, col0=16, row0=3, below=64),
}
OUTPUTS = {                                   # ldc = J + pad; the view starts ldc + off elements into the flat buffer
    "wide": dict(pad=0, off=0),
    "wide-pitch": dict(pad=24, off=8),
    "narrow-ld": dict(pad=4, off=0),          # ldc % 4 == 0 only
    "narrow-ld12": dict(pad=12, off=4),
    "narrow-base": dict(pad=0, off=4),        # ldc == J, the view 8-byte aligned
    "narrow-base-pitch": dict(pad=8, off=4),
}


class Case:
    def __init__(self, id, Kc, I, J, la="whole", lb="whole", lc="wide", why=""):
        self.id, self.Kc, self.I, self.J, self.la, self.lb, self.lc, self.why = id, Kc, I, J, la, lb, lc, why
        self.shared = la == "shared"
        K = kernel_constants()
        self.nk = (Kc + K["TN_BK"] - 1) // K["TN_BK"]
        self.tiles_i, self.tiles_j = (I + K["TN_BI"] - 1) // K["TN_BI"], (J + K["TN_BJ"] - 1) // K["TN_BJ"]
        self.grid = self.tiles_i * self.tiles_j
        self.lda = LD_BIG if self.shared else I + OPERANDS[la]["pad"]
        self.ldb = LD_BIG if self.shared else J + OPERANDS[lb]["pad"]
        self.ldc, self.c_off = J + OUTPUTS[lc]["pad"], J + OUTPUTS[lc]["pad"] + OUTPUTS[lc]["off"]
        self.wide = self.ldc % 8 == 0 and (self.c_off * 2) % 16 == 0
        self.span_a, self.span_b = ((Kc - 1) * self.lda + I) * 2, ((Kc - 1) * self.ldb + J) * 2      # bytes the descriptor covers
        self.refused = max(self.span_a, self.span_b) >= 1 << 32
        self.kappa = 64.0 * self.nk

    def __repr__(self):
        return self.id


def _cases():
    C, out = Case, []
    # step counts at one full tile, every K tail among them; the layouts rotate
    lay = [("whole", "whole", "wide"), ("cols", "cols16", "wide-pitch"), ("rows", "whole", "narrow-ld"), ("whole", "cols", "narrow-base"),
           ("cols16", "rows", "wide"), ("rows", "rows", "narrow-base-pitch"), ("cols", "whole", "wide-pitch"), ("whole", "rows", "narrow-ld12")]
    why = {1: "one step: no second stage, Kc = 1", 2: "stage_a(1, 1) is the last stage, both steps non-FULL", 3: "one FULL run-time step",
           4: "aslot walks round, a_next wraps", 5: "63 rows in the last step", 6: "four FULL run-time steps", 7: "the most the run-time loops take alone",
           8: "first entry into the unrolled block, FULL run-time loop skipped", 9: "one FULL step behind the block", 13: "five FULL run-time steps behind one unrolled block",
           14: "two unrolled blocks and the last two steps"}
    for n, (nk, Kc) in enumerate(((1, 1), (2, 72), (3, 160), (4, 225), (5, 319), (6, 384), (7, 385), (8, 456), (9, 545), (13, 800), (14, 896))):
        out.append(C(f"nk{nk}-k{Kc}", Kc, 256, 256, *lay[n % len(lay)], why=why[nk]))
    for nk, Kc in ((10, 577), (11, 704), (12, 767)):                  # the residues nk mod 6 = 4, 5, 0 behind an unrolled block
        out.append(C(f"nk{nk}-k{Kc}-small", Kc, 16, 24, "cols", "rows", "narrow-ld", why=f"nk mod 6 = {nk % 6} behind the unrolled block"))
    # tile tails
    for Kc, I, J, la, lb, lc in ((63, 8, 8, "whole", "cols", "wide"), (64, 16, 120, "cols", "whole", "narrow-ld"), (100, 120, 16, "rows", "cols16", "wide-pitch"),
                                 (33, 136, 248, "cols16", "rows", "narrow-base"), (96, 248, 136, "whole", "whole", "wide"),
                                 (65, 264, 520, "cols", "cols", "wide-pitch"), (40, 520, 264, "rows", "whole", "narrow-ld12"),
                                 (129, 8, 520, "cols", "rows", "wide"), (72, 520, 8, "whole", "cols16", "narrow-base-pitch")):
        out.append(C(f"tail-k{Kc}-i{I}-j{J}", Kc, I, J, la, lb, lc, why="tails of the 16-column fragment, the wave tile and the tile; clamped loads"))
    # tile mapping: every branch of xcd_remap, short last groups of i-tiles
    for ti, tj, Kc in ((2, 1, 8), (7, 1, 40), (4, 2, 64), (9, 1, 33), (9, 3, 72), (11, 1, 1), (11, 3, 65)):
        out.append(C(f"grid{ti * tj}-t{ti}x{tj}", Kc, ti * 256 - 8, tj * 256 - (0 if tj == 1 else 8), "whole", "cols", "wide" if ti % 2 else "narrow-ld",
                     why=f"grid {ti * tj}: {ti} x {tj} tiles"))
    # stores: both paths, ldc == J and ldc > J, a full tile and tile tails
    for lc in OUTPUTS:
        out.append(C(f"store-{lc}-full", 40, 256, 256, "whole", "whole", lc, why="store path at a full tile"))
        out.append(C(f"store-{lc}-tail", 40, 136, 264, "cols", "cols16", lc, why="store path at tile tails"))
    out.append(C("near-4g", 2047, 8, 8, "shared", "shared", "wide", why="the padding row of the last step lies past 2^32 bytes"))
    out.append(C("near-4g-twin", 2048, 8, 8, "shared", "shared", "wide", why="the span reaches 2^32 bytes: refused"))
    return tuple(out)


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}
RUN_CASES = tuple(c for c in CASES if not c.refused)
SMALL_CASES = tuple(c for c in RUN_CASES if not c.shared)
STEP_CASES = tuple(c for c in CASES if c.id.startswith("nk") and c.I == 256 and c.J == 256)


def shared_cols(which):
    return 8 if which == "a" else 24


def wrap_target(c, which, r):
    """(row, column) inside the shared buffer that a 32-bit offset of padding row r (>= Kc) of the near-4g case points at."""
    e = (r * LD_BIG * 2 - (1 << 32)) // 2 + LD_BIG + shared_cols(which)       # element from the buffer's start (the views begin in row 1)
    return e // LD_BIG, e % LD_BIG


# ---- inputs, reference, bars ---------------------------------------------------------------------------------------------------------
def bar_of(family):
    return "exact" if family == "exact" else "diffuse"


def inputs(c, family):
    """a [Kc, I], b [Kc, J] as compact bf16 CPU tensors; the device test places them into their backing buffers."""
    g = rng_of("gemm_tn", c.Kc, c.I, c.J, family)

    def draw(n):
        if family == "exact":
            x = np.where(g.random((c.Kc, n)) < 0.5, 1.0, -1.0) * (g.random((c.Kc, n)) < 0.5)
            dead = np.flatnonzero(~x.any(1))
            x[dead, g.integers(0, n, dead.size)] = np.where(g.random(dead.size) < 0.5, 1.0, -1.0)
            return x
        x = g.standard_normal((c.Kc, n))
        return np.abs(x) * np.where(g.random(n) < 0.5, -1.0, 1.0) if family == "one-sign" else x
    return NS(a=bf(draw(c.I)), b=bf(draw(c.J)))


def as_out(c, family, x, M=None):
    return Out(x, kind="exact") if bar_of(family) == "exact" else Out(x, M, c.kappa)


def reference(c, inp, family):
    a, b = f64(inp.a), f64(inp.b)
    return as_out(c, family, a.T @ b, np.abs(a).T @ np.abs(b))


def product_f32(inp):
    return f64((inp.a.float().t() @ inp.b.float()).to(BF))


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
def _padded(c, x, K):
    out = np.zeros((c.nk * K["TN_BK"], x.shape[1]))
    out[:c.Kc] = x
    return out


def tail_rows(c, how):
    """What the padding rows Kc..64 nk - 1 of (a, b) hold if they are not zeroed: 'behind' the views, or at the 'wrap'ped offsets."""
    n = c.nk * kernel_constants()["TN_BK"] - c.Kc
    v = (P_TAIL if how == "behind" else P_WRAP) if c.shared else np.nan
    return np.full((n, c.I), v), np.full((n, c.J), v)


def drop_rows(c, K=None):
    """The contraction rows whose loss must be seen: the first rows of an 8-row group, of a 32-row half, of every step, and the last."""
    K = K or kernel_constants()
    BK = K["TN_BK"]
    rows = {0, 3, 4, 7, 8, 31, 32, 63} | {BK * k for k in range(1, c.nk)} | {c.Kc - 1, BK * (c.nk - 1)}
    return sorted(r for r in rows if r < c.Kc)


def mutate(c, inp, mut, arg=None):
    """The float64 result of a kernel with the named fault (NaN: an element that was never written)."""
    K = kernel_constants()
    BK, BI, BJ = K["TN_BK"], K["TN_BI"], K["TN_BJ"]
    a, b = f64(inp.a), f64(inp.b)
    x = a.T @ b
    I, J = c.I, c.J
    if mut == "drop-row":
        return x - np.outer(a[arg], b[arg])
    if mut in ("stale-a", "stale-b"):
        kt, ap, bp = arg, _padded(c, a, K), _padded(c, b, K)
        step = lambda p, k: p[k * BK:(k + 1) * BK]
        if mut == "stale-a":
            return x - step(ap, kt).T @ step(bp, kt) + step(ap, kt - K["A_RING"]).T @ step(bp, kt)
        return x - step(ap, kt).T @ step(bp, kt) + step(ap, kt).T @ step(bp, kt - K["B_RING"])
    if mut in ("k-tail-leak", "offset-wrap"):
        ta, tb = tail_rows(c, "behind" if mut == "k-tail-leak" else "wrap")
        return x + ta.T @ tb
    if mut == "fragment-swap":                                   # fragments n = 0 and 1 of wave row 0
        y = x.copy()
        y[0:16], y[16:32] = x[16:32], x[0:16]
        return y
    if mut == "swizzle":                                         # pieces q = 0 and 1 of LDS row 5 of every step
        a2 = a.copy()
        r = np.arange(c.Kc) % BK == 5
        a2[r, 0:16], a2[r, 16:32] = a[r, 16:32], a[r, 0:16]
        return a2.T @ b
    if mut == "store-transposed":                                # every whole 16 x 16 fragment of wave tile (0, 0)
        y = x.copy()
        for n in range(min(I, 128) // 16):
            for m in range(min(J, 64) // 16):
                y[16 * n:16 * n + 16, 16 * m:16 * m + 16] = x[16 * n:16 * n + 16, 16 * m:16 * m + 16].T
        return y
    if mut == "store-tail-dropped":
        y = x.copy()
        y[:, J - 8:] = np.nan
        return y
    if mut == "store-halves":                                    # the 16-byte store without the permlane swap
        y = x.copy()
        for base in range(0, J // 32 * 32, 32):
            for kg in range(4):
                d = base + 16 * (kg & 1) + 8 * (kg >> 1)
                y[:, d:d + 4], y[:, d + 4:d + 8] = x[:, base + 4 * kg:base + 4 * kg + 4], x[:, base + 16 + 4 * kg:base + 16 + 4 * kg + 4]
        return y
    if mut == "clamp-a":                                         # min(i0 + col, I - 16): the last chunk reads the one before it
        y = x.copy()
        y[I - 8:] = x[I - 16:I - 8]
        return y
    if mut == "clamp-b":
        y = x.copy()
        y[:, J - 8:] = x[:, J - 16:J - 8]
        return y
    if mut == "tile-swap":                                       # tile (ti, tj) lands at (tj, ti)
        y = x.copy()
        for ti in range(c.tiles_i):
            for tj in range(c.tiles_j):
                blk = x[ti * BI:(ti + 1) * BI, tj * BJ:(tj + 1) * BJ]
                h, w = min(blk.shape[0], I - tj * BI), min(blk.shape[1], J - ti * BJ)
                if h > 0 and w > 0:
                    y[tj * BI:tj * BI + h, ti * BJ:ti * BJ + w] = blk[:h, :w]
        return y
    if mut == "tile-gsz8":                                       # tile ids decoded as if every group of i-tiles were full
        y = np.full_like(x, np.nan)
        for t in range(c.grid):
            ti, tj = tile_of(xcd_remap(t, c.grid), c.tiles_i, c.tiles_j, K["GM"], short_groups=False)
            if ti < c.tiles_i and tj < c.tiles_j:
                y[ti * BI:(ti + 1) * BI, tj * BJ:(tj + 1) * BJ] = x[ti * BI:(ti + 1) * BI, tj * BJ:(tj + 1) * BJ]
        return y
    if mut == "narrow-accumulator":                              # the accumulator rounded to bf16 after every K-step
        ap, bp = _padded(c, a, K), _padded(c, b, K)
        acc = np.zeros_like(x)
        for kt in range(c.nk):
            acc = f64(bf(acc + ap[kt * BK:(kt + 1) * BK].T @ bp[kt * BK:(kt + 1) * BK]))
        return acc
    raise KeyError(mut)


def stale_steps(c, depth, K=None):
    """{loop: the first step kt >= depth that the loop runs}"""
    out = {}
    for kt, loop in enumerate(loops(c.nk, K)):
        if kt >= depth:
            out.setdefault(loop, kt)
    return out


def _mutations():
    """mutation -> (bar family, [(case id, argument)]): every listed pair must break the bar."""
    K = kernel_constants()
    m = {"drop-row": ("exact", [(c.id, r) for c in STEP_CASES for r in drop_rows(c, K)])}
    for mut, depth in (("stale-a", K["A_RING"]), ("stale-b", K["B_RING"])):
        m[mut] = ("exact", [(c.id, kt) for c in STEP_CASES for kt in sorted(set(stale_steps(c, depth, K).values()))])
    m["k-tail-leak"] = ("exact", [(c.id, None) for c in RUN_CASES if c.Kc % K["TN_BK"]])
    m["offset-wrap"] = ("exact", [("near-4g", None)])
    m["fragment-swap"] = ("exact", [("nk1-k1", None), ("tail-k33-i136-j248", None)])
    m["swizzle"] = ("exact", [("nk2-k72", None), ("tail-k96-i248-j136", None)])
    m["store-transposed"] = ("exact", [("store-wide-full", None), ("store-narrow-ld-tail", None)])
    m["store-tail-dropped"] = ("exact", [("store-wide-pitch-tail", None), ("store-narrow-base-tail", None)])
    m["store-halves"] = ("exact", [(c.id, None) for c in SMALL_CASES if c.id.startswith("store-wide")])
    m["clamp-a"] = ("exact", [("tail-k100-i120-j16", None), ("tail-k72-i520-j8", None)])
    m["clamp-b"] = ("exact", [("tail-k64-i16-j120", None), ("tail-k129-i8-j520", None)])
    m["tile-swap"] = ("exact", [("tail-k65-i264-j520", None), ("grid27-t9x3", None)])
    m["tile-gsz8"] = ("exact", [("grid27-t9x3", None), ("grid33-t11x3", None)])        # with one j tile both decodes coincide
    m["narrow-accumulator"] = ("diffuse", [("nk13-k800", None), ("nk14-k896", None)])
    return m


MUTATIONS = _mutations()

"""Case tables, input families, float64 references, bars and reference mutations of the small forward kernels in front of every GEMM and
every decode step: norm_bf16_kernel<RMS|LN>, norm_f32_kernel<RMS|LN>, row_stats_kernel (aux_kernels.hip), quant_rows_fp8_kernel<RMS>
(fp8_quant.hip), kv_cache_quant_fp8_kernel and rope_append_kernel (decode.hip).

numpy and CPU torch only.  tests/test_fwd_row_cases_cpu.py checks the table itself, tests/test_fwd_row_gpu.py runs every case on the
device.  EPS, MIN_RATIO and the bar itself - Out.tol(x) = half_ulp(|x| + a) + a + floor, a = KAPPA 2^-24 M(x), half_ulp = 2^-8 or 2^-24 of
the binade, floor = 2^-126 - are those of tests/train_kernel_cases.py, imported and not copied.  Nothing is tuned on a kernel's output.

KAPPA of the norms and the row statistics (eps = 2^-24 is one f32 operation; the library is built with -ffp-contract=off).
  A row sum is a chain of R additions: the thread's own values, 6 wave steps, 4 partial sums.
      norm_bf16_kernel   MAXC * 8 = 32 values per thread at most                       R = 32 + 10 = 42
      row_stats_kernel   ceil(cols / 2048) * 8 values per thread                       R = that + 10   (82 at 16392 columns)
      norm_f32_kernel    ceil(cols / 256) values per thread                            R = that + 10   (22 at 3072 columns)
  K_sum  = R + 2     the additions, the product under the sum (x x, d d) and the division by cols
  mean   = s1 / cols                       K_mean = K_sum on mean|x|                   (f32 output of row_stats)
  var    RMS: s2 / cols, K_var = K_sum.  LN: mean(d^2), d = x - mean: one rounding of d (2 eps on d^2), K_var = K_sum + 2; the error
         e of the mean enters as -2 e mean(d) + e^2 = e^2 (sum d = 0): second order, kept as the absolute term
         (K_mean eps mean|x|)^2 on var (0.5 eps relative on the offset family).
  rstd   = rsqrtf(var + eps): the addition 1, the root halves, rsqrtf 1 ulp = 2 eps:   K_rstd = (K_var + 1) / 2 + 2 on rstd, plus
         rstd (K_mean eps mean|x|)^2 / (2 (var + eps))                                 (f32 output of row_stats)
  LN y   = (d rstd) w + b.  d is off by K_mean eps mean|x| + eps |d|, n = d rstd by rstd times that + (K_rstd + 1) eps |n|, the
         product and the sum add eps (|w n| + |y|):  KAPPA_y = K_mean + K_rstd + 4 on M = |w| (|x| + mean|x|) rstd + |b|, one final
         cast (bf16 or f32).  An all-zero row has d = n = 0 exactly and y is the bias bit for bit.
  RMS y  f32: y = w (x rstd): KAPPA = K_rstd + 2 on |w n|.  bf16 rounds twice, y = bf16(w * bf16(x rstd)) (HF Phi3RMSNorm).  With n
         the float64 x rstd and a = (K_rstd + 1) eps |n|, an element is DECIDED when n - a and n + a round to the same bf16 value; it
         is then held to the outer cast alone, half_ulp(|w bf16(n)|) + floor (the product of two bf16 values is exact in f32).  An
         undecided element may come from either neighbour.  An all-zero row gives exact zeros.
  sum x^2 stays below 2^127: beyond it the kernels' f32 sums overflow, and so does the float32 reference the CPU test holds to the bar.

fp8 (OCP e4m3fn) quantisers.  scale: the float64 max(amax, 1e-12f) / 448 to 2^-23 relative for quant_rows_fp8 (s = amax * fl(1 / 448):
  a rounded reciprocal and one product) and to 2^-24 for the KV kernel (one correctly rounded division).  In RMS mode amax may come from
  either admissible bf16 value of an undecided element.  bytes: judged against t = y / s_dev in float64 with s_dev the device's scale
  (held to its own bar), so an admissible last bit of the scale does not leak into the byte verdict; admissible are the round-to-
  nearest-even images (e4m3_rne, numpy) of clamp(t (1 +- delta), +-448): delta = 2^-23 for quant_rows (inv = fl(1 / s), one product),
  2^-24 for the KV kernel (one division), 0 where amax = 448 * 2^k makes s a power of two and every operation exact - there a tie
  must go to even.  That holds for quant_rows too: fl(1 / 448) = (1 / 448) (1 + 0.75 * 2^-24) (8/7 = 1.001001..b rounds up at bit 24),
  so 448 * 2^k * fl(1 / 448) = 2^k (1 + 0.375 * 2^-23) rounds to 2^k, inv = 2^-k and every product v * inv is exact.  A zero carries the sign of its input (0x00 / 0x80).  Padding (columns cols..ldq, cache rows >= rows, scales >= rows)
  stays bit-identical to its poison.
rope_append.  q and k: two products and one addition, KAPPA 3 on |x cos| + |x' sin| (as rope_bwd_merge); v bit for bit; every cache
  element outside the appended row keeps its poison.

Families (rounded to the input type first).  diffuse: 3 N(0,1) + 0.5.  offset: row mean 64 standard deviations.  small: N(0,1) 2^-8
(var ~ eps).  special: an all-zero row, then one-hot rows whose element sits at column 0, in lane 63, in the first lane of wave 3, in
register chunk 3 and in the last column (where the width has them).  Quantisers add: peak (the row maximum alone at one of those places,
everything else at most 1/8 of it), subnormal (|t| from 2^-6 down to what rounds to zero, kept off exact midpoints) and ties
(amax = 448 * 2^k, every other value on the midpoint of two e4m3 neighbours, subnormal ones included).

Mutations are named changes to the float64 reference (MUTATIONS); the mutated reference stands in for the kernel and must exceed the
unmutated bar by MIN_RATIO on a case listed with it.  For the byte output of a quantiser, whose verdict is admissible or not, the
measure is the number of inadmissible bytes.  CAPPED lists what a bar structurally holds lower:
  gain-before-inner-cast (norm_bf16 RMS): bf16(w n) against bf16(w bf16(n)) differs by at most |w| half_ulp(n) + half_ulp(w n)
      < 3 half_ulp(w n) since |w| hb(n) <= |w n| < 2 hb(w n): one cast cannot show it at 4; it must reach 2.
  no-saturation (both quantisers): with s = amax / 448 to 2^-23, |t| <= 448 (1 + 2^-22) < 464, which rounds to 448 with or without
      the clamp: a correct scale leaves the clamp nothing to do, and a wrong one is caught as a scale.  Cap 0.
Listed for row_stats alone:
  one-pass-variance: E[x^2] - mean^2 in f32 loses 2^-24 * 4096 of var at 64 standard deviations, 1.2e-4 of rstd: 80 times the bar of
      the f32 rstd of row_stats, where it is listed, and below the 2^-9 of a bf16 y, which cannot see it.
"""
import functools
import os
import re

import numpy as np
import torch

from train_kernel_cases import BF, EPS, F32, F64, MIN_RATIO, ROOT, Case, Out, bf, f64, rng_of, rope_table  # noqa: F401 (MIN_RATIO: the tests')

NORM_EPS = float(np.float32(1e-5))
AMAX_FLOOR = float(np.float32(1e-12))
ROWS = 5
CAPPED = {("norm_bf16", "gain-before-inner-cast"): 2.0, ("quant_rows", "no-saturation"): 0.0, ("kv_quant", "no-saturation"): 0.0}


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """The constants the edges of this table stand on, read from the sources the library is built from."""
    def src(name):
        with open(os.path.join(ROOT, "aki_amd", "csrc", name)) as f:
            return f.read()

    def one(pattern, text, what):
        m = re.search(pattern, text, re.S)
        assert m, f"{what} not found"
        return int(m.group(1))
    aux, q8, dec = src("aux_kernels.hip"), src("fp8_quant.hip"), src("decode.hip")
    nb = aux[aux.index("void norm_bf16_kernel"):aux.index("void norm_f32_kernel")]
    rs = aux[aux.index("void row_stats_kernel"):aux.index("int row_stats_launch")]
    kv = dec[dec.index("void kv_cache_quant_fp8_kernel"):dec.index("int kv_cache_quant_fp8_launch")]
    K = {
        "NORM_MAXC": one(r"constexpr int MAXC = (\d+);", nb, "MAXC of norm_bf16_kernel"),
        "NORM_THREADS": one(r"threadIdx\.x \+ i \* (\d+)", nb, "the chunk stride of norm_bf16_kernel"),
        "NORM_MAX_COLS": one(r"cols % 8 \|\| cols > (\d+) \|\| ldx % 8 \|\| ldy % 8", aux, "the column limit of norm_launch"),
        "F32_THREADS": one(r"c < cols; c \+= (\d+)\)", aux[aux.index("void norm_f32_kernel"):], "the stride of norm_f32_kernel"),
        "STATS_STRIDE": one(r"c \+= (\d+) \* 8\)", rs, "the loop stride of row_stats_kernel") * 8,
        "QUANT_MAXC": one(r"constexpr int MAXC = (\d+);", q8, "MAXC of quant_rows_fp8_kernel"),
        "QUANT_THREADS": one(r"tid \+ i \* (\d+)", q8, "the chunk stride of quant_rows_fp8_kernel"),
        "QUANT_MAX_COLS": one(r"cols % 8 \|\| cols > (\d+)", q8, "the column limit of quant_rows_fp8_launch"),
        "KV_ROWS_PER_BLOCK": one(r"blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 4\)", kv, "rows per block of the KV quantiser"),
        "KV_LANES": one(r"threadIdx\.x & (\d+);", kv, "lanes per row of the KV quantiser") + 1,
        "KV_LIVE_LANES": one(r"i < (\d+);", kv, "live lanes per row of the KV quantiser"),
        "ROPE_THREADS": one(r"blockIdx\.y \* (\d+) \+ threadIdx\.x", dec[dec.index("void rope_append_kernel"):], "threads of rope_append_kernel"),
    }
    return K


def placed_columns(cols):
    """Column 0, a column of lane 63, the first of wave 3, the first of register chunk 3, the last column - those the width has."""
    out = []
    for p in (0, 63 * 8 + 3, 192 * 8, 3 * 256 * 8, cols - 1):
        if p < cols and p not in out:
            out.append(p)
    return out


# =================================================== e4m3 =============================================================================
def e4m3_rne(t):
    """float64 -> OCP e4m3fn codes, round to nearest even, the sign kept on zeros, 0x7f / 0xff above 464 (as torch's cast)."""
    t = np.asarray(t, dtype=np.float64)
    sign = np.signbit(t).astype(np.uint8) << 7
    a = np.abs(t)
    _, ex = np.frexp(np.maximum(a, 2.0 ** -6))
    q = np.ldexp(1.0, np.minimum(ex - 1, 8) - 3)            # spacing: 2^-9 below 2^-6, then 2^(e - 3)
    return _encode(np.rint(a / q) * q, a > 464.0) | sign


def _encode(v, nan):
    """v >= 0 on the e4m3 grid (or above it) -> code without sign."""
    m, ex = np.frexp(np.where(v > 0, v, 1.0))
    e = ex - 1
    normal = (((e + 7) << 3) + np.rint((m * 2.0 - 1.0) * 8.0).astype(np.int64))
    code = np.where(v >= 2.0 ** -6, normal, np.rint(v * 512.0).astype(np.int64))
    return np.where(nan | (v > 448.0), 0x7F, code).astype(np.uint8)


def e4m3_decode(code):
    code = np.asarray(code, dtype=np.uint8).astype(np.int64)
    e, m = (code >> 3) & 15, code & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.ldexp(1.0, e - 10))
    v = np.where((code & 0x7F) == 0x7F, np.nan, v)
    return np.where(code & 0x80, -v, v)


def e4m3_mutated(t, how):
    """The roundings a wrong kernel could use: 'trunc', 'away' (ties away from zero), 'flush' (subnormal results to zero)."""
    t = np.asarray(t, dtype=np.float64)
    sign = np.signbit(t).astype(np.uint8) << 7
    a = np.abs(t)
    _, ex = np.frexp(np.maximum(a, 2.0 ** -6))
    q = np.ldexp(1.0, np.minimum(ex - 1, 8) - 3)
    k = {"trunc": np.floor(a / q), "away": np.floor(a / q + 0.5), "flush": np.rint(a / q)}[how]
    v = k * q
    if how == "flush":
        v = np.where(v < 2.0 ** -6, 0.0, v)
    return _encode(v, a > 464.0) | sign


# =================================================== norms and row statistics =========================================================
NORM_BF16_COLS = (8, 64, 2040, 2048, 2056, 4096, 4104, 6152, 8192)
NORM_F32_COLS = (1, 255, 256, 257, 1000, 3072)
STATS_COLS = (8, 2040, 2048, 2056, 4104, 8192, 16392)
NORM_MODES = ("rms", "ln", "ln-nobias")
NORM_FAMILIES = ("diffuse", "offset", "small", "special")
OFFSET_SALT = 1
NORM_REJECTED =("cols-8200", "cols-12", "ldx-2060", "x-misaligned")


def _norm_cases():
    out = []
    for mode in NORM_MODES:
        for cols in NORM_BF16_COLS:
            out.append(Case("norm_bf16", f"{mode}-c{cols}", mode=mode, rows=ROWS, cols=cols, ldx=cols, ldy=cols, f32=False))
        for cols in (64, 2056, 8192):
            out.append(Case("norm_bf16", f"{mode}-c{cols}-ld", mode=mode, rows=ROWS, cols=cols, ldx=cols + 8, ldy=cols + 16, f32=False))
        for cols in NORM_F32_COLS:
            out.append(Case("norm_f32", f"{mode}-c{cols}", mode=mode, rows=ROWS, cols=cols, ldx=cols, ldy=cols, f32=True))
        for cols in (257, 1000):
            out.append(Case("norm_f32", f"{mode}-c{cols}-ld", mode=mode, rows=ROWS, cols=cols, ldx=cols + 3, ldy=cols + 5, f32=True))
    for mode in ("rms", "ln"):
        for cols in STATS_COLS:
            out.append(Case("row_stats", f"{mode}-c{cols}", mode=mode, rows=ROWS, cols=cols, ldx=cols, ldy=cols, f32=False))
        for cols in (2056, 16392):
            out.append(Case("row_stats", f"{mode}-c{cols}-ld", mode=mode, rows=ROWS, cols=cols, ldx=cols + 8, ldy=cols, f32=False))
    return tuple(out)


NORM_CASES = _norm_cases()


def chain_length(c):
    """R: the longest chain of f32 additions under a row sum of the case's kernel."""
    K = kernel_constants()
    if c.kernel == "norm_f32":
        per = -(-c.cols // K["F32_THREADS"])
    elif c.kernel == "row_stats":
        per = -(-c.cols // K["STATS_STRIDE"]) * 8
    else:
        per = K["NORM_MAXC"] * 8
    return per + 10


def _round_in(a, f32):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)) if f32 else bf(a)


def norm_inputs(c, family):
    # At 64 standard deviations a bf16 row holds about 12 distinct values: one of them within a of an inner-cast midpoint would make a
    # twelfth of the row undecided.  The salt picks draws without one; the CPU test holds every case to the 1 % cap.
    g = rng_of("fwd-norm", c.kernel, c.mode, c.cols, c.ldx, family, OFFSET_SALT if family == "offset" else 0)
    R, Cn = c.rows, c.cols
    x = 3.0 * g.standard_normal((R, Cn)) + 0.5
    if family == "offset":
        z = g.standard_normal((R, Cn))
        sd = z.std(axis=1, keepdims=True) if Cn > 1 else np.ones((R, 1))
        x = z + 64.0 * sd * np.where(g.random((R, 1)) < 0.5, -1.0, 1.0)
    if family == "small":
        x = g.standard_normal((R, Cn)) * 2.0 ** -8
    if family == "special":
        x = np.zeros((R, Cn))
        at = placed_columns(Cn) if not c.f32 else sorted({0, Cn - 1, min(Cn - 1, 3 * 256), min(Cn - 1, 192)})
        for r in range(1, R):
            x[r, at[(r - 1) % len(at)]] = (3.0, -2.5, 0.75, 7.0)[(r - 1) % 4]
    w = 1.0 + 0.2 * g.standard_normal(Cn)
    b = 0.5 * g.standard_normal(Cn)
    return dict(x=_round_in(x, c.f32), w=_round_in(w, c.f32), b=None if c.mode != "ln" else _round_in(b, c.f32), family=family)


class Either:
    """An output with up to two admissible exact values per element (the bf16 neighbours of an undecided inner cast); each is held to
    its own bar and the better one counts."""

    def __init__(self, lo, hi, undecided):
        self.alts, self.undecided = (lo, hi), undecided
        self.x, self.kind = lo.x, lo.kind

    def ratio(self, got):
        return np.minimum(self.alts[0].ratio(got), self.alts[1].ratio(got))

    def worst(self, got):
        r = self.ratio(got)
        return float(r.max()) if r.size else 0.0


def _sum_keep(c, mut):
    """Columns that enter the row sums under a mutation of the reduction."""
    K = kernel_constants()
    col = np.arange(c.cols)
    if c.kernel == "norm_f32":
        thread, it, last = col % K["F32_THREADS"], col // K["F32_THREADS"], col == c.cols - 1
    else:
        stride = K["STATS_STRIDE"] if c.kernel == "row_stats" else K["NORM_THREADS"] * 8
        thread, it, last = (col % stride) // 8, col // stride, col // 8 == (c.cols - 1) // 8
    if mut == "chunk-dropped":
        return ~last
    if mut == "chunk3-out":
        return it != 3
    if mut == "wave3-out":
        return thread < 192
    return np.ones(c.cols, dtype=bool)


def rms_two_casts(n, a, w):
    """y = bf16(w * bf16(n)) with n known to +-a: the two admissible exact values and the undecided mask."""
    lo, hi = f64(bf(n - a)), f64(bf(n + a))
    ylo, yhi = f64(bf(w * lo)), f64(bf(w * hi))
    return ylo, yhi, lo != hi, (w * lo, w * hi)


def norm_reference(c, inp, mut=None):
    """-> {'y': Out | Either} for the norm kernels, {'rstd': Out, 'mean': Out (ln)} for row_stats; 'zero_rows' where y is exact."""
    x, w = f64(inp["x"]), f64(inp["w"])
    rms = c.mode == "rms"
    b = np.zeros_like(w) if inp["b"] is None else f64(inp["b"])
    if mut == "bias-missing":
        b = 0 * b
    if mut == "bias-invented":
        b = b + 0.5
    Cn = c.cols
    n_div = c.ldx if mut == "divide-by-ldx" else Cn
    keep = _sum_keep(c, mut)
    R = chain_length(c)
    K_sum = R + 2.0
    ax = np.abs(x)
    amean = np.zeros((c.rows, 1)) if rms else ax.sum(1, keepdims=True) / Cn
    mean = np.zeros((c.rows, 1)) if rms else x[:, keep].sum(1, keepdims=True) / n_div
    d = x - mean
    var = (d * d)[:, keep].sum(1, keepdims=True) / n_div
    if mut == "one-pass-variance-f32" and not rms:
        s2 = np.float32((x * x).sum(1, keepdims=True) / Cn)
        m32 = np.float32(mean)
        var = np.maximum((s2 - m32 * m32).astype(np.float64), 0.0)
    rstd = 1.0 / (np.sqrt(var) + NORM_EPS) if mut == "eps-outside-root" else 1.0 / np.sqrt(var + NORM_EPS)
    K_var = K_sum if rms else K_sum + 2.0
    K_rstd = (K_var + 1.0) / 2.0 + 2.0
    second = rstd * (K_sum * EPS * amean) ** 2 / (2.0 * (var + NORM_EPS))
    zero_rows = np.flatnonzero((x == 0).all(1))
    if c.kernel == "row_stats":
        out = {"rstd": Out(rstd[:, 0], rstd[:, 0], K_rstd, "f32", extra=second[:, 0])}
        if not rms:
            out["mean"] = Out(mean[:, 0], amean[:, 0], K_sum, "f32")
        return out
    kind = "f32" if c.f32 else "bf16"
    n = d * rstd
    if not rms:
        y = n * w + b
        M = np.abs(w) * (ax + amean) * rstd + np.abs(b)
        return {"y": Out(y, M, K_sum + K_rstd + 4.0, kind, extra=np.abs(w * d) * second), "zero_rows": zero_rows}
    if c.f32:
        return {"y": Out(n * w, None, K_rstd + 2.0, "f32"), "zero_rows": zero_rows}
    a = (K_rstd + 1.0) * EPS * np.abs(n)
    if mut == "gain-before-inner-cast":
        y1 = f64(bf(n * w))
        return {"y": Out(y1, kind="exact"), "zero_rows": zero_rows}
    _, _, undecided, (plo, phi) = rms_two_casts(n, a, w)
    return {"y": Either(Out(plo, None, 0.0, "bf16"), Out(phi, None, 0.0, "bf16"), undecided), "zero_rows": zero_rows}


def norm_f32(c, inp):
    """The documented formulas in plain float32 torch (two-pass variance), outputs cast to the kernel's output type."""
    x, w = inp["x"].float(), inp["w"].float()
    rms = c.mode == "rms"
    mean = torch.zeros(c.rows, 1) if rms else x.mean(1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + torch.tensor(NORM_EPS, dtype=F32))
    if c.kernel == "row_stats":
        out = {"rstd": f64(rstd[:, 0])}
        if not rms:
            out["mean"] = f64(mean[:, 0])
        return out
    n = d * rstd
    if rms:
        y = w * n if c.f32 else (w * n.to(BF).float()).to(BF)
    else:
        y = n * w + (0.0 if inp["b"] is None else inp["b"].float())
        y = y if c.f32 else y.to(BF)
    return {"y": f64(y)}


def norm_torch64(c, inp):
    """torch's own float64 layer_norm / the HF RMSNorm formula without its casts: what the reference is checked against."""
    x, w = inp["x"].to(F64), inp["w"].to(F64)
    if c.mode == "rms":
        rstd = torch.rsqrt((x * x).mean(1, keepdim=True) + NORM_EPS)
        return {"y": (w * (x * rstd)).numpy(), "rstd": rstd[:, 0].numpy()}
    b = None if inp["b"] is None else inp["b"].to(F64)
    y = torch.nn.functional.layer_norm(x, (c.cols,), w, b, NORM_EPS)
    return {"y": y.numpy(), "rstd": torch.rsqrt(x.var(1, unbiased=False) + NORM_EPS).numpy(), "mean": x.mean(1).numpy()}


# =================================================== quantisers =======================================================================
QUANT_COLS = (8, 2040, 2048, 2056, 6152, 8192)
QUANT_FAMILIES = {"plain": ("diffuse", "special", "peak", "subnormal", "ties"), "rms": ("diffuse", "special", "peak", "subnormal")}
KV_SHAPES = ((1, 1, 1, 1), (3, 5, 8, 16), (4, 16, 16, 16), (7, 9, 12, 10), (2, 33, 40, 64), (4, 5, 6, 5))    # the last: one block over four slabs
KV_FAMILIES = ("diffuse", "zero", "ties")
KV_DH = 96
TIE_K = (-3, 0, 2, 5, -10)
Q_POISON, S_POISON = 0xA5, 0x5A5A5A5A


def _quant_cases():
    out = [Case("quant_rows", f"{mode}-c{cols}", mode=mode, cols=cols, ldx=cols + 8, ldq=cols + 16, delta=2.0 ** -23, srel=2.0 ** -23)
           for mode in ("plain", "rms") for cols in QUANT_COLS]
    return tuple(out)


QUANT_CASES = _quant_cases()
KV_CASES = tuple(Case("kv_quant", f"s{s}-r{r}-src{a}-dst{b}", slabs=s, rows=r, src_cap=a, dst_cap=b, mode="plain", cols=KV_DH,
                      delta=2.0 ** -24, srel=2.0 ** -24) for s, r, a, b in KV_SHAPES)


def tie_values(g, shape, k):
    """Midpoints of adjacent e4m3 values (subnormal ones included, 448 excluded as an upper neighbour's partner), times 2^k."""
    codes = g.integers(0, 0x7E, shape)                       # code and code + 1 are both finite
    mid = 0.5 * (e4m3_decode(codes) + e4m3_decode(codes + 1))
    return mid * np.where(g.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** k


def _off_midpoints(t):
    """t (already bf16 values, in units of the scale): anything on an exact e4m3 midpoint moves one bf16 step up."""
    tb = bf(t)
    on = e4m3_rne(f64(tb) * (1 - 2.0 ** -20)) != e4m3_rne(f64(tb) * (1 + 2.0 ** -20))
    bits = tb.view(torch.int16).clone()
    bits[torch.from_numpy(on)] += 1
    return f64(bits.view(BF))


def quant_inputs(c, family):
    g = rng_of("fwd-quant", c.mode, c.cols, family)
    Cn = c.cols
    at = placed_columns(Cn)
    if family == "diffuse":
        x = 3.0 * g.standard_normal((ROWS, Cn)) + 0.5
    elif family == "special":
        x = np.zeros((2, Cn))
        x[1, Cn - 1] = -2.5
    elif family == "peak":
        x = g.uniform(-1.0, 1.0, (len(at), Cn))
        for r, p in enumerate(at):
            x[r, p] = 8.0 * (-1.0) ** r
    elif family == "subnormal":
        x = np.exp2(g.uniform(-13.0, -6.01, (ROWS, Cn))) * np.where(g.random((ROWS, Cn)) < 0.5, -1.0, 1.0)
        x = _off_midpoints(x) * 2.0 ** np.array(TIE_K)[:, None]
        x[:, 0] = 448.0 * 2.0 ** np.array(TIE_K)
    else:
        x = np.stack([tie_values(g, Cn, k) for k in TIE_K])
        x[:, at[-1]] = 448.0 * 2.0 ** np.array(TIE_K)
    w = bf(1.0 + 0.2 * g.standard_normal(Cn)) if c.mode == "rms" else None
    return dict(x=bf(x), w=w, family=family)


def kv_inputs(c, family):
    g = rng_of("fwd-kv", c.slabs, c.rows, c.src_cap, c.dst_cap, family)
    shape = (c.slabs, c.src_cap, KV_DH)
    x = 3.0 * g.standard_normal(shape) + 0.5
    if family == "zero":
        flat = x.reshape(-1, KV_DH)
        flat[::3] = 0.0
        flat[1::6] = 0.0
        flat[1::6, 95] = -1.25
        flat[::6, 40] = -0.0
    if family == "ties":
        k = g.integers(-12, 9, shape[:2])
        x = tie_values(g, shape, 0) * 2.0 ** k[..., None]
        pos = g.integers(0, KV_DH, shape[:2])
        np.put_along_axis(x, pos[..., None], (448.0 * 2.0 ** k)[..., None], axis=2)
    return dict(x=bf(x), w=None, family=family)


def quant_y(c, inp):
    """The values that are quantised, [rows, cols] float64: (y_a, y_b) - equal except on undecided elements of the RMS mode."""
    if c.kernel == "kv_quant":
        x = f64(inp["x"])[:, :c.rows].reshape(-1, KV_DH)
        return x, x, np.zeros(x.shape, dtype=bool)
    x = f64(inp["x"])
    if c.mode == "plain":
        return x, x, np.zeros(x.shape, dtype=bool)
    K = kernel_constants()
    R = K["QUANT_MAXC"] * 8 + 10
    K_rstd = (R + 2.0 + 1.0) / 2.0 + 2.0
    rstd = 1.0 / np.sqrt((x * x).sum(1, keepdims=True) / c.cols + NORM_EPS)
    n = x * rstd
    ylo, yhi, und, _ = rms_two_casts(n, (K_rstd + 1.0) * EPS * np.abs(n), f64(inp["w"]))
    return ylo, yhi, und


class QuantRef:
    """The verdict on a quantiser's output.  scale [rows] f32 and bytes [rows, cols] uint8 of the device (or of a stand-in)."""

    def __init__(self, c, inp):
        self.c = c
        self.ya, self.yb, self.undecided = quant_y(c, inp)
        exact = inp["family"] == "ties"                      # amax = 448 * 2^k: the scale is 2^k and every operation exact (docstring)
        self.delta = 0.0 if exact else c.delta
        ma, mb = np.abs(self.ya), np.abs(self.yb)
        lo = np.minimum(ma, mb).max(1)                        # the smallest amax any admissible choice gives
        self.amax = []                                        # per row: every admissible amax
        for r in range(ma.shape[0]):
            cand = np.concatenate([ma[r], mb[r]])
            self.amax.append(np.unique(cand[cand >= lo[r]]))

    def scale_ratio(self, s):
        """|s - s_ref| / (srel s_ref) per row, the best admissible amax taken."""
        s = np.asarray(s, dtype=np.float64)
        out = np.empty(len(self.amax))
        for r, cand in enumerate(self.amax):
            ref = np.maximum(cand, AMAX_FLOOR) / 448.0
            out[r] = (np.abs(s[r] - ref) / (self.c.srel * ref)).min() if np.isfinite(s[r]) else np.inf
        return out

    def admissible(self, s):
        """[4, rows, cols] codes: the images of clamp(t (1 -+ delta)) for both admissible y."""
        s = np.asarray(s, dtype=np.float64)[:, None]
        out = []
        for y in (self.ya, self.yb):
            t = y / s
            for f in (1.0 - self.delta, 1.0 + self.delta):
                out.append(e4m3_rne(np.clip(t * f, -448.0, 448.0)))
        return np.stack(out)

    def bad_bytes(self, s, q):
        """Mask of the bytes outside the admissible set."""
        return ~(self.admissible(s) == np.asarray(q, dtype=np.uint8)[None]).any(0)

    def choices(self, s):
        """Number of distinct admissible bytes per element."""
        a = np.sort(self.admissible(s), axis=0)
        return 1 + (a[1:] != a[:-1]).sum(0)

    def byte_ratio(self, s, q):
        """|decode(q) - t| over half the e4m3 spacing at t plus delta |t|: the continuous figure that is recorded (<= 1)."""
        s = np.asarray(s, dtype=np.float64)[:, None]
        v = e4m3_decode(q)
        best = np.full(self.ya.shape, np.inf)
        for y in (self.ya, self.yb):
            t = np.clip(y / s, -448.0, 448.0)
            _, ex = np.frexp(np.maximum(np.abs(t), 2.0 ** -6))
            bar = 0.5 * np.ldexp(1.0, np.minimum(ex - 1, 8) - 3) + self.delta * np.abs(t)
            best = np.minimum(best, np.where(np.isfinite(v), np.abs(v - t) / bar, np.inf))
        return best


def quant_stand_in(c, inp, mut=None, f32=False):
    """(scale f32 [rows], bytes uint8 [rows, cols]) as a kernel would leave them: the float64 rule (f32 = False), the kernel's own
    float32 operations in torch (f32 = True), or a mutated float64 rule."""
    ya, _, _ = quant_y(c, inp)
    kv = c.kernel == "kv_quant"
    if f32:
        y = torch.from_numpy(ya).float()
        amax = torch.clamp(y.abs().amax(1), min=torch.tensor(AMAX_FLOOR, dtype=F32))
        if kv:
            s = amax / 448.0
            t = y / s[:, None]
        else:
            s = amax * torch.tensor(1.0 / 448.0, dtype=F32)
            t = y * (1.0 / s)[:, None]
        q = torch.clamp(t, -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        return s.numpy(), q.numpy()
    col = np.arange(c.cols)
    keep = np.ones(c.cols, dtype=bool)
    if mut == "amax-without-wave3":
        keep = (col // 8) % 256 < 192
    if mut == "amax-without-chunk3":
        keep = col // 2048 != 3
    if mut == "amax-without-last-lane":
        keep = col // 8 != (c.cols - 1) // 8
    amax = np.abs(ya[:, keep]).max(1) if keep.any() else np.zeros(ya.shape[0])
    s = np.maximum(amax, AMAX_FLOOR) / (480.0 if mut == "scale-over-480" else 448.0)
    if mut == "scale-of-next-row":
        s = np.concatenate([np.roll(s[i:i + 16], -1) for i in range(0, len(s), 16)]) if kv else np.roll(s, -1)
    s = np.float32(s).astype(np.float64)
    t = ya / s[:, None]
    if mut != "no-saturation":
        t = np.clip(t, -448.0, 448.0)
    how = {"truncation": "trunc", "ties-away": "away", "subnormals-flushed": "flush"}.get(mut)
    q = e4m3_rne(t) if how is None else e4m3_mutated(t, how)
    if mut == "pair-swapped":
        q = q.reshape(q.shape[0], -1, 2)[:, :, ::-1].reshape(q.shape)
    return s, q


# =================================================== rope_append ======================================================================
ROPE_SHAPES = ((1, 1, 96), (3, 5, 96), (2, 3, 64), (2, 8, 128))
ROPE_CAP = 7
ROPE_TABLE_ROWS = ROPE_CAP + 9
KAPPA_ROPE = 3.0
ROPE_CASES = tuple(Case("rope_append", f"b{B}-h{H}-d{Dh}-{'f32' if f32 else 'bf16'}-at-{at}", B=B, H=H, Dh=Dh, f32=f32, at=at, cap=ROPE_CAP)
                   for B, H, Dh in ROPE_SHAPES for f32 in (False, True) for at in ("0", "last", "mid"))


def rope_inputs(c):
    g = rng_of("fwd-rope", c.B, c.H, c.Dh, c.f32, c.at)
    cos, sin = rope_table(ROPE_TABLE_ROWS, c.Dh, "synthetic")
    qkv = _round_in(g.standard_normal((c.B, 3 * c.H * c.Dh)), c.f32)
    cl = {"0": np.zeros(c.B), "last": np.full(c.B, c.cap - 1), "mid": (np.arange(c.B) * 2 + 2) % (c.cap - 1)}[c.at].astype(np.int32)
    pos = ((cl + 3 + 4 * np.arange(c.B)) % ROPE_TABLE_ROWS).astype(np.int32)      # never cache_len, up to the last row of the table
    pos[0] = ROPE_TABLE_ROWS - 1 if cl[0] != ROPE_TABLE_ROWS - 1 else pos[0]
    return dict(qkv=qkv, cos=torch.from_numpy(cos), sin=torch.from_numpy(sin), pos=torch.from_numpy(pos), cache_len=torch.from_numpy(cl))


def rope_reference(c, inp, mut=None):
    """-> {'q': Out [B, H, Dh], 'k': Out [B, H, Dh] (the appended row), 'v': exact [B, H, Dh]}"""
    B, H, Dh = c.B, c.H, c.Dh
    half = Dh // 2
    row = f64(inp["qkv"])
    pos = (inp["cache_len"] if mut == "cos-row-at-cache_len" else inp["pos"]).numpy().astype(np.int64)
    cs, sn = f64(inp["cos"])[pos][:, None], f64(inp["sin"])[pos][:, None]        # [B, 1, Dh]
    q = row[:, :H * Dh].reshape(B, H, Dh)
    k = row[:, H * Dh:2 * H * Dh].reshape(B, H, Dh)
    if mut == "k-head-stride":
        k = row[:, Dh:Dh + H * Dh].reshape(B, H, Dh)
    v = row[:, 2 * H * Dh:].reshape(B, H, Dh)
    out = {}
    for name, t in (("q", q), ("k", k)):
        rot = np.concatenate([-t[..., half:], t[..., :half]], -1)
        if mut == "rotated-half-sign":
            rot = -rot
        a, b = t * cs, rot * sn
        out[name] = Out(a + b, np.abs(a) + np.abs(b), KAPPA_ROPE, "f32" if c.f32 else "bf16")
    out["v"] = Out(v, kind="exact")
    return out


def rope_f32(c, inp):
    B, H, Dh = c.B, c.H, c.Dh
    half = Dh // 2
    row = inp["qkv"].float()
    pos = inp["pos"].long()
    cs, sn = inp["cos"][pos][:, None], inp["sin"][pos][:, None]
    out = {}
    for name, lo in (("q", 0), ("k", H * Dh)):
        t = row[:, lo:lo + H * Dh].reshape(B, H, Dh)
        y = t * cs + torch.cat([-t[..., half:], t[..., :half]], -1) * sn
        out[name] = f64(y if c.f32 else y.to(BF))
    out["v"] = f64(row[:, 2 * H * Dh:].reshape(B, H, Dh))
    return out


# =================================================== mutations ========================================================================
# kernel -> {mutation: ids of the cases on which it must be visible (over the case's families)}
MUTATIONS = {
    "norm_bf16": {
        "chunk-dropped": ("rms-c64", "ln-c64", "ln-nobias-c4104"), "chunk3-out": ("rms-c8192", "ln-c6152", "rms-c6152"),
        "wave3-out": ("rms-c2048", "ln-c4104"), "eps-outside-root": ("rms-c2056", "ln-c64"), "divide-by-ldx": ("rms-c64-ld", "ln-c64-ld"),
        "gain-before-inner-cast": ("rms-c2048",), "bias-missing": ("ln-c8", "ln-c8192"), "bias-invented": ("ln-nobias-c8", "ln-nobias-c8192-ld"),
    },
    "norm_f32": {
        "chunk-dropped": ("rms-c1", "ln-c257"), "chunk3-out": ("rms-c1000", "ln-c3072"), "wave3-out": ("rms-c256", "ln-c3072"),
        "eps-outside-root": ("rms-c255", "ln-c1000"), "divide-by-ldx": ("rms-c257-ld", "ln-c257-ld"),
        "bias-missing": ("ln-c1", "ln-c3072"), "bias-invented": ("ln-nobias-c257",),
    },
    "row_stats": {
        "chunk-dropped": ("rms-c8", "ln-c16392", "rms-c2056"), "chunk3-out": ("rms-c8192", "ln-c16392"), "wave3-out": ("rms-c2048", "ln-c4104"),
        "one-pass-variance-f32": ("ln-c2048", "ln-c16392"), "eps-outside-root": ("rms-c2040", "ln-c8"), "divide-by-ldx": ("rms-c2056-ld", "ln-c16392-ld"),
    },
    "quant_rows": {
        "amax-without-wave3": ("plain-c2048", "rms-c6152"), "amax-without-chunk3": ("plain-c8192", "rms-c6152"),
        "amax-without-last-lane": ("plain-c8", "rms-c2056", "plain-c2040"), "truncation": ("plain-c2056", "rms-c8192"),
        "ties-away": ("plain-c8", "plain-c2048"), "no-saturation": ("plain-c2048",), "subnormals-flushed": ("plain-c2040", "rms-c2048"),
        "scale-over-480": ("plain-c8", "rms-c8192"), "pair-swapped": ("plain-c8", "rms-c2056"), "scale-of-next-row": ("plain-c2048", "rms-c8"),
    },
    "kv_quant": {
        "amax-without-last-lane": ("s3-r5-src8-dst16",), "truncation": ("s1-r1-src1-dst1", "s2-r33-src40-dst64"),
        "ties-away": ("s3-r5-src8-dst16", "s2-r33-src40-dst64"), "no-saturation": ("s4-r16-src16-dst16",),
        "subnormals-flushed": ("s7-r9-src12-dst10",), "scale-over-480": ("s1-r1-src1-dst1",), "pair-swapped": ("s7-r9-src12-dst10",),
        "scale-of-next-row": ("s3-r5-src8-dst16", "s2-r33-src40-dst64"),
    },
    "rope_append": {
        "rotated-half-sign": ("b1-h1-d96-bf16-at-0", "b2-h8-d128-f32-at-mid"), "cos-row-at-cache_len": ("b3-h5-d96-bf16-at-last", "b2-h3-d64-f32-at-0"),
        "k-head-stride": ("b3-h5-d96-bf16-at-mid", "b2-h3-d64-f32-at-last"),
    },
}

CASES = {"norm_bf16": tuple(c for c in NORM_CASES if c.kernel == "norm_bf16"), "norm_f32": tuple(c for c in NORM_CASES if c.kernel == "norm_f32"),
         "row_stats": tuple(c for c in NORM_CASES if c.kernel == "row_stats"), "quant_rows": QUANT_CASES, "kv_quant": KV_CASES,
         "rope_append": ROPE_CASES}
CASE_BY_ID = {(k, c.id): c for k, cs in CASES.items() for c in cs}


def families_of(c):
    if c.kernel in ("norm_bf16", "norm_f32", "row_stats"):
        return NORM_FAMILIES
    if c.kernel == "quant_rows":
        return QUANT_FAMILIES[c.mode]
    return KV_FAMILIES if c.kernel == "kv_quant" else (None,)

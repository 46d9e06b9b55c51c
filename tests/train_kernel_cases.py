"""Case tables, input families, float64 references, componentwise bars and reference mutations of the row and elementwise kernels of
the training step (aki_amd/csrc/train_kernels.hip: norm_bwd_kernel<RMS|LN> + fold_partials_kernel, colsum_part_kernel,
swiglu_fwd/bwd_kernel, gelu_kernel<0|1>, rope_bwd_merge_kernel, ce_count_kernel + ce_fwd_bwd_kernel<ROWS>, grad_sqnorm_kernel<G32> +
fold_scalar_kernel, adamw_kernel<G32>, adamw_t_kernel<G32>).

numpy and CPU torch only.  tests/test_train_kernel_cases_cpu.py checks the table itself - every reference against float64 autograd /
torch.optim.AdamW, every structural edge reached (from the constants parsed out of train_kernels.hip), every mutation visible, a plain
float32 implementation inside the bar - and tests/test_train_kernels_gpu.py runs every case on the device.

The bar.  Every output element is a sum of terms x = sum_i t_i in the float64 reference and is held to

    tol(x) = half_ulp(|x| + a) + a + floor,      a = KAPPA * 2^-24 * M(x),      M(x) = sum_i |t_i|  (from the float64 reference)

  half_ulp  the ONE round-to-nearest-even cast of the output: 2^-8 hb for bf16 (8 significant bits), 2^-24 hb for f32, with
            hb(y) = 2^floor(log2 y) <= y the binade of the largest value the pre-cast result may have.  It lies in (2^-9 |x|, 2^-8 |x|]:
            x = 1 + 2^-8 sits midway between the bf16 neighbours 1 and 1 + 2^-7, so ANY correct cast is off by 2^-8 = 0.996 * 2^-8 |x|
            there, and a bar of 2^-9 |x| (unit roundoff taken as 2^-9) cannot be met by exact arithmetic followed by the cast - the CPU
            test shows this on the cast of the float64 reference itself.  Half an ulp of the binade is the smallest bar one cast meets.
  a         the f32 arithmetic before the cast, to first order, in units of eps = 2^-24 (one f32 operation, round to nearest).
            Documented accuracies (HIP math API, AMD GCN3/CDNA ISA): rsqrtf 1 ulp = 2 eps, erff 4 ulp = 8 eps, sqrtf and / correctly
            rounded (counted 2 eps), __expf(a) = v_exp_f32(a * log2e): 1 ulp + the multiply's |a| log2e eps in the exponent, i.e.
            (2 + |a|) eps relative; __logf 2 ulp = 4 eps.
  floor     one minimum normal of the output type (2^-126 for both): a flushed denormal is not a failure.
Nothing here is tuned on a kernel's output; the CPU test proves the bars reachable with a plain float32 torch implementation.

KAPPA, kernel by kernel (R = the longest chain of f32 additions on an element's path).
  norm_bwd.  Row sums: a thread adds <= 16 values (MAXC * 8), the wave 6, the workgroup 4: R_row = 26, + 2 for the product and the
      division by cols: 28.  mean: 28 on mean|x|.  d = x - mean: 1.  var = mean(d^2): the error of mean enters at second order
      (sum d = 0), 28 + 2.  rstd = rsqrt(var + eps): (30 + 1) / 2 + 2 = 18.  xhat = d rstd: 28 (mean) + 1 + 18 + 1 = 48 on
      A = (|x| + mean|x|) rstd  (RMS: |x| rstd).  dxhat = dy w: 1.  c1 = mean(dxhat xhat): 28 + 1 + 48 = 77 on C1 = mean(|dxhat| A);
      c2: 29 on C2 = mean|dxhat|.  dx = rstd (dxhat - c2 - xhat c1) + dres: the worst term is xhat c1, 48 + 77 + 1, then two
      subtractions, rstd (18 + 1) and the residual add: 147.  KAPPA_dx = 160 on M = rstd (|dxhat| + C2 + A C1) + |dres|.
      dw = sum_r dy xhat: 48 + 1 per term, <= ceil(rows / 512) additions in the workgroup's registers (3 at 1025 rows), the fold's
      16 + 1 + 16, the optional accumulate: 86.  KAPPA_dw = 96 on M = sum_r |dy| A (+ |dw0| when accumulating: the old bf16 value is
      read exactly, added in f32 and the sum is cast once).  db = sum_r dy: 3 + 33 + 1: KAPPA_db = 40 on sum_r |dy|.
  colsum.  <= 2 rows per lane below 4096 rows, 32 lanes through LDS, the fold's 33, accumulate: KAPPA = 72 on sum_r |x| (+ |out0|).
  swiglu.  s = 1 / (1 + __expf(-g)): (2 + |g|) + 1 + 2 = 5 + |g|.  a = u g s: KAPPA = 8 + |g|.  du = da g s: the same.
      dg = da u s (1 + g (1 - s)) = da u s + da u s g - da u s g s: three terms, M = |da u s| (1 + |g| + |g| s) (the cancellation of
      1 - s for large g is in M), each carrying s twice at most: KAPPA = 16 + 2 |g|.  |g| is capped at 128: beyond +-88.7 the
      exponential saturates and the result is exact up to the products.
  gelu.  y = 0.5 x + 0.5 x erf(x / sqrt 2): erff 8, its argument 1, the add 1, two products: KAPPA = 16 on M = 0.5 |x| (1 + |erf|).
      dx = dy (cdf + x pdf), pdf = c __expf(-x^2 / 2): KAPPA = 16 + x^2 / 2 (capped at 128) on M = |dy| (0.5 (1 + |erf|) + |x| pdf).
      On the negative tail 1 + erf cancels and M says so: the bar there is KAPPA eps |x|, not a share of the tiny result.
  rope_bwd_merge.  Two products and one addition: KAPPA = 3 on |y0 cos| + |y1 sin|.  The dv part is a copy: bit for bit.
  cross-entropy.  Every term exp(l_i - gm) is reached through <= 3 rescalings whose arguments add up to l_i - gm:
      (6 + 2 |l_i - gm|) eps each; <= 3 * 2 + 6 + 4 + 4 additions: the row sum st is off by (20 + 6 + 2 Q) eps relative,
      Q = sum_i p_i |l_i - gm|.  lse = gm + __logf(st): 4 |log st| + |lse|.  loss = lse - l_t (f32): KAPPA_loss = 32 on
      M_loss = 1 + Q + |gm| + |log st| + |lse| + |l_t|.  p = __expf(l - lse): (2 + 2 |l - lse|) eps + the error of lse;
      grad = (p - [target]) k, k = gscale / n_valid (3 more): KAPPA_grad = 32 on M = k (p (1 + |l - lse| + M_loss) + [target]) -
      "p + 1" on the target column.  Mean loss = sum(loss_rows) / n_valid in f32: the rows' own bars / n + (rows + 2) eps mean|loss|.
      n_valid is an integer and exact; ignored rows give exactly 0 loss and exactly 0 gradients; columns V..ld are never touched.
  grad_sqnorm.  <= 2 chunks per thread at the capped grid: 16 squares and 16 additions, wave 6, workgroup 4, fold_scalar 4 + 10,
      accumulate 1: KAPPA = 64 on sum g^2 (+ |out0|), f32 output.
  adamw.  clip = min(1, max_norm / (sqrt(sq) gscale + 1e-6)): 2 + 1 + 1 + 2; gs = gscale clip, g' = g gs: 8 eps relative.
      m = b1 m0 + (1 - b1) g' (1 - b1 is exact): KAPPA_m = 10 on |b1 m0| + |(1 - b1) g'|.  v = b2 v0 + (1 - b2) g'^2: KAPPA_v = 20 on v.
      U = lr (m / bc1) / (sqrt(v / bc2) + eps): m's error is 10 eps M_m / |m|, bc = 1 - powf(b, step) (4 ulp on a value <= 1: 8),
      sqrt halves v's (20 + 8 + 2) / 2 + 2, the add, the division and lr: KAPPA_p = 48 on M_p = |p0 (1 - lr wd)| + |U| M_m / |m|.
      p, m, v are f32 outputs.  w16 = bf16(p of the device), bit for bit.  The hyper-parameters are the f32 values the ABI receives.
  adamw_step_t.  p, m, v, w16 bit for bit those of adamw_step; wT = w16^T with zero padding, bit for bit.

Input families (everything rounded to the kernel's input type first).
  norm      diffuse: N(0, 1).  offset (LN): row mean 64 times the row's standard deviation (the two-pass variance).  small: x scaled by
            2^-8 (var ~ eps) with one sign per column, dy with one sign per column and w > 0: dy w and dy xhat keep their sign down a
            column, dw and db do not cancel and one lost row is a fixed share of the element.
  colsum    one sign per column / mixed signs.
  ce        diffuse: 3 N(0, 1).  peaked: the target (even rows) or a non-target column (odd rows) 80 above N(0, 1).  shifted: diffuse
            + 200 (exp overflows f32 without the max subtraction).
  swiglu / gelu   every finite bf16 value, against partners 1, -1.5 and one N(0, 1) draw.

Mutations are named changes to the float64 reference (MUTATIONS); a mutated reference stands in for the kernel and must exceed the
unmutated bar by MIN_RATIO on one of the cases listed with it.  CAPPED lists those the bar itself holds lower, with the derivation:
  adamw "clip without 1e-6": g' moves by 1e-6 / (norm + 1e-6) relative, and clipping is active only for norm >= max_norm = 1 (the 'barely' cases sit at 1.0625), so the
      relative change is <= 1e-6 = 16.8 eps; on v = (1 - b2) g'^2 (v0 = 0) that is 33.6 eps against a bar of (0.5..1 + 20) eps: <= 1.64.
"""
import math
import os
import re
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
FLOOR = 2.0 ** -126                       # minimum normal of bf16 and of f32
BF16_MAX = 3.3895313892515355e38
MIN_RATIO = 4.0
CAPPED = {("adamw", "clip-without-1e-6"): 1.2}
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def kernel_constants():
    """MAXC, NORM_BWD_GROUPS, FOLD_COLS, SQNORM_GROUPS and the grid cap of ew_grid as train_kernels.hip is compiled: a changed
    constant moves an edge, and the CPU test then fails the table instead of silently testing beside it."""
    with open(os.path.join(ROOT, "aki_amd", "csrc", "train_kernels.hip")) as f:
        src = f.read()
    out = {}
    for name in ("MAXC", "NORM_BWD_GROUPS", "FOLD_COLS", "SQNORM_GROUPS"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, f"{name} not found in train_kernels.hip"
        out[name] = int(m.group(1))
    m = re.search(r"static inline int ew_grid\(size_t work_items\)\s*\{[^}]*?g\s*>\s*(\d+)\s*\?\s*(\d+)", src)
    assert m and m.group(1) == m.group(2), "the grid cap of ew_grid not found in train_kernels.hip"
    out["EW_GRID"] = int(m.group(1))
    return out


# ---- small helpers -------------------------------------------------------------------------------------------------------------------
def rng_of(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def bf(a):
    """float array -> bf16 torch tensor (round to nearest even)."""
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(BF)


def f64(t):
    return t.to(F64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def all_finite_bf16():
    """Every finite bf16 value (65280 of them, both zeros included) as a bf16 tensor."""
    bits = np.arange(65536, dtype=np.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80].astype(np.uint16).view(np.int16)
    return torch.from_numpy(bits.copy()).view(BF)


def hb(y):
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(y > 0, 2.0 ** np.floor(np.log2(np.where(y > 0, y, 1.0))), 0.0)


class Out:
    """One output: x (float64 reference), M (sum of |terms|), kappa (scalar or per element), kind 'bf16' | 'f32' | 'exact'.
    ok: elements the header specifies (finite results); the rest is not compared."""

    def __init__(self, x, M=None, kappa=0.0, kind="bf16", extra=0.0):
        self.x = np.asarray(x, dtype=np.float64)
        self.M = np.abs(self.x) if M is None else np.asarray(M, dtype=np.float64)
        self.kappa, self.kind, self.extra = kappa, kind, extra
        self.ok = np.isfinite(self.x) & (np.abs(self.x) <= 0.997 * BF16_MAX if kind == "bf16" else np.isfinite(self.x))

    def tol(self):
        if self.kind == "exact":
            return np.zeros_like(self.x)
        with np.errstate(invalid="ignore", over="ignore"):
            a = self.kappa * EPS * self.M + self.extra
            return (2.0 ** -8 if self.kind == "bf16" else EPS) * hb(np.abs(self.x) + a) + a + FLOOR

    def ratio(self, got):
        """err / tol per element (0 where err is 0, inf where got is not finite), over the specified elements."""
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(got - self.x)
            tol = self.tol()
            r = np.where(err > 0, err / np.where(tol > 0, tol, 1e-300), 0.0)
        r = np.where(np.isfinite(got), r, np.inf)
        return np.where(self.ok, r, 0.0)

    def worst(self, got):
        r = self.ratio(got)
        return float(r.max()) if r.size else 0.0


class Case:
    def __init__(self, kernel, id, **kw):
        self.kernel, self.id = kernel, id
        self.__dict__.update(kw)

    def __repr__(self):
        return f"{self.kernel}:{self.id}"


def pitch(cols):
    """A row pitch above the width that keeps the 16-byte alignment of a column slice."""
    return cols + 24


# =========================================================== norm_bwd =================================================================
NORM_EPS = 1e-5
NORM_COLS = (8, 1152, 2048, 2056, 3072, 4096)
NORM_ROWS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 511, 512, 513, 1025)
NORM_REFUSED_COLS = (4104, 12)
KAPPA_NORM = {"dx": 160.0, "dw": 96.0, "db": 40.0}


def norm_families(rms):
    return ("diffuse", "small") if rms else ("diffuse", "offset", "small")


def _norm_cases():
    out = []
    for rms in (True, False):
        tag = "rms" if rms else "ln"
        for cols in NORM_COLS:
            for rows in (NORM_ROWS if cols in (8, 2056) else (1, 33, 513)):
                out.append(Case("norm", f"{tag}-r{rows}-c{cols}", rms=rms, rows=rows, cols=cols, accumulate=False))
        for rows, cols in ((33, 8), (513, 2056)):
            out.append(Case("norm", f"{tag}-r{rows}-c{cols}-acc", rms=rms, rows=rows, cols=cols, accumulate=True))
    return tuple(out)


NORM_CASES = _norm_cases()


def norm_inputs(c, family, with_dres):
    g = rng_of("norm", c.rows, c.cols, c.rms, family)
    R, Cn = c.rows, c.cols
    x = g.standard_normal((R, Cn))
    dy = g.standard_normal((R, Cn))
    w = 1.0 + 0.2 * g.standard_normal(Cn)
    if family == "offset":
        x = x + 64.0 * x.std(axis=1, keepdims=True) * np.where(g.random((R, 1)) < 0.5, -1.0, 1.0)
    if family == "small":
        sx, sy = (np.where(g.random(Cn) < 0.5, -1.0, 1.0) for _ in range(2))
        x = np.abs(x) * sx * 2.0 ** -8
        dy = np.abs(dy) * sy
        w = np.abs(w) + 0.05
    inp = NS(x=bf(x), dy=bf(dy), w=bf(w), dres=bf(g.standard_normal((R, Cn))) if with_dres else None, dw0=None, db0=None)
    if c.accumulate:
        inp.dw0, inp.db0 = bf(3.0 * g.standard_normal(Cn)), bf(3.0 * g.standard_normal(Cn))
    return inp


def fold_partial_rows(rows, G, k, block=1):
    """Rows whose sum is partial k of G (norm: row r belongs to workgroup r % G; colsum: 32-row blocks, block b to b % G)."""
    r = np.arange(rows)
    return ((r // block) % G) == k


def norm_reference(c, inp, mut=None):
    K = kernel_constants()
    x, dy, w = f64(inp.x), f64(inp.dy), f64(inp.w)
    R, Cn = x.shape
    n = Cn + 1 if mut == "mean-over-cols+1" else Cn
    ax = np.abs(x)
    mean = np.zeros((R, 1)) if c.rms else x.sum(1, keepdims=True) / n
    amean = np.zeros((R, 1)) if c.rms else ax.sum(1, keepdims=True) / n
    d = x - mean
    var = (d * d).sum(1, keepdims=True) / n
    rstd = 1.0 / np.sqrt(var + (0.0 if mut == "eps-omitted" else NORM_EPS))
    xh, A = d * rstd, (ax + amean) * rstd
    dxh = dy * w
    c1, C1 = (dxh * xh).sum(1, keepdims=True) / n, (np.abs(dxh) * A).sum(1, keepdims=True) / n
    c2 = np.zeros((R, 1)) if c.rms else dxh.sum(1, keepdims=True) / n
    C2 = np.zeros((R, 1)) if c.rms else np.abs(dxh).sum(1, keepdims=True) / n
    if mut == "c1-dropped":
        c1 = 0 * c1
    if mut == "c2-dropped":
        c2 = 0 * c2
    dres = np.zeros_like(x) if inp.dres is None else f64(inp.dres)
    dx = rstd * (dxh - c2 - xh * c1) + (0 if mut == "dres-not-added" else dres)
    Mdx = rstd * (np.abs(dxh) + C2 + A * C1) + np.abs(dres)
    keep = np.ones(R, dtype=bool)
    G = min(R, K["NORM_BWD_GROUPS"])
    if mut == "dw-misses-last-row":
        keep[R - 1] = False
    if mut == "dw-misses-row-512" and R > 512:
        keep[512] = False
    if mut in ("fold-partial-16-dropped", "fold-partial-32-dropped", "fold-partial-last-dropped"):
        k = {"fold-partial-16-dropped": 16, "fold-partial-32-dropped": 32}.get(mut, G - 1)
        if k < G:
            keep &= ~fold_partial_rows(R, G, k)
    xh_dw = f64(bf(xh)) if mut == "xhat-bf16-before-dw" else xh
    dw = (dy * xh_dw)[keep].sum(0)
    Mdw = (np.abs(dy) * A).sum(0)
    db, Mdb = dy[keep].sum(0), np.abs(dy).sum(0)
    if mut == "dw-cols-from-2048-zero":
        dw[2048:] = 0.0
    if mut == "db-equals-dw":
        db = dw.copy()
    if c.accumulate:
        dw0, db0 = f64(inp.dw0), f64(inp.db0)
        if mut != "accumulate-ignored":
            dw, db = dw + dw0, db + db0
        Mdw, Mdb = Mdw + np.abs(dw0), Mdb + np.abs(db0)
    out = {"dx": Out(dx, Mdx, KAPPA_NORM["dx"]), "dw": Out(dw, Mdw, KAPPA_NORM["dw"])}
    if not c.rms:
        out["db"] = Out(db, Mdb, KAPPA_NORM["db"])
    return out


def norm_f32(c, inp):
    """The header's formula in plain float32 torch, outputs cast to bf16."""
    x, dy, w = inp.x.float(), inp.dy.float(), inp.w.float()
    mean = torch.zeros(x.shape[0], 1) if c.rms else x.mean(1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + NORM_EPS)
    xh, dxh = d * rstd, dy * w
    c1 = (dxh * xh).mean(1, keepdim=True)
    c2 = torch.zeros_like(c1) if c.rms else dxh.mean(1, keepdim=True)
    dx = rstd * (dxh - c2 - xh * c1)
    if inp.dres is not None:
        dx = dx + inp.dres.float()
    dw, db = (dy * xh).sum(0), dy.sum(0)
    if c.accumulate:
        dw, db = dw + inp.dw0.float(), db + inp.db0.float()
    out = {"dx": f64(dx.to(BF)), "dw": f64(dw.to(BF))}
    if not c.rms:
        out["db"] = f64(db.to(BF))
    return out


def norm_autograd(c, inp):
    x = inp.x.to(F64).requires_grad_()
    w = inp.w.to(F64).requires_grad_()
    b = torch.zeros_like(w).requires_grad_()
    if c.rms:
        y = x * torch.rsqrt((x * x).mean(1, keepdim=True) + NORM_EPS) * w
    else:
        y = torch.nn.functional.layer_norm(x, (x.shape[1],), w, b, NORM_EPS)
    (y * inp.dy.to(F64)).sum().backward()
    dx = x.grad if inp.dres is None else x.grad + inp.dres.to(F64)
    out = {"dx": dx.numpy(), "dw": w.grad.numpy()}
    if not c.rms:
        out["db"] = b.grad.numpy()
    if c.accumulate:
        out["dw"] = out["dw"] + f64(inp.dw0)
        if not c.rms:
            out["db"] = out["db"] + f64(inp.db0)
    return out


# ============================================================ colsum ==================================================================
COLSUM_ROWS = (1, 31, 32, 33, 2048, 2049, 2081)
COLSUM_COLS = (8, 24, 64, 72, 1152)
COLSUM_FAMILIES = ("one-sign", "mixed")
KAPPA_COLSUM = 72.0


def _colsum_cases():
    out = [Case("colsum", f"r{r}-c{cn}", rows=r, cols=cn, ld=cn, accumulate=False) for r in COLSUM_ROWS for cn in COLSUM_COLS]
    out.append(Case("colsum", "r2081-c72-pitch", rows=2081, cols=72, ld=pitch(72), accumulate=False))
    out.append(Case("colsum", "r33-c24-acc", rows=33, cols=24, ld=24, accumulate=True))
    out.append(Case("colsum", "r2049-c1152-acc-pitch", rows=2049, cols=1152, ld=pitch(1152), accumulate=True))
    return tuple(out)


COLSUM_CASES = _colsum_cases()


def colsum_G(rows):
    return min((rows + 31) // 32, 64)


def colsum_inputs(c, family):
    g = rng_of("colsum", c.rows, c.cols, family)
    x = g.standard_normal((c.rows, c.cols))
    if family == "one-sign":
        x = np.abs(x) * np.where(g.random(c.cols) < 0.5, -1.0, 1.0)
    return NS(x=bf(x), out0=bf(3.0 * g.standard_normal(c.cols)) if c.accumulate else None)


def colsum_reference(c, inp, mut=None):
    x = f64(inp.x)
    keep = np.ones(c.rows, dtype=bool)
    G = colsum_G(c.rows)
    if mut in ("fold-partial-16-dropped", "fold-partial-32-dropped", "fold-partial-last-dropped"):
        k = {"fold-partial-16-dropped": 16, "fold-partial-32-dropped": 32}.get(mut, G - 1)
        if k < G:
            keep &= ~fold_partial_rows(c.rows, G, k, 32)
    s, M = x[keep].sum(0), np.abs(x).sum(0)
    if c.accumulate:
        if mut != "accumulate-ignored":
            s = s + f64(inp.out0)
        M = M + np.abs(f64(inp.out0))
    return {"out": Out(s, M, KAPPA_COLSUM)}


def colsum_f32(c, inp):
    s = inp.x.float().sum(0)
    if c.accumulate:
        s = s + inp.out0.float()
    return {"out": f64(s.to(BF))}


# ====================================================== swiglu / gelu =================================================================
PARTNERS = (1.0, -1.5, "random")
SWIGLU_SHAPES = ((1, 8), (3, 24), (257, 40))


def _expit(g):
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-np.abs(g))
        return np.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def exhaustive_inputs(kernel, partner):
    """Every finite bf16 value as g (or x), padded to a multiple of 8 with zeros, against the partner (u, da / dy)."""
    v = all_finite_bf16()
    n = (v.numel() + 7) // 8 * 8
    val = torch.zeros(n, dtype=BF)
    val[:v.numel()] = v
    g = rng_of(kernel, "partner", partner)

    def other(k):
        return bf(g.standard_normal(n)) if partner == "random" else torch.full((n,), float(partner) if k == 0 else (-1.5 if partner == 1.0 else 1.0), dtype=BF)
    return NS(val=val, a=other(0), b=other(1))


def swiglu_reference(g, u, da=None, mut=None):
    """g, u (, da) float64 arrays of one shape.  Forward: {'a'}; backward: {'dg', 'du'}."""
    if mut == "halves-swapped":
        g, u = u, g
    s = _expit(g)
    ag = np.minimum(np.abs(g), 128.0)
    with np.errstate(over="ignore", invalid="ignore"):
        if da is None:
            return {"a": Out(u * (g * s), None, 8.0 + ag)}
        du = da * (g * s)
        t = da * u * s
        one_minus = _expit(-g)
        dg = t if mut == "silu-without-g(1-s)" else t + t * (g * one_minus)
        Mdg = np.abs(t) * (1.0 + np.abs(g) * (1.0 + s))
        Mdg = np.where(np.isfinite(Mdg), Mdg, np.abs(dg))
    if mut == "halves-swapped":
        dg, du = du, dg
        return {"dg": Out(dg, None, 8.0 + ag), "du": Out(du, Mdg, 16.0 + 2 * ag)}
    return {"dg": Out(dg, Mdg, 16.0 + 2 * ag), "du": Out(du, None, 8.0 + ag)}


def _sigmoid32(g):
    e = torch.exp(-g.abs())
    return torch.where(g >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def swiglu_f32(g, u, da=None):
    g, u = g.float(), u.float()
    s = _sigmoid32(g)
    if da is None:
        return {"a": f64((u * (g * s)).to(BF))}
    da = da.float()
    return {"dg": f64((da * u * s * (1.0 + g * (1.0 - s))).to(BF)), "du": f64((da * (g * s)).to(BF))}


def swiglu_autograd(g, u, da):
    g, u = (torch.from_numpy(t).clone().requires_grad_() for t in (g, u))
    a = u * torch.nn.functional.silu(g)
    (a * torch.from_numpy(da)).sum().backward()
    return {"a": a.detach().numpy(), "dg": g.grad.numpy(), "du": u.grad.numpy()}


def swiglu_shape_inputs(rows, F):
    g = rng_of("swiglu", rows, F)
    return NS(gu=bf(2.0 * g.standard_normal((rows, 2 * F))), da=bf(g.standard_normal((rows, F))))


GELU_N = (8, 8 * 257)
GELU_REFUSED_N = 12


def gelu_reference(x, dy=None, mut=None):
    erf = f64(torch.erf(torch.from_numpy(x / math.sqrt(2.0))))
    cdf = 0.5 * f64(torch.erfc(torch.from_numpy(-x / math.sqrt(2.0))))       # 0.5 (1 + erf) without the cancellation
    half = 0.5 * (1.0 + np.abs(erf))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if mut == "tanh-form":
            t = np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))
            cdf = 0.5 * (1.0 + t)
            if dy is not None:
                raise ValueError("tanh-form is a forward mutation")
        if dy is None:
            y = np.where(cdf == 0, 0.0, x * cdf)
            return {"y": Out(y, np.abs(x) * half, 16.0)}
        pdf = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        xp = np.where(pdf == 0, 0.0, x * pdf)
        dx = dy * (cdf + (0.0 if mut == "x-pdf-dropped" else xp))
        return {"dx": Out(dx, np.abs(dy) * (half + np.abs(xp)), 16.0 + np.minimum(0.5 * x * x, 128.0))}


def gelu_f32(x, dy=None):
    x = x.float()
    if dy is None:
        return {"y": f64((0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))).to(BF))}
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
    pdf = 0.39894228040143267794 * torch.exp(-0.5 * x * x)
    return {"dx": f64((dy.float() * (cdf + x * pdf)).to(BF))}


def gelu_autograd(x, dy):
    x = torch.from_numpy(x).clone().requires_grad_()
    y = torch.nn.functional.gelu(x)
    (y * torch.from_numpy(dy)).sum().backward()
    return {"y": y.detach().numpy(), "dx": x.grad.numpy()}


# =========================================================== rope =====================================================================
ROPE_DH = (16, 64, 96, 128)
ROPE_REFUSED_DH = 24
ROPE_TABLES = ("real", "synthetic")
KAPPA_ROPE = 3.0
ROPE_EXTRA = 9                             # rows of the cos / sin table past L that position_ids reach


def _rope_cases():
    out = []
    for Dh in ROPE_DH:
        for H in (1, 3):
            for L in (1, 50):
                for pos in (False, True):
                    out.append(Case("rope", f"d{Dh}-h{H}-l{L}-{'pos' if pos else 'nopos'}", B=2, H=H, L=L, Dh=Dh, pos=pos))
    return tuple(out)


ROPE_CASES = _rope_cases()


def rope_table(P, Dh, table):
    """cos, sin f32 [P, Dh].  real: aki_oracle.rope_cos_sin (both halves equal).  synthetic: two halves that differ."""
    if table == "real":
        import aki_oracle as O              # oracle/ is on the path of every test (tests/conftest.py)
        cos, sin = O.rope_cos_sin(np.arange(P)[None], Dh)
        return np.ascontiguousarray(cos[0], dtype=np.float32), np.ascontiguousarray(sin[0], dtype=np.float32)
    g = rng_of("rope-table", P, Dh)
    return g.uniform(-1, 1, (P, Dh)).astype(np.float32), g.uniform(-1, 1, (P, Dh)).astype(np.float32)


def rope_inputs(c, table):
    g = rng_of("rope", c.H, c.L, c.Dh, c.pos, table)
    P = c.L + ROPE_EXTRA
    cos, sin = rope_table(P, c.Dh, table)
    dq, dk, dv = (bf(g.standard_normal((c.B, c.H, c.L, c.Dh))) for _ in range(3))
    pos = None
    if c.pos:                              # non-monotone, different per sample, reaching the last row of the longer table
        pos = np.stack([g.permutation(P)[:c.L] for _ in range(c.B)]).astype(np.int32)
        pos[0, 0], pos[1, -1] = P - 1, P - 2
    return NS(dq=dq, dk=dk, dv=dv, cos=torch.from_numpy(cos), sin=torch.from_numpy(sin), pos=None if pos is None else torch.from_numpy(pos))


def rope_reference(c, inp, mut=None):
    """-> {'dqk': [B, L, 2 * H * Dh] (the dq and dk thirds), 'dv': [B, L, H * Dh] exact}"""
    B, H, L, Dh = c.B, c.H, c.L, c.Dh
    half = Dh // 2
    cos, sin = f64(inp.cos), f64(inp.sin)
    pos = np.tile(np.arange(L), (B, 1)) if inp.pos is None else inp.pos.numpy().astype(np.int64)
    if mut == "t-in-place-of-pos":
        pos = np.tile(np.arange(L), (B, 1))
    if mut == "sample-0-positions-for-sample-1":
        pos = np.stack([pos[0]] * B)
    cs, sn = cos[pos][:, None], sin[pos][:, None]                  # [B, 1, L, Dh]
    if mut == "sin-sign-flipped":
        sn = -sn
    outs, Ms = [], []
    for y in (f64(inp.dq), f64(inp.dk)):
        y0, y1 = y[..., :half], y[..., half:]
        c_lo, c_hi, s_lo, s_hi = cs[..., :half], cs[..., half:], sn[..., :half], sn[..., half:]
        if mut == "sin[d]-in-place-of-sin[half+d]":
            s_hi = s_lo
        if mut == "cos[d]-in-place-of-cos[half+d]":
            c_hi = c_lo
        a0, b0, a1, b1 = y0 * c_lo, y1 * s_hi, y1 * c_hi, -y0 * s_lo
        r = np.concatenate([a0 + b0, a1 + b1], -1)
        M = np.concatenate([np.abs(a0) + np.abs(b0), np.abs(a1) + np.abs(b1)], -1)
        outs.append(r.transpose(0, 2, 1, 3).reshape(B, L, H * Dh))
        Ms.append(M.transpose(0, 2, 1, 3).reshape(B, L, H * Dh))
    dv = f64(inp.dv).transpose(0, 2, 1, 3).reshape(B, L, H * Dh)
    return {"dqk": Out(np.concatenate(outs, -1), np.concatenate(Ms, -1), KAPPA_ROPE), "dv": Out(dv, kind="exact")}


def rope_f32(c, inp):
    B, H, L, Dh = c.B, c.H, c.L, c.Dh
    half = Dh // 2
    pos = torch.arange(L).repeat(B, 1) if inp.pos is None else inp.pos.long()
    cs, sn = inp.cos[pos][:, None], inp.sin[pos][:, None]
    outs = []
    for y in (inp.dq.float(), inp.dk.float()):
        y0, y1 = y[..., :half], y[..., half:]
        r = torch.cat([y0 * cs[..., :half] + y1 * sn[..., half:], y1 * cs[..., half:] - y0 * sn[..., :half]], -1)
        outs.append(r.to(BF).transpose(1, 2).reshape(B, L, H * Dh))
    return {"dqk": f64(torch.cat(outs, -1)), "dv": f64(inp.dv.transpose(1, 2).reshape(B, L, H * Dh))}


def rope_autograd(c, inp):
    B, H, L, Dh = c.B, c.H, c.L, c.Dh
    pos = torch.arange(L).repeat(B, 1) if inp.pos is None else inp.pos.long()
    cs, sn = inp.cos.to(F64)[pos][:, None], inp.sin.to(F64)[pos][:, None]
    rot = lambda t: torch.cat((-t[..., Dh // 2:], t[..., :Dh // 2]), -1)
    q, k = (torch.zeros(B, H, L, Dh, dtype=F64, requires_grad=True) for _ in range(2))
    ((q * cs + rot(q) * sn) * inp.dq.to(F64)).sum().backward()
    ((k * cs + rot(k) * sn) * inp.dk.to(F64)).sum().backward()
    return {"dqk": torch.cat([t.grad.transpose(1, 2).reshape(B, L, H * Dh) for t in (q, k)], -1).numpy()}


# ======================================================= cross-entropy ================================================================
CE_V = (2, 511, 512, 513, 1003, 1025)
CE_FAMILIES = ("diffuse", "peaked", "shifted")
KAPPA_CE = {"loss_rows": 32.0, "grad": 32.0}
CE_POISON = 0x5A5A                          # bit pattern of the columns V..ld


def _ce_cases():
    out = []
    r8 = lambda v: (v + 7) // 8 * 8
    for V in CE_V:
        for wide in (False, True):
            ld = r8(V) + (40 if wide else 0)
            out.append(Case("ce", f"v{V}-ld{ld}-b3-l40", V=V, ld=ld, B=3, L=40, gscale=0.25 if wide else 1.0, labels="mix"))
    for V in (2, 513):
        for L in (1, 2):
            for B in (1, 3):
                out.append(Case("ce", f"v{V}-ld{r8(V)}-b{B}-l{L}", V=V, ld=r8(V), B=B, L=L, gscale=1.0, labels="mix"))
    out.append(Case("ce", "v513-ld520-b3-l40-all-ignored", V=513, ld=520, B=3, L=40, gscale=1.0, labels="none"))
    out.append(Case("ce", "v1025-ld1072-b1-l2-g0.25", V=1025, ld=1072, B=1, L=2, gscale=0.25, labels="mix"))
    return tuple(out)


CE_CASES = _ce_cases()


def ce_inputs(c, family):
    g = rng_of("ce", c.V, c.ld, c.B, c.L, family)
    B, L, V = c.B, c.L, c.V
    labels = g.integers(0, V, (B, L)).astype(np.int64)
    if c.labels == "none":
        labels[:] = -100
    else:
        for b in range(B):                   # row (b, t) is scored against labels[b][t + 1]
            special = (0, V - 1, -100, V + 3, V)
            if L == 2:
                labels[b, 1] = (V - 1, 0, V)[b % 3]
            for t in range(1, min(L, 6)):
                if L > 2:
                    labels[b, t] = special[(t - 1 + b) % 5]
        if L > 8:
            labels[0, 7] = -100
    lo = g.standard_normal((B, L, V)) * (1.0 if family == "peaked" else 3.0)
    if family == "peaked":
        for b in range(B):
            for t in range(L):
                tg = labels[b, t + 1] if t + 1 < L else -100
                tg = tg if 0 <= tg < V else 0
                col = tg if (t % 2 == 0 or V == 1) else (tg + 1) % V
                lo[b, t, col] += 80.0
    if family == "shifted":
        lo = lo + 200.0
    buf = torch.empty((B, L, c.ld), dtype=torch.int16).fill_(CE_POISON).view(BF)
    buf[..., :V] = bf(lo)
    return NS(logits=buf, labels=torch.from_numpy(labels))


def ce_targets(c, labels, mut=None):
    """[B * L] shifted targets with -100 on ignored rows."""
    lab = labels.numpy()
    tgt = np.full((c.B, c.L), -100, dtype=np.int64)
    if mut == "labels-not-shifted":
        tgt[:] = lab
    else:
        tgt[:, :-1] = lab[:, 1:]
    if mut == "label>=V-counted-valid":
        return tgt.reshape(-1)
    tgt[(tgt < 0) | (tgt >= c.V)] = -100
    return tgt.reshape(-1)


def ce_reference(c, inp, mut=None):
    V, rows = c.V, c.B * c.L
    lg = f64(inp.logits)[..., :V].reshape(rows, V)
    tgt = ce_targets(c, inp.labels, mut)
    n_valid = int((tgt != -100).sum())
    valid = (tgt >= 0) & (tgt < V)
    gscale = 1.0 if mut == "gscale-ignored" else c.gscale
    k = gscale / (rows if mut == "divide-by-B*L" else max(n_valid, 1))
    if mut == "no-max-subtraction-f32":
        with np.errstate(over="ignore", invalid="ignore"):
            st32 = np.exp(lg.astype(np.float32)).sum(1, dtype=np.float32)
            lse = np.log(st32).astype(np.float64)
        gm = np.zeros(rows)
    else:
        gm = lg.max(1)
        e = np.exp(lg - gm[:, None])
        if mut == "last-odd-column-left-out" and V % 2:
            e[:, V - 1] = 0.0
        st = e.sum(1)
        lse = gm + np.log(st)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.exp(lg - lse[:, None])
        Q = (p * np.abs(lg - gm[:, None])).sum(1)
    tcol = np.where(valid, tgt, 0)
    lt = lg[np.arange(rows), tcol]
    loss = np.where(valid, lse - lt, 0.0)
    Mloss = np.where(valid, 1.0 + Q + np.abs(gm) + np.abs(lse - gm) + np.abs(lse) + np.abs(lt), 0.0)
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows), tcol] = 1.0
    with np.errstate(invalid="ignore"):
        grad = np.where(valid[:, None], (p - onehot) * k, 0.0)
        Mg = np.where(valid[:, None], k * (p * (1.0 + np.abs(lg - lse[:, None]) + Mloss[:, None]) + onehot), 0.0)
    out = {"loss_rows": Out(loss, Mloss, KAPPA_CE["loss_rows"], "f32"), "grad": Out(grad, Mg, KAPPA_CE["grad"]),
           "n_valid": Out(np.array([n_valid]), kind="exact"), "ignored": ~valid}
    n = max(n_valid, 1) if mut != "divide-by-B*L" else rows
    lt_ = out["loss_rows"].tol()
    out["loss"] = Out(np.array([loss.sum() / n]), np.array([np.abs(loss).sum() / n]), rows + 2.0, "f32",
                      extra=float(np.where(valid, lt_, 0.0).sum() / n))
    return out


def ce_f32(c, inp):
    V, rows = c.V, c.B * c.L
    lg = inp.logits[..., :V].reshape(rows, V).float()
    tgt = torch.from_numpy(ce_targets(c, inp.labels))
    valid = tgt != -100
    n = max(int(valid.sum()), 1)
    lse = torch.logsumexp(lg, 1)
    tc = torch.where(valid, tgt, torch.zeros_like(tgt))
    loss = torch.where(valid, lse - lg[torch.arange(rows), tc], torch.zeros(()))
    p = torch.exp(lg - lse[:, None])
    p[torch.arange(rows), tc] -= 1.0
    grad = torch.where(valid[:, None], p * torch.tensor(c.gscale / n, dtype=F32), torch.zeros(())).to(BF)
    return {"loss_rows": f64(loss), "grad": f64(grad), "n_valid": np.array([int(valid.sum())]),
            "loss": f64((loss.sum() / n).reshape(1))}


def ce_autograd(c, inp):
    V, rows = c.V, c.B * c.L
    lg = inp.logits[..., :V].to(F64).reshape(rows, V).clone().requires_grad_()
    tgt = torch.from_numpy(ce_targets(c, inp.labels))
    per = torch.nn.functional.cross_entropy(lg, tgt, ignore_index=-100, reduction="none")
    n = max(int((tgt != -100).sum()), 1)
    (per.sum() / n * c.gscale).backward()
    return {"loss_rows": per.detach().numpy(), "grad": lg.grad.numpy(), "loss": np.array([float(per.detach().sum() / n)])}


# =========================================================== grad_sqnorm ==============================================================
KAPPA_SQNORM = 64.0
SQNORM_REFUSED_N = 12


def _sqnorm_cases():
    K = kernel_constants()
    out = []
    for n in (8, 8 * 255, 8 * 256 * K["SQNORM_GROUPS"] + 8):
        for g32 in (False, True):
            for acc in (False, True):
                out.append(Case("sqnorm", f"n{n}-{'f32' if g32 else 'bf16'}-{'acc' if acc else 'set'}", n=n, g32=g32, accumulate=acc))
    return tuple(out)


SQNORM_CASES = _sqnorm_cases()


def sqnorm_inputs(c):
    g = rng_of("sqnorm", c.n, c.g32)
    v = g.standard_normal(c.n) * 0.5
    gt = torch.from_numpy(v.astype(np.float32)) if c.g32 else bf(v)
    return NS(g=gt, out0=np.float32(37.25) if c.accumulate else None)


def sqnorm_reference(c, inp, mut=None):
    v = f64(inp.g)
    if mut == "last-chunk-dropped":
        v = v[:-8]
    s = float((v * v).sum())
    M = float((f64(inp.g) ** 2).sum())
    if c.accumulate:
        if mut != "accumulate-ignored":
            s += float(inp.out0)
        M += abs(float(inp.out0))
    return {"out": Out(np.array([s]), np.array([M]), KAPPA_SQNORM, "f32")}


def sqnorm_f32(c, inp):
    s = (inp.g.float() ** 2).sum()
    if c.accumulate:
        s = s + torch.tensor(inp.out0)
    return {"out": f64(s.reshape(1))}


# ============================================================= adamw ==================================================================
KAPPA_ADAMW = {"p": 48.0, "m": 10.0, "v": 20.0}
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8)
ADAMW_STEPS = (1, 2, 1000, 100000)
ADAMW_T_SHAPES = ((1, 4), (63, 4), (64, 64), (65, 68), (100, 132))
ADAMW_PERIOD = 8 * 257                      # the grid-cap case repeats this many elements


def _adamw_cases():
    K = kernel_constants()
    out, i = [], 0
    for g32 in (False, True):
        for gscale in (1.0, 0.25):
            for clip in ("off", "active", "inactive"):
                for wd in (0.0, 0.1):
                    step = ADAMW_STEPS[i % 4]
                    i += 1
                    out.append(Case("adamw", f"n2056-{'f32' if g32 else 'bf16'}-gs{gscale}-clip-{clip}-wd{wd}-step{step}", n=8 * 257, g32=g32,
                                    gscale=gscale, clip=clip, max_norm=0.0 if clip == "off" else 1.0, wd=wd, step=step, reps=1))
    for j, step in enumerate(ADAMW_STEPS):
        out.append(Case("adamw", f"n8-step{step}", n=8, g32=bool(j % 2), gscale=(1.0, 0.25, 0.25, 1.0)[j], clip=("active", "off", "inactive", "active")[j],
                        max_norm=(1.0, 0.0, 1.0, 1.0)[j], wd=0.1, step=step, reps=1))
    for g32 in (False, True):                 # the norm just above max_norm: where the 1e-6 of the clip weighs most
        out.append(Case("adamw", f"n2056-{'f32' if g32 else 'bf16'}-clip-barely-step1", n=8 * 257, g32=g32, gscale=1.0, clip="barely", max_norm=1.0,
                        wd=0.0, step=1, reps=1))
    reps = K["EW_GRID"] * 256 * 8 // ADAMW_PERIOD + 1
    out.append(Case("adamw", "past-the-grid-cap", n=ADAMW_PERIOD * reps, g32=False, gscale=1.0, clip="active", max_norm=1.0, wd=0.1, step=2, reps=reps))
    return tuple(out)


ADAMW_CASES = _adamw_cases()


def adamw_inputs(c, n=None):
    """One period of the inputs (the grid-cap case tiles it c.reps times); sqnorm is the f32 sum of squares of ALL gradients."""
    n = min(c.n, ADAMW_PERIOD) if n is None else n
    g = rng_of("adamw", n, c.g32, c.gscale, c.clip, c.step)
    gr = 3.0 * g.standard_normal(n)
    gr[0], gr[1], gr[2] = 0.0, 0.0, 2.0 ** -60
    first = c.step == 1
    m0 = np.zeros(n) if first else 0.1 * g.standard_normal(n)
    v0 = np.zeros(n) if first else 0.01 * g.standard_normal(n) ** 2
    v0[0] = v0[1] = 0.0
    m0[1] = 0.0
    if c.clip in ("inactive", "barely"):    # gscale * norm = 0.5 < max_norm, or just above it
        gr = gr * ((0.5 if c.clip == "inactive" else 1.0625) / (c.gscale * math.sqrt((gr * gr).sum() * c.reps)))
    gt = torch.from_numpy(gr.astype(np.float32)) if c.g32 else bf(gr)
    sq = np.float32((f64(gt) ** 2).sum() * c.reps)
    return NS(p=torch.from_numpy(g.standard_normal(n).astype(np.float32)), m=torch.from_numpy(m0.astype(np.float32)),
              v=torch.from_numpy(v0.astype(np.float32)), g=gt, sqnorm=sq)


def adamw_reference(c, inp, mut=None):
    h = {k: float(np.float32(v)) for k, v in ADAMW_HYPER.items()}
    lr, b1, b2, eps, wd = h["lr"], h["beta1"], h["beta2"], h["eps"], float(np.float32(c.wd))
    gscale, max_norm = float(np.float32(c.gscale)), float(np.float32(c.max_norm))
    p0, m0, v0, g = f64(inp.p), f64(inp.m), f64(inp.v), f64(inp.g)
    norm = math.sqrt(float(inp.sqnorm)) * (1.0 if mut == "gscale-after-the-clip-norm" else gscale)
    clip = 1.0
    if max_norm > 0 or mut == "clip-applied-at-max_norm-0":
        clip = min(1.0, max_norm / (norm + (0.0 if mut == "clip-without-1e-6" else 1e-6)))
    g1 = g * gscale * clip
    if mut == "weight-decay-coupled":
        g1 = g1 + wd * p0
        pd = p0
    else:
        pd = p0 * (1.0 - lr * wd)
    step = c.step + 1 if mut == "powf-step-off-by-one" else c.step
    bc1, bc2 = (1.0, 1.0) if mut == "no-bias-correction" else (1.0 - b1 ** step, 1.0 - b2 ** step)
    ta, tb = b1 * m0, (1.0 - b1) * g1
    m = ta + tb
    v = b2 * v0 + (1.0 - b2) * g1 * g1
    den = np.sqrt(v / bc2 + eps) if mut == "eps-inside-sqrt" else np.sqrt(v / bc2) + eps
    U = lr * (m / bc1) / den
    Mm = np.abs(ta) + np.abs(tb)
    with np.errstate(invalid="ignore", divide="ignore"):
        MU = np.where(m != 0, np.abs(U) * Mm / np.where(m != 0, np.abs(m), 1.0), lr * (Mm / bc1) / den)
    return {"p": Out(pd - U, np.abs(pd) + MU, KAPPA_ADAMW["p"], "f32"), "m": Out(m, Mm, KAPPA_ADAMW["m"], "f32"),
            "v": Out(v, v, KAPPA_ADAMW["v"], "f32")}


def adamw_f32(c, inp):
    f = lambda x: torch.tensor(x, dtype=F32)
    lr, b1, b2, eps, wd = f(ADAMW_HYPER["lr"]), f(ADAMW_HYPER["beta1"]), f(ADAMW_HYPER["beta2"]), f(ADAMW_HYPER["eps"]), f(c.wd)
    clip = f(1.0)
    if c.max_norm > 0:
        clip = torch.minimum(f(1.0), f(c.max_norm) / (torch.sqrt(torch.tensor(inp.sqnorm)) * f(c.gscale) + f(1e-6)))
    g = inp.g.float() * (f(c.gscale) * clip)
    p = inp.p * (1.0 - lr * wd)
    m = b1 * inp.m + (1.0 - b1) * g
    v = b2 * inp.v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - torch.pow(b1, f(float(c.step))), 1.0 - torch.pow(b2, f(float(c.step)))
    p = p - lr * (m / bc1) / (torch.sqrt(v / bc2) + eps)
    return {"p": f64(p), "m": f64(m), "v": f64(v)}


def adamw_torch(c, inp):
    """clip_grad_norm_ + torch.optim.AdamW in float64 on the same state (the optimizer's state is set to m0, v0, step - 1)."""
    h = {k: float(np.float32(v)) for k, v in ADAMW_HYPER.items()}
    pt = torch.nn.Parameter(inp.p.to(F64).clone())
    opt = torch.optim.AdamW([pt], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=float(np.float32(c.wd)))
    opt.state[pt] = dict(step=torch.tensor(float(c.step - 1)), exp_avg=inp.m.to(F64).clone(), exp_avg_sq=inp.v.to(F64).clone())
    pt.grad = inp.g.to(F64) * float(np.float32(c.gscale))
    if c.max_norm > 0:                       # the norm the kernel is handed: sqrt of the f32 sum of squares, times gscale
        total = math.sqrt(float(inp.sqnorm)) * float(np.float32(c.gscale))
        pt.grad.mul_(min(1.0, float(np.float32(c.max_norm)) / (total + 1e-6)))
    opt.step()
    st = opt.state[pt]
    return {"p": pt.detach().numpy(), "m": st["exp_avg"].numpy(), "v": st["exp_avg_sq"].numpy()}


# ============================================================ mutations ===============================================================
# kernel -> {mutation: ids of the cases (and, where it matters, the family) on which it must be visible}
MUTATIONS = {
    "norm": {
        "c2-dropped": ("ln-r33-c8", "ln-r33-c1152"), "c1-dropped": ("rms-r33-c8", "ln-r33-c1152"),
        "mean-over-cols+1": ("rms-r33-c8", "ln-r33-c8"), "eps-omitted": ("rms-r33-c1152", "ln-r33-c1152"),
        "dres-not-added": ("rms-r1-c8",), "dw-misses-last-row": ("rms-r513-c2056", "ln-r33-c8", "rms-r1025-c2056"),
        "dw-misses-row-512": ("rms-r513-c2056", "ln-r1025-c2056"), "dw-cols-from-2048-zero": ("rms-r1-c2056", "ln-r513-c4096"),
        "db-equals-dw": ("ln-r33-c8",), "xhat-bf16-before-dw": ("rms-r513-c2056", "ln-r513-c4096"),
        "fold-partial-16-dropped": ("rms-r17-c8", "ln-r513-c2056"), "fold-partial-32-dropped": ("rms-r33-c8", "ln-r49-c2056"),
        "fold-partial-last-dropped": ("rms-r16-c8", "ln-r512-c2056", "rms-r48-c2056"), "accumulate-ignored": ("rms-r33-c8-acc", "ln-r513-c2056-acc"),
    },
    "colsum": {
        "fold-partial-16-dropped": ("r2081-c72-pitch", "r2048-c8"), "fold-partial-32-dropped": ("r2049-c24", "r2048-c1152"),
        "fold-partial-last-dropped": ("r33-c8", "r2081-c64", "r31-c24"), "accumulate-ignored": ("r33-c24-acc", "r2049-c1152-acc-pitch"),
    },
    "swiglu": {"silu-without-g(1-s)": None, "halves-swapped": None},
    "gelu": {"tanh-form": None, "x-pdf-dropped": None},
    "rope": {
        "sin-sign-flipped": ("d96-h3-l50-nopos",), "sin[d]-in-place-of-sin[half+d]": ("d16-h1-l1-nopos", "d128-h3-l50-pos"),
        "cos[d]-in-place-of-cos[half+d]": ("d16-h1-l1-nopos", "d64-h3-l50-pos"), "t-in-place-of-pos": ("d64-h1-l50-pos",),
        "sample-0-positions-for-sample-1": ("d96-h1-l1-pos", "d128-h3-l50-pos"),
    },
    "ce": {
        "labels-not-shifted": ("v513-ld520-b3-l40",), "divide-by-B*L": ("v1003-ld1008-b3-l40", "v2-ld8-b3-l2"),
        "gscale-ignored": ("v1025-ld1072-b1-l2-g0.25", "v512-ld552-b3-l40"), "last-odd-column-left-out": ("v513-ld520-b3-l40", "v1003-ld1008-b3-l40"),
        "label>=V-counted-valid": ("v513-ld520-b3-l40", "v2-ld8-b3-l2"), "no-max-subtraction-f32": ("v512-ld512-b3-l40",),
    },
    "sqnorm": {"last-chunk-dropped": ("n8-bf16-set", "n2040-f32-set"), "accumulate-ignored": ("n8-bf16-acc", "n2097160-f32-acc")},
    "adamw": {
        "weight-decay-coupled": ("n2056-bf16-gs1.0-clip-off-wd0.1-step2",), "no-bias-correction": ("n8-step1", "n8-step2"),
        "eps-inside-sqrt": ("n2056-bf16-gs1.0-clip-off-wd0.1-step2",), "clip-without-1e-6": tuple(c.id for c in ADAMW_CASES if c.clip == "barely"),
        "clip-applied-at-max_norm-0": ("n8-step2", "n2056-bf16-gs1.0-clip-off-wd0.0-step1"),
        "gscale-after-the-clip-norm": tuple(c.id for c in ADAMW_CASES if c.gscale == 0.25 and c.clip != "off"),
        "powf-step-off-by-one": ("n8-step1", "n8-step2"),
    },
}

CASES = {"norm": NORM_CASES, "colsum": COLSUM_CASES, "rope": ROPE_CASES, "ce": CE_CASES, "sqnorm": SQNORM_CASES, "adamw": ADAMW_CASES}
CASE_BY_ID = {(k, c.id): c for k, cs in CASES.items() for c in cs}

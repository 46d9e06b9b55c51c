"""Case table, input families, float64 reference, componentwise bar and reference mutations of the decode linears
(aki_amd/csrc/decode.hip: gemv_bf16_kernel<M, SWIGLU, FPW, W8>, skinny_gemm_bf16_kernel<KS, SWIGLU, FT, NORM>,
skinny_gemm_w8_kernel<KS, SWIGLU, NORM>) and of the host planner in front of them (api.hip: aki_linear_fwd / aki_decode_linear_fwd;
decode.hip: gemv_bf16, skinny_gemm_bf16, skinny_gemm_w8, launch_gemv).  The one-launch decode chain and the batched chain are tested as
bit-identical to these per-layer calls (tests/test_decode_gpu.py), so what holds here carries over to them.

numpy and CPU torch only.  tests/test_decode_linear_cases_cpu.py checks the table itself (the planner in dry-run mode through the lab
library's route log, the coverage of the product library's instantiations, every structural corner, every mutation, a plain float32
implementation inside the bar, the tie cap); tests/test_decode_linear_gpu.py runs every case on the device.

A case names an entry point ("linear" = aki_linear_fwd on bf16, "decode_linear" = aki_decode_linear_fwd on bf16 (fused RMSNorm),
"linear_w8" = aki_linear_fwd on W8A16, "linear_w8_norm" = aki_decode_linear_fwd on W8A16), a shape (M, N, K) with N = weight rows
(2 n_out for SwiGLU), the options of the call, the records the route log must show (aki_amd._lib.DECODE_LOG_FIELDS) or the status a
refusal returns, and why it exists.  A retune of the planner moves shapes onto other kernels: the thresholds and unroll depths are
parsed out of decode.hip (kernel_constants), the shapes are computed from them, and the CPU test fails the table loudly.

The reference.  Inputs are rounded to the kernel's input types first (bf16; W8: e4m3 bytes and one f32 scale per weight row).  The
reference is the exact float64 product of those, the activation in float64, one cast.  The fused RMSNorm has the rounding points of
aki_device.h: round_bf16(x * rstd) is an f32 product cast to bf16 (round to nearest even), the product with the gain is exact in f32
(two 8-bit significands) and pack_bf16x2 casts it once more - HF Phi3RMSNorm, weight * (x * rstd).to(bf16).  The reference takes rstd
in float64, bf16(x * rstd), and bf16 of the product with the gain.

The bar (the shape of tests/train_kernel_cases.py).  tol = half_ulp(|y| + a) + a + floor + ties, a = EPS * (KAPPA * M(y) + ...),
M(y) = sum_k |x_k w_k|, half_ulp the one cast of the output, floor = 2^-126, EPS = 2^-24 (one f32 operation).
  KAPPA of the product = the longest chain of f32 additions on an element's path:
    gemv_bf16_kernel        a lane takes ceil(nchunk / 64) chunks of 8 k, four v_dot2 each counted as two roundings (the pair sum and the
                            accumulate): 8 ceil(K / 512), + the 6 shuffle steps.  W8: chunks of 16 k, 16 ceil(K / 1024) + 6, + 1 for the
                            row scale on the finished sum.
    skinny_gemm_bf16_kernel two MFMAs per step of 64 k, one rounding per MFMA (its internal sum): 2 K / (64 KS), + the KS - 1 folds.
    skinny_gemm_w8_kernel   four MFMAs per step of 128 k: 4 K / (128 KS) + KS - 1, + 1 for the row scale.
  Epilogue (added to a):  bias: EPS (|v| + |b|).  residual: EPS (|v| + |r|).
    fast_sigmoid(t) = v_rcp_f32(1 + v_exp_f32(-log2e t)): the argument's rounding moves the exponential by |t| e^-|t| EPS <= 0.37 EPS
    of the result's scale, v_exp_f32 and v_rcp_f32 are 1 ulp = 2 EPS each, the add 1: <= 6 EPS relative (on the negative side the
    relative error grows with |t| but the value falls as e^-|t|: the same absolute bound relative to 1).
    silu_fast(g) = g sigmoid(g): + the product: KAPPA 8 on |g|.  Its argument's error a_g passes with |silu'(g)|.
    gelu_tanh_fast(v) = v sigmoid(2u), u = c (v + 0.044715 v^3): u carries 5 roundings, so the sigmoid's argument 7: 7 * 0.37 + 5 + 1:
    KAPPA 12 on |v|; the pre-activation's error passes with |gelu'| <= 1.13.
    gelu_erf_fast: Abramowitz-Stegun 7.1.26, |error of erf| <= 1.5e-7 = 2.5 EPS, v_rcp_f32 2, v_exp_f32 2 (argument: <= 0.37 * 3), five
    FMAs of two roundings on values below 1.5: 15; y = 0.5 v (1 + erf): 0.5 * 24 + 3: KAPPA 16 on |v|; |gelu'| <= 1.13.
    SwiGLU: y = u silu(g): a = |silu(g)| a_u + |u silu'(g)| a_g + EPS (8 |u| |g| + |y|).
  Ties.  The kernel's x * rstd is an f32 product with rstd = rsqrtf(ss / K + eps): rsqrtf 1 ulp (2 EPS), the division and the add (3),
    the row sum ss (R = 8 chunks-per-lane FMAs + 6 shuffles [+ 3 for the four waves of the GEMV], halved by the square root) and the
    product (1): delta = ((R + 3) / 2 + 3) EPS relative.  A normalised operand within delta |u| of a bf16 tie may legitimately round
    the other way: the reference marks those elements and adds |w_nk| ulp(xn_k) |gain_k| for them only.  The share of marked elements
    is capped at TIE_CAP = 1 % per case (the CPU test checks it).
Nothing is tuned on a kernel's output; the CPU test shows a plain float32 torch implementation inside every bar.

Input families.
  one-sign   x_k w_nk keeps one sign down k (the sign of feature n): no cancellation, M(y) = |y|, and a lost wave partial, K slice,
             ladder rung or tile is a fixed share of the element.
  sentinel   at most 32 k positions per row carry about all the mass in about equal shares, the rest 2^-10 of a share each.  The
             positions come from the route (structure()): first and last k of every wave's K slice, both sides of every ladder-rung
             boundary and of the early-sweep boundary, the two 16-byte halves of a lane's 32 bytes, first and last lane, the last
             partial chunk.  Rows carry 1 + m / 16 and features 1 + (n % 128) / 128 (W8: e4m3 bytes 1 + (n % 8) / 8 times
             2^-((n / 8) % 4), scales that differ by >= 2x between neighbouring rows and between a gate row and its up row).
  one-hot    (routes without the norm) row m of x is 1.0 at one structural k, a different one per row: without an epilogue y[m, n] is
             w[n, k_m] bit for bit on bf16 weights, and the bf16 rounding of the f32 product w8 * scale on W8.
  norm-*     (fused-norm routes) the two families above with rows of scale 1 and 2^-7 in turn, the last row scaled so that its mean
             square is about eps, and a gain with a distinct value per k (period 251).

Mutations are named changes to the float64 reference (MUTATIONS: name -> (case id, family)); a mutated reference stands in for a wrong
kernel and must exceed the unmutated bar by MIN_RATIO on the case listed with it.  CAPPED lists those the bar itself holds lower:
  gain-before-cast   bf16(x rstd g) against bf16(bf16(x rstd) g): the inner cast moves an operand by at most 2^-9 relative, with either
      sign, so a sum of P comparable terms moves by about 2^-9 / sqrt(P) of itself - 1 / sqrt(P) of the output's own half ulp, which
      the bar must grant.  With the sentinel family's P = 32 that is 0.18 - 0.35 of the bar (the half ulp is 2^-9 to 2^-8 of the
      element): no input makes one output element see it four times over, and a single nonzero operand (P = 1) reaches 2 at most.
      The two are told apart where they matter - in the operand itself - by the one-sign family only statistically: capped at 0.25.
"""
import math
import os
import re
from dataclasses import dataclass, field
from types import SimpleNamespace as NS

import numpy as np
import torch

from train_kernel_cases import EPS, FLOOR, hb, rng_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MIN_RATIO = 4.0
CAPPED = {"gain-before-cast": 0.25}
TIE_CAP = 0.01
NORM_EPS = 1e-5
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3
OK, ERR_UNSUPPORTED = 0, -2
GEMV, SKINNY, SKINNY_W8 = 0, 1, 2
GUARD_ROWS = 2                           # NaN rows behind every operand and poisoned rows around the output (the GPU test)


def kernel_constants():
    """Thresholds and unroll depths as decode.hip is compiled: a retune moves a corner, and the table (whose shapes are computed from
    these) then fails the CPU test instead of silently testing beside it."""
    with open(os.path.join(ROOT, "aki_amd", "csrc", "decode.hip")) as f:
        src = f.read()

    def one(pattern, what):
        m = re.search(pattern, src)
        assert m, f"{what} not found in decode.hip"
        return [int(g) for g in m.groups()]

    c = {}
    c["KU_NARROW"], c["KU_WIDE"] = one(r"constexpr int KU = NR <= 2 \? (\d+) : (\d+);", "the GEMV's unroll depth KU")
    c["PU_W8"], c["PU"] = one(r"constexpr int PU = W8 \? (\d+) : (\d+);", "the GEMV's early sweep PU")
    assert re.search(r"if constexpr \(M == 1 && !W8\)", src), "the early sweep is no longer bf16 / one row only"
    c["FPW4_N"], = one(r"if \(n_out >= (\d+)\) return launch_gemv_cfg<M, false, 4>", "the FPW = 4 threshold")
    assert re.search(r"if constexpr \(M <= 2\) \{", src), "FPW = 4 is no longer for M <= 2"
    c["GEMV_WGS"], g2 = one(r"const int per = M == 1 \? 1 : \(groups \+ (\d+)\) / (\d+);", "the GEMV's workgroup cap")
    assert g2 == c["GEMV_WGS"] + 1
    c["GEMV_WGS"] = g2
    a, b = one(r"\(size_t\)a->M \* a->K \* 2 > (\d+) \* (\d+) \* 2", "the GEMV's LDS limit")
    c["GEMV_MK"] = a * b
    c["UN_4"], c["UN_2"], c["UN_1"] = one(r"constexpr int UN = NS >= 4 \? (\d+) : \(NS == 2 \? (\d+) : (\d+)\);", "the skinny GEMM's UN")
    c["UP_SWIGLU"], c["UP"] = one(r"constexpr int UP = NS >= 2 \? (\d+) : (\d+);", "the skinny GEMM's UP")
    c["UN_W8_SWIGLU"], c["UN_W8"] = one(r"constexpr int UN = SWIGLU \? (\d+) : (\d+);", "the W8 skinny GEMM's UN")
    m = re.search(r"if \(tiles < (\d+) && a->K % (\d+) == 0\) return launch_skinny<8, 1>\(p, stream\);\s*"
                  r"if \(tiles < (\d+) && a->K % (\d+) == 0\) return launch_skinny<4, 1>\(p, stream\);\s*"
                  r"if \(a->K % (\d+) == 0\) return launch_skinny<2, 1>", src)
    assert m, "the skinny GEMM's K split rule not found in decode.hip"
    c["T8"], c["K8"], c["T4"], c["K4"], c["K2"] = (int(g) for g in m.groups())
    m = re.search(r"if \(tiles < (\d+) && a->K % (\d+) == 0\) return launch_skinny<8, 1, true>\(p, stream\);\s*"
                  r"if \(tiles < (\d+) && a->K % (\d+) == 0\) return launch_skinny<4, 1, true>", src)
    assert m and tuple(int(g) for g in m.groups()) == (c["T8"], c["K8"], c["T4"], c["K4"]), "the NORM rule differs from the plain one"
    m = re.search(r"const bool k8 = a->K % (\d+) == 0 && a->K / 8 >= (\d+), k4 = a->K % (\d+) == 0;", src)
    assert m, "the W8 skinny GEMM's K split rule not found in decode.hip"
    c["W8_K8"], c["W8_K8_MIN"], c["W8_K4"] = (int(g) for g in m.groups())
    c["W8_K2"], = one(r"if \(a->K % (\d+) == 0\) return launch_skinny_w8<2, false>", "the W8 KS = 2 gate")
    assert re.search(r"if \(k8 && tiles < %d\) return launch_skinny_w8<8, false>" % c["T8"], src)
    assert re.search(r"if \(k4 && tiles < %d\) return launch_skinny_w8<4, false>" % c["T4"], src)
    assert re.search(r"if \(tiles >= %d\) return AKI_ERR_UNSUPPORTED;" % c["T4"], src)
    c["NORM_MAX_K"], = one(r"if \(rms_w && \(a->M > 8 \|\| a->K > (\d+)\)\) return AKI_ERR_UNSUPPORTED;", "the NORM K limit")
    return c


KC = kernel_constants()


# ---- records -------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def gemv(M, n_out, K, swiglu=0, fpw=2, w8=0, norm=0):
    groups = cdiv(n_out, 4 * fpw)
    per = 1 if M == 1 else cdiv(groups, KC["GEMV_WGS"])
    return (GEMV, M, swiglu, fpw, w8, norm, cdiv(groups, per), per, M * K * 2)


def skinny(ks, M, n_out, K, swiglu=0, norm=0, family=SKINNY):
    smem = max(M * (K * 2 + 16), ks * 2 * 1024) if norm else 0
    return (family, ks, swiglu, 1, norm, norm, cdiv(n_out, 16), 0, smem)


def skinny_w8(ks, M, n_out, K, swiglu=0, norm=0):
    return skinny(ks, M, n_out, K, swiglu, norm, SKINNY_W8)


def kernel_of(record):
    """(template name, template arguments) of a record, as `nm -C` prints them."""
    fam, a, sw, b, c = record[:5]
    if fam == GEMV:
        return ("gemv_bf16_kernel", (a, sw, b, c))
    if fam == SKINNY:
        return ("skinny_gemm_bf16_kernel", (a, sw, b, c))
    return ("skinny_gemm_w8_kernel", (a, sw, c))


@dataclass(frozen=True)
class Case:
    id: str
    entry: str                  # "linear" | "decode_linear" | "linear_w8" | "linear_w8_norm"
    shape: tuple                # (M, N, K), N = weight rows
    expect: tuple = ()          # the decode-linear records of one call
    status: int = OK            # what the call returns (a refusal logs nothing and leaves the output alone)
    gemm: bool = False          # the call falls through to the MFMA GEMM (its own log shows the launch)
    opts: dict = field(default_factory=dict)   # act, bias, residual, res_row_mod, ldx_pad, ldw_pad, ldy_pad, ldr_pad
    why: str = ""

    def opt(self, name, default=0):
        return self.opts.get(name, default)

    @property
    def swiglu(self):
        return self.opt("act") == ACT_SWIGLU

    @property
    def n_out(self):
        return self.shape[1] // 2 if self.swiglu else self.shape[1]

    @property
    def norm(self):
        return self.entry in ("decode_linear", "linear_w8_norm")

    @property
    def w8(self):
        return self.entry.startswith("linear_w8")

    @property
    def runs(self):
        return self.status == OK

    @property
    def epilogue(self):
        return bool(self.opt("act") or self.opt("bias") or self.opt("residual"))


G1, G2, SW = ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU
PRE_K = 64 * KC["PU"] * 8                               # the M = 1 early sweep starts here (2048)
LADDER_NARROW = 64 * 8 * (8 + 4 + 2 + 1) if KC["KU_NARROW"] == 8 else None     # every rung 8 / 4 / 2 / 1 once (7680 k)
LADDER_WIDE = 64 * 8 * (4 + 2 + 1)                      # NR > 2: 4 / 2 / 1 (3584 k)
LADDER_W8 = 64 * 16 * (4 + 2 + 1)                       # W8 GEMV: 4 / 2 / 1 (7168 k)
N_FPW4 = KC["FPW4_N"]
N_T8, N_T4 = 16 * KC["T8"], 16 * KC["T4"]
assert LADDER_NARROW, "the GEMV's deepest unroll is no longer 8: rebuild the K ladder cases"


def _cases():
    C = []

    def add(id, entry, shape, expect=(), why="", status=OK, gemm=False, **opts):
        C.append(Case(id, entry, shape, tuple(expect), status, gemm, opts, why))

    # ---- gemv_bf16_kernel: M = 1 (aki_linear_fwd never offers one row to the skinny GEMM) ------------------------------------------------
    add("gemv-m1-k8", "linear", (1, 7, 8), [gemv(1, 7, 8)], "one chunk: only lane 0 has work; n_out odd, one wave with a single feature", bias=1)
    add("gemv-m1-ladder", "linear", (1, 38, PRE_K + LADDER_NARROW + 40), [gemv(1, 38, PRE_K + LADDER_NARROW + 40)],
        "early sweep, then every rung 8 / 4 / 2 / 1 once, then a five-lane tail; n_out % 8 = 6", residual=1, ldr_pad=3)
    add("gemv-m1-swiglu", "linear", (1, 2 * 37, PRE_K + LADDER_WIDE + 24), [gemv(1, 37, PRE_K + LADDER_WIDE + 24, swiglu=1)],
        "SwiGLU (NR = 4): early sweep, rungs 4 / 2 / 1, a three-lane tail; up rows at n_out + f with n_out odd", act=SW, residual=1)
    for k, what in ((PRE_K - 8, "no early sweep"), (PRE_K, "early sweep and nothing left"), (PRE_K + 8, "early sweep, then a one-lane tail")):
        add(f"gemv-m1-pre-k{k}", "linear", (1, 24, k), [gemv(1, 24, k)], what, bias=1, act=G1 if k == PRE_K else 0)
        add(f"gemv-m1-norm-pre-k{k}", "decode_linear", (1, 24, k), [gemv(1, 24, k, norm=1)], what + ", fused norm", ldx_pad=256 if k == PRE_K else 0)
    add("gemv-m1-fpw2-below", "linear", (1, N_FPW4 - 1, 64), [gemv(1, N_FPW4 - 1, 64)], "n_out just below the FPW = 4 threshold", act=G2, bias=1)
    add("gemv-m1-fpw4-at", "linear", (1, N_FPW4, 64), [gemv(1, N_FPW4, 64, fpw=4)], "n_out at the FPW = 4 threshold", residual=1)
    add("gemv-m1-fpw4-ragged", "linear", (1, N_FPW4 + 11, PRE_K + LADDER_WIDE + 8), [gemv(1, N_FPW4 + 11, PRE_K + LADDER_WIDE + 8, fpw=4)],
        "FPW = 4 (NR = 4): early sweep, rungs 4 / 2 / 1; n_out % 16 = 11: clamped rows and the n >= n_out guard", bias=1, ldw_pad=8)
    add("gemv-m1-norm-swiglu", "decode_linear", (1, 2 * 22, 520), [gemv(1, 22, 520, swiglu=1, norm=1)], "fused norm + SwiGLU, nchunk % 64 = 1", act=SW)
    # ---- gemv_bf16_kernel: 2 <= M <= 8, where the skinny GEMM refuses (K % 64, n_out % 4, ldy % 4) ---------------------------------------
    add("gemv-m2-nout", "linear", (2, 38, 128), [gemv(2, 38, 128)], "n_out % 4 = 2 keeps the skinny GEMM away", bias=1, residual=1, res_row_mod=1)
    add("gemv-m3-ladder", "linear", (3, 40, LADDER_NARROW + 40), [gemv(3, 40, LADDER_NARROW + 40)],
        "K % 64 = 40: every rung 8 / 4 / 2 / 1 once and a five-lane tail, three rows in LDS")
    add("gemv-m2-swiglu-ladder", "linear", (2, 2 * 22, LADDER_WIDE + 40), [gemv(2, 22, LADDER_WIDE + 40, swiglu=1)],
        "K % 64 = 40, SwiGLU: rungs 4 / 2 / 1 at NR = 4", act=SW, residual=1, ldr_pad=2)
    add("gemv-m4-ldy", "linear", (4, 40, 256), [gemv(4, 40, 256)], "ldy % 4 = 2 keeps the skinny GEMM away", ldy_pad=2, bias=1, act=G1)
    add("gemv-m5-k", "linear", (5, 33, 72), [gemv(5, 33, 72)], "K % 64 = 8, n_out odd", residual=1, res_row_mod=3, ldx_pad=8, ldw_pad=16, ldy_pad=1, ldr_pad=5)
    add("gemv-m6-nout", "linear", (6, 45, 64), [gemv(6, 45, 64)], "n_out % 4 = 1", bias=1, act=G2)
    add("gemv-m7-ldy", "linear", (7, 36, 192), [gemv(7, 36, 192)], "ldy % 4 = 2", ldy_pad=6, residual=1, ldr_pad=4)
    add("gemv-m8-k8", "linear", (8, 40, 8), [gemv(8, 40, 8)], "K = 8: one chunk per row")
    for m, (k, n, why) in zip(range(3, 9), ((72, 22, "K % 64 = 8"), (128, 21, "n_out odd"), (200, 20, "K % 64 = 8"), (64, 19, "n_out odd"),
                                            (136, 18, "K % 64 = 8, n_out % 4 = 2"), (8, 17, "K = 8"))):
        add(f"gemv-m{m}-swiglu", "linear", (m, 2 * n, k), [gemv(m, n, k, swiglu=1)], "SwiGLU at M = %d: %s" % (m, why), act=SW, residual=m % 2, ldr_pad=m % 3)
    add("gemv-m2-fpw2-below", "linear", (2, N_FPW4 - 1, 72), [gemv(2, N_FPW4 - 1, 72)], "M = 2 just below the FPW = 4 threshold: per = 3, short last lists")
    add("gemv-m2-fpw4-at", "linear", (2, N_FPW4, 72), [gemv(2, N_FPW4, 72, fpw=4)], "M = 2 at the FPW = 4 threshold: 512 groups, per = 1", bias=1)
    add("gemv-m3-wide", "linear", (3, N_FPW4, 72), [gemv(3, N_FPW4, 72)], "M = 3 never takes FPW = 4; 1024 groups: per = 2, every list full", residual=1)
    add("gemv-m3-short-list", "linear", (3, 8 * (2 * KC["GEMV_WGS"] + 6) - 3, 72), [gemv(3, 8 * (2 * KC["GEMV_WGS"] + 6) - 3, 72)],
        "1030 groups: per = 3 on 344 workgroups, the last two with two groups; n_out % 8 = 5")
    add("gemv-m8-lds-limit", "linear", (8, 6, KC["GEMV_MK"] // 8), [gemv(8, 6, KC["GEMV_MK"] // 8)], "M K at the 64 Ki limit of the LDS staging")
    add("gemv-m8-beyond-lds", "linear", (8, 6, KC["GEMV_MK"] // 8 + 8), [], "one chunk beyond: the GEMV refuses, and so does the MFMA GEMM (K % 64 = 8)",
        status=ERR_UNSUPPORTED)
    add("gemv-m1-lds-limit", "linear", (1, 8, KC["GEMV_MK"]), [gemv(1, 8, KC["GEMV_MK"])], "one row of 64 Ki: the whole LDS staging")
    add("gemv-m1-beyond-lds", "linear", (1, 8, KC["GEMV_MK"] + 64), [], "one MFMA K-step beyond: the GEMV refuses and the MFMA GEMM takes the call "
        "(at 2 <= M <= 8 everything that keeps the skinny GEMM away - K % 64, n_out % 4, ldy % 4 - is refused by the MFMA GEMM as well)", gemm=True)
    add("gemv-m3-norm", "decode_linear", (3, 40, 200), [gemv(3, 40, 200, norm=1)], "K % 64 = 8: the NORM skinny GEMM refuses, the GEMV normalises", bias=1)
    add("gemv-m2-norm-wide", "decode_linear", (2, N_T4, 256), [gemv(2, N_T4, 256, fpw=4, norm=1)],
        "tiles = 1536: lm_head-wide outputs are refused by the NORM skinny GEMM and land on the GEMV")
    add("gemv-m2-norm-longk", "decode_linear", (2, 20, KC["NORM_MAX_K"] + 512), [gemv(2, 20, KC["NORM_MAX_K"] + 512, norm=1)],
        "K beyond the NORM skinny GEMM's LDS rows")
    add("decode-m9-refused", "decode_linear", (9, 32, 512), [], "more than eight rows: aki_decode_linear_fwd has no route", status=ERR_UNSUPPORTED)
    # ---- W8A16, one row -------------------------------------------------------------------------------------------------------------------
    add("gemv-w8-k48", "linear_w8", (1, 38, 48), [gemv(1, 38, 48, w8=1)], "K % 16 = 0 only: three lanes, rung 1", bias=1, act=G1)
    add("gemv-w8-ladder", "linear_w8", (1, 38, LADDER_W8 + 80), [gemv(1, 38, LADDER_W8 + 80, w8=1)], "rungs 4 / 2 / 1 and a five-lane tail", residual=1, ldw_pad=16)
    add("gemv-w8-swiglu", "linear_w8", (1, 2 * 21, LADDER_W8 + 16), [gemv(1, 21, LADDER_W8 + 16, swiglu=1, w8=1)],
        "SwiGLU: the scale rows are n_out + f (n_out odd)", act=SW, residual=1)
    add("gemv-w8-norm", "linear_w8_norm", (1, 38, 528), [gemv(1, 38, 528, w8=1, norm=1)], "fused norm in front of e4m3 weights", bias=1, act=G2)
    add("w8-m2-k128-refused", "linear_w8", (2, 24, 128), [], "M >= 2 with K % 256 != 0: neither W8 kernel serves it", status=ERR_UNSUPPORTED)
    add("w8-norm-wide-refused", "linear_w8_norm", (2, N_T4, 512), [], "NORM with tiles >= 1536", status=ERR_UNSUPPORTED)
    # ---- skinny_gemm_bf16_kernel ----------------------------------------------------------------------------------------------------------
    add("skinny-ks8-m2", "linear", (2, 36, 512), [skinny(8, 2, 36, 512)], "KS = 8 by K % 512: one step per wave; n_out % 16 = 4", bias=1, act=G1)
    add("skinny-ks4-m3", "linear", (3, 40, 256), [skinny(4, 3, 40, 256)], "KS = 4 by K % 256; n_out % 16 = 8", residual=1, res_row_mod=2, ldr_pad=4)
    add("skinny-ks2-m8", "linear", (8, 44, 128), [skinny(2, 8, 44, 128)], "KS = 2 by K % 128; n_out % 16 = 12", bias=1, act=G2, ldx_pad=8, ldw_pad=24, ldy_pad=4)
    add("skinny-ks1-m9", "linear", (9, 48, 64), [skinny(1, 9, 48, 64)], "KS = 1: one step, no fold", bias=1, residual=1)
    add("skinny-ks1-ladder", "linear", (15, 20, 960), [skinny(1, 15, 20, 960)], "15 steps on one wave: rungs 8 / 4 / 2 / 1")
    add("skinny-ks2-ladder", "linear", (16, 20, 1920), [skinny(2, 16, 20, 1920)], "15 steps per wave on two waves; sixteen rows")
    add("skinny-ks1-swiglu-ladder", "linear", (3, 2 * 20, 448), [skinny(1, 3, 20, 448, swiglu=1)], "SwiGLU: 7 steps: rungs 4 / 2 / 1", act=SW, residual=1, ldr_pad=8)
    add("skinny-ks8-swiglu", "linear", (9, 2 * 28, 512 * 7), [skinny(8, 9, 28, 512 * 7, swiglu=1)], "SwiGLU on eight waves, 7 steps each", act=SW)
    add("skinny-ks4-swiglu", "linear", (2, 2 * 36, 256 * 3), [skinny(4, 2, 36, 256 * 3, swiglu=1)], "SwiGLU on four waves, three steps: rungs 2 / 1", act=SW)
    add("skinny-ks2-swiglu", "linear", (16, 2 * 24, 128 * 5), [skinny(2, 16, 24, 128 * 5, swiglu=1)], "SwiGLU on two waves, five steps: rungs 4 / 1", act=SW, residual=1)
    add("skinny-t767", "linear", (2, N_T8 - 16, 512), [skinny(8, 2, N_T8 - 16, 512)], "tiles = 767: still KS = 8")
    add("skinny-t768", "linear", (2, N_T8, 512), [skinny(4, 2, N_T8, 512)], "tiles = 768: KS = 4 by the tile threshold", bias=1)
    add("skinny-t1535", "linear", (16, N_T4 - 16, 256), [skinny(4, 16, N_T4 - 16, 256)], "tiles = 1535: still KS = 4")
    add("skinny-t1536", "linear", (2, N_T4, 256), [skinny(2, 2, N_T4, 256)], "tiles = 1536: KS = 2 by the tile threshold", residual=1)
    # ---- skinny_gemm_bf16_kernel<.., NORM> --------------------------------------------------------------------------------------------------
    up, ups = KC["UP"], KC["UP_SWIGLU"]
    add("norm-ks8-below-up", "decode_linear", (2, 36, 512), [skinny(8, 2, 36, 512, norm=1)],
        "one step < UP: no early loads; M < KS: six waves normalise no row; the rows' LDS (2080 B) under the reduction area (16 KiB)", bias=1)
    add("norm-ks8-at-up", "decode_linear", (3, 40, 512 * up), [skinny(8, 3, 40, 512 * up, norm=1)], "steps == UP: the early loads are all of it", residual=1)
    add("norm-ks8-above-up", "decode_linear", (8, 24, 512 * (up + 1)), [skinny(8, 8, 24, 512 * (up + 1), norm=1)], "steps == UP + 1, M == KS", act=G1, bias=1)
    add("norm-ks8-swiglu-below-up", "decode_linear", (2, 2 * 20, 512 * (ups - 1)), [skinny(8, 2, 20, 512 * (ups - 1), swiglu=1, norm=1)], "SwiGLU: steps < UP = 3", act=SW)
    add("norm-ks8-swiglu-at-up", "decode_linear", (5, 2 * 20, 512 * ups), [skinny(8, 5, 20, 512 * ups, swiglu=1, norm=1)], "SwiGLU: steps == UP", act=SW, residual=1)
    add("norm-ks8-swiglu-above-up", "decode_linear", (4, 2 * 24, 512 * (ups + 2)), [skinny(8, 4, 24, 512 * (ups + 2), swiglu=1, norm=1)], "SwiGLU: steps == UP + 2", act=SW)
    add("norm-ks4-below-up", "decode_linear", (3, 20, 256), [skinny(4, 3, 20, 256, norm=1)], "KS = 4 by K % 512 = 256, one step, M < KS", ldx_pad=16, ldy_pad=4)
    add("norm-ks4-m8", "decode_linear", (8, 28, 256 * 5), [skinny(4, 8, 28, 256 * 5, norm=1)], "KS = 4, five steps > UP, M > KS: two rows per wave", bias=1, act=G2)
    add("norm-ks4-swiglu", "decode_linear", (6, 2 * 20, 256 * 3), [skinny(4, 6, 20, 256 * 3, swiglu=1, norm=1)], "KS = 4, SwiGLU at UP", act=SW)
    add("norm-ks4-t768", "decode_linear", (2, N_T8, 512), [skinny(4, 2, N_T8, 512, norm=1)], "tiles = 768: NORM on four waves")
    add("norm-ks8-k8192", "decode_linear", (8, 20, KC["NORM_MAX_K"]), [skinny(8, 8, 20, KC["NORM_MAX_K"], norm=1)], "the largest LDS footprint: 8 rows of 8192", residual=1)
    # ---- skinny_gemm_w8_kernel --------------------------------------------------------------------------------------------------------------
    k8min = max(KC["W8_K8"], 8 * KC["W8_K8_MIN"])
    add("w8-ks8", "linear_w8", (2, 36, k8min), [skinny_w8(8, 2, 36, k8min)], "KS = 8: K % 1024 == 0 and K / 8 >= 512; four steps: rung 4", bias=1, act=G1)
    add("w8-ks8-t768", "linear_w8", (3, N_T8, k8min), [skinny_w8(4, 3, N_T8, k8min)], "tiles = 768: KS = 4 although K qualifies for 8")
    add("w8-ks4-short", "linear_w8", (3, 40, 1024), [skinny_w8(4, 3, 40, 1024)], "K % 1024 == 0 but K / 8 < 512: KS = 4, two steps: rung 2", residual=1, res_row_mod=2)
    add("w8-ks4-ladder", "linear_w8", (16, 44, 512 * 7), [skinny_w8(4, 16, 44, 512 * 7)], "seven steps: rungs 4 / 2 / 1", bias=1, ldx_pad=8, ldw_pad=32, ldy_pad=8)
    add("w8-ks4-swiglu", "linear_w8", (9, 2 * 20, 512 * 3), [skinny_w8(4, 9, 20, 512 * 3, swiglu=1)], "SwiGLU: three steps: rungs 2 / 1", act=SW, residual=1, ldr_pad=4)
    add("w8-ks8-swiglu", "linear_w8", (5, 2 * 24, k8min), [skinny_w8(8, 5, 24, k8min, swiglu=1)], "SwiGLU on eight waves, four steps: rung 2 twice", act=SW)
    add("w8-ks2-swiglu", "linear_w8", (2, 2 * 28, 256 * 3), [skinny_w8(2, 2, 28, 256 * 3, swiglu=1)], "SwiGLU on two waves, three steps", act=SW, residual=1)
    add("w8-ks2", "linear_w8", (8, 24, 256), [skinny_w8(2, 8, 24, 256)], "KS = 2 by K % 256: one step", act=G2, bias=1)
    add("w8-ks2-k768", "linear_w8", (15, 28, 768), [skinny_w8(2, 15, 28, 768)], "KS = 2: three steps: rungs 2 / 1")
    add("w8-t1536", "linear_w8", (2, N_T4, 512), [skinny_w8(2, 2, N_T4, 512)], "tiles = 1536: KS = 2 although K % 512 == 0")
    add("w8-norm-ks8", "linear_w8_norm", (4, 24, k8min), [skinny_w8(8, 4, 24, k8min, norm=1)], "NORM on eight waves", bias=1)
    add("w8-norm-ks8-swiglu", "linear_w8_norm", (8, 2 * 20, k8min), [skinny_w8(8, 8, 20, k8min, swiglu=1, norm=1)], "NORM + SwiGLU on eight waves", act=SW, residual=1)
    add("w8-norm-ks4", "linear_w8_norm", (8, 20, 512 * 3), [skinny_w8(4, 8, 20, 512 * 3, norm=1)], "NORM on four waves, M > KS", residual=1)
    add("w8-norm-ks4-swiglu", "linear_w8_norm", (3, 2 * 20, 512), [skinny_w8(4, 3, 20, 512, swiglu=1, norm=1)], "NORM + SwiGLU, M < KS", act=SW)
    add("w8-norm-k256-gemv-refused", "linear_w8_norm", (2, 24, 256), [], "NORM needs K % 512: refused, and the one-row GEMV does not take two rows",
        status=ERR_UNSUPPORTED)
    return C


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
RUN_IDS = [c.id for c in CASES if c.runs and c.expect]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def families(case):
    if case.norm:
        return ("norm-one-sign", "norm-sentinel")
    return ("one-sign", "sentinel", "one-hot")


# ---- dry run: the planner on fake, aligned pointers (nothing is dereferenced before a launch) -----------------------------------------
def _fake(i):
    return (1 << 32) + (i << 28)


def lds(case):
    M, N, K = case.shape
    n_out = case.n_out
    return NS(ldx=K + case.opt("ldx_pad"), ldw=K + case.opt("ldw_pad"), ldy=n_out + case.opt("ldy_pad"),
              ldr=n_out + case.opt("ldr_pad") if case.opt("residual") else 0, res_rows=case.opt("res_row_mod") or M)


def make_args(case, x, w, bias, res, y, w_scale):
    from aki_amd import _lib as L
    M, N, K = case.shape
    ld = lds(case)
    return L.LinearArgs(x, w, bias if case.opt("bias") else None, res if case.opt("residual") else None, y, M, N, K, ld.ldx, ld.ldw, ld.ldy,
                        ld.ldr, case.opt("res_row_mod"), case.opt("act"), L.AKI_DT_W8A16 if case.w8 else L.AKI_DT_BF16, None,
                        w_scale if case.w8 else None)


def call(lib, case, args, gain, stream=None):
    import ctypes as C
    if case.norm:
        return lib.aki_decode_linear_fwd(C.byref(args), gain, NORM_EPS, stream)
    return lib.aki_linear_fwd(C.byref(args), stream)


def dry_run(lib, case):
    """(status, decode-linear records, MFMA GEMM records) of `case` through the lab library in dry-run mode."""
    from aki_amd import _lib as L
    lib.aki_lab_set_decode_dry_run(1)
    lib.aki_lab_set_gemm_dry_run(1)
    lib.aki_lab_decode_log_reset()
    lib.aki_lab_gemm_log_reset()
    try:
        rc = call(lib, case, make_args(case, _fake(1), _fake(2), _fake(3), _fake(4), _fake(5), _fake(6)), _fake(7))
        return rc, L.decode_log(lib), L.gemm_log(lib)
    finally:
        lib.aki_lab_set_decode_dry_run(0)
        lib.aki_lab_set_gemm_dry_run(0)
        lib.aki_lab_decode_log_reset()
        lib.aki_lab_gemm_log_reset()


# ---- the route's structure: which k a lane / wave takes on which rung -----------------------------------------------------------------
def structure(case):
    """The K walk of the case's kernel, restated from decode.hip with the parsed constants: unit (k per chunk / step), slices (one per
    wave: [k0, k1)), sweeps (slice, rung, first k, end k; rung 'pre' = the early sweep / the NORM prologue's loads), rungs visited, the
    sentinel positions (<= 32) and one mutation range each for the tail, the early sweep and a slice's last unit."""
    rec = case.expect[0]
    fam, M, K = rec[0], case.shape[0], case.shape[2]
    sweeps = []
    if fam == GEMV:
        w8 = rec[4]
        NR = rec[3] * (2 if rec[2] else 1)
        unit = 16 if w8 else 8
        nch = K // unit
        ladder = [4, 2, 1] if w8 else ([KC["KU_NARROW"], 4, 2, 1] if NR <= 2 else [KC["KU_WIDE"], 2, 1])
        pre = rec[1] == 1 and not w8 and nch >= 64 * KC["PU"]
        slices = [(0, K)]
        lanes = sorted({0, 63, (nch - 1) % 64})
        for lane in range(64):
            c = lane
            if pre:
                if lane in lanes:
                    sweeps.append((0, "pre", lane, unit * (c - lane), unit * (c - lane + 64 * KC["PU"])))
                c += 64 * KC["PU"]
            for U in ladder:
                while c + 64 * (U - 1) < nch:
                    sweeps.append((0, U, lane, unit * (c - lane), min(unit * (c - lane + 64 * U), K)))
                    c += 64 * U
        rungs = {s[1] for s in sweeps}
        sweeps = [s for s in sweeps if s[2] in lanes]
        lane_k = unit
    else:
        KS, sw = rec[1], rec[2]
        w8 = fam == SKINNY_W8
        unit = 128 if w8 else 64
        Kw = K // KS
        nsteps = Kw // unit
        UN = (KC["UN_W8_SWIGLU"] if sw else KC["UN_W8"]) if w8 else (KC["UN_2"] if sw else KC["UN_1"])
        ladder = sorted({UN, 4 if UN > 4 else UN, 2 if UN > 2 else UN, 1}, reverse=True)
        UP = KC["UP_SWIGLU"] if sw else KC["UP"]
        pre = bool(rec[4]) and not w8 and nsteps >= UP
        slices = [(w * Kw, (w + 1) * Kw) for w in range(KS)]
        for w in range(KS):
            it = 0
            if pre:
                sweeps.append((w, "pre", 0, w * Kw, w * Kw + unit * UP))
                it = UP
            for U in ladder:
                while it + U <= nsteps:
                    sweeps.append((w, U, 0, w * Kw + unit * it, w * Kw + unit * (it + U)))
                    it += U
        rungs = {s[1] for s in sweeps}
        lane_k = unit // 4                   # a lane's 32 bytes: 16 k (bf16) / 32 k (e4m3)
    pos = []

    def put(*ks):
        for k in ks:
            if 0 <= k < K and k not in pos:
                pos.append(k)

    put(0, K - 1)
    for k0, k1 in slices:                   # first and last k of every wave's slice
        put(k0, k1 - 1)
    for s in sweeps:                        # both sides of every rung boundary (and of the early-sweep boundary) on the first and last slice
        if s[0] in (0, len(slices) - 1):
            put(s[3] - 1, s[3], s[4] - 1, s[4])
    h = lane_k // 2
    put(h - 1, h, lane_k - 1, lane_k, unit - 1, unit, K - unit, K - h - 1, K - h)     # the halves of a lane's bytes, first and last lane
    if fam == GEMV:
        put(unit * ((K // unit - 1) // 64 * 64), unit * 63, unit * 63 + unit - 1)     # the last partial round of chunks; lane 63's first chunk
    pos = sorted(pos[:32])
    last = [s for s in sweeps if s[0] == len(slices) - 1]
    tail = max(last, key=lambda s: s[3])
    pres = [s for s in sweeps if s[1] == "pre"]
    return NS(family=fam, unit=unit, slices=slices, sweeps=sweeps, rungs=rungs, pre=pre, positions=pos, lane_k=lane_k,
              tail=(tail[3], K), early=(pres[0][3], pres[0][4]) if pres else None, KS=len(slices))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF)


def f64(t):
    return t.to(F64).numpy()


def e4m3_bytes(a):
    """float array (|a| <= 448) -> e4m3 bytes (round to nearest even), uint8 torch tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(q):
    return q.view(torch.float8_e4m3fn).to(F64).numpy()


def quant_rows_fp8(w):
    """The project's row quantisation (fp8_quant.hip): scale = max(amax, 1e-12) / 448 in f32, q = e4m3(clamp(w * (1 / scale)))."""
    w = np.asarray(w, dtype=np.float32)
    s = np.maximum(np.abs(w).max(axis=1), np.float32(1e-12)) * np.float32(1.0 / 448.0)
    inv = (np.float32(1.0) / s).astype(np.float32)
    return e4m3_bytes(np.clip(w * inv[:, None], -448.0, 448.0)), torch.from_numpy(s.astype(np.float32))


def inputs(case, family):
    """x bf16 [M, K]; w bf16 [N, K] or (wq uint8 [N, K], ws f32 [N]); bias bf16 [n_out]; res bf16 [res rows, n_out]; gain bf16 [K]."""
    M, N, K = case.shape
    n_out = case.n_out
    rng = rng_of("decode-linear", case.id, family)
    st = structure(case) if case.expect else None
    base = family.replace("norm-", "")
    sgn_k = np.where(rng.random(K) < 0.5, -1.0, 1.0)
    sgn_n = np.where(np.arange(N) % 3 == 1, -1.0, 1.0)
    inp = NS(family=family, ws=None, wq=None, gain=None, hot=None)
    if base == "one-sign":
        x = (0.25 + np.abs(rng.standard_normal((M, K)))) * sgn_k
        w = (0.25 + np.abs(rng.standard_normal((N, K), dtype=np.float32))) * (sgn_k * (1.5 / K))[None, :] * sgn_n[:, None]
        x *= (1.0 + np.arange(M) / 16.0)[:, None]
    elif base == "sentinel":
        pos = np.asarray(st.positions)
        share = 1.0 + (np.arange(len(pos)) % 4) / 4.0
        x = rng.uniform(0.5, 1.0, (M, K)) * 2.0 ** -5
        x[:, pos] = 1.0
        x *= (1.0 + np.arange(M) / 16.0)[:, None]
        w = rng.uniform(0.5, 1.0, (N, K)).astype(np.float32) * np.float32(2.0 ** -5)
        w[:, pos] = share[None, :]
        if case.w8:
            mag = (1.0 + (np.arange(N) % 8) / 8.0) * 2.0 ** -((np.arange(N) // 8) % 4)
        else:
            mag = 1.0 + (np.arange(N) % 128) / 128.0
        w *= (mag * sgn_n * (2.0 / len(pos)))[:, None].astype(np.float32)
    elif base == "one-hot":
        pos = list(st.positions) + [k for k in range(K) if k not in st.positions][:max(0, M - len(st.positions))]
        inp.hot = [pos[m % len(pos)] for m in range(M)]
        x = np.zeros((M, K))
        x[np.arange(M), inp.hot] = 1.0
        w = rng.standard_normal((N, K), dtype=np.float32)
    else:
        raise KeyError(family)
    if case.norm:
        scale = np.where(np.arange(M) % 2 == 0, 1.0, 2.0 ** -7)
        x *= scale[:, None]
        if M > 1 or base == "one-sign":                   # the last row: mean square about eps
            x[M - 1] *= math.sqrt(NORM_EPS) / math.sqrt(np.mean(x[M - 1] ** 2))
        inp.gain = bf(0.5 + (np.arange(K) % 251) / 256.0)
        w = w * np.float32(1.0 / 4.0) if base == "one-sign" else w      # the normalised rows have unit mean square: keep the pre-activations moderate
    inp.x = bf(x)
    if case.w8:
        if base == "sentinel":                            # hand-made scales: >= 2x between neighbouring rows and between gate and up row
            e = (np.arange(N) % 2) * 2 + (np.arange(N) >= n_out) * (1 if case.swiglu else 0) * 1
            s = (2.0 ** -(2 + e)) * (1.0 + (np.arange(N) % 5) / 8.0) * np.where(np.arange(N) % 2 == 0, 1.0, 0.5)
            if case.swiglu:
                s[n_out:] = s[:n_out] * np.where(np.arange(n_out) % 2 == 0, 4.0, 0.25)
            inp.ws = torch.from_numpy(s.astype(np.float32))
            inp.wq = e4m3_bytes(w * 16.0)
        else:
            inp.wq, inp.ws = quant_rows_fp8(bf(w).float().numpy())
        inp.w = None
    else:
        inp.w = bf(w)
    inp.bias = bf(rng.standard_normal(n_out) * 0.5) if case.opt("bias") else None
    rr = lds(case).res_rows
    inp.res = bf(rng.standard_normal((rr, n_out)) * (1.0 + np.arange(rr))[:, None]) if case.opt("residual") else None
    return inp


# ---- float64 reference ----------------------------------------------------------------------------------------------------------------
def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F32).to(BF).to(F64).numpy()


def _silu(g):
    return g / (1.0 + np.exp(-g))


def _dsilu(g):
    s = 1.0 / (1.0 + np.exp(-g))
    return s * (1.0 + g * (1.0 - s))


def _erf(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v))).numpy()


def tie_delta(case):
    """Relative f32 error of the kernel's x * rstd (docstring, Ties), in units of 1."""
    K = case.shape[2]
    gemv_route = case.expect[0][0] == GEMV
    R = 8 * cdiv(K // 8, 256 if gemv_route else 64) + 6 + (3 if gemv_route else 0)
    return ((R + 3) / 2.0 + 3.0) * EPS


def kappa_product(case):
    rec = case.expect[0]
    K = case.shape[2]
    if rec[0] == GEMV:
        return (16 * cdiv(K // 16, 64) + 6 + 1) if rec[4] else (8 * cdiv(K // 8, 64) + 6)
    KS = rec[1]
    if rec[0] == SKINNY:
        return 2 * (K // KS // 64) + KS - 1
    return 4 * (K // KS // 128) + KS - 1 + 1


def reference(case, inp, mut=None):
    """NS(y [M, n_out] float64, tol, image / tol_image: the whole output buffer [GUARD + M + GUARD, ldy] with NaN where nothing may be
    written, tie_share).  `mut`: a named wrong kernel (MUTATIONS)."""
    M, N, K = case.shape
    n_out = case.n_out
    ld = lds(case)
    st = structure(case)
    x = f64(inp.x)
    extra_op = None
    tie_share = 0.0
    if case.norm:
        g = f64(inp.gain)
        div = ld.ldx if mut == "mean-over-ldx" else K
        ms = (x * x).sum(axis=1) / div
        rstd = 1.0 / np.sqrt(ms + (0.0 if mut == "eps-omitted" else float(np.float32(NORM_EPS))))
        if mut == "rstd-shared":
            rstd = np.full_like(rstd, rstd[0])
        u = x * rstd[:, None]
        if mut == "gain-before-cast":
            a = _bf16_round(u * g)
        else:
            xn = _bf16_round(u)
            a = _bf16_round(xn * g)
        au = np.abs(u)
        with np.errstate(divide="ignore"):
            ulp = np.where(au > 0, 2.0 ** (np.floor(np.log2(np.where(au > 0, au, 1.0))) - 7), 0.0)
        frac = np.where(ulp > 0, au / np.where(ulp > 0, ulp, 1.0) % 1.0, 0.0)
        marked = (np.abs(frac - 0.5) * ulp <= tie_delta(case) * au) & (au > 0)
        tie_share = float(marked.mean())
        extra_op = marked * ulp * np.abs(g)
        x = a
    # operand-side mutations: k multiplicities and k permutations of the x operand
    mult = np.ones(K)
    perm = np.arange(K)
    if mut == "last-chunk-dropped":
        k1 = st.slices[0][1]
        mult[k1 - (st.unit if st.family != GEMV else st.unit):k1] = 0.0
    elif mut == "wave-partial-dropped":
        k0, k1 = st.slices[min(1, st.KS - 1)]
        mult[k0:k1] = 0.0
    elif mut == "tail-dropped":
        mult[st.tail[0]:st.tail[1]] = 0.0
    elif mut == "early-sweep-twice":
        mult[st.early[0]:st.early[1]] = 2.0
    elif mut == "halves-swapped":
        h = st.lane_k // 2
        perm = perm.reshape(-1, 2, h)[:, ::-1, :].reshape(-1)
    xm = x[:, perm] * mult
    if case.w8:
        wv = e4m3_values(inp.wq)
        if mut == "w8-bytes-reversed":
            wv = wv.reshape(N, K // 4, 4)[:, :, ::-1].reshape(N, K)
        ws = f64(inp.ws).copy()
        if mut == "up-scale-from-gate" and case.swiglu:
            ws[n_out:] = ws[:n_out]
    else:
        wv, ws = f64(inp.w), None
    rows = np.arange(N)
    if case.swiglu and mut == "up-rows-offset":
        rows = np.concatenate([rows[:n_out], np.minimum(rows[n_out:] + 1, N - 1)])
    if mut == "clamp-row":                               # the last feature but one of the (partial) last tile reads row n_out - 1
        rows = rows.copy()
        rows[n_out - 2] = n_out - 1
    acc = np.empty((M, N))
    Mabs = np.empty((M, N))
    ext = np.zeros((M, N))
    for r0 in range(0, N, 2048):
        blk = wv[rows[r0:r0 + 2048]]
        sc = 1.0 if ws is None else ws[rows[r0:r0 + 2048]][None, :]
        acc[:, r0:r0 + 2048] = (xm @ blk.T) * sc
        Mabs[:, r0:r0 + 2048] = (np.abs(x) @ np.abs(blk).T) * sc
        if extra_op is not None:
            ext[:, r0:r0 + 2048] = (extra_op @ np.abs(blk).T) * sc
    a_lin = kappa_product(case) * EPS * Mabs
    act = case.opt("act")
    if act == ACT_SWIGLU:
        gte, up = acc[:, :n_out], acc[:, n_out:]
        a_g, a_u, e_g, e_u = a_lin[:, :n_out], a_lin[:, n_out:], ext[:, :n_out], ext[:, n_out:]
        if mut == "gate-up-swapped":
            gte, up = up, gte
        v = up * _silu(gte)
        a = np.abs(_silu(gte)) * a_u + np.abs(up * _dsilu(gte)) * a_g + EPS * (8.0 * np.abs(up * gte) + np.abs(v))
        ext = np.abs(_silu(gte)) * e_u + np.abs(up * _dsilu(gte)) * e_g
    else:
        v, a = acc, a_lin
        if inp.bias is not None:
            b = f64(inp.bias)[None, :].repeat(M, 0)
            if mut == "bias-skipped-last-tile":
                b[:, (n_out - 1) // 16 * 16:] = 0.0
            v = v + b
            a = a + EPS * (np.abs(v) + np.abs(b))
        if act == ACT_GELU_ERF:
            a = 1.13 * a + 16.0 * EPS * np.abs(v)
            ext = 1.13 * ext
            v = 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))
        elif act == ACT_GELU_TANH:
            a = 1.13 * a + 12.0 * EPS * np.abs(v)
            ext = 1.13 * ext
            v = 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    if inp.res is not None:
        mod = case.opt("res_row_mod")
        ridx = np.arange(M) % mod if (mod and mut != "row-mod-ignored") else np.arange(M)
        rimg = np.full((max(ld.res_rows, M) + GUARD_ROWS, ld.ldr), np.nan)
        rimg[:ld.res_rows, :n_out] = f64(inp.res)
        if mut == "residual-ldy":
            r = rimg.reshape(-1)[(ridx[:, None] * ld.ldy + np.arange(n_out)[None, :])]
        else:
            r = rimg[ridx][:, :n_out]
        v = v + r
        a = a + EPS * (np.abs(v) + np.abs(r))
    with np.errstate(invalid="ignore"):
        tol = 2.0 ** -8 * hb(np.abs(v) + a + ext) + a + ext + FLOOR
    image = np.full((GUARD_ROWS + M + GUARD_ROWS, ld.ldy), np.nan)
    image[GUARD_ROWS:GUARD_ROWS + M, :n_out] = v
    if mut == "row-beyond-m":
        image[GUARD_ROWS + M, :n_out] = v[M - 1]
    tol_image = np.zeros_like(image)
    tol_image[GUARD_ROWS:GUARD_ROWS + M, :n_out] = tol
    return NS(y=v, tol=tol, image=image, tol_image=tol_image, tie_share=tie_share)


def ratio(ref, got_image):
    """err / tol over the whole output buffer: inf where a protected element was written or a result is not finite."""
    got = np.asarray(got_image, dtype=np.float64)
    want = ref.image
    free = np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        r = np.where(err > 0, err / np.where(ref.tol_image > 0, ref.tol_image, 1e-300), 0.0)
    r = np.where(free, np.where(np.isnan(got), 0.0, np.inf), np.where(np.isfinite(got), r, np.inf))
    return r


def worst(ref, got_image):
    r = ratio(ref, got_image)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), (int(i[0]) - GUARD_ROWS, int(i[1]))


def image_of(case, y):
    """[M, n_out] values -> the output buffer image (NaN where nothing may be written)."""
    ld = lds(case)
    img = np.full((GUARD_ROWS + case.shape[0] + GUARD_ROWS, ld.ldy), np.nan)
    img[GUARD_ROWS:GUARD_ROWS + case.shape[0], :case.n_out] = np.asarray(y, dtype=np.float64)
    return img


def one_hot_expected(case, inp):
    """Routes without norm and without epilogue: y[m, n] = w[n, k_m] bit for bit (W8: bf16 of the f32 product w8 * scale)."""
    if case.w8:
        w = e4m3_values(inp.wq)[:, inp.hot].astype(np.float32) * inp.ws.numpy()[:, None]          # one f32 rounding
        return torch.from_numpy(np.ascontiguousarray(w.T)).to(BF)
    return inp.w[:, inp.hot].T.contiguous()


def f32_impl(case, inp):
    """A plain float32 torch implementation with the kernel's rounding points: it must sit inside every bar."""
    M, N, K = case.shape
    n_out = case.n_out
    x = inp.x.float()
    if case.norm:
        r = torch.rsqrt((x * x).sum(dim=1, keepdim=True) / K + NORM_EPS)
        x = ((x * r).to(BF).float() * inp.gain.float()).to(BF).float()
    # the product in the kernel's shape: one f32 rounding per MFMA-sized piece of K (per round of the 64 lanes' chunks for the GEMV), pieces
    # added in f32 in order, the slices of the KS waves folded in f32 - torch's own f32 matmul would bring its own, longer chain
    st = structure(case)
    piece = 64 * st.unit if st.family == GEMV else st.unit // (4 if case.w8 else 2)
    wt = (inp.wq.view(torch.float8_e4m3fn) if case.w8 else inp.w).to(F64).T
    xd = x.to(F64)
    acc = None
    for k0, k1 in st.slices:
        part = torch.zeros((M, N), dtype=F32)
        for k in range(k0, k1, piece):
            part = part + (xd[:, k:min(k + piece, k1)] @ wt[k:min(k + piece, k1)]).to(F32)
        acc = part if acc is None else acc + part
    if case.w8:
        acc = acc * inp.ws[None, :]
    act = case.opt("act")
    if act == ACT_SWIGLU:
        g, u = acc[:, :n_out], acc[:, n_out:]
        v = u * (g * torch.sigmoid(g))
    else:
        v = acc
        if inp.bias is not None:
            v = v + inp.bias.float()
        if act == ACT_GELU_ERF:
            v = torch.nn.functional.gelu(v)
        elif act == ACT_GELU_TANH:
            v = torch.nn.functional.gelu(v, approximate="tanh")
    if inp.res is not None:
        mod = case.opt("res_row_mod")
        idx = torch.arange(M) % mod if mod else torch.arange(M)
        v = v + inp.res.float()[idx]
    return v.to(BF)


# ---- mutations: name -> (case id, family) on which the mutated reference must exceed the bar by MIN_RATIO -----------------------------
MUTATIONS = {
    "last-chunk-dropped": [("skinny-ks8-swiglu", "one-sign"), ("gemv-m3-ladder", "sentinel"), ("w8-ks4-ladder", "sentinel")],
    "wave-partial-dropped": [("skinny-ks8-m2", "one-sign"), ("norm-ks8-above-up", "norm-one-sign"), ("w8-ks8", "one-sign")],
    "tail-dropped": [("gemv-m1-ladder", "sentinel"), ("skinny-ks1-ladder", "sentinel"), ("gemv-w8-ladder", "sentinel"), ("w8-ks2-k768", "one-sign")],
    "early-sweep-twice": [("gemv-m1-pre-k%d" % (PRE_K + 8), "one-sign"), ("gemv-m1-norm-pre-k%d" % PRE_K, "norm-one-sign"),
                          ("norm-ks8-above-up", "norm-sentinel")],
    "gate-up-swapped": [("gemv-m1-swiglu", "one-sign"), ("skinny-ks1-swiglu-ladder", "sentinel"), ("w8-ks4-swiglu", "one-sign")],
    "up-rows-offset": [("gemv-m2-swiglu-ladder", "sentinel"), ("norm-ks4-swiglu", "norm-sentinel"), ("gemv-w8-swiglu", "sentinel")],
    "up-scale-from-gate": [("gemv-w8-swiglu", "sentinel"), ("w8-ks4-swiglu", "sentinel"), ("w8-norm-ks4-swiglu", "norm-sentinel")],
    "w8-bytes-reversed": [("gemv-w8-k48", "sentinel"), ("w8-ks2", "sentinel"), ("w8-ks2", "one-hot")],
    "halves-swapped": [("skinny-ks4-m3", "sentinel"), ("skinny-ks4-m3", "one-hot"), ("w8-ks4-short", "sentinel")],
    "clamp-row": [("skinny-ks8-m2", "sentinel"), ("gemv-m5-k", "sentinel"), ("w8-ks4-ladder", "sentinel")],
    "row-beyond-m": [("skinny-ks4-m3", "one-sign"), ("gemv-m2-nout", "one-sign"), ("w8-ks2-k768", "one-sign")],
    "bias-skipped-last-tile": [("skinny-ks8-m2", "one-sign"), ("gemv-m4-ldy", "one-sign"), ("w8-ks4-ladder", "one-sign")],
    "row-mod-ignored": [("skinny-ks4-m3", "one-sign"), ("gemv-m5-k", "one-sign"), ("w8-ks4-short", "one-sign")],
    "residual-ldy": [("skinny-ks4-m3", "one-sign"), ("gemv-m7-ldy", "one-sign"), ("w8-ks4-swiglu", "one-sign")],
    "gain-before-cast": [("norm-ks8-at-up", "norm-one-sign"), ("gemv-m3-norm", "norm-one-sign")],
    "rstd-shared": [("norm-ks8-at-up", "norm-one-sign"), ("gemv-m3-norm", "norm-sentinel"), ("w8-norm-ks4", "norm-one-sign")],
    "eps-omitted": [("norm-ks8-at-up", "norm-one-sign"), ("gemv-m1-norm-swiglu", "norm-one-sign"), ("w8-norm-ks8", "norm-one-sign")],
    "mean-over-ldx": [("norm-ks4-below-up", "norm-one-sign"), ("gemv-m1-norm-pre-k%d" % PRE_K, "norm-one-sign")],
}


# ---- structural corners: name -> the ids of the cases that reach it (from the records and structure(), not from the comments) ---------
def corners():
    out = {}

    def reach(name, pred):
        out[name] = [c.id for c in CASES if c.runs and c.expect and pred(c, c.expect[0], structure(c))]

    for m in range(1, 9):
        reach(f"gemv M={m}", lambda c, r, s, m=m: r[0] == GEMV and r[1] == m)
    reach("gemv M>=2 by K % 64", lambda c, r, s: r[0] == GEMV and r[1] >= 2 and not c.norm and c.shape[2] % 64 != 0)
    reach("gemv M>=2 by n_out % 4", lambda c, r, s: r[0] == GEMV and r[1] >= 2 and c.shape[2] % 64 == 0 and c.n_out % 4 != 0)
    reach("gemv M>=2 by ldy % 4", lambda c, r, s: r[0] == GEMV and r[1] >= 2 and c.shape[2] % 64 == 0 and c.n_out % 4 == 0 and lds(c).ldy % 4 != 0)
    for m in (1, 2):
        reach(f"gemv M={m} FPW=2 just below the threshold", lambda c, r, s, m=m: r[:2] == (GEMV, m) and r[3] == 2 and c.n_out == KC["FPW4_N"] - 1)
        reach(f"gemv M={m} FPW=4 at the threshold", lambda c, r, s, m=m: r[:2] == (GEMV, m) and r[3] == 4 and c.n_out == KC["FPW4_N"])
    reach("gemv M>=3 above the FPW threshold stays FPW=2", lambda c, r, s: r[0] == GEMV and r[1] >= 3 and r[3] == 2 and c.n_out >= KC["FPW4_N"])
    reach("gemv SwiGLU", lambda c, r, s: r[0] == GEMV and r[2] == 1)
    for norm in (0, 1):
        t = " with norm" if norm else ""
        reach("gemv no early sweep at K = threshold - 8" + t, lambda c, r, s, n=norm: r[:2] == (GEMV, 1) and r[5] == n and c.shape[2] == PRE_K - 8 and not s.pre)
        reach("gemv early sweep and nothing left" + t, lambda c, r, s, n=norm: r[:2] == (GEMV, 1) and r[5] == n and c.shape[2] == PRE_K and s.rungs == {"pre"})
        reach("gemv early sweep then a one-lane tail" + t, lambda c, r, s, n=norm: r[:2] == (GEMV, 1) and r[5] == n and c.shape[2] == PRE_K + 8 and s.rungs == {"pre", 1})
    reach("gemv nchunk % 64 != 0", lambda c, r, s: r[0] == GEMV and not r[4] and (c.shape[2] // 8) % 64 != 0 and c.shape[2] > 512)
    reach("gemv rungs 8/4/2/1", lambda c, r, s: r[0] == GEMV and not r[4] and {8, 4, 2, 1} <= s.rungs)
    reach("gemv rungs 4/2/1 at NR > 2 (SwiGLU)", lambda c, r, s: r[0] == GEMV and not r[4] and r[2] == 1 and {4, 2, 1} <= s.rungs and 8 not in s.rungs)
    reach("gemv rungs 4/2/1 at NR > 2 (FPW=4)", lambda c, r, s: r[0] == GEMV and r[3] == 4 and {4, 2, 1} <= s.rungs and 8 not in s.rungs)
    reach("gemv n_out odd", lambda c, r, s: r[0] == GEMV and c.n_out % 2 == 1)
    reach("gemv n_out % (4 FPW) != 0 at FPW=4", lambda c, r, s: r[0] == GEMV and r[3] == 4 and c.n_out % 16 != 0)
    reach("gemv per > 1", lambda c, r, s: r[0] == GEMV and r[7] > 1)
    reach("gemv per > 1 with a short last list", lambda c, r, s: r[0] == GEMV and r[7] > 1 and cdiv(c.n_out, 4 * r[3]) % r[6] != 0)
    reach("gemv M K at the LDS limit", lambda c, r, s: r[0] == GEMV and c.shape[0] * c.shape[2] == KC["GEMV_MK"])
    reach("gemv W8 K % 16 only", lambda c, r, s: r[0] == GEMV and r[4] == 1 and c.shape[2] % 64 != 0)
    reach("gemv W8 rungs 4/2/1", lambda c, r, s: r[0] == GEMV and r[4] == 1 and {4, 2, 1} <= s.rungs)
    reach("gemv W8 SwiGLU", lambda c, r, s: r[0] == GEMV and r[4] == 1 and r[2] == 1)
    reach("gemv W8 norm", lambda c, r, s: r[0] == GEMV and r[4] == 1 and r[5] == 1)
    reach("gemv norm at M >= 2", lambda c, r, s: r[0] == GEMV and r[1] >= 2 and r[5] == 1)
    for ks in (8, 4, 2, 1):
        reach(f"skinny KS={ks} by K", lambda c, r, s, ks=ks: r[:2] == (SKINNY, ks) and not r[4] and cdiv(c.n_out, 16) < KC["T8"] - 1)
    reach("skinny tiles = T8 - 1 -> KS 8", lambda c, r, s: r[:2] == (SKINNY, 8) and cdiv(c.n_out, 16) == KC["T8"] - 1)
    reach("skinny tiles = T8 -> KS 4", lambda c, r, s: r[:2] == (SKINNY, 4) and not r[4] and cdiv(c.n_out, 16) == KC["T8"] and c.shape[2] % KC["K8"] == 0)
    reach("skinny tiles = T4 - 1 -> KS 4", lambda c, r, s: r[:2] == (SKINNY, 4) and cdiv(c.n_out, 16) == KC["T4"] - 1)
    reach("skinny tiles = T4 -> KS 2", lambda c, r, s: r[:2] == (SKINNY, 2) and cdiv(c.n_out, 16) == KC["T4"] and c.shape[2] % KC["K4"] == 0)
    for m in (2, 3, 8, 9, 15, 16):
        reach(f"skinny M={m}", lambda c, r, s, m=m: r[0] == SKINNY and c.shape[0] == m)
    for rem in (4, 8, 12):
        reach(f"skinny n_out % 16 = {rem}", lambda c, r, s, rem=rem: r[0] == SKINNY and c.n_out % 16 == rem)
    reach("skinny rungs 8/4/2/1", lambda c, r, s: r[0] == SKINNY and not r[2] and {8, 4, 2, 1} <= s.rungs)
    reach("skinny SwiGLU rungs 4/2/1", lambda c, r, s: r[0] == SKINNY and r[2] == 1 and {4, 2, 1} <= s.rungs)
    for ks in (8, 4):
        reach(f"skinny NORM KS={ks}", lambda c, r, s, ks=ks: r[:2] == (SKINNY, ks) and r[4] == 1)
    for sw in (0, 1):
        UP = KC["UP_SWIGLU"] if sw else KC["UP"]
        for name, cmp in (("<", lambda n, u: n < u), ("==", lambda n, u: n == u), (">", lambda n, u: n > u)):
            reach(f"skinny NORM{' SwiGLU' if sw else ''} nsteps {name} UP", lambda c, r, s, sw=sw, cmp=cmp, UP=UP:
                  r[0] == SKINNY and r[4] == 1 and r[2] == sw and cmp(c.shape[2] // r[1] // 64, UP) and s.pre == (c.shape[2] // r[1] // 64 >= UP))
    reach("skinny NORM M < KS", lambda c, r, s: r[0] == SKINNY and r[4] == 1 and c.shape[0] < r[1])
    reach("skinny NORM M > KS", lambda c, r, s: r[0] == SKINNY and r[4] == 1 and c.shape[0] > r[1])
    reach("skinny NORM M = 8, K = the limit", lambda c, r, s: r[0] == SKINNY and r[4] == 1 and c.shape[0] == 8 and c.shape[2] == KC["NORM_MAX_K"] and r[8] == 8 * (2 * KC["NORM_MAX_K"] + 16))
    reach("skinny NORM rows smaller than the reduction area", lambda c, r, s: r[0] == SKINNY and r[4] == 1 and c.shape[0] * (2 * c.shape[2] + 16) < r[1] * 2048 == r[8])
    for ks in (8, 4, 2):
        reach(f"w8 KS={ks}", lambda c, r, s, ks=ks: r[:2] == (SKINNY_W8, ks) and not r[4])
    reach("w8 K % 1024 == 0 but short -> KS 4", lambda c, r, s: r[:2] == (SKINNY_W8, 4) and c.shape[2] % KC["W8_K8"] == 0 and c.shape[2] // 8 < KC["W8_K8_MIN"])
    reach("w8 tiles = T8 -> KS 4", lambda c, r, s: r[:2] == (SKINNY_W8, 4) and cdiv(c.n_out, 16) == KC["T8"] and c.shape[2] % KC["W8_K8"] == 0 and c.shape[2] // 8 >= KC["W8_K8_MIN"])
    reach("w8 tiles = T4 -> KS 2", lambda c, r, s: r[:2] == (SKINNY_W8, 2) and cdiv(c.n_out, 16) == KC["T4"] and c.shape[2] % KC["W8_K4"] == 0)
    for ks in (8, 4):
        reach(f"w8 NORM KS={ks}", lambda c, r, s, ks=ks: r[:2] == (SKINNY_W8, ks) and r[4] == 1)
    reach("w8 rungs 4/2/1", lambda c, r, s: r[0] == SKINNY_W8 and not r[2] and {4, 2, 1} <= s.rungs)
    reach("w8 SwiGLU rungs 2/1", lambda c, r, s: r[0] == SKINNY_W8 and r[2] == 1 and {2, 1} <= s.rungs)
    for fam, name in ((GEMV, "gemv"), (SKINNY, "skinny"), (SKINNY_W8, "w8")):
        f = lambda c, r, fam=fam: r[0] == fam or (fam == SKINNY_W8 and r[0] == GEMV and r[4] == 1 and False)
        reach(f"{name} bias", lambda c, r, s, f=f: f(c, r) and c.opt("bias"))
        reach(f"{name} GELU-erf", lambda c, r, s, f=f: f(c, r) and c.opt("act") == G1)
        reach(f"{name} GELU-tanh", lambda c, r, s, f=f: f(c, r) and c.opt("act") == G2)
        reach(f"{name} residual", lambda c, r, s, f=f: f(c, r) and c.opt("residual"))
        reach(f"{name} res_row_mod in 1..M-1", lambda c, r, s, f=f: f(c, r) and 1 <= c.opt("res_row_mod") < c.shape[0])
        for pad in ("ldx_pad", "ldw_pad", "ldy_pad", "ldr_pad"):
            reach(f"{name} {pad}", lambda c, r, s, f=f, pad=pad: f(c, r) and c.opt(pad) > 0)
        reach(f"{name} SwiGLU with residual", lambda c, r, s, f=f: f(c, r) and c.swiglu and c.opt("residual"))
    out["refusal: W8, M >= 2, K % 256 != 0"] = [c.id for c in CASES if c.status == ERR_UNSUPPORTED and c.entry == "linear_w8" and c.shape[0] >= 2 and c.shape[2] % 256]
    out["refusal: W8 NORM, tiles >= T4"] = [c.id for c in CASES if c.status == ERR_UNSUPPORTED and c.entry == "linear_w8_norm" and cdiv(c.n_out, 16) >= KC["T4"]]
    out["one chunk beyond the LDS limit is refused"] = [c.id for c in CASES if c.status == ERR_UNSUPPORTED and c.entry == "linear" and c.shape[0] * c.shape[2] == KC["GEMV_MK"] + 8 * c.shape[0]]
    out["beyond the LDS limit falls through to the MFMA GEMM"] = [c.id for c in CASES if c.gemm and c.shape[0] * c.shape[2] > KC["GEMV_MK"]]
    out["NORM refusals land on the GEMV"] = [c.id for c in CASES if c.entry == "decode_linear" and c.shape[0] >= 2 and c.expect and c.expect[0][0] == GEMV]
    return out

"""Case tables, input families, float64 references, bars and reference mutations of the normalisation folded into the bf16 GEMM
(aki_amd/csrc/gemm_bf16.hip): the PRODUCER - the statistics block of gemm_bf16_kernel: the per-lane sums in write_rows, the write-through
partials behind the arrival counter, the last tile's fold through LDS - and the CONSUMER, the line v = (acc - mu * colc) * rs.

numpy and CPU torch only.  tests/test_norm_fold_cases_cpu.py checks the table itself - every structural edge reached (from the constants
parsed out of gemm_bf16.hip), every route the one the lab library's dry run shows, every reference against a float64 torch norm + linear,
a plain float32 restatement of the kernel's summation order inside every producer bar, every mutation visible - and
tests/test_norm_fold_f64_gpu.py runs every case on the device.

Tile configurations (tile_configs()).  Every launch_gemm<NF, NT, WN, WM, .., NST, PIPE, SK> an EPI_PLAIN bf16 launch can reach is parsed out
of launch_small, launch_big, launch_small_m and run_planned:  BN = 16 NF WN features x BM = 16 NT WM tokens; a SLOT is one wave column of
one tile column (slot = tn * WN + wn, 16 NF features wide), a lane adds 4 NF values, and the last tile of a row panel folds
CH = (NST * (BN + BM) * 128 - 16) / (BM * 8) slots per pass through LDS.
    256x256 (PIPE 4 / 5 / 6)  CH 63      128x128 two stages  CH 63      128x128 four stages  CH 127     64x128 four stages  CH 95
    128x96 (PIPE 8)           CH 74      128x96 split-K      CH 74      128x64 split-K       CH 143     64x64 four stages   CH 127
WN = 2 everywhere, so a launch has an even number of slots: where CH is odd the table holds the largest launch of one pass (CH - 1 slots)
and the second pass with a single slot (CH + 1); where it is even, CH and CH + 2.  The planner's own limits keep some edges out of reach,
and the CPU test computes which: split-K needs n_out <= 4096 (<= 64 slots: one pass), the 128x64 split M <= 256 (four panels), the
four-stage rings of launch_small M <= 128 (one panel), and the 128-feature ring more than 128 tiles (>= 258 slots: three passes).

Producer cases (PRODUCER).  (id, lab tile mode, M, N, K, ln, eps, epilogue, family, launches, edge).  K is 64 to 256 except on split-K
(2304).  The stored y is steered through the residual with x = 0 in the families that need exact values ('res' families) and comes out of
a real GEMM otherwise; the reference always reads the y the device stored.
  plain       x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0, 1/4), residual ~ N(0, 1): through the GEMM.
  offset-R    rows of mean R standard deviations, R = 4, 32, 128, the sign alternating and the scale 2^(m % 3 - 1).
  constant    every element of a row equal (another bf16 value per row): the true variance is 0, the device's the clamp or rounding noise.
  zero        even rows zero - rstd is rsqrt(eps), the mean exactly 0 - odd rows N(0, 1).
  spike       2^-6 everywhere and one feature of 2^6.  Rows m % 8 == 0 carry it at the position the case names (first slot, last slot,
              slot CH - 1, slot CH, the last valid feature), the other rows one slot each in turn: every slot's partial is visible alone
              (the one-panel rings have fewer rows than slots above 112 slots).
  zero-sum    +a, -a pairs: s1 cancels exactly.
  row-ladder  N(0, 1) rows scaled 2^-12 .. 2^12: a neighbouring row's statistics are wrong by a factor.
sum y^2 stays below 2^100 (the CPU test asserts it).

Producer reference and bar.  In float64 on the stored bf16 y:  mu = mean(y), v = mean((y - mu)^2) + eps (LayerNorm), v = mean(y^2) + eps
(RMSNorm), eps the f32 value the ABI receives.  The device is held on mean and on 1 / rstd^2 - the error of s2 / n - mean^2 is absolute
in v, and the form stays meaningful on a constant row:
    |mean_dev - mu|     <= K_mean 2^-24 mean|y|
    |1 / rstd_dev^2 - v| <= 2^-24 (K_sq mean(y^2) + K_cross |mu| mean|y|) + K_rsqrt 2^-24 v
Derivation, operation by operation (first order, units of 2^-24 = one f32 operation rounded to nearest):
    s1 of a lane   4 NF sequential additions of exact bf16 values                                   4 NF        on sum|y|
    s2 of a lane   one product per square (1; an FMA has none) and 4 NF additions                    4 NF + 1    on sum y^2
    the wave       two shuffle additions (xor 16, xor 32)                                            + 2
    the fold       `slots` sequential additions down the parked column                               + slots
    1 / n          inv_n = 1.0f / n rounded (1), the product by it (1)                               + 2
  K_mean  = 4 NF + 2 + slots + 2.          s2 / n: 4 NF + 1 + 2 + slots + 2.
    mean * mean    d(mean^2) = 2 |mu| d(mean) + the product's rounding of mu^2 <= |mu| mean|y|:  K_cross = 2 K_mean + 1  on |mu| mean|y|
    subtraction    one rounding of a value <= mean(y^2):                                         K_sq = 4 NF + slots + 5 + 1 (LN; RMS: + 0)
    fmaxf(.., 0)   moves the value towards the truth (var >= 0): nothing
    + eps          one rounding of v (1);  rsqrtf: 1 ulp = 2 units on rstd, 4 on 1 / rstd^2:     K_rsqrt = 5
RMS rows are the same form with mu = 0 (no cross term, no subtraction).  Nothing is tuned on a kernel's output.
Consequence.  With r = |mean| / std of a row, mean(y^2) = (1 + r^2) std^2 and |mu| mean|y| ~ r^2 std^2 while v ~ std^2: the two cancelling
terms s2 / n and mean^2 are each r^2 times the variance and each carries its own rounding, so the relative error of the GEMM-produced
rstd grows as 1 + 2 (mean/std)^2 (half the relative error of v); aki_row_stats (two-pass variance) has no such growth.  The restated-f32
model below (kernel_stats_f32: the kernel's summation order in numpy float32), measured by the CPU test against float64, worst relative
error of rstd over 64 rows, 64x128 tile:
    mean/std      0        4        16       32       64       128
    N = 1152    1.5e-07  2.1e-06  3.0e-05  1.5e-04  5.7e-04  2.3e-03
    N = 3072    2.4e-07  3.0e-06  6.2e-05  2.3e-04  8.5e-04  2.6e-03
(the figures the CPU test prints; each is inside the bound 0.5 2^-24 (K_sq (1 + r^2) + K_cross r^2 + K_rsqrt)).  The bar is a worst-case
bound, not the expected accuracy: every rounding is counted at its full size and with one sign, so it lies about 30 times above the
restated-f32 error at every ratio (4.9e-3 against 1.5e-4 at ratio 32, N = 1152), and a correct device uses 0.05 to 0.4 of it.
Measured on an MI355X by tests/test_norm_fold_f64_gpu.py (LayerNorm offset cases, worst relative error of rstd, N = 60 .. 16512): 1.6e-6 to
7.1e-6 at 4 standard deviations, 3.5e-5 to 3.1e-4 at 32, 6.0e-4 to 5.0e-3 at 128 - the restatement's figures, and never above 0.1 of the bar.  At 128 the error
exceeds a bf16 half-ulp (2^-9 = 1.95e-3), and the rtol = 3e-5 of the older tests is the error at 16 standard deviations.

Consumer cases (CONSUMER).  ops.linear with row_scale alone (plain and SwiGLU epilogues) and with row_scale + row_shift + col_shift (plain,
bias, GELU-tanh, residual), forced tiles and the planner's routes, tile-interior (the straight-line variants: keys 8 and 25) and tail shapes
(the run-time path), K in {64, 256, 1152}.  Operands are exact: bf16 x and w', f32 rs, mu, c handed in directly.
  x0 / x4 / x32   x rows of mean 0, 4, 32 standard deviations (sign alternating); mu the f32 row mean, rs 1 / std, c the f32 row sums of w'.
  wmean           w' with a column mean of 8 standard deviations and x rows of mean 4: mu c is many times the result.
  ladder          rs = 2^(m % 21 - 10).
  mu and c have mixed signs in every family (alternating row means, feature-wise signs of the column mean).
Reference: rs (x w'^T - mu c) [+ bias -> act] [+ res] in float64.  Bar: the house form tol = half_ulp_bf16(|ref| + a) + a + floor (Out of
tests/train_kernel_cases.py, imported), a = KAPPA 2^-24 M, M = rs (sum_k |x_k w'_k| + |mu c|) + |bias| + |res|.
  KAPPA   the MFMA accumulation as tests/gemm_tn_cases.py counts it - one f32 rounding per accumulated term whatever the order, K in all
          (tests/decode_linear_cases.py counts one per MFMA, 2 per 64 k: the smaller figure, inside this one) - the split-K fold has no
          consumer with row_shift; + the product mu c (1), the subtraction (1), the product by rs (1):  KAPPA = K + 3.
          bias: + 2^-24 (|v| + |b|).  GELU-tanh (gelu_tanh_fast): the pre-activation's error passes with |gelu'| <= 1.13, + 12 2^-24 |v|
          (decode_linear_cases.py).  residual: + 2^-24 (|v| + |r|).  SwiGLU y = u silu(g): a = |silu(g)| a_u + |u silu'(g)| a_g +
          2^-24 (8 |u g| + |y|).
QKV + RoPE with row_scale stays with the route tests.

Chained cases (CHAINED).  A producer launch leaves its statistics, a consumer launch applies them: LayerNorm at row means of 0, 4 and 32
standard deviations, RMSNorm plainly.  Reference: norm-then-linear of the stored intermediate in float64, on the rounded w' and b' the
device multiplies.  Bar: the consumer's bar with the float64 statistics, plus the producer's bars propagated to first order:
|d rstd| = rstd^3 dv / 2, so  + |d rstd| |x w'^T - mu c| + rstd d mean |c| + rstd |mu| dc, dc = K 2^-24 sum_k |w'_k| the f32 summation error
of fold_layernorm's c, which is also held to the float64 row sums of the ROUNDED w' within dc.

Mutations (PRODUCER_MUTATIONS, CONSUMER_MUTATIONS) are named changes to the reference; a mutated reference stands in for the device and
must exceed the bar by MIN_RATIO (train_kernel_cases.py) on the case listed with it.
"""
import math
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import torch

import gemm_routes as R
from train_kernel_cases import BF, EPS, FLOOR, MIN_RATIO, ROOT, Out, bf, f64, rng_of      # the bar's pieces are imported, not copied

GM = 8
SPLITK_MAX_N, SPLITK_MIN_K = 4096, 2304
ACT_NONE, ACT_GELU_TANH, ACT_SWIGLU = R.ACT_NONE, R.ACT_GELU_TANH, R.ACT_SWIGLU
K_RSQRT = 5.0


# ---- constants from the source -------------------------------------------------------------------------------------------------------
def _body(src, name):
    m = re.search(r"static int %s\(GemmParams& p[^)]*\)\s*\{" % name, src)
    assert m, f"{name} not found in gemm_bf16.hip"
    end = src.index("\n}\n", m.end())
    return src[m.end():end]


def _launches(text):
    out = set()
    for m in re.finditer(r"launch_gemm<([^>]*)>\(", text):
        a = [s.strip() for s in m.group(1).split(",")]
        assert a[4:6] == ["EPI", "ACT"] and a[6] in ("FP8", "false"), f"launch_gemm<{m.group(1)}>: unexpected arguments"
        tail = [int(s) for s in a[7:]] + [None] * 3
        out.add(tuple(int(s) for s in a[:4]) + (2 if tail[0] is None else tail[0], tail[1] or 0, tail[2] or 0))
    return out


def kernel_constants():
    """The statistics block's constants as gemm_bf16.hip is compiled, and every (NF, NT, WN, WM, NST, PIPE, SK) an EPI_PLAIN bf16 launch can
    reach.  A changed formula or a new instantiation fails here (an error, not a skip) instead of leaving the table beside the kernel."""
    with open(os.path.join(ROOT, "aki_amd", "csrc", "gemm_bf16.hip")) as f:
        src = f.read()
    for what in (r"constexpr int WROWS = NF \* 16;", r"constexpr int BN = WN \* WROWS;", r"constexpr int WTOK = NT \* 16;", r"constexpr int BM = WM \* WTOK;",
                 r"constexpr int ROWS = BN \+ BM;", r"constexpr int STAGE_BYTES = ROWS \* 128;",
                 r"constexpr int CH = \(NST \* STAGE_BYTES - 16\) / \(BM \* 8\);", r"const int slots = p\.tiles_n \* WN;",
                 r"p\.st_part \+ \(size_t\)\(tn \* WN \+ wn\) \* p\.M \+ mrow", r"s1 \+= __shfl_xor\(s1, 16\); s2 \+= __shfl_xor\(s2, 16\);",
                 r"s1 \+= __shfl_xor\(s1, 32\); s2 \+= __shfl_xor\(s2, 32\);", r"const float inv_n = 1\.0f / \(float\)n_out;",
                 r"rsqrtf\(fmaxf\(s2 \* inv_n - mean \* mean, 0\.f\) \+ p\.st_eps\)", r"rsqrtf\(s2 \* inv_n \+ p\.st_eps\)",
                 r"v\[n\]\[r\] = \(acc\[n\]\[m\]\[r\] - mu \* colc4\[n\]\[r\]\) \* rs;"):
        assert re.search(what, src), f"gemm_bf16.hip no longer holds /{what}/: the case table restates it"
    m = re.search(r"constexpr int GM = (\d+);", src)
    assert m and int(m.group(1)) == GM, "the row-panel grouping GM changed"
    big = _body(src, "launch_big")
    assert "if constexpr (FP8)" in big and "} else {" in big, "launch_big: the fp8 / bf16 branches not found"
    small_m = _body(src, "launch_small_m")
    assert "else if constexpr (ACT == 0)" in small_m, "launch_small_m: the plain branch not found"
    reach = _launches(_body(src, "launch_small")) | _launches(big.split("} else {", 1)[1]) | _launches(small_m.split("else if constexpr (ACT == 0)", 1)[1]) \
        | _launches(_body(src, "run_planned"))
    assert reach, "no launch_gemm instantiation parsed out of gemm_bf16.hip"
    return NS(reach=reach)


def _config(NF, NT, WN, WM, NST, SK, pipes):
    BN, BM = WN * NF * 16, WM * NT * 16
    return NS(NF=NF, NT=NT, WN=WN, WM=WM, NST=NST, SK=SK, pipes=tuple(sorted(pipes)), BN=BN, BM=BM, lane=4 * NF, slot_w=16 * NF,
              CH=(NST * (BN + BM) * 128 - 16) // (BM * 8), tile=f"{BN}x{BM}")


def tile_configs():
    """name -> configuration; PIPE variants of one tile share their statistics block (CH does not depend on PIPE)."""
    groups = {}
    for NF, NT, WN, WM, NST, PIPE, SK in kernel_constants().reach:
        groups.setdefault((NF, NT, WN, WM, NST, SK), set()).add(PIPE)
    out = {}
    for (NF, NT, WN, WM, NST, SK), pipes in groups.items():
        c = _config(NF, NT, WN, WM, NST, SK, pipes)
        c.name = c.tile + ("-sk" if SK else f"-ring{NST}" if NST > 2 else "")
        assert c.name not in out, f"two configurations named {c.name}"
        out[c.name] = c
    return out


CFG = tile_configs()
EXPECTED_CONFIGS = {"256x256": (63, (4, 5, 6)), "128x128": (63, (0,)), "128x128-ring4": (127, (0,)), "64x128-ring4": (95, (0,)), "128x96": (74, (8,)),
                    "128x96-sk": (74, (0,)), "128x64-sk": (143, (0,)), "64x64-ring4": (127, (0,))}


def slots_of(cfg, n_out):
    return cfg.WN * ((n_out + cfg.BN - 1) // cfg.BN)


def k_mean(cfg, slots):
    return 4.0 * cfg.NF + 2 + slots + 2


def k_sq(cfg, slots, ln):
    return 4.0 * cfg.NF + 1 + 2 + slots + 2 + (1 if ln else 0)


def k_cross(cfg, slots):
    return 2.0 * k_mean(cfg, slots) + 1


# ---- the producer table ----------------------------------------------------------------------------------------------------------------
class PCase:
    """epi: subset of {'bias', 'residual', 'gelu', 'fold-rms', 'fold-ln', 'w2'}; launches: ((config name, PIPE, ksplit, rows, first row), ...)."""

    def __init__(self, id, mode, M, N, K, ln, family, launches, edge, epi=("residual",), arg=None, eps=None):
        self.id, self.mode, self.M, self.N, self.K, self.ln, self.family, self.launches, self.edge = id, mode, M, N, K, ln, family, launches, edge
        self.epi, self.arg = frozenset(epi), arg
        self.eps = (1e-6 if ln else 1e-5) if eps is None else eps
        self.cfg = CFG[launches[0][0]]
        self.act = ACT_GELU_TANH if "gelu" in self.epi else ACT_NONE
        self.exact = family != "plain"                        # y steered through the residual, x = 0
        assert not self.exact or "residual" in self.epi, f"{id}: a steered family needs the residual"

    def __repr__(self):
        return self.id

    def cfg_of_row(self, m):
        for name, _, _, rows, first in self.launches:
            if first <= m < first + rows:
                return CFG[name]
        raise IndexError(m)

    @property
    def records(self):
        out = []
        for name, pipe, ks, rows, first in self.launches:
            c = CFG[name]
            grid = ((rows + c.BM - 1) // c.BM) * ((self.N + c.BN - 1) // c.BN) * ks
            out.append((c.NF, c.NT, c.WN, c.WM, R.EPI_PLAIN, self.act, 0, c.NST, pipe, c.SK, ks, rows, first, grid))
        return out

    def route(self):
        """The gemm_routes.Route of this launch, for the lab library's dry run."""
        o = dict(bias="bias" in self.epi, residual="residual" in self.epi, act=self.act, stats="ln" if self.ln else "rms")
        if "fold-rms" in self.epi or "fold-ln" in self.epi:
            o["fold"] = "ln" if "fold-ln" in self.epi else "rms"
        if "w2" in self.epi:
            o["w2"] = w2_row0(self.N)
        return R.Route(self.id, "linear", (self.M, self.N, self.K), tuple(self.records), opts=o)


def w2_row0(N):
    return N // 2 // 4 * 4 + 4


def _single(name, M, pipe=0, ks=1):
    return ((name, pipe, ks, M, 0),)


def slot_edges(cfg):
    """(slots of the largest one-pass launch, slots of the smallest launch with a second pass): both even (WN = 2)."""
    one = cfg.CH // cfg.WN * cfg.WN
    return one, one + cfg.WN


LN_FAMILIES = ("offset-4", "offset-32", "offset-128", "zero-sum", "constant")
FORCED = {"256x256": 1, "128x128": 2, "128x128-ring4": 2, "64x128-ring4": 2, "128x96": 3, "64x64-ring4": 5}       # aki_lab_set_gemm_tile
SPIKES = ("first", "last", "ch-1", "ch", "tail")


def _producer():
    out = []
    fams = ["offset-4", "row-ladder", "constant", "offset-32", "zero-sum", "zero", "offset-128", "plain"]
    nfam = [0]

    def fam():
        nfam[0] += 1
        return fams[nfam[0] % len(fams)]

    def add(id, name, M, N, K, edge, family=None, ln=None, pipe=None, ks=1, mode=None, **kw):
        family = family or fam()
        if ln is None:         # the kind follows the family: offset, zero-sum and constant rows are about the mean and s2 / n - mean^2, LayerNorm's alone
            ln = True if family in LN_FAMILIES else len(out) % 2 == 0
        epi = kw.get("epi", ("residual",))
        c = CFG[name]
        if pipe is None:
            pipe = c.pipes[0] if len(c.pipes) == 1 else (5 if "residual" in epi and N % 8 == 0 and "gelu" not in epi and "fold-ln" not in epi else 4)
        out.append(PCase(id, FORCED.get(name, 0) if mode is None else mode, M, N, K, ln, family, _single(name, M, pipe, ks), edge, **kw))

    # ---- the tiles the lab library can force: 256x256, 128x128, 128x96 (PIPE 8), 64x64 ----
    for name in ("256x256", "128x128", "128x96", "64x64-ring4"):
        c = CFG[name]
        K = 128 if name == "128x128" else 64          # (the 128x128 tile at M <= 128 stays on two stages below K = 256)
        add(f"{name}-m1-n60", name, 1, 60, K, "one tile column, M < BM, M % BM == 1, n_out % 64 == 60 (narrow stores)")
        add(f"{name}-one-column", name, c.BM - 1, c.BN, K, "one tile column, M % BM == BM - 1, M < BM")
        add(f"{name}-m+1-n+4", name, c.BM + 1, c.BN + 4, K, "M % BM == 1 behind a full panel; n_out % 64 == 4: p.wide off, a last slot of 4 features")
        add(f"{name}-m-1-n+8", name, 2 * c.BM - 1, c.BN + 8, K, "M % BM == BM - 1 behind a full panel; n_out % 64 == 8: the fin mask on 16-byte stores")
        add(f"{name}-9panels-n+20", name, 9 * c.BM - 3, 2 * c.BN + 20, K, "nine row panels: a full group of GM = 8 and a group of one; n_out % 64 == 20")
        add(f"{name}-11panels-plain", name, 10 * c.BM + 5, c.BN + 60, K, "eleven row panels (groups of 8 and 3), n_out % 64 == 60, through the GEMM", family="plain",
            epi=("bias", "residual"))
        one, two = slot_edges(c)
        add(f"{name}-slots{one}", name, c.BM + 7, one // c.WN * c.BN, K, f"{one} slots: the largest launch of one pass (CH = {c.CH})", family="offset-4", ln=False)
        add(f"{name}-slots{two}", name, c.BM + 7, two // c.WN * c.BN - 4, K, f"{two} slots: a second pass through LDS with {two - c.CH} slot(s)", family="offset-32", ln=True)
        add(f"{name}-slots{two}-offset128", name, c.BM + 7, two // c.WN * c.BN - 4, K, f"{two} slots, LayerNorm rows 128 standard deviations off zero", family="offset-128")
        for pos in SPIKES:
            add(f"{name}-spike-{pos}", name, two * 8 // 7 + 10, two // c.WN * c.BN - 4, K, f"spike at {pos}; the other rows: one slot each",
                family="spike", arg=pos, ln=pos in ("first", "ch", "tail"))
    add("256x256-pipe6", "256x256", 300, 256, 64, "tokens on the three-deep ring (PIPE 6) forced", family="plain", pipe=6, mode=1 | 4096, epi=("bias", "residual"))
    add("256x256-pipe4-plain", "256x256", 300, 264, 64, "no residual: PIPE 4, run-time path", family="plain", epi=())
    # ---- the four-stage rings of launch_small: M <= 128, K >= 256 (one row panel) ----
    c = CFG["64x128-ring4"]
    one, two = slot_edges(c)
    add("64x128-m1-n60", "64x128-ring4", 1, 60, 256, "one tile column, M == 1, n_out % 64 == 60")
    add("64x128-m127-n+4", "64x128-ring4", 127, 64 + 4, 256, "M % BM == BM - 1, n_out % 64 == 4")
    add("64x128-m128-n+8", "64x128-ring4", 128, 128 + 8, 256, "a full panel, n_out % 64 == 8")
    add("64x128-m65-n+20", "64x128-ring4", 65, 192 + 20, 256, "n_out % 64 == 20, rows 48..63 and 64 of the panel present")
    add(f"64x128-slots{one}", "64x128-ring4", 100, one // 2 * 64, 256, f"{one} slots: one pass (CH = {c.CH})", family="offset-4", ln=False)
    add(f"64x128-slots{two}-n3072", "64x128-ring4", 120, two // 2 * 64, 256, f"{two} slots = CH + 1: the second pass with a single slot; N = 3072, the o_proj tail",
        family="offset-32", ln=True)
    assert two // 2 * 64 == 3072
    for f_ in ("offset-4", "offset-128", "zero-sum"):
        add(f"64x128-n3072-{f_}", "64x128-ring4", 120, 3072, 256, f"N = 3072, the second pass with a single slot: LayerNorm, {f_}", family=f_)
    for pos in SPIKES:
        add(f"64x128-spike-{pos}", "64x128-ring4", 128, 3072 - 4, 256, f"spike at {pos}; the other rows: one slot each", family="spike", arg=pos,
            ln=pos in ("first", "ch", "tail"))
    add("64x128-plain-bias", "64x128-ring4", 52, 1152, 256, "through the GEMM, bias + residual", family="plain", epi=("bias", "residual"))
    c = CFG["128x128-ring4"]
    add("128x128-ring4-slots258", "128x128-ring4", 100, 128 * 128 + 128, 256, "129 tiles: the 128-feature ring; 258 slots = 2 CH + 4: three passes", family="offset-4")
    add("128x128-ring4-spike", "128x128-ring4", 128, 128 * 128 + 64 + 20, 256, "spike at slot CH = 127 of the ring; the other rows: the first 112 slots", family="spike", arg="ch")
    add("128x128-ring4-m1", "128x128-ring4", 1, 128 * 128 + 60, 256, "M == 1, n_out % 64 == 60", family="row-ladder")
    # ---- split-K with statistics (plan_small_m; the planner, no forcing) ----
    add("128x64-sk-n136", "128x64-sk", 40, 136, 2304, "split-K 3 ways, M < BM, two tile columns, n_out % 64 == 8", ks=3, family="plain", epi=("bias", "residual"))
    add("128x64-sk-m65", "128x64-sk", 65, 128, 2304, "split-K, M % BM == 1, one tile column", ks=3, family="offset-32")
    add("128x64-sk-m127-n+20", "128x64-sk", 127, 256 + 20, 2304, "split-K, M % BM == BM - 1, n_out % 64 == 20", ks=3, family="row-ladder")
    add("128x64-sk-m256-n60", "128x64-sk", 256, 60, 2304, "split-K, four panels (the most M <= 256 gives), n_out % 64 == 60", ks=3, family="constant", ln=True)
    add("128x64-sk-n+4", "128x64-sk", 70, 128 + 4, 2304, "split-K, n_out % 64 == 4", ks=3, family="zero-sum")
    add("128x96-sk-m289", "128x96-sk", 289, 136, 2304, "split-K, M % BM == 1, n_out % 64 == 8", ks=3, family="plain", epi=("residual",))
    add("128x96-sk-m383-n+4", "128x96-sk", 383, 128 + 4, 2304, "split-K, M % BM == BM - 1, n_out % 64 == 4", ks=3, family="offset-4")
    add("128x96-sk-9panels", "128x96-sk", 800, 256 + 20, 2304, "split-K, nine row panels, n_out % 64 == 20", ks=3, family="zero")
    add("128x96-sk-n60-fold", "128x96-sk", 300, 60, 2304, "split-K with row_scale and statistics, n_out % 64 == 60", ks=3, family="plain", epi=("fold-rms", "residual"),
        ln=False)
    # ---- plan 2: a 256x256 launch and a tail launch on one counter area and one partial area ----
    out.append(PCase("plan2-ring64", 0, 1076, 16384, 256, True, "row-ladder", (("256x256", 5, 1, 1024, 0), ("64x128-ring4", 0, 1, 52, 1024)),
                     "plan 2: the tail's statistics at st_rstd + m_main, both launches on one workspace"))
    out.append(PCase("plan2-small-plain", 0, 1176, 16384, 64, False, "plain", (("256x256", 5, 1, 1024, 0), ("128x128", 0, 1, 152, 1024)),
                     "plan 2 with a two-panel tail on the two-stage loop, through the GEMM", epi=("bias", "residual")))
    # ---- statistics behind every epilogue (128x128 forced; with statistics only keys 6 and 7 have straight-line variants, on interior tiles) ----
    for tag, M, N, K in (("interior", 256, 256, 64), ("tail", 300, 328, 128)):
        for i, epi in enumerate(((), ("bias",), ("residual",), ("bias", "residual"), ("bias", "gelu"), ("fold-rms",), ("fold-ln", "bias"), ("w2",), ("w2", "bias", "residual"))):
            why = {(): "key 4: no straight-line variant, the run-time path", ("bias",): "key 5: the run-time path",
                   ("residual",): "key 6 (o_proj, down): straight-line on interior tiles", ("bias", "residual"): "key 7 (SigLIP out_proj, fc2): straight-line on interior tiles",
                   ("bias", "gelu"): "behind GELU-tanh: the run-time path", ("fold-rms",): "key 12, consumer of 1/rms and producer: the run-time path",
                   ("fold-ln", "bias"): "the key-25 combination + statistics = key 29: the run-time path", ("w2",): "two-segment weight",
                   ("w2", "bias", "residual"): "two-segment weight, bias, residual"}[epi]
            add(f"epi-{tag}-{'+'.join(epi) or 'none'}", "128x128", M, N, K, f"statistics behind {why}; {tag} tiles", family="plain", ln=i % 2 == 0, epi=epi)
    return tuple(out)


PRODUCER = _producer()
PRODUCER_BY_ID = {c.id: c for c in PRODUCER}
assert len(PRODUCER_BY_ID) == len(PRODUCER)


def spike_feature(c, pos):
    cfg, n = c.cfg, c.N
    slots = slots_of(cfg, n)
    return {"first": 0, "last": (slots - 1) * cfg.slot_w, "ch-1": min(cfg.CH - 1, slots - 1) * cfg.slot_w + 5, "ch": min(cfg.CH, slots - 1) * cfg.slot_w + 2,
            "tail": n - 1}[pos]


def producer_inputs(c):
    """NS(x [M, K], w [N, K], bias, res, rs, mu, col: bf16 / f32 CPU tensors or None)."""
    g = rng_of("norm_fold", c.id)
    M, N, K = c.M, c.N, c.K
    o = NS(bias=None, res=None, rs=None, mu=None, col=None)
    o.w = bf(g.standard_normal((N, K)) / math.sqrt(K))
    if not c.exact:
        o.x = bf(g.standard_normal((M, K)))
        if "bias" in c.epi:
            o.bias = bf(g.standard_normal(N) * 0.5)
        if "residual" in c.epi:
            o.res = bf(g.standard_normal((M, N)))
        if "fold-rms" in c.epi or "fold-ln" in c.epi:
            o.rs = torch.from_numpy((0.5 + g.random(M)).astype(np.float32))
            if "fold-ln" in c.epi:
                o.mu = torch.from_numpy((0.3 * g.standard_normal(M)).astype(np.float32))
                o.col = torch.from_numpy((0.5 * g.standard_normal(N)).astype(np.float32))
        return o
    o.x = torch.zeros((M, K), dtype=BF)
    m = np.arange(M)[:, None]
    z = g.standard_normal((M, N))
    fam = c.family
    if fam.startswith("offset-"):
        y = (z + float(fam[7:]) * np.where(m % 2, -1.0, 1.0)) * 2.0 ** (m % 3 - 1)
    elif fam == "constant":
        y = np.broadcast_to((1.0 + (m % 7) * 0.375) * 2.0 ** ((m % 5) * 3 - 6) * np.where(m % 3 == 1, -1.0, 1.0), (M, N)).copy()
    elif fam == "zero":
        y = z * (m % 2)
    elif fam == "spike":
        y = np.full((M, N), 2.0 ** -6)
        slots = slots_of(c.cfg, N)
        for r in range(M):
            f = spike_feature(c, c.arg) if r % 8 == 0 else min(((r - r // 8 - 1) % slots) * c.cfg.slot_w + (r % 4), N - 1)
            y[r, f] = 2.0 ** 6
    elif fam == "zero-sum":
        a = (1.0 + (np.arange(N) // 2 % 4) * 0.25)[None, :] * 2.0 ** (m % 4)
        y = a * np.where(np.arange(N) % 2, -1.0, 1.0)[None, :]
    elif fam == "row-ladder":
        y = z * 2.0 ** ((m % 25) - 12)
    else:
        raise KeyError(fam)
    o.res = bf(y)
    return o


def _gelu_tanh(v):
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def producer_parts(c, inp):
    """The float64 pieces of the launch's value before the cast: NS(acc, pre (after fold, bias, act), res, full = pre + res)."""
    x, w = f64(inp.x), f64(inp.w)
    acc = np.zeros((c.M, c.N)) if c.exact else x @ w.T
    v = acc
    if inp.rs is not None:
        v = f64(inp.rs)[:, None] * (acc - (f64(inp.mu)[:, None] * f64(inp.col)[None, :] if inp.mu is not None else 0.0))
    nobias = v
    if inp.bias is not None:
        v = v + f64(inp.bias)[None, :]
    if c.act == ACT_GELU_TANH:
        v = _gelu_tanh(v)
    res = f64(inp.res) if inp.res is not None else np.zeros((c.M, c.N))
    return NS(acc=acc, nobias=nobias, pre=v, res=res, full=v + res)


def stored_model(c, inp):
    """The bf16 y a correct launch stores, as float64 (the CPU stand-in for the device's output)."""
    return f64(bf(producer_parts(c, inp).full))


def producer_reference(c, y, eps=None, ln=None):
    """Statistics of the stored y [M, n] (float64) and their bars: NS(mean, v, bar_mean, bar_v)."""
    ln = c.ln if ln is None else ln
    eps = float(np.float32(c.eps if eps is None else eps))
    n = y.shape[1]
    mu = y.mean(1) if ln else np.zeros(y.shape[0])
    msq, mabs = (y * y).mean(1), np.abs(y).mean(1)
    v = ((y - mu[:, None]) ** 2).mean(1) + eps if ln else msq + eps
    slots = np.array([slots_of(c.cfg_of_row(m), n) for m in range(y.shape[0])], dtype=np.float64)
    nf = np.array([c.cfg_of_row(m).NF for m in range(y.shape[0])], dtype=np.float64)
    kmean = 4 * nf + 2 + slots + 2
    ksq = 4 * nf + 1 + 2 + slots + 2 + (1 if ln else 0)
    kcross = 2 * kmean + 1
    bar_mean = kmean * EPS * mabs
    bar_v = EPS * (ksq * msq + (kcross * np.abs(mu) * mabs if ln else 0.0)) + K_RSQRT * EPS * v
    return NS(mean=mu, v=v, bar_mean=bar_mean, bar_v=bar_v, ln=ln)


def producer_ratio(ref, mean_dev, rstd_dev):
    """err / bar per row: NS(mean [M] (zeros for RMS), v [M]); a non-finite device value counts as inf."""
    rstd_dev = np.asarray(rstd_dev, dtype=np.float64)
    with np.errstate(all="ignore"):
        ev = np.abs(1.0 / (rstd_dev * rstd_dev) - ref.v)
        rv = np.where(ev > 0, ev / ref.bar_v, 0.0)
        rv = np.where(np.isfinite(rstd_dev) & (rstd_dev > 0), rv, np.inf)
        if ref.ln:
            mean_dev = np.asarray(mean_dev, dtype=np.float64)
            em = np.abs(mean_dev - ref.mean)
            rm = np.where(em > 0, em / (ref.bar_mean + FLOOR), 0.0)
            rm = np.where(np.isfinite(mean_dev), rm, np.inf)
        else:
            rm = np.zeros_like(rv)
    return NS(mean=rm, v=rv, worst=float(max(rm.max(), rv.max())))


def kernel_stats_f32(cfg, y, ln, eps, clamp=True):
    """The statistics block restated in numpy float32, in the kernel's order: a lane's 4 NF values one after another, the two shuffle
    additions, the slots top to bottom, inv_n, the clamp, rsqrt.  y [M, n] holds bf16 values.  Returns (mean, rstd) as float32."""
    f = np.float32
    M, n = y.shape
    slots = slots_of(cfg, n)
    pad = np.zeros((M, slots * cfg.slot_w), dtype=f)
    pad[:, :n] = y
    v = pad.reshape(M, slots, cfg.NF, 4, 4)                      # [row, slot, block n, lane row kg, r]
    s1 = np.zeros((M, slots, 4), dtype=f)
    s2 = np.zeros((M, slots, 4), dtype=f)
    for nb in range(cfg.NF):
        for r in range(4):
            vb = v[:, :, nb, :, r]
            s1 = (s1 + vb).astype(f)
            s2 = (s2 + (vb * vb).astype(f)).astype(f)
    w1 = ((s1[:, :, 0] + s1[:, :, 1]).astype(f) + (s1[:, :, 2] + s1[:, :, 3]).astype(f)).astype(f)     # lane kg = 0 after xor 16, xor 32
    w2 = ((s2[:, :, 0] + s2[:, :, 1]).astype(f) + (s2[:, :, 2] + s2[:, :, 3]).astype(f)).astype(f)
    t1, t2 = np.zeros(M, dtype=f), np.zeros(M, dtype=f)
    for s in range(slots):
        t2 = (t2 + w2[:, s]).astype(f)
        t1 = (t1 + w1[:, s]).astype(f)
    inv_n = f(1.0) / f(n)
    mean = (t1 * inv_n).astype(f)
    with np.errstate(invalid="ignore"):
        if ln:
            var = ((t2 * inv_n).astype(f) - (mean * mean).astype(f)).astype(f)
            if clamp:
                var = np.maximum(var, f(0))
            rstd = (f(1.0) / np.sqrt((var + f(eps)).astype(f), dtype=f)).astype(f)
        else:
            rstd = (f(1.0) / np.sqrt(((t2 * inv_n).astype(f) + f(eps)).astype(f), dtype=f)).astype(f)
    return mean, rstd


def producer_f32(c, y, clamp=True):
    mean, rstd = np.empty(c.M, dtype=np.float32), np.empty(c.M, dtype=np.float32)
    for name, _, _, rows, first in c.launches:
        mean[first:first + rows], rstd[first:first + rows] = kernel_stats_f32(CFG[name], y[first:first + rows].astype(np.float32), c.ln, c.eps, clamp)
    return mean, rstd


# ---- producer mutations --------------------------------------------------------------------------------------------------------------
def _stats64(y, n, ln, eps, s1=None, s2=None):
    s1 = y.sum(1) if s1 is None else s1
    s2 = (y * y).sum(1) if s2 is None else s2
    mean = s1 / n
    with np.errstate(all="ignore"):
        v = s2 / n - mean * mean if ln else s2 / n
        return mean, 1.0 / np.sqrt(np.maximum(v, 0.0) + eps)


def named_slot(c, which):
    slots = slots_of(c.cfg, c.N)
    return {"first": 0, "last": slots - 1, "ch-1": c.cfg.CH - 1, "ch": c.cfg.CH}[which]


def producer_mutant(c, inp, mut, arg=None):
    """(mean, rstd) in float64 of a kernel with the named fault, on the stored y of the CPU model."""
    y = stored_model(c, inp)
    n, ln, eps, cfg = c.N, c.ln, float(np.float32(c.eps)), c.cfg
    cols = lambda s: slice(s * cfg.slot_w, min((s + 1) * cfg.slot_w, n))
    if mut == "slot-dropped":
        y2 = y.copy()
        y2[:, cols(named_slot(c, arg))] = 0.0
        return _stats64(y2, n, ln, eps)
    if mut in ("sum-half-missing", "squares-half-missing"):
        part = y[:, cols(named_slot(c, arg))]
        rows = (np.arange(c.M) % cfg.BM >= 48) & (np.arange(c.M) % cfg.BM < 64) if mut == "sum-half-missing" else np.ones(c.M, dtype=bool)
        s1, s2 = y.sum(1), (y * y).sum(1)
        if mut == "sum-half-missing":
            s1 = s1 - part.sum(1) * rows
        else:
            s2 = s2 - (part * part).sum(1) * rows
        return _stats64(y, n, ln, eps, s1, s2)
    p = producer_parts(c, inp)
    if mut == "unrounded":
        return _stats64(p.full, n, ln, eps)
    if mut == "before-residual":
        return _stats64(f64(bf(p.pre)), n, ln, eps)
    if mut == "before-bias":
        return _stats64(f64(bf(p.nobias + p.res)), n, ln, eps)
    if mut == "tail-columns-counted":                       # the padding columns of the last slot hold what the clamped weight row gives: column n - 1
        width = slots_of(cfg, n) * cfg.slot_w
        y2 = np.concatenate([y, np.repeat(y[:, -1:], width - n, 1)], 1)
        return _stats64(y2, n, ln, eps)
    if mut in ("n-padded-64", "n-padded-bn"):
        q = 64 if mut == "n-padded-64" else cfg.BN
        return _stats64(y, (n + q - 1) // q * q, ln, eps)
    if mut == "other-norm":
        mean, rstd = _stats64(y, n, not ln, eps)
        return mean, rstd
    if mut == "eps-dropped":
        return _stats64(y, n, ln, 0.0)
    if mut == "eps-after-root":
        mean, r0 = _stats64(y, n, ln, 0.0)
        with np.errstate(all="ignore"):
            return mean, 1.0 / (1.0 / r0 + eps)
    if mut == "row-shifted":
        mean, rstd = _stats64(y, n, ln, eps)
        return np.roll(mean, 1), np.roll(rstd, 1)
    if mut == "tail-at-zero":                               # plan 2: the tail launch writes its rows at 0 instead of m_main
        mean, rstd = _stats64(y, n, ln, eps)
        first, rows = c.launches[1][4], c.launches[1][3]
        m2, r2 = mean.copy(), rstd.copy()
        m2[:rows], r2[:rows] = mean[first:], rstd[first:]
        m2[first:], r2[first:] = np.nan, np.nan
        return m2, r2
    if mut == "clamp-removed":
        mean, rstd = producer_f32(c, y, clamp=False)
        return mean.astype(np.float64), rstd.astype(np.float64)
    raise KeyError(mut)


# mutation -> [(case id, argument)]; every pair must break the bar by MIN_RATIO
PRODUCER_MUTATIONS = {
    "slot-dropped": [(f"{t}-spike-{p}", p if p != "tail" else "last") for t in ("256x256", "128x128", "128x96", "64x64-ring4", "64x128") for p in SPIKES]
    + [("128x128-ring4-spike", "ch")],
    "sum-half-missing": [("64x128-slots96-n3072", "ch"), ("128x128-slots64", "ch"), ("128x96-slots76", "last"), ("64x64-ring4-slots128", "ch"), ("256x256-slots64", "ch-1")],
    "squares-half-missing": [("64x128-spike-ch", "ch"), ("128x96-spike-ch-1", "ch-1"), ("256x256-spike-first", "first"), ("64x64-ring4-spike-last", "last")],
    "unrounded": [("epi-tail-none", None), ("epi-interior-bias+residual", None)],
    "before-residual": [("epi-tail-residual", None), ("epi-interior-bias+residual", None), ("128x96-sk-m289", None)],
    "before-bias": [("epi-tail-bias", None), ("epi-interior-bias+residual", None), ("epi-tail-bias+gelu", None)],
    "tail-columns-counted": [("128x128-m+1-n+4", None), ("64x128-m65-n+20", None), ("256x256-m-1-n+8", None), ("128x96-m1-n60", None), ("128x64-sk-m256-n60", None)],
    "n-padded-64": [("128x128-m+1-n+4", None), ("64x128-m65-n+20", None), ("128x96-sk-9panels", None)],
    "n-padded-bn": [("256x256-m-1-n+8", None), ("128x96-9panels-n+20", None), ("64x64-ring4-m+1-n+4", None)],
    "other-norm": [("64x128-slots96-n3072", None), ("128x128-slots62", None), ("128x64-sk-m65", None)],
    "eps-dropped": [("128x64-sk-m256-n60", None), ("128x96-sk-9panels", None), ("128x64-sk-m127-n+20", None)],
    "eps-after-root": [("128x64-sk-m127-n+20", None), ("128x96-sk-9panels", None)],
    "row-shifted": [("plan2-ring64", None), ("128x64-sk-m127-n+20", None), ("128x128-ring4-slots258", None)],
    "tail-at-zero": [("plan2-ring64", None), ("plan2-small-plain", None)],
    "clamp-removed": [("128x64-sk-m256-n60", None)],
}


# ---- the consumer table ----------------------------------------------------------------------------------------------------------------
class CCase:
    """epi: 'rms' | 'rms-swiglu' | 'ln' | 'ln-bias' | 'ln-gelu' | 'ln-res'; N = output features (the weight has 2 N rows for SwiGLU);
    launches: ((tile, EPI, NST, PIPE, SK, ksplit, rows, first row), ...)."""

    def __init__(self, id, mode, M, N, K, epi, family, launches, edge):
        self.id, self.mode, self.M, self.N, self.K, self.epi, self.family, self.launches, self.edge = id, mode, M, N, K, epi, family, launches, edge
        self.swiglu = epi == "rms-swiglu"
        self.ln = epi.startswith("ln")
        self.act = ACT_SWIGLU if self.swiglu else ACT_GELU_TANH if epi == "ln-gelu" else ACT_NONE
        self.bias = epi in ("ln-bias", "ln-gelu", "ln-res")
        self.residual = epi == "ln-res"
        self.kappa = K + 3.0

    def __repr__(self):
        return self.id

    @property
    def records(self):
        out = []
        for tile, epi, nst, pipe, sk, ks, rows, first in self.launches:
            NF, NT, WN, WM = R.TILES[tile]
            bn_out, BM = WN * NF * 16 // (2 if epi == R.EPI_SWIGLU else 1), WM * NT * 16
            out.append((NF, NT, WN, WM, epi, 0 if self.swiglu else self.act, 0, nst, pipe, sk, ks, rows, first, ((rows + BM - 1) // BM) * ((self.N + bn_out - 1) // bn_out) * ks))
        return out

    def route(self):
        o = dict(bias=self.bias, residual=self.residual, act=self.act, fold="ln" if self.ln else "rms")
        return R.Route(self.id, "linear", (self.M, 2 * self.N if self.swiglu else self.N, self.K), tuple(self.records), opts=o)


def _consumer():
    out = []
    P, S = R.EPI_PLAIN, R.EPI_SWIGLU
    fams = ("x0", "x4", "x32", "wmean", "ladder")

    def add(id, mode, M, N, K, epi, launch, edge):
        tile, e, nst, pipe = launch
        out.append(CCase(id, mode, M, N, K, epi, fams[len(out) % len(fams)], ((tile, e, nst, pipe, 0, 1, M, 0),), edge))

    forced = ((1, "256x256", 2, 4, 256, 256), (2, "128x128", 2, 0, 128, 128), (3, "128x96", 2, 8, 128, 96), (5, "64x64", 4, 0, 64, 64))
    for mode, tile, nst, pipe, BN, BM in forced:
        add(f"{tile}-interior-ln-bias-k64", mode, 2 * BM, BN, 64, "ln-bias", (tile, P, nst, pipe), "interior tiles: the straight-line variant key 25")
        add(f"{tile}-interior-rms-k256", mode, 2 * BM, 2 * BN, 256, "rms", (tile, P, nst, pipe), "interior tiles: key 8")
        add(f"{tile}-tail-ln-k256", mode, BM + 5, BN + 20, 256, "ln", (tile, P, nst, pipe), "row_shift without bias: the run-time path; tails in M and N")
        add(f"{tile}-tail-ln-gelu-k64", mode, BM + 1, BN + 60, 64, "ln-gelu", (tile, P, nst, pipe), "GELU-tanh behind the fold; tails")
        add(f"{tile}-tail-ln-res-k1152", mode, 2 * BM - 1, BN + 8, 1152, "ln-res", (tile, P, nst, pipe), "bias + residual behind the fold, K = 1152")
        add(f"{tile}-tail-ln-bias-k1152", mode, 2 * BM + 3, BN + 4, 1152, "ln-bias", (tile, P, nst, pipe), "key 25 on interior tiles, the run-time path on the tails; n_out % 8 == 4")
    # SwiGLU under a forced tile: mode 1 -> 256x256 (128 output features per tile), mode 2 -> 128x128 (64 output features)
    add("256x256-swiglu-interior-k256", 1, 256, 256, 256, "rms-swiglu", ("256x256", S, 2, 4), "row_scale on gate and up, interior: key 8")
    add("256x256-swiglu-tail-k64", 1, 300, 128 + 20, 64, "rms-swiglu", ("256x256", S, 2, 4), "row_scale on gate and up, tails")
    add("128x128-swiglu-interior-k1152", 2, 256, 128, 1152, "rms-swiglu", ("128x128", S, 2, 0), "interior: key 8, K = 1152")
    add("128x128-swiglu-tail-k256", 2, 129, 64 + 8, 256, "rms-swiglu", ("128x128", S, 2, 0), "tails")
    # the planner's own routes
    add("plan-128x96-ln-bias", 0, 300, 512, 256, "ln-bias", ("128x96", P, 2, 8), "plan 3 (SigLIP's qkv / fc1 route)")
    add("plan-128x96-ln-gelu-tail", 0, 300, 520 + 20, 1152, "ln-gelu", ("128x96", P, 2, 8), "plan 3, GELU-tanh, tails, K = 1152")
    add("ring-64x128-rms", 2, 100, 1152, 256, "rms", ("64x128", P, 4, 0), "one row of tiles: the weight-streaming ring of launch_small")
    add("ring-64x128-ln-res", 2, 77, 512 + 4, 256, "ln-res", ("64x128", P, 4, 0), "the ring with row_shift, n_out % 8 == 4")
    add("plan-swiglu-ring3", 0, 200, 256, 1152, "rms-swiglu", ("128x128", S, 3, 0), "plan_small_m variant 1 (M <= 256, K >= 512)")
    add("plan-swiglu-small", 0, 300, 192 + 20, 256, "rms-swiglu", ("128x128", S, 2, 0), "gate_up above 256 rows: 128x128 tiles")
    return tuple(out)


CONSUMER = _consumer()
CONSUMER_BY_ID = {c.id: c for c in CONSUMER}
assert len(CONSUMER_BY_ID) == len(CONSUMER)


def consumer_inputs(c):
    """NS(x bf16 [M, K], w bf16 [rows, K] (= w'), wu float64 (w' before its rounding), rs, mu, col f32, bias, res)."""
    g = rng_of("norm_fold_consumer", c.id)
    M, N, K = c.M, c.N, c.K
    rows = 2 * N if c.swiglu else N
    ratio = {"x0": 0.0, "x4": 4.0, "x32": 32.0, "wmean": 4.0, "ladder": 4.0}[c.family]
    m = np.arange(M)[:, None]
    std = 2.0 ** (m % 3 - 1)
    x = bf((g.standard_normal((M, K)) + ratio * np.where(m % 2, -1.0, 1.0)) * std)
    wmean = 8.0 if c.family == "wmean" else 0.5
    wu = (g.standard_normal((rows, K)) + wmean * np.where(np.arange(rows)[:, None] % 3 == 0, -1.0, 1.0)) / math.sqrt(K)
    w = bf(wu)
    xd = f64(x)
    rs = 1.0 / np.sqrt(xd.var(1) + 1e-6)
    if c.family == "ladder":
        rs = 2.0 ** ((np.arange(M) % 21) - 10.0)
    o = NS(x=x, w=w, wu=wu, rs=torch.from_numpy(rs.astype(np.float32)), mu=None, col=None, bias=None, res=None)
    if c.ln:
        o.mu = torch.from_numpy(xd.mean(1).astype(np.float32))
        o.col = torch.from_numpy(f64(w).sum(1).astype(np.float32))
    if c.bias:
        o.bias = bf(g.standard_normal(N) * 0.5)
    if c.residual:
        o.res = bf(g.standard_normal((M, N)))
    return o


def _silu(a):
    with np.errstate(over="ignore"):
        return a / (1.0 + np.exp(-a))


def _dsilu(a):
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-a))
    return s * (1.0 + a * (1.0 - s))


def consumer_reference(c, inp, mut=None, rs=None, mu=None, col=None, extra=0.0):
    """Out of the launch: rs (x w'^T - mu c) [+ bias -> act] [+ res] in float64 with its bar.  rs / mu / col override the operands (the
    chained cases hand in float64 statistics); `extra` is added to the bar's a (the producer's share there).  `mut`: a named wrong kernel."""
    x, w = f64(inp.x), f64(inp.w)
    rs = f64(inp.rs) if rs is None else rs
    N = c.N
    acc = x @ w.T
    A = np.abs(x) @ np.abs(w).T
    if c.ln:
        mu = f64(inp.mu) if mu is None else mu
        col = f64(inp.col) if col is None else col
        if mut == "shift-ignored":
            mu = np.zeros_like(mu)
        elif mut == "mu-of-neighbour":
            mu = np.roll(mu, 1)
        elif mut == "c-shifted-4":
            col = np.roll(col, -4)
        elif mut == "c-unrounded":
            col = inp.wu.sum(1)
        shift = mu[:, None] * col[None, :]
        acc, A = acc - shift, A + np.abs(shift)
    if mut == "rs-of-neighbour":
        rs = np.roll(rs, 1)
    r = rs[:, None]
    v, M_ = r * acc, np.abs(r) * A
    a = c.kappa * EPS * M_
    if c.swiglu:
        gte, up, a_g, a_u = v[:, :N], v[:, N:], a[:, :N], a[:, N:]
        y = up * _silu(gte)
        a = np.abs(_silu(gte)) * a_u + np.abs(up * _dsilu(gte)) * a_g + EPS * (8.0 * np.abs(up * gte) + np.abs(y))
        return Out(y, (a + extra) / EPS, 1.0)
    res = f64(inp.res) if inp.res is not None else None
    if inp.bias is not None:
        b = f64(inp.bias)[None, :]
        if mut == "bias-scaled":
            v = v + r * b
        elif mut == "scale-after-residual":
            v = r * (acc + b + res)
            res = None
        else:
            v = v + b
        a = a + EPS * (np.abs(v) + np.abs(b))
    if c.act == ACT_GELU_TANH:
        a = 1.13 * a + 12.0 * EPS * np.abs(v)
        extra = 1.13 * extra
        v = _gelu_tanh(v)
    if res is not None:
        v = v + res
        a = a + EPS * (np.abs(v) + np.abs(res))
    return Out(v, (a + extra) / EPS, 1.0)


CONSUMER_MUTATIONS = {
    "shift-ignored": [("128x128-tail-ln-k256", None), ("256x256-interior-ln-bias-k64", None), ("ring-64x128-ln-res", None)],
    "mu-of-neighbour": [("128x96-tail-ln-k256", None), ("64x64-interior-ln-bias-k64", None), ("plan-128x96-ln-bias", None)],
    "rs-of-neighbour": [("256x256-tail-ln-gelu-k64", None), ("128x128-interior-rms-k256", None), ("plan-swiglu-ring3", None)],
    "c-shifted-4": [("128x128-tail-ln-bias-k1152", None), ("64x64-tail-ln-k256", None), ("plan-128x96-ln-gelu-tail", None)],
    "c-unrounded": [("128x128-tail-ln-k256", None), ("128x96-interior-ln-bias-k64", None), ("256x256-tail-ln-k256", None)],
    "bias-scaled": [("128x128-tail-ln-gelu-k64", None), ("64x64-tail-ln-res-k1152", None), ("plan-128x96-ln-bias", None)],
    "scale-after-residual": [("128x128-tail-ln-res-k1152", None), ("ring-64x128-ln-res", None), ("256x256-tail-ln-res-k1152", None)],
}


# ---- chained cases: a producer's statistics into a consumer ----------------------------------------------------------------------------
class Chain:
    def __init__(self, id, ln, ratio, M=300, N1=1152, N2=256 + 20, K1=128):
        self.id, self.ln, self.ratio, self.M, self.N1, self.N2, self.K1 = id, ln, ratio, M, N1, N2, K1
        self.eps = 1e-6 if ln else 1e-5

    def __repr__(self):
        return self.id


CHAINED = (Chain("chain-ln-0", True, 0.0), Chain("chain-ln-4", True, 4.0), Chain("chain-ln-32", True, 32.0), Chain("chain-rms", False, 0.0))
CHAIN_TILE = "128x96"               # both launches take plan 3 at these shapes (the dry run and the device's route log are held to it)


def chain_records(c):
    """The route-log records of the producer and of the consumer launch."""
    cfg = CFG[CHAIN_TILE]
    rec = lambda n: (cfg.NF, cfg.NT, cfg.WN, cfg.WM, R.EPI_PLAIN, ACT_NONE, 0, cfg.NST, cfg.pipes[0], 0, 1, c.M, 0, ((c.M + cfg.BM - 1) // cfg.BM) * ((n + cfg.BN - 1) // cfg.BN))
    return [rec(c.N1), rec(c.N2)]


def chain_inputs(c):
    """Producer: y1 = x0 w0^T + b0 + r0 with statistics; r0 carries the row mean.  Consumer: norm(y1; gamma, beta) w^T + b."""
    g = rng_of("norm_fold_chain", c.id)
    m = np.arange(c.M)[:, None]
    o = NS()
    o.x0 = bf(g.standard_normal((c.M, c.K1)))
    o.w0 = bf(g.standard_normal((c.N1, c.K1)) / math.sqrt(c.K1))
    o.b0 = bf(g.standard_normal(c.N1) * 0.25)
    o.r0 = bf((g.standard_normal((c.M, c.N1)) + 1.5 * c.ratio * np.where(m % 2, -1.0, 1.0)) * 2.0 ** (m % 3 - 1))
    o.gamma = bf(1.0 + 0.3 * g.standard_normal(c.N1))
    o.beta = bf(0.2 * g.standard_normal(c.N1)) if c.ln else None
    o.w = bf(g.standard_normal((c.N2, c.N1)) / math.sqrt(c.N1))
    o.b = bf(g.standard_normal(c.N2) * 0.1) if c.ln else None
    return o


def chain_fold(c, inp):
    """(w', b', col) as the model's host code folds them (aki_amd.siglip.fold_layernorm / aki_amd.ops.fold_gain), CPU tensors."""
    from aki_amd import ops
    if not c.ln:
        return ops.fold_gain(inp.w, inp.gamma), None, None
    from aki_amd.siglip import fold_layernorm
    ln = torch.nn.LayerNorm(c.N1, eps=c.eps).to(BF)
    with torch.no_grad():
        ln.weight.copy_(inp.gamma)
        ln.bias.copy_(inp.beta)
    wf, bfold, col = fold_layernorm(inp.w, inp.b, ln)
    return wf, bfold, col[:c.N2]


def chain_col_bar(wf):
    """(float64 row sums of the rounded w', dc): fold_layernorm's f32 sum is held to them within dc = K 2^-24 sum_k |w'_k|."""
    w = f64(wf)
    return w.sum(1), w.shape[1] * EPS * np.abs(w).sum(1)


def chain_reference(c, y1, wf, bfold):
    """Out of the consumer launch on the stored intermediate y1 [M, N1] (float64): norm-then-linear with the rounded w' and b', the
    consumer's bar plus the producer's bars to first order."""
    cfg = CFG[CHAIN_TILE]
    pc = NS(cfg=cfg, ln=c.ln, eps=c.eps, cfg_of_row=lambda m: cfg)
    st = producer_reference(pc, y1)
    rstd = 1.0 / np.sqrt(st.v)
    cc = NS(N=c.N2, K=c.N1, ln=c.ln, swiglu=False, act=ACT_NONE, kappa=c.N1 + 3.0)
    inp = NS(x=torch.from_numpy(y1), w=wf, rs=None, mu=None, col=None, bias=bfold, res=None)
    w = f64(wf)
    col, dcol = chain_col_bar(wf)
    d_rstd = 0.5 * rstd ** 3 * st.bar_v
    centred = y1 @ w.T - (st.mean[:, None] * col[None, :] if c.ln else 0.0)
    extra = d_rstd[:, None] * np.abs(centred)
    if c.ln:
        extra = extra + rstd[:, None] * (st.bar_mean[:, None] * np.abs(col)[None, :] + np.abs(st.mean)[:, None] * dcol[None, :])
    return consumer_reference(cc, inp, rs=rstd, mu=st.mean, col=col, extra=extra)


def chain_torch(c, y1, inp):
    """float64 torch LayerNorm / RMSNorm followed by a linear, with the UNROUNDED fold (W diag(gamma), W beta + b)."""
    y = torch.from_numpy(y1)
    g, w = inp.gamma.double(), inp.w.double()
    if c.ln:
        normed = torch.nn.functional.layer_norm(y, (c.N1,), g, inp.beta.double(), c.eps)
        return (normed @ w.T + inp.b.double()).numpy()
    normed = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + c.eps) * g
    return (normed @ w.T).numpy()


# ---- the rstd error by mean / std (docstring) -----------------------------------------------------------------------------------------
RATIOS = (0, 4, 16, 32, 64, 128)


def rstd_error_by_ratio(N, rows=64, name="64x128-ring4"):
    """{ratio: (worst relative error of the restated-f32 rstd against float64, the bound the K's give)} for LayerNorm rows of width N."""
    cfg = CFG[name]
    out = {}
    for r in RATIOS:
        g = rng_of("rstd_by_ratio", N, r)
        y = f64(bf(g.standard_normal((rows, N)) + float(r)))
        _, rstd = kernel_stats_f32(cfg, y.astype(np.float32), True, 1e-6)
        mu = y.mean(1)
        v = ((y - mu[:, None]) ** 2).mean(1) + float(np.float32(1e-6))
        want = 1.0 / np.sqrt(v)
        slots = slots_of(cfg, N)
        bound = 0.5 * EPS * (k_sq(cfg, slots, True) * (y * y).mean(1) + k_cross(cfg, slots) * np.abs(mu) * np.abs(y).mean(1) + K_RSQRT * v) / v
        out[r] = (float(np.abs(rstd.astype(np.float64) / want - 1.0).max()), float(bound.max()))
    return out

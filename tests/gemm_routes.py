"""Route table of the bf16 / fp8 GEMM (aki_amd/csrc/gemm_bf16.hip): which gemm_bf16_kernel instantiation each shape reaches.

The planner (plan_small_m, plan_tiles, launch_small, launch_big and the plan-2 big + M-tail pair) picks one of the product
library's instantiations per launch.  Each entry below names an entry point, a shape, the options of the call and the launches
the lab library's route log (aki_lab_gemm_log) must show for it.  tests/test_gemm_routes_cpu.py checks the records in dry-run
mode (the planner without a GPU) and that the entries cover every instantiation the product library exports;
tests/test_gemm_routes_gpu.py runs every entry on the device against a float64 reference.

A record is (NF, NT, WN, WM, EPI, ACT, FP8, NST, PIPE, SK, ksplit, M, m_offset, grid) - the ten template arguments, the runtime
K split, the rows of the launch, the global index of its first row and the workgroup count.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

EPI_PLAIN, EPI_SWIGLU, EPI_QKV = 0, 1, 3
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3

# tile name (features x tokens) -> NF, NT, WN, WM
TILES = {"256x256": (8, 4, 2, 4), "128x128": (4, 4, 2, 2), "64x128": (2, 4, 2, 2), "128x96": (4, 3, 2, 2), "128x64": (4, 2, 2, 2),
         "64x64": (2, 2, 2, 2)}


def rec(tile, epi, act, fp8, nst, pipe, sk, ksplit, M, m_offset, grid):
    return TILES[tile] + (epi, act, int(fp8), nst, pipe, sk, ksplit, M, m_offset, grid)


def big(epi, act, pipe, M, grid, m_offset=0, fp8=False):                 # launch_big: 256 x 256 (bf16: PIPE 4 / 5 / 6, fp8: the two-stage loop)
    return rec("256x256", epi, act, fp8, 2, 0 if fp8 else pipe, 0, 1, M, m_offset, grid)


def small(epi, act, M, grid, m_offset=0, fp8=False, ring=None):           # launch_small: 128 x 128 two-stage, or a four-stage ring (64- or 128-feature)
    if ring is None:
        return rec("128x128", epi, act, fp8, 2, 0, 0, 1, M, m_offset, grid)
    return rec(ring, epi, act, fp8, 4, 0, 0, 1, M, m_offset, grid)


def splitk(tile, ksplit, M, grid):                                         # plan_small_m, plain bf16: variant 3 (128 x 96) or 5 (128 x 64, three stages)
    return rec(tile, EPI_PLAIN, ACT_NONE, False, 2 if tile == "128x96" else 3, 0, 1, ksplit, M, 0, grid)


def kernel_of(record):
    return tuple(record[:10])


@dataclass(frozen=True)
class Route:
    id: str
    entry: str                  # "linear" | "linear_fp8" | "qkv_rope" | "qkv_rope_fp8"
    shape: tuple                # linear: (M, N, K) with N = weight rows (2 n_out for SwiGLU); qkv_rope: (B, L, H, d_model)
    expect: tuple               # the records of one call
    opts: dict = field(default_factory=dict)
    expect_res8: Optional[tuple] = None   # the records when the residual is only 8-byte aligned (default: `expect`)
    # act, bias, residual, res_row_mod, fold ("rms" / "ln": row_scale [, row_shift, col_shift]), stats ("rms" / "ln"), preact,
    # w2 (first logical row of the second weight segment), ldy_pad (output row stride - n_out), ldx_pad (input row stride - K);
    # qkv_rope: fold ("rms": row_scale), pos (per-sample position ids), kv_pad (KV capacity - L)
    why: str = ""

    def opt(self, name, default=None):
        return self.opts.get(name, default)

    @property
    def n_out(self):
        if self.entry.startswith("qkv"):
            return 3 * self.shape[2] * 96
        return self.shape[1] // 2 if self.opt("act", 0) == ACT_SWIGLU else self.shape[1]

    @property
    def uses_splitk(self):
        return any(r[9] for r in self.expect)


P, S, Q = EPI_PLAIN, EPI_SWIGLU, EPI_QKV
G1, G2 = ACT_GELU_ERF, ACT_GELU_TANH

ROUTES = [
    # ---- split-K (plan_small_m, plain bf16 without activation, 17 <= M <= 1024, n_out <= 4096, K >= 2304): ksplit = min(512 / tiles, 3) ----
    Route("splitk2-m960", "linear", (960, 3072, 2304), (splitk("128x96", 2, 960, 480),), opts=dict(bias=True, residual=True),
          why="10 x 24 = 240 tiles of 128 x 96: 512 / 240 = 2, the last M of ksplit 2 at N = 3072"),
    Route("small-m961", "linear", (961, 3072, 2304), (small(P, 0, 961, 192),), opts=dict(bias=True, residual=True),
          why="11 x 24 = 264 tiles: no split; 128 x 128 tiles on the two-stage loop"),
    Route("splitk2-k2368", "linear", (800, 3072, 2368), (splitk("128x96", 2, 800, 432),), opts=dict(bias=True, residual=True, res_row_mod=37),
          why="37 K-steps over two slices (18 + 19)"),
    Route("splitk3-k2368", "linear", (300, 3072, 2368), (splitk("128x96", 3, 300, 288),), opts=dict(bias=True, residual=True, ldy_pad=8),
          why="37 K-steps over three slices (12 + 12 + 13)"),
    Route("splitk3-128x64-m256", "linear", (256, 3072, 2304), (splitk("128x64", 3, 256, 288),), opts=dict(bias=True, ldx_pad=64),
          why="M <= 256: variant 5"),
    Route("splitk3-k2304", "linear", (207, 1152, 2304), (splitk("128x64", 3, 207, 108),), opts=dict(residual=True),
          why="36 K-steps: the shortest K that splits"),
    Route("plan4-k2240", "linear", (207, 1152, 2240), (rec("64x64", P, 0, False, 4, 0, 0, 1, 207, 0, 72),), opts=dict(residual=True),
          why="35 K-steps: no split; 64 x 64 tiles on the four-stage ring"),
    Route("splitk3-m1024", "linear", (1024, 1152, 2304), (splitk("128x96", 3, 1024, 297),), opts=dict(bias=True, stats="ln"),
          why="the last M plan_small_m considers; statistics beside the fold"),
    Route("plan4-m1025", "linear", (1025, 1152, 2304), (rec("64x64", P, 0, False, 4, 0, 0, 1, 1025, 0, 306),), opts=dict(bias=True),
          why="M > 1024: no split"),
    Route("splitk3-fold-stats", "linear", (700, 1152, 2304), (splitk("128x96", 3, 700, 216),), opts=dict(fold="rms", stats="rms", residual=True),
          why="row_scale and the producer statistics on the split-K fold"),
    Route("row-shift-nosplit", "linear", (700, 1152, 2304), (rec("64x64", P, 0, False, 4, 0, 0, 1, 700, 0, 198),), opts=dict(fold="ln", bias=True),
          why="row_shift never takes split-K"),
    Route("w2-nosplit", "linear", (300, 3072, 2304), (rec("64x64", P, 0, False, 4, 0, 0, 1, 300, 0, 240),), opts=dict(w2=2000),
          why="a two-segment weight never takes the small-M variants"),
    # ---- plan 3 / plan 4 (plain bf16): 128 x 96 tiles on a three-deep token ring, 64 x 64 tiles on a four-stage ring ----
    Route("plan3-m128", "linear", (128, 1152, 2048), (rec("128x96", P, 0, False, 2, 8, 0, 1, 128, 0, 18),), opts=dict(bias=True, residual=True),
          why="M = 128 is not given the 64 x 64 tiles (the weight-streaming regime)"),
    Route("plan4-m129", "linear", (129, 1152, 2048), (rec("64x64", P, 0, False, 4, 0, 0, 1, 129, 0, 54),), opts=dict(bias=True, residual=True),
          why="M > 128, one round of 128 x 96 tiles, 32 K-steps"),
    Route("plan3-gelu-erf", "linear", (700, 1152, 640), (rec("128x96", P, G1, False, 2, 8, 0, 1, 700, 0, 72),), opts=dict(act=G1, bias=True)),
    Route("plan3-gelu-tanh", "linear", (700, 1152, 640), (rec("128x96", P, G2, False, 2, 8, 0, 1, 700, 0, 72),),
          opts=dict(act=G2, bias=True, residual=True, fold="ln")),
    Route("plan4-gelu-erf", "linear", (129, 1152, 2048), (rec("64x64", P, G1, False, 4, 0, 0, 1, 129, 0, 54),), opts=dict(act=G1, bias=True)),
    Route("plan4-gelu-tanh", "linear", (129, 1152, 2048), (rec("64x64", P, G2, False, 4, 0, 0, 1, 129, 0, 54),), opts=dict(act=G2, bias=True)),
    # ---- launch_small: one row of tiles on the four-stage ring (128-feature tiles: 129-256 of them), else the two-stage loop ----
    Route("ring128-plain", "linear", (100, 32768, 256), (small(P, 0, 100, 256, ring="128x128"),), opts=dict(bias=True, residual=True)),
    Route("ring128-gelu-erf", "linear", (100, 32768, 256), (small(P, G1, 100, 256, ring="128x128"),), opts=dict(act=G1, bias=True)),
    Route("ring128-gelu-tanh", "linear", (100, 32768, 256), (small(P, G2, 100, 256, ring="128x128"),), opts=dict(act=G2, bias=True)),
    Route("small-gelu-erf", "linear", (3073, 2048, 512), (small(P, G1, 3073, 400),), opts=dict(act=G1, bias=True, residual=True)),
    Route("small-gelu-tanh", "linear", (3073, 2048, 512), (small(P, G2, 3073, 400),), opts=dict(act=G2, bias=True, ldy_pad=4)),
    # ---- plan 2: 256 x 256 tiles on the first M / 256 * 256 rows, small tiles on the M tail (m_offset, shifted pointers) ----
    Route("plan2-ring64-row-mod", "linear", (2100, 16384, 256),
          (big(P, 0, 4, 2048, 512), small(P, 0, 52, 256, m_offset=2048, ring="64x128")), opts=dict(bias=True, residual=True, res_row_mod=729),
          why="the tail's residual row is (m + m_offset) % res_row_mod"),
    Route("plan2-ring64-gelu-erf", "linear", (2100, 16384, 256),
          (big(P, G1, 4, 2048, 512), small(P, G1, 52, 256, m_offset=2048, ring="64x128")), opts=dict(act=G1, bias=True)),
    Route("plan2-ring64-gelu-tanh", "linear", (2100, 16384, 256),
          (big(P, G2, 4, 2048, 512), small(P, G2, 52, 256, m_offset=2048, ring="64x128")), opts=dict(act=G2, bias=True, fold="ln")),
    Route("plan2-residual-stats", "linear", (2200, 16384, 256),
          (big(P, 0, 5, 2048, 512), small(P, 0, 152, 256, m_offset=2048)), opts=dict(bias=True, residual=True, stats="ln"),
          expect_res8=(big(P, 0, 4, 2048, 512), small(P, 0, 152, 256, m_offset=2048)),
          why="residual and statistics pointers shifted for the tail; PIPE 5 on the big part"),
    Route("plan2-gelu-tanh", "linear", (2200, 16384, 256),
          (big(P, G2, 4, 2048, 512), small(P, G2, 152, 256, m_offset=2048)), opts=dict(act=G2, bias=True, residual=True)),
    # ---- launch_big: PIPE 4, 5 (residual prefetch) and 6 (+ tokens three deep: M > 1.5 N and K >= 4096) ----
    Route("big-pipe4", "linear", (4608, 3072, 512), (big(P, 0, 4, 4608, 216),), opts=dict(bias=True, fold="rms")),
    Route("big-gelu-erf", "linear", (4608, 3072, 512), (big(P, G1, 4, 4608, 216),), opts=dict(act=G1, bias=True, residual=True)),
    Route("big-gelu-tanh", "linear", (4608, 3072, 512), (big(P, G2, 4, 4608, 216),), opts=dict(act=G2, bias=True)),
    Route("big-pipe5-m4608", "linear", (4608, 3072, 4096), (big(P, 0, 5, 4608, 216),), opts=dict(residual=True),
          expect_res8=(big(P, 0, 4, 4608, 216),), why="M = 1.5 N: tokens not deep"),
    Route("big-pipe6-m4609", "linear", (4609, 3072, 4096), (big(P, 0, 6, 4609, 228),), opts=dict(residual=True, bias=True),
          expect_res8=(big(P, 0, 4, 4609, 228),), why="M > 1.5 N, K = 4096"),
    Route("big-pipe5-k4032", "linear", (4609, 3072, 4032), (big(P, 0, 5, 4609, 228),), opts=dict(residual=True),
          expect_res8=(big(P, 0, 4, 4609, 228),), why="K = 4032 < 4096: tokens not deep"),
    Route("big-narrow-n3076", "linear", (4609, 3076, 4096), (big(P, 0, 4, 4609, 247),), opts=dict(residual=True, bias=True),
          why="n_out % 8 == 4: narrow stores, no residual prefetch"),
    # ---- gate_up + SwiGLU ----
    Route("swiglu-smallm", "linear", (200, 4096, 1024), (rec("128x128", S, 0, False, 3, 0, 0, 1, 200, 0, 64),), opts=dict(act=ACT_SWIGLU, preact=True),
          why="M <= 256, K >= 512: variant 1 (three-stage ring)"),
    Route("swiglu-ring64", "linear", (100, 4096, 256), (small(S, 0, 100, 64, ring="64x128"),), opts=dict(act=ACT_SWIGLU, fold="rms")),
    Route("swiglu-ring128", "linear", (100, 24576, 256), (small(S, 0, 100, 192, ring="128x128"),), opts=dict(act=ACT_SWIGLU, preact=True)),
    Route("swiglu-small", "linear", (257, 4096, 1024), (small(S, 0, 257, 96),), opts=dict(act=ACT_SWIGLU, preact=True, ldy_pad=8)),
    Route("swiglu-big", "linear", (3073, 4096, 512), (big(S, 0, 4, 3073, 208),), opts=dict(act=ACT_SWIGLU, fold="rms")),
    Route("swiglu-plan2", "linear", (2200, 16384, 256), (big(S, 0, 4, 2048, 512), small(S, 0, 152, 256, m_offset=2048)),
          opts=dict(act=ACT_SWIGLU, preact=True)),
    # ---- QKV + RoPE ----
    Route("qkv-smallm-ring-l255", "qkv_rope", (1, 255, 32, 768), (rec("128x96", Q, 0, False, 3, 0, 0, 1, 255, 0, 216),), opts=dict(fold="rms"),
          why="M <= 256: variant 4"),
    Route("qkv-smallm-l655", "qkv_rope", (1, 655, 32, 768), (rec("128x96", Q, 0, False, 2, 0, 0, 1, 655, 0, 504),), why="M > 256: variant 3"),
    Route("qkv-small-h8", "qkv_rope", (5, 255, 8, 768), (small(Q, 0, 1275, 180),), opts=dict(pos=True)),
    Route("qkv-big-l255", "qkv_rope", (5, 255, 32, 768), (big(Q, 0, 4, 1275, 180),), opts=dict(pos=True),
          why="L < 256: a 256-token tile spans two samples"),
    Route("qkv-big-l256", "qkv_rope", (5, 256, 32, 768), (big(Q, 0, 4, 1280, 180),), opts=dict(kv_pad=3)),
    Route("qkv-plan2-l1000", "qkv_rope", (2, 1000, 32, 768), (big(Q, 0, 4, 1792, 252), small(Q, 0, 208, 144, m_offset=1792)), opts=dict(pos=True)),
    Route("qkv-plan2-ring-l950", "qkv_rope", (2, 950, 32, 768), (big(Q, 0, 4, 1792, 252), small(Q, 0, 108, 72, m_offset=1792, ring="128x128")),
          opts=dict(pos=True, kv_pad=3, fold="rms")),
    # ---- fp8 (e4m3) operands: 256 x 256 and 128 x 128 tiles on the two-stage loop ----
    Route("fp8-plan2", "linear_fp8", (2200, 16384, 256), (big(P, 0, 0, 2048, 512, fp8=True), small(P, 0, 152, 256, m_offset=2048, fp8=True)),
          opts=dict(bias=True, residual=True)),
    Route("fp8-swiglu-plan2", "linear_fp8", (2200, 16384, 256),
          (big(S, 0, 0, 2048, 512, fp8=True), small(S, 0, 152, 256, m_offset=2048, fp8=True)), opts=dict(act=ACT_SWIGLU)),
    Route("fp8-big", "linear_fp8", (4608, 3072, 512), (big(P, 0, 0, 4608, 216, fp8=True),), opts=dict(bias=True, residual=True)),
    Route("fp8-small", "linear_fp8", (1380, 16384, 256), (small(P, 0, 1380, 1408, fp8=True),), opts=dict(bias=True)),
    Route("fp8-swiglu-small", "linear_fp8", (100, 16384, 256), (small(S, 0, 100, 128, fp8=True),), opts=dict(act=ACT_SWIGLU),
          why="fp8 has no four-stage ring: one row of tiles stays on the two-stage loop"),
    Route("qkv-fp8-big", "qkv_rope_fp8", (5, 256, 32, 768), (big(Q, 0, 0, 1280, 180, fp8=True),)),
    Route("qkv-fp8-small", "qkv_rope_fp8", (1, 655, 32, 768), (small(Q, 0, 655, 432, fp8=True),), opts=dict(pos=True),
          why="fp8 has no small-M variants: 128 x 128 tiles"),
    Route("qkv-fp8-plan2", "qkv_rope_fp8", (2, 1000, 32, 768),
          (big(Q, 0, 0, 1792, 252, fp8=True), small(Q, 0, 208, 144, m_offset=1792, fp8=True)), opts=dict(pos=True)),
]

ROUTE_IDS = [r.id for r in ROUTES]


def by_id(rid: str) -> Route:
    return next(r for r in ROUTES if r.id == rid)


# ---- dry run: the planner on fake, aligned pointers (aki_lab_set_gemm_dry_run: no HIP call, nothing dereferenced) ---------------------
FAKE = 1 << 32          # base of the fake address space; every operand gets its own 256 MiB-aligned window


def _fake(i, offset=0):
    return FAKE + (i << 28) + offset


def dry_run(lib, route: Route, splitk_bytes: Optional[int] = None, splitk_offset: int = 0, res8: bool = False):
    """Run `route` through the lab library in dry-run mode; returns the route log.  `splitk_bytes` overrides the split-K workspace
    handed over (default: what aki_amd.ops.linear passes - max(aki_linear_splitk_workspace_bytes, 32 MiB), for plain bf16 launches of
    at most 2048 rows)."""
    from aki_amd import _lib as L
    lib.aki_lab_set_gemm_dry_run(1)
    lib.aki_lab_gemm_log_reset()
    try:
        rc = _call(lib, route, splitk_bytes, splitk_offset, res8)
        if rc != 0:
            raise L.AkiError(f"{route.id}: status {rc} in dry run")
        return L.gemm_log(lib)
    finally:
        lib.aki_lab_set_gemm_dry_run(0)
        lib.aki_lab_gemm_log_reset()


def _call(lib, route, splitk_bytes, splitk_offset, res8):
    from aki_amd import _lib as L
    o = route.opt
    if route.entry.startswith("qkv"):
        B, Lq, H, d = route.shape
        fp8 = route.entry == "qkv_rope_fp8"
        ldx = d + o("ldx_pad", 0)
        a = L.MmaAttnArgs(_fake(1), _fake(2), _fake(3), _fake(4), None, None, None, None, None, None, 0, B, H, Lq, 96, d, ldx, d,
                          Lq, 96 ** -0.5, L.AKI_DT_FP8_E4M3 if fp8 else L.AKI_DT_BF16, 0, Lq + o("kv_pad") if o("kv_pad") else 0,
                          _fake(5) if fp8 else None, _fake(6) if fp8 else None, _fake(7) if o("fold") else None)
        return lib.aki_qkv_rope_fwd(C.byref(a), _fake(8), _fake(9), _fake(10), None, 0, None)
    M, N, K = route.shape
    act = o("act", ACT_NONE)
    n_out = route.n_out
    fp8 = route.entry == "linear_fp8"
    ldy = n_out + o("ldy_pad", 0)
    ldx = K + o("ldx_pad", 0)
    res = o("residual", False)
    mod = o("res_row_mod", 0)
    a = L.LinearArgs(_fake(1), _fake(2), _fake(3) if o("bias") else None, _fake(4, 8 if res8 else 0) if res else None, _fake(5),
                     M, N, K, ldx, K, ldy, n_out + 8 if res else 0, mod, act,
                     L.AKI_DT_FP8_E4M3 if fp8 else L.AKI_DT_BF16, _fake(6) if fp8 else None, _fake(7) if fp8 else None)
    if o("w2") is not None:
        a.w2, a.w2_row0, a.w2_rows = _fake(8), o("w2"), N - o("w2")
    if o("fold"):
        a.row_scale = _fake(9)
        if o("fold") == "ln":
            a.row_shift, a.col_shift = _fake(10), _fake(11)
    if o("stats"):
        a.stats_rstd = _fake(12)
        a.stats_mean = _fake(13) if o("stats") == "ln" else None
        a.stats_eps = 1e-5
        a.stats_workspace, a.stats_workspace_bytes = _fake(14), lib.aki_linear_stats_workspace_bytes(M, n_out)
    if o("preact"):
        a.preact_out, a.ld_preact = _fake(15), N
    if not fp8:
        need = lib.aki_linear_splitk_workspace_bytes(M, N, K)
        if splitk_bytes is not None:
            a.splitk_workspace, a.splitk_workspace_bytes = _fake(16, splitk_offset), splitk_bytes
        elif act == ACT_NONE and M <= 2048 and need:
            a.splitk_workspace, a.splitk_workspace_bytes = _fake(16), max(need, 32 << 20)
    return lib.aki_linear_fwd(C.byref(a), None)

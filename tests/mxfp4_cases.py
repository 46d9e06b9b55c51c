"""Shared by test_mxfp4_cpu.py and test_mxfp4_gpu.py: the numpy reference of the MXFP4 weight format (float64 and integers only), the
weight families and case table of the ops.linear_w4 tests, their f64 linear reference with its tolerances, and the mutation table that
shows the cases can tell a wrong kernel from a right one.

Format (include/aki_mi355x.h, aki_quant_mxfp4): a row [K] is cut into blocks of 32 consecutive k.  Per block e = floor(log2(amax)) - 2,
scale byte = clamp(e + 127, 0, 254) (an all-zero block: 127 and zero nibbles), elements v / 2^e rounded to the nearest e2m1 magnitude
(0, 0.5, 1, 1.5, 2, 3, 4, 6), ties to the even code, saturating at 6, sign in bit 3.  Byte j of a row = k 2j (low nibble), k 2j+1 (high)."""
import functools

import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3     # aki_act

# what a WRONG implementation might do; every one must be visible in the outputs of at least one case (test_mxfp4_cpu.py)
MUTATIONS = ("nibble_order_swapped", "scale_index_off_by_one_block", "exponent_bias_126", "last_block_dropped", "saturation_at_4",
             "ties_away_from_zero", "swiglu_up_rows_at_wrong_offset")


def to_bf16(a):
    """float values rounded to bf16 (nearest even), returned as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def quant_ref(w, mutation=None):
    """bf16-valued [N, K] -> (wq uint8 [N, K/2], ws uint8 [N, K/32]) by the documented rule, in float64 and integers."""
    w = np.asarray(w, dtype=np.float64)
    N, K = w.shape
    assert K % 32 == 0 and np.isfinite(w).all()
    blk = w.reshape(N, K // 32, 32)
    amax = np.abs(blk).max(-1)
    _, ex = np.frexp(amax)                                   # amax = m * 2^ex with m in [0.5, 1): floor(log2(amax)) = ex - 1
    byte = np.where(amax > 0, np.clip(ex - 1 - 2 + 127, 0, 254), 127).astype(np.int64)
    a = np.ldexp(np.abs(blk), -(byte - 127)[..., None])      # exact: a power-of-two scaling
    d = np.abs(a[..., None] - E2M1)
    near = d == d.min(-1, keepdims=True)                     # one code, or the two neighbours of a tie
    lo, hi = near.argmax(-1), 7 - near[..., ::-1].argmax(-1)
    if mutation == "ties_away_from_zero":
        code = hi
    else:
        code = np.where(lo % 2 == 0, lo, hi)                 # neighbours differ by one: exactly one of them is even
    if mutation == "saturation_at_4":
        code = np.minimum(code, 6)
    nib = np.where(amax[..., None] > 0, code | (np.signbit(blk).astype(np.int64) << 3), 0).reshape(N, K)
    wq = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    return wq, byte.astype(np.uint8)


def dequant_ref(wq, ws, mutation=None):
    """(wq, ws) -> float64 [N, K]: nibble * 2^(byte - 127), exact."""
    wq, ws = np.asarray(wq).astype(np.int64), np.asarray(ws).astype(np.int64)
    N, K2 = wq.shape
    nib = np.empty((N, K2 * 2), dtype=np.int64)
    first, second = (wq >> 4, wq & 15) if mutation == "nibble_order_swapped" else (wq & 15, wq >> 4)
    nib[:, 0::2], nib[:, 1::2] = first, second
    val = np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7]
    if mutation == "scale_index_off_by_one_block":
        ws = np.roll(ws, -1, axis=1)
    e = ws - (126 if mutation == "exponent_bias_126" else 127)
    return (np.ldexp(val.reshape(N, -1, 32), e[..., None])).reshape(N, K2 * 2)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def x_rows(M, K):
    """bf16-valued x [M, K]: magnitudes in [0.25, 1.75) that differ from k to k (golden-ratio sequence), deterministic signs."""
    k = np.arange(K)
    out = np.empty((M, K), dtype=np.float32)
    for m in range(M):
        mag = 0.25 + 1.5 * np.modf((k + 17 * m + 1) * 0.6180339887498949)[0]
        sign = np.where(((k * 7 + (k // 3) + m * 5) % 11) < 5, -1.0, 1.0)
        out[m] = sign * mag * (1.0 + 0.125 * m)
    return to_bf16(out)


def block_exponents(N, K):
    """Amplitude exponent of every (row, block): spread over 2^-6 .. 2^3 within a row, every block position large in some row."""
    r, b = np.arange(N)[:, None], np.arange(K // 32)[None, :]
    return -6 + (r * 3 + b * 7 + (b // 10)) % 10


def weights(family, N, K, seed=0):
    """bf16-valued W [N, K].
    'spread': normal values times the block amplitudes - every block's scale byte differs from its neighbours'.
    'edges':  every block sits on the quantiser's edges: its largest value is 7 x 2^e (in (6, 8): saturates), the others are the exact ties
              0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 x 2^e; the sign of element k follows x_rows' row 0, so that a wrong tie rule shifts every
              product of a row the same way; block 1 of each row is all zero and block 2 holds a single non-zero value (5 x 2^e': a tie)."""
    rng = np.random.RandomState(1234 + seed)
    ex = block_exponents(N, K).astype(np.float64)
    nb = K // 32
    if family == "spread":
        w = rng.standard_normal((N, nb, 32)) * np.exp2(ex)[..., None]
        return to_bf16(w.reshape(N, K))
    assert family == "edges"
    ties = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    r, b, i = np.arange(N)[:, None, None], np.arange(nb)[None, :, None], np.arange(32)[None, None, :]
    w = np.where(i == (5 * r + b) % 32, 7.0, ties[(i + r + 3 * b) % 7]) * np.exp2(ex)[..., None]
    sx = np.sign(x_rows(1, K)[0]).reshape(nb, 32)
    w *= sx[None] * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None, None]
    if nb > 1:
        w[:, 1] = 0.0
    if nb > 2:
        one = np.zeros((N, 32))
        one[np.arange(N), (np.arange(N) * 3) % 32] = 5.0 * np.exp2(ex[:, 2])
        w[:, 2] = one
    return to_bf16(w.reshape(N, K))


class Case:
    def __init__(self, name, family, M, N, K, act=ACT_NONE, bias=False, residual=False, res_row_mod=0, norm=False):
        self.name, self.family, self.M, self.N, self.K = name, family, M, N, K
        self.act, self.bias, self.residual, self.res_row_mod, self.norm = act, bias, residual, res_row_mod, norm
        self.n_out = N // 2 if act == ACT_SWIGLU else N

    def __repr__(self):
        return self.name


def _cases():
    """K: 32 one block; 256 two waves per tile; 2048 exactly one 64-lane sweep; 2080 a one-lane tail; 3072 the model's d; 8192 the model's F and the
    deepest unroll.  M: 1 the GEMV, 2..16 the skinny GEMM (3 / 9: partly filled tiles; 9 and 16: no fused norm).  N: 13 and 26 (GEMV: not a
    multiple of the 8 features of a workgroup, two workgroups), 20 / 36 / 40 / 72 (skinny: N_out % 4 == 0 but no multiple of the 16-feature tile,
    more than one tile).  K = 32 / 2080 with M >= 2 and odd N lie outside the skinny GEMM's gates: ops.linear_w4 serves them row by row."""
    out = []
    kinds = [dict(), dict(bias=True), dict(residual=True), dict(act=ACT_SWIGLU), dict(norm=True), dict(norm=True, act=ACT_SWIGLU),
             dict(act=ACT_GELU_TANH, bias=True), dict(residual=True, bias=True)]
    i = 0
    for K in (32, 256, 2048, 2080, 3072, 8192):
        for M in (1, 2, 3, 8, 9, 16):
            for rep in range(2):
                kw = dict(kinds[i % len(kinds)])
                fam = "edges" if (i % 3 == 1) else "spread"
                if kw.get("residual") and M > 1:
                    kw["res_row_mod"] = (0, 2, 1)[i % 3] if M > 2 else 0
                n_out = (13, 26)[i % 2] if M == 1 else (20, 36)[i % 2]
                if rep == 1 and M == 3:
                    n_out = 13                     # an odd N_out at several rows: row by row
                N = 2 * n_out if kw.get("act") == ACT_SWIGLU else n_out
                name = f"K{K}-M{M}-N{N}-{fam}" + "".join(f"-{k}" + (str(v) if k in ("act", "res_row_mod") else "") for k, v in sorted(kw.items()))
                out.append(Case(name, fam, M, N, K, **kw))
                i += 1
    # the paths the cycle above might miss, named
    out += [Case("K3072-M1-N26-edges-swiglu", "edges", 1, 52, 3072, act=ACT_SWIGLU),
            Case("K8192-M1-N13-edges-residual", "edges", 1, 13, 8192, residual=True),
            Case("K3072-M1-N24-spread-norm-swiglu", "spread", 1, 48, 3072, act=ACT_SWIGLU, norm=True),
            Case("K8192-M8-N72-edges-swiglu", "edges", 8, 72, 8192, act=ACT_SWIGLU),
            Case("K3072-M8-N40-spread-norm-swiglu", "spread", 8, 80, 3072, act=ACT_SWIGLU, norm=True),
            Case("K2048-M4-N36-edges-norm", "edges", 4, 36, 2048, norm=True),
            Case("K8192-M16-N36-edges-residual-mod4", "edges", 16, 36, 8192, residual=True, res_row_mod=4),
            Case("K8192-M5-N20-spread-norm-bias", "spread", 5, 20, 8192, norm=True, bias=True)]
    return out


CASES = _cases()
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def inputs(case):
    """{'x', 'w', 'bias', 'residual', 'g'}: bf16-valued float32 arrays (None where the case has none).  Computed once per case, read-only."""
    c = case
    rng = np.random.RandomState(77 + c.M + c.N + c.K)
    d = dict(x=x_rows(c.M, c.K), w=weights(c.family, c.N, c.K, seed=c.M), bias=None, residual=None, g=None)
    if c.bias:
        d["bias"] = to_bf16(rng.standard_normal(c.n_out) * 4.0)
    if c.residual:
        rows = c.res_row_mod if c.res_row_mod > 0 else c.M
        d["residual"] = to_bf16(rng.standard_normal((rows, c.n_out)) * 4.0)
    if c.norm:
        d["g"] = to_bf16(1.0 + 0.2 * rng.standard_normal(c.K))
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def norm_rows(x, g, eps=EPS):
    """The fused RMSNorm with its documented rounding points (norm_bf16_kernel<true>): bf16(bf16(x * rstd) * g), rstd and both products in f32."""
    x32 = np.asarray(x, dtype=np.float32)
    rstd = (1.0 / np.sqrt((x32.astype(np.float64) ** 2).mean(-1, keepdims=True) + eps)).astype(np.float32)
    return to_bf16(to_bf16(x32 * rstd) * np.asarray(g, dtype=np.float32))


def linear_ref(case, wd, mutation=None):
    """f64 reference of ops.linear_w4 on the DEQUANTISED weights wd [N, K] -> (ref [M, n_out], tol [M, n_out])."""
    c, d = case, inputs(case)
    x = d["x"].astype(np.float64) if not c.norm else norm_rows(d["x"], d["g"]).astype(np.float64)
    wd = np.asarray(wd, dtype=np.float64)
    if mutation == "last_block_dropped":
        x, wd = x[:, :-32], wd[:, :-32]
    y = x @ wd.T
    S = np.abs(x) @ np.abs(wd).T
    if c.act == ACT_SWIGLU:
        off = c.n_out + (1 if mutation == "swiglu_up_rows_at_wrong_offset" else 0)
        up = y[:, np.minimum(off + np.arange(c.n_out), c.N - 1)]
        gate = y[:, :c.n_out]
        y = up * gate * 0.5 * (1.0 + np.tanh(0.5 * gate))          # silu(gate), overflow-free
    else:
        if c.bias:
            y = y + d["bias"].astype(np.float64)
            S = S + np.abs(d["bias"])
        if c.act == ACT_GELU_TANH:
            y = 0.5 * y * (1.0 + np.tanh(0.7978845608028654 * (y + 0.044715 * y ** 3)))
    if c.residual:
        r = d["residual"].astype(np.float64)
        r = r[np.arange(c.M) % c.res_row_mod] if c.res_row_mod > 0 else r
        y = y + r
        S = S + np.abs(r)
    if c.act != ACT_NONE:
        # the project's bar for these epilogues (tests/test_fp8_gpu.py): fast exp / rcp forms in front of the bf16 rounding
        tol = 2.0 ** -7 * np.abs(y) + 2e-3 * np.abs(y).max()
    else:
        # derived: products of bf16 pairs are exact in f32; one f32 rounding per accumulation (K * 2^-24 * S bounds their sum) and one
        # bf16 rounding of the output (2^-8 |ref|)
        tol = 2.0 ** -8 * np.abs(y) + c.K * 2.0 ** -24 * S
    return y, tol


@functools.lru_cache(maxsize=None)
def reference(case):
    """(wq, ws, ref, tol) of a case: the reference quantisation of its weights and the f64 output on the dequantised weights."""
    wq, ws = _quant_of(case, None)
    ref, tol = linear_ref(case, dequant_ref(wq, ws))
    for a in (wq, ws, ref, tol):
        a.setflags(write=False)
    return wq, ws, ref, tol


@functools.lru_cache(maxsize=None)
def _quant_of(case, mutation):
    return quant_ref(inputs(case)["w"], mutation)


@functools.lru_cache(maxsize=None)
def mutated(case, mutation):
    """The output a wrong implementation would give on this case."""
    wq, ws = _quant_of(case, mutation if mutation in ("saturation_at_4", "ties_away_from_zero") else None)
    wd = dequant_ref(wq, ws, mutation if mutation in ("nibble_order_swapped", "scale_index_off_by_one_block", "exponent_bias_126") else None)
    return linear_ref(case, wd, mutation if mutation in ("last_block_dropped", "swiglu_up_rows_at_wrong_offset") else None)[0]

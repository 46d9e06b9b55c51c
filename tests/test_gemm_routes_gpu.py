"""GPU parity of every GEMM route (tests/gemm_routes.py) against a float64 reference of the exact operands the kernel gets.

Each entry runs through aki_amd.ops on the lab library in heuristic mode (use_lab(0)); the route log must show the entry's launches,
then the output is compared with the f64 model of the epilogue (bias, GELU, residual with the row modulo on the global row, folded
RMSNorm / LayerNorm, SwiGLU, QKV + RoPE) under the suite's bar (test_kernels_gpu.check).  Operands are views into larger buffers
whose every element outside the view is NaN (rows above and below, columns past K), and the outputs sit inside buffers with a wider
row stride and guard rows that hold a bit pattern which must survive the launch.  A residual runs once 16-byte and once only 8-byte
aligned.  After a split-K or statistics launch the ticket / counter areas of the shared workspaces read zero again.
"""
import math

import numpy as np
import pytest
import torch

import aki_oracle as O
import gemm_routes as R
from test_kernels_gpu import DEV, check, n

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 0x7FA5                 # bf16 NaN with a payload: what a guard element must still hold after the launch
NAN_E4M3 = 0x7F


def _ops():
    from aki_amd import ops
    return ops


def _gen(key):
    return torch.Generator(device="cpu").manual_seed(sum(ord(c) * 131 ** i for i, c in enumerate(key)) % (1 << 31))


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _nan_view(data, col0=8, pad=16):
    """`data` [rows, cols] copied into a NaN-filled buffer of rows + 2 rows and a row stride of col0 + cols + pad elements (e4m3
    bytes: 0x7F, the e4m3 NaN)."""
    rows, cols = data.shape
    fill = NAN_E4M3 if data.dtype == torch.uint8 else float("nan")
    buf = torch.full((rows + 2, col0 + cols + pad), fill, dtype=data.dtype, device=DEV)
    v = buf[1:1 + rows, col0:col0 + cols]
    v.copy_(data)
    return v


def _nan_vec(data, off=4):
    buf = torch.full((data.numel() + 2 * off,), float("nan"), dtype=data.dtype, device=DEV)
    v = buf[off:off + data.numel()]
    v.copy_(data)
    return v


class Guarded:
    """A [rows, cols] output view inside a buffer with `pad` extra columns and a guard row above and below, filled with GUARD."""

    def __init__(self, rows, cols, pad, dtype=BF):
        self.buf = torch.empty((rows + 2, cols + pad), dtype=dtype, device=DEV)
        self.buf.view(torch.int16 if dtype == BF else torch.int32).fill_(GUARD)
        self.view = self.buf[1:1 + rows, :cols]
        self.rows, self.cols = rows, cols

    def assert_guard(self, what):
        mask = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        mask[1:1 + self.rows, :self.cols] = False
        bits = self.buf.view(torch.int16 if self.buf.dtype == BF else torch.int32)[mask]
        bad = int((bits != GUARD).sum())
        assert bad == 0, f"{what}: {bad} elements outside the output view were written"


def _gelu(a, act):
    if act == R.ACT_GELU_ERF:
        return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))


def _silu(a):
    return a / (1.0 + torch.exp(-a))


def _f64_bf16(a):
    """Round f64 values to bf16 and back: the kernel's contract for values it stores and then reuses (preact_out)."""
    return a.to(torch.float32).to(BF).to(torch.float64)


def _counters_zero(what):
    ops = _ops()
    for ws in ops._SPLITK_WS.values():
        nz = int((ws[:64 << 10] != 0).sum())
        assert nz == 0, f"{what}: {nz} bytes of the split-K ticket area are not zero after the launch"
    for ws in ops._STATS_WS.values():
        nz = int((ws[:1 << 20] != 0).sum())
        assert nz == 0, f"{what}: {nz} bytes of the statistics counter area are not zero after the launch"


def _assert_records(lib, route, res8):
    from aki_amd import _lib
    got = _lib.gemm_log(lib)
    want = list(route.expect_res8 or route.expect) if res8 else list(route.expect)
    assert got == want, f"{route.id}: launched {got}, expected {want}"


def run_linear(route, res8=False, seed=""):
    """Run a linear / linear_fp8 route on the lab library; returns (output, f64 reference, extras) after asserting the route log."""
    from aki_amd import _lib
    ops = _ops()
    o = route.opt
    M, N, K = route.shape
    act, n_out = o("act", R.ACT_NONE), route.n_out
    fp8 = route.entry == "linear_fp8"
    g = _gen(route.id + seed)
    x = _randn(g, M, K)
    w = _randn(g, N, K, scale=1.0 / math.sqrt(K))
    ex = {}
    if fp8:
        xs = (0.5 + torch.rand(M, generator=g)).to(DEV)
        ws = (0.5 + torch.rand(N, generator=g)).to(DEV)
        xq = _nan_view(x.to(torch.float8_e4m3fn).view(torch.uint8), col0=16)
        wq = _nan_view(w.mul(8.0).to(torch.float8_e4m3fn).view(torch.uint8), col0=16)
        X = xq.view(torch.float8_e4m3fn).double() * xs.double()[:, None]
        W = wq.view(torch.float8_e4m3fn).double() * ws.double()[:, None]
    else:
        xv, wv = _nan_view(x.to(BF), pad=max(16, o("ldx_pad", 0))), _nan_view(w.to(BF))
        X, W = xv.double(), wv.double()
    bias = _nan_vec(_randn(g, n_out, scale=0.5).to(BF)) if o("bias") else None
    res = None
    if o("residual"):
        rows = o("res_row_mod") or M
        rbuf = torch.full((rows + 2, (n_out + 7) // 8 * 8 + 16), float("nan"), dtype=BF, device=DEV)   # row starts 16-byte aligned
        c0 = 4 if res8 else 8
        res = rbuf[1:1 + rows, c0:c0 + n_out]
        res.copy_(_randn(g, rows, n_out).to(BF))
        assert (res.data_ptr() % 16 == 0) != res8
    kw = dict(bias=bias, residual=res, act=act, res_row_mod=o("res_row_mod", 0))
    with _lib.use_lab(0) as lib:
        lib.aki_lab_gemm_log_reset()
        if fp8:
            y = ops.linear_fp8(xq, xs, wq, ws, bias=bias, residual=res, act=act)
            out = None
        else:
            out = Guarded(M, n_out, o("ldy_pad") or 8)
            if o("fold"):
                rs = (0.5 + torch.rand(M, generator=g)).to(DEV)
                kw["row_scale"] = _nan_vec(rs)
                if o("fold") == "ln":
                    kw["row_shift"] = _nan_vec(_randn(g, M, scale=0.3))
                    kw["col_shift"] = _randn(g, N, scale=0.5).float()
            if o("stats"):
                st = ops.RowStats(_nan_vec(torch.zeros(M, device=DEV)), _nan_vec(torch.zeros(M, device=DEV)) if o("stats") == "ln" else None)
                kw.update(stats_out=st, stats_eps=1e-5)
                ex["stats"] = st
            if o("preact"):
                pre = Guarded(M, N, 8)
                kw["preact_out"] = pre.view
                ex["preact"] = pre
            if o("w2") is not None:
                r0 = o("w2")
                w2v = _nan_view(w[r0:].to(BF))
                kw.update(w2=w2v, w2_row0=r0)
                wv = _nan_view(w[:r0].to(BF))
                W = torch.cat([wv.double(), w2v.double()])
            y = ops.linear(xv, wv, out=out.view, **kw)
        torch.cuda.synchronize()
        _assert_records(lib, route, res8)
    acc = X @ W.T
    if o("fold"):
        rs = kw["row_scale"].double()[:, None]
        acc = rs * (acc - kw["row_shift"].double()[:, None] * kw["col_shift"].double()[None, :]) if o("fold") == "ln" else rs * acc
    if act == R.ACT_SWIGLU:
        if o("preact"):
            ex["preact_ref"] = acc
            acc = _f64_bf16(acc)
        want = acc[:, n_out:] * _silu(acc[:, :n_out])
    else:
        if bias is not None:
            acc = acc + bias.double()
        want = _gelu(acc, act) if act in (R.ACT_GELU_ERF, R.ACT_GELU_TANH) else acc
        if res is not None:
            rows = torch.arange(M, device=DEV) % (o("res_row_mod") or M)
            want = want + res.double()[rows]
    return y, want, out, ex


def _check_stats(y, st, ln, what):
    yd = n(y).astype(np.float64)
    if ln:
        mu = yd.mean(-1)
        rstd = 1.0 / np.sqrt(((yd - mu[:, None]) ** 2).mean(-1) + 1e-5)
        np.testing.assert_allclose(n(st.mean), mu, rtol=3e-5, atol=2e-6, err_msg=what + ": mean")
    else:
        rstd = 1.0 / np.sqrt((yd * yd).mean(-1) + 1e-5)
    np.testing.assert_allclose(n(st.rstd), rstd, rtol=3e-5, err_msg=what + ": rstd")


def _positions(route):
    B, L = route.shape[:2]
    if not route.opt("pos"):
        return None, np.tile(np.arange(L), (B, 1))
    pos = np.stack([np.arange(L)[::-1] if b % 2 else (np.arange(L) * 7 + 3 * b) % L for b in range(B)]).astype(np.int64)
    return torch.from_numpy(pos).to(DEV), pos


def run_qkv(route, seed=""):
    from aki_amd import _lib
    ops = _ops()
    o = route.opt
    B, L, H, d = route.shape
    fp8 = route.entry == "qkv_rope_fp8"
    g = _gen(route.id + seed)
    x = _randn(g, B * L, d)
    w = _randn(g, 3 * H * 96, d, scale=1.0 / math.sqrt(d))
    cos, sin = O.rope_cos_sin(np.arange(L)[None], 96)
    cos_t, sin_t = torch.from_numpy(cos[0]).to(DEV), torch.from_numpy(sin[0]).to(DEV)
    pos_t, pos = _positions(route)
    cap = L + (o("kv_pad") or 0)
    kv = [Guarded(B * H * cap, 96, 0) for _ in range(2)]
    kv_out = [k.buf[1:1 + B * H * cap].view(B, H, cap, 96) for k in kv]
    rs = None
    with _lib.use_lab(0) as lib:
        lib.aki_lab_gemm_log_reset()
        if fp8:
            xs = (0.5 + torch.rand(B * L, generator=g)).to(DEV)
            ws = (0.5 + torch.rand(3 * H * 96, generator=g)).to(DEV)
            xq = _nan_view(x.to(torch.float8_e4m3fn).view(torch.uint8), col0=16)
            wq = _nan_view(w.mul(8.0).to(torch.float8_e4m3fn).view(torch.uint8), col0=16)
            q, k, v = ops.qkv_rope_fp8(xq, xs, wq, ws, cos_t, sin_t, B, H, position_ids=pos_t, k_out=kv_out[0], v_out=kv_out[1])
            X = xq.view(torch.float8_e4m3fn).double() * xs.double()[:, None]
            W = wq.view(torch.float8_e4m3fn).double() * ws.double()[:, None]
        else:
            xv, wv = _nan_view(x.to(BF)), _nan_view(w.to(BF))
            if o("fold"):
                rs = _nan_vec((0.5 + torch.rand(B * L, generator=g)).to(DEV))
            q, k, v = ops.qkv_rope(xv.view(B, L, d), wv, cos_t, sin_t, H, position_ids=pos_t, k_out=kv_out[0], v_out=kv_out[1], row_scale=rs)
            X, W = xv.double(), wv.double()
        torch.cuda.synchronize()
        _assert_records(lib, route, False)
    qkv = X @ W.T
    if rs is not None:
        qkv = qkv * rs.double()[:, None]
    qkv = qkv.view(B, L, 3, H, 96).permute(2, 0, 3, 1, 4)          # [3, B, H, L, 96]
    c = torch.from_numpy(cos[0][pos]).to(DEV).double()[:, None]    # [B, 1, L, 96]
    s = torch.from_numpy(sin[0][pos]).to(DEV).double()[:, None]
    rot = lambda a: torch.cat([-a[..., 48:], a[..., :48]], -1)
    want = [qkv[0] * c + rot(qkv[0]) * s, qkv[1] * c + rot(qkv[1]) * s, qkv[2]]
    for kk, name in zip(kv, ("k", "v")):
        inside = kk.buf[1:1 + B * H * cap].view(B, H, cap, 96)
        if cap > L:                                                  # the KV-cache rows past L belong to nobody
            tail = inside[:, :, L:].reshape(-1).view(torch.int16)
            assert int((tail != GUARD).sum()) == 0, f"{route.id}: {name} cache rows past L were written"
        kk.assert_guard(f"{route.id}: {name} buffer")
    return (q, k[:, :, :L], v[:, :, :L]), want


@pytest.mark.parametrize("rid", R.ROUTE_IDS)
def test_route_parity(rid):
    route = R.by_id(rid)
    if route.entry.startswith("qkv"):
        got, want = run_qkv(route)
        for name, a, b in zip("qkv", got, want):
            check(n(a), b.cpu().numpy(), BF, f"route {rid}: {name}")
        return
    for res8 in ([False, True] if route.opt("residual") else [False]):
        tag = f"route {rid}" + (" (residual 8-byte aligned)" if res8 else "")
        y, want, out, ex = run_linear(route, res8)
        if out is not None:
            out.assert_guard(tag)
        check(n(y), want.cpu().numpy(), BF, tag)
        if "preact" in ex:
            ex["preact"].assert_guard(tag + ": preact_out")
            check(n(ex["preact"].view), ex["preact_ref"].cpu().numpy(), BF, tag + ": preact_out")
        if "stats" in ex:
            _check_stats(y, ex["stats"], route.opt("stats") == "ln", tag)
        if route.uses_splitk or "stats" in ex:
            _counters_zero(tag)


def test_splitk_3_2_3_on_one_workspace_and_repeatable():
    """ksplit 3, then 2, then 3 again through the one cached workspace: every launch correct, the tickets zero after each, and the
    same split-K launch twice is bit-identical (the fold adds the slices in slice order, whatever order they arrive in)."""
    ops = _ops()
    seq = ["splitk3-k2368", "splitk2-k2368", "splitk3-k2368"]
    firsts = {}
    for i, rid in enumerate(seq):
        route = R.by_id(rid)
        y, want, out, _ = run_linear(route)
        check(n(y), want.cpu().numpy(), BF, f"{rid} (sequence step {i})")
        out.assert_guard(rid)
        _counters_zero(f"{rid} (sequence step {i})")
        if rid in firsts:
            assert torch.equal(y, firsts[rid]), f"{rid}: a repeated split-K launch is not bit-identical"
        firsts[rid] = y.clone()
    assert len(ops._SPLITK_WS) >= 1
    y2, _, _, _ = run_linear(R.by_id("splitk2-k2368"))
    assert torch.equal(y2, firsts["splitk2-k2368"]), "splitk2-k2368: a repeated split-K launch is not bit-identical"

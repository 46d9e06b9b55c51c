"""Torch-tensor front end of the C ABI (include/aki_mi355x.h).

PyTorch is plumbing here: device memory, the current HIP stream and autograd bookkeeping.  Every
function below hands raw device pointers to libaki_mi355x.so; there is NO eager/CPU fallback -
CPU tensors or a missing library raise :class:`aki_amd._lib.AkiError`.
"""
from __future__ import annotations

import ctypes as C
import struct
import threading
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import AkiError

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_SWIGLU = L.AKI_ACT_NONE, L.AKI_ACT_GELU_ERF, L.AKI_ACT_GELU_TANH, L.AKI_ACT_SWIGLU
DEAD_ROWS_ZERO, DEAD_ROWS_UNIFORM = L.AKI_DEAD_ROWS_ZERO, L.AKI_DEAD_ROWS_UNIFORM


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return L.AKI_DT_BF16
    if t.dtype == torch.float32:
        return L.AKI_DT_F32
    raise AkiError(f"unsupported dtype {t.dtype}: the AKI HIP path computes in bf16 or f32")


def _dev(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise AkiError("the AKI MMA path runs on MI355X only: got a CPU tensor and there is no CPU fallback")
        dev = dev or t.device
        if t.device != dev:
            raise AkiError("tensors on different devices")
    return dev


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _rows2d(t: torch.Tensor) -> torch.Tensor:
    """View as [rows, cols] with unit inner stride (copy only if the layout forces it)."""
    t2 = t.reshape(-1, t.shape[-1])
    if t2.stride(-1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]):
        t2 = t2.contiguous()
    return t2


def _ws(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


class EventTap:
    """Optional per-kernel timing with HIP events on the stream the kernels are launched on (torch's current
    stream).  bench.py installs one for the timed region; when no tap is installed the cost is one `is None` test."""

    def __init__(self, tags=None, select=None, every=1):
        self.tags = tags          # None = every tagged launch
        self.select = select      # optional predicate on the full tag (e.g. only one GEMM shape): every bracketed launch
        self.events = {}          # costs two event records on the stream (~6 us of dispatch gap each on MI355X, see
        self.every = every        # tools/trace_gaps.py), so time only what is reported - and only every `every`-th launch of it
        self.calls = {}

    def want(self, tag) -> bool:
        if self.tags is not None and tag[0] not in self.tags:
            return False
        return self.select is None or bool(self.select(tag))

    def begin(self, tag):
        n = self.calls[tag] = self.calls.get(tag, 0) + 1
        if (n - 1) % self.every:
            return None
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        self.events.setdefault(tag, []).append((a, b))
        a.record()
        return b

    def summary(self):
        torch.cuda.synchronize()
        return {tag: (self.calls[tag], sum(a.elapsed_time(b) for a, b in ev) / len(ev)) for tag, ev in self.events.items()}


class Prepared:
    """Cache of one-time weight transforms (K padding, QKV concatenation, folded norm gains), rebuilt when a parameter changes
    (version counter, storage, dtype, device) or when the trainer announces raw-pointer weight writes (`epoch`)."""

    def __init__(self):
        self._c = {}

    def get(self, name, params, fn, epoch=0):
        key = (epoch,) + tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)
        hit = self._c.get(name)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                self._c[name] = (key, fn())
        return self._c[name][1]

    def clear(self) -> None:
        """Drop every cached transform (model.train(): the folded copies are only read by inference forwards)."""
        self._c.clear()


def fold_gain(w: torch.Tensor, gain: torch.Tensor) -> torch.Tensor:
    """W' = W * diag(gain), rounded once to W's dtype: x_normed(gain) @ W^T == (x * rstd) @ W'^T up to that rounding."""
    ct = torch.float64 if w.dtype == torch.float64 else torch.float32          # computed in f32 (f64 stays f64), rounded once
    return (w.detach().to(ct) * gain.detach().to(ct)[None, :]).to(w.dtype).contiguous()


@dataclass
class RowStats:
    """Per-row statistics of an activation [M, N], produced by the epilogue of the GEMM that wrote it (or by `row_stats`) and
    consumed by the next GEMM as `row_scale` / `row_shift`: the block's pre-norm then costs no launch of its own.
    The GEMM takes the LayerNorm variance as s2 / N - mean^2 in f32: the relative error of its `rstd` grows as 1 + 2 (mean/std)^2 of the
    row (about 2e-7 at mean = 0, 3e-4 at 32 and 5e-3 at 128 standard deviations; bound in tests/norm_fold_cases.py); `row_stats` (two-pass
    variance) does not have this growth."""
    rstd: torch.Tensor                      # f32 [M]: 1/sqrt(mean(y^2) + eps) (RMSNorm) or 1/sqrt(var(y) + eps) (LayerNorm)
    mean: Optional[torch.Tensor] = None     # f32 [M] (LayerNorm only)


_STATS_WS = {}


def _stats_ws(M: int, n_out: int, dev) -> torch.Tensor:
    """Workspace of the producer side (arrival counters + partial sums): zero-filled once per (device, stream).  The counter
    area at its front has one size for every M (include/aki_mi355x.h), so a buffer serves launches of any size in any order."""
    need = int(L.load().aki_linear_stats_workspace_bytes(M, n_out))
    key = (torch.device(dev).index, torch.cuda.current_stream().cuda_stream)
    hit = _STATS_WS.get(key)
    if hit is None or hit.numel() < need:
        hit = _STATS_WS[key] = torch.zeros(max(need, 8 << 20), dtype=torch.uint8, device=dev)
    return hit


_SPLITK_WS = {}
SPLITK_WS_MIN_BYTES = 0          # tools / tests: a floor for the split-K workspace (the lab library's forced splits need more than the planner's)
SPLITK_MAX_M = 2048              # rows above which linear() hands no split-K workspace over (the planner splits below 1024 only; tools raise it)


def _splitk_ws(M: int, N: int, K: int, dev) -> Optional[torch.Tensor]:
    """Split-K workspace (tickets + f32 partial tiles; include/aki_mi355x.h): zero-filled once per (device, stream), None when the
    library never splits this shape."""
    need = max(int(L.load().aki_linear_splitk_workspace_bytes(M, N, K)), SPLITK_WS_MIN_BYTES)
    if need == 0:
        return None
    key = (torch.device(dev).index, torch.cuda.current_stream().cuda_stream)
    hit = _SPLITK_WS.get(key)
    if hit is None or hit.numel() < need:
        hit = _SPLITK_WS[key] = torch.zeros(max(need, 32 << 20), dtype=torch.uint8, device=dev)
    return hit


def new_stats(M: int, dev, ln: bool = False) -> RowStats:
    return RowStats(torch.empty((M,), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev) if ln else None)


def row_stats(x: torch.Tensor, eps: float, ln: bool = False) -> RowStats:
    """Statistics of a tensor no GEMM of this library produced (the first block's input): one HBM pass, no output tensor."""
    dev = _dev(x)
    x2 = _rows2d(x)
    st = new_stats(x2.shape[0], dev, ln)
    L.check(L.load().aki_row_stats(_ptr(x2), x2.shape[0], x2.shape[1], x2.stride(0), float(eps), _ptr(st.rstd), _ptr(st.mean), _dt(x),
                                   _stream()), "aki_row_stats")
    return st


_TAP: Optional[EventTap] = None


def set_event_tap(tap: Optional[EventTap]) -> None:
    global _TAP
    _TAP = tap


# ------------------------------------------------------------------------------------------------
@dataclass
class MaskTable:
    """Device-resident description of the modality-mutual mask (what replaces the dense (B,1,L,L) tensor)."""
    rects: Optional[torch.Tensor]          # int32 [B, max_rects, 4]
    col_valid_bits: Optional[torch.Tensor]  # int64 (bit pattern of uint64) [B, ceil(L/64)]
    seq_lens: Optional[torch.Tensor]       # int32 [B]
    L: int
    mask_1d: Optional[torch.Tensor] = None  # int64 [B, L] spliced 1-D mask (for callers that want it)

    @property
    def max_rects(self) -> int:
        return 0 if self.rects is None else int(self.rects.shape[1])

    def token_counts(self, B: int, device) -> torch.Tensor:
        """int32 [B]: index of the last valid column + 1 (the sample's own length when right-padded; L when left-padded).
        NOT `seq_lens`, which is the reference mask's causal extent (the padded length for samples that hold an image)."""
        if self.col_valid_bits is None:
            return torch.full((B,), self.L, dtype=torch.int32, device=device)
        nw = self.col_valid_bits.shape[1]
        shifts = torch.arange(64, device=device, dtype=torch.int64)
        valid = ((self.col_valid_bits[:, :, None] >> shifts) & 1).view(B, nw * 64)[:, : self.L]
        pos = torch.arange(1, self.L + 1, device=device, dtype=torch.int64)
        return (valid * pos).amax(dim=1).to(torch.int32)

    @staticmethod
    def causal(B: int, Lq: int, device) -> "MaskTable":
        return MaskTable(None, None, None, Lq)

    @staticmethod
    def from_host(rects, mask_1d, seq_lens, device) -> "MaskTable":
        """rects: [B][k] of (row_lo,row_hi,col_lo,col_hi); mask_1d: bool/int [B,L]; seq_lens: [B] or None."""
        import numpy as np
        m = np.asarray(mask_1d).astype(bool)
        B, Lq = m.shape
        k = max(1, max(len(r) for r in rects))
        ra = np.zeros((B, k, 4), dtype=np.int32)
        for b, rs in enumerate(rects):
            for i, r in enumerate(rs):
                ra[b, i] = r
        nw = (Lq + 63) // 64
        pad = np.zeros((B, nw * 64), dtype=bool)
        pad[:, :Lq] = m
        bits = np.packbits(pad.reshape(B, nw, 64), axis=-1, bitorder="little").view(np.uint64).reshape(B, nw)
        t = MaskTable(torch.from_numpy(ra).to(device), torch.from_numpy(bits.view(np.int64).copy()).to(device),
                      None if seq_lens is None else torch.tensor(list(seq_lens), dtype=torch.int32, device=device), Lq,
                      torch.from_numpy(m.astype(np.int64)).to(device))
        return t


# ------------------------------------------------------------------------------------------------
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           act: int = ACT_NONE, res_row_mod: int = 0, out: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
           w2_row0: int = 0, n_rows: Optional[int] = None, row_scale: Optional[torch.Tensor] = None,
           row_shift: Optional[torch.Tensor] = None, col_shift: Optional[torch.Tensor] = None,
           stats_out: Optional[RowStats] = None, stats_eps: float = 0.0, preact_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(x W^T + bias) [+ residual]; W is an nn.Linear weight [N,K] (K a multiple of 64 for bf16).
    `preact_out` (act SWIGLU, bf16; the training forward): [M, N] buffer that receives the pre-activations g | u; y is then the
    activation of those bf16 values - what linear + swiglu_fwd compute, in one launch.
    Two-segment weight (DecoupledLinear, src/helpers.py:594-603): with `w2`, logical weight row r is w[r] for r < w2_row0 and
    w2[r - w2_row0] beyond; `n_rows` = logical rows (output width, may include padding columns that repeat w2's last row).
    Folded normalisation (see include/aki_mi355x.h, aki_linear_args): `row_scale` / `row_shift` / `col_shift` apply the input's
    RMSNorm / LayerNorm in the epilogue (w then carries the gain), `stats_out` makes this GEMM produce the statistics of ITS
    output for the next one."""
    dev = _dev(x, w, bias, residual, out, w2, row_scale, row_shift, col_shift)
    lib = L.load()
    x2 = _rows2d(x)
    M, K = x2.shape
    N = w.shape[0] if w2 is None else int(n_rows if n_rows is not None else w2_row0 + w2.shape[0])
    if w2 is not None and (w2.shape[1] != K or w2.stride(1) != 1 or w2.stride(0) != w.stride(0) or not 0 < w2_row0 <= w.shape[0]):
        raise AkiError("linear: the second weight segment must have the layout of the first")
    if w.shape[1] != K or w.stride(1) != 1:
        raise AkiError(f"linear: weight {tuple(w.shape)} does not match input K={K}")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out is None:
        out = torch.empty((*x.shape[:-1], n_out), dtype=x.dtype, device=dev)
    o2 = out.view(-1, out.shape[-1])
    if o2.shape != (M, n_out) or o2.stride(1) != 1:
        raise AkiError("linear: bad output buffer")
    r2 = None
    if residual is not None:
        r2 = _rows2d(residual)
    a = L.LinearArgs(_ptr(x2), _ptr(w), _ptr(bias), _ptr(r2), _ptr(o2), M, N, K, x2.stride(0), w.stride(0), o2.stride(0),
                     0 if r2 is None else r2.stride(0), res_row_mod, act, _dt(x), None, None,
                     _ptr(w2), int(w2_row0) if w2 is not None else 0, int(w2.shape[0]) if w2 is not None else 0)
    a.row_scale, a.row_shift, a.col_shift = _ptr(row_scale), _ptr(row_shift), _ptr(col_shift)
    if stats_out is not None:
        sws = _stats_ws(M, n_out, dev)
        a.stats_rstd, a.stats_mean, a.stats_eps = _ptr(stats_out.rstd), _ptr(stats_out.mean), float(stats_eps)
        a.stats_workspace, a.stats_workspace_bytes = sws.data_ptr(), sws.numel()
    if preact_out is not None:
        p2 = preact_out.view(-1, preact_out.shape[-1])
        if act != ACT_SWIGLU or p2.shape != (M, N) or p2.stride(1) != 1 or p2.dtype != torch.bfloat16 or p2.device != x2.device:
            raise AkiError("linear: preact_out must be a bf16 [M, N] buffer of an act=SWIGLU launch")
        a.preact_out, a.ld_preact = p2.data_ptr(), p2.stride(0)
    if act == ACT_NONE and M <= SPLITK_MAX_M and x.dtype == torch.bfloat16:
        sk = _splitk_ws(M, N, K, dev)
        if sk is not None:
            a.splitk_workspace, a.splitk_workspace_bytes = sk.data_ptr(), sk.numel()
    end = _TAP.begin(("linear", M, N, K, act)) if (_TAP is not None and _TAP.want(("linear", M, N, K, act))) else None
    L.check(lib.aki_linear_fwd(C.byref(a), _stream()), "aki_linear_fwd")
    if end is not None:
        end.record()
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    dev = _dev(x, w)
    x2 = _rows2d(x)
    y = torch.empty_like(x2)
    L.check(L.load().aki_rmsnorm_fwd(_ptr(x2), _ptr(w), _ptr(y), x2.shape[0], x2.shape[1], x2.stride(0), y.stride(0),
                                     float(eps), _dt(x), _stream()), "aki_rmsnorm_fwd")
    return y.reshape(x.shape)


def layernorm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    dev = _dev(x, w, b)
    x2 = _rows2d(x)
    y = torch.empty_like(x2)
    L.check(L.load().aki_layernorm_fwd(_ptr(x2), _ptr(w), _ptr(b), _ptr(y), x2.shape[0], x2.shape[1], x2.stride(0),
                                       y.stride(0), float(eps), _dt(x), _stream()), "aki_layernorm_fwd")
    return y.reshape(x.shape)


def mma_attn_core(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, table: MaskTable, scale: float,
                  dead_rows: int = DEAD_ROWS_UNIFORM, return_lse: bool = False):
    """q [B,H,L,Dh]; k,v [B,H,cap,Dh] with cap >= L (cap > L: a KV cache whose first L rows are used) -> o [B,L,H*Dh]."""
    dev = _dev(q, k, v)
    B, H, Lq, Dh = q.shape
    cap = k.shape[2]
    if v.shape[2] != cap or cap < Lq:
        raise AkiError("mma_attn_core: k/v capacity mismatch")
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    o = torch.empty((B, Lq, H * Dh), dtype=q.dtype, device=dev)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=dev) if return_lse else None
    lib = L.load()
    ws = _ws(lib.aki_mma_attn_core_workspace_bytes(B, H, Lq, Dh, _dt(q)), dev)
    a = L.MmaAttnCoreArgs(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(table.rects), _ptr(table.col_valid_bits),
                          _ptr(table.seq_lens), table.max_rects, B, H, Lq, Dh, float(scale), _dt(q), dead_rows,
                          0 if cap == Lq else cap)
    end = _TAP.begin(("mma_attn_core", B, H, Lq, Dh)) if (_TAP is not None and _TAP.want(("mma_attn_core",))) else None
    L.check(lib.aki_mma_attn_core_fwd(C.byref(a), _ptr(ws), ws.numel(), _stream()), "aki_mma_attn_core_fwd")
    if end is not None:
        end.record()
    return (o, lse) if return_lse else o


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, return_lse: bool = False):
    """Plain multi-head attention for the vision side.  q [B,Lq,H,Dh], k/v [B,Lk,H,Dh] as (possibly strided) VIEWS of
    the projection outputs (channel stride 1) -> o [B,Lq,H*Dh].  bf16 reads the views in place; f32 (parity path)
    gathers them into contiguous head-major tensors first."""
    dev = _dev(q, k, v)
    B, Lq, H, Dh = q.shape
    Lk = k.shape[1]
    o = torch.empty((B, Lq, H * Dh), dtype=q.dtype, device=dev)
    lib = L.load()
    if q.dtype == torch.float32:
        if Lq > Lk:
            raise AkiError(f"attention: the f32 parity path needs Lq <= Lk (its kernel is square and shorter queries are padded to Lk rows); got Lq = {Lq}, Lk = {Lk}")
        if Lq != Lk:  # the f32 parity kernel is square: pad the queries (extra rows are discarded)
            qp = torch.zeros((B, Lk, H, Dh), dtype=q.dtype, device=dev)
            qp[:, :Lq] = q
            return attention(qp, k, v, scale)[:, :Lq].contiguous()
        q, k, v = (t_.permute(0, 2, 1, 3).contiguous() for t_ in (q, k, v))     # [B,H,L,Dh]
        st = lambda t_: (t_.stride(0), t_.stride(1), t_.stride(2))
    else:
        for t_ in (q, k, v):
            if t_.stride(3) != 1:
                raise AkiError("attention: channel stride must be 1")
        st = lambda t_: (t_.stride(0), t_.stride(2), t_.stride(1))               # (batch, head, token)
    ws = _ws(B * H * Dh * 4 + 256, dev)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=dev) if return_lse else None
    if return_lse and q.dtype != torch.bfloat16:
        raise AkiError("attention: the log-sum-exp output exists on the bf16 path only")
    a = L.AttnArgs(_ptr(q), _ptr(k), _ptr(v), _ptr(o), *st(q), *st(k), *st(v), B, H, Lq, Lk, Dh, float(scale), _dt(q), _ptr(lse))
    end = _TAP.begin(("attention", B, H, Lq, Lk, Dh)) if (_TAP is not None and _TAP.want(("attention",))) else None
    L.check(lib.aki_attn_fwd(C.byref(a), _ptr(ws), ws.numel(), _stream()), "aki_attn_fwd")
    if end is not None:
        end.record()
    return (o, lse) if return_lse else o


def _fused_args(x2, w_qkv, cos, sin, position_ids, o, lse, table, B, H, Lq, Dh, scale, dead_rows, kv_capacity=0, row_scale=None):
    return L.MmaAttnArgs(_ptr(x2), _ptr(w_qkv), _ptr(cos), _ptr(sin), _ptr(position_ids), _ptr(o), _ptr(lse),
                         _ptr(table.rects), _ptr(table.col_valid_bits), _ptr(table.seq_lens), table.max_rects,
                         B, H, Lq, Dh, x2.shape[1], x2.stride(0), w_qkv.stride(0), cos.shape[0], float(scale),
                         _dt(x2), dead_rows, kv_capacity, None, None, _ptr(row_scale))


def mma_attn(x: torch.Tensor, w_qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, table: MaskTable, num_heads: int,
             scale: Optional[float] = None, position_ids: Optional[torch.Tensor] = None,
             dead_rows: int = DEAD_ROWS_UNIFORM, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused QKV projection + RoPE + span-driven attention.  x [B,L,d] -> o [B,L,H*Dh] (before o_proj).
    cos/sin: f32 [pos_rows, Dh].  row_scale: folded input RMSNorm (x raw, w_qkv carries the gain)."""
    dev = _dev(x, w_qkv, cos, sin, position_ids, row_scale)
    B, Lq, d = x.shape
    Dh = w_qkv.shape[0] // (3 * num_heads)
    x2 = _rows2d(x)
    cos = cos.to(torch.float32).reshape(-1, Dh).contiguous()
    sin = sin.to(torch.float32).reshape(-1, Dh).contiguous()
    if position_ids is not None:
        position_ids = position_ids.to(torch.int32).expand(B, Lq).contiguous()
    o = torch.empty((B, Lq, num_heads * Dh), dtype=x.dtype, device=dev)
    lib = L.load()
    ws = _ws(lib.aki_mma_attn_workspace_bytes(B, num_heads, Lq, Dh, _dt(x)), dev)
    a = _fused_args(x2, w_qkv, cos, sin, position_ids, o, None, table, B, num_heads, Lq, Dh,
                    scale if scale is not None else Dh ** -0.5, dead_rows, row_scale=row_scale)
    end = _TAP.begin(("mma_attn", B, num_heads, Lq, Dh)) if (_TAP is not None and _TAP.want(("mma_attn",))) else None
    L.check(lib.aki_mma_attn_fwd(C.byref(a), _ptr(ws), ws.numel(), _stream()), "aki_mma_attn_fwd")
    if end is not None:
        end.record()
    return o


def qkv_rope(x: torch.Tensor, w_qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, num_heads: int,
             position_ids: Optional[torch.Tensor] = None, k_out: Optional[torch.Tensor] = None,
             v_out: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Stage 1 of the fused op: rotated q [B,H,L,Dh], rotated k and v.  With k_out / v_out ([B,H,cap,Dh], cap >= L)
    the keys/values are written straight into a KV cache (prefill)."""
    dev = _dev(x, w_qkv, cos, sin, k_out, v_out)
    B, Lq, d = x.shape
    Dh = w_qkv.shape[0] // (3 * num_heads)
    x2 = _rows2d(x)
    cos = cos.to(torch.float32).reshape(-1, Dh).contiguous()
    sin = sin.to(torch.float32).reshape(-1, Dh).contiguous()
    if position_ids is not None:
        position_ids = position_ids.to(torch.int32).expand(B, Lq).contiguous()
    q = torch.empty((B, num_heads, Lq, Dh), dtype=x.dtype, device=dev)
    if k_out is None:
        k_out = torch.empty((B, num_heads, Lq, Dh), dtype=x.dtype, device=dev)
        v_out = torch.empty((B, num_heads, Lq, Dh), dtype=x.dtype, device=dev)
    cap = k_out.shape[2]
    if not (k_out.is_contiguous() and v_out.is_contiguous()) or v_out.shape != k_out.shape or cap < Lq:
        raise AkiError("qkv_rope: bad KV output buffers")
    a = _fused_args(x2, w_qkv, cos, sin, position_ids, None, None, MaskTable(None, None, None, Lq), B, num_heads, Lq, Dh,
                    Dh ** -0.5, 0, 0 if cap == Lq else cap, row_scale=row_scale)
    ws = _ws(B * Lq * 3 * num_heads * Dh * 4 if x.dtype == torch.float32 else 256, dev)
    L.check(L.load().aki_qkv_rope_fwd(C.byref(a), _ptr(q), _ptr(k_out), _ptr(v_out), _ptr(ws), ws.numel(), _stream()),
            "aki_qkv_rope_fwd")
    return q, k_out, v_out


def rope_append(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, cache_len: torch.Tensor,
                k_cache: torch.Tensor, v_cache: torch.Tensor, num_heads: int) -> torch.Tensor:
    """Decode step: qkv [B, 3*H*Dh] of the new tokens -> rotated q [B,H,Dh]; k/v appended to the caches in place."""
    dev = _dev(qkv, cos, sin, pos, cache_len, k_cache, v_cache)
    B = qkv.shape[0]
    Dh = qkv.shape[1] // (3 * num_heads)
    q = torch.empty((B, num_heads, Dh), dtype=qkv.dtype, device=dev)
    L.check(L.load().aki_rope_append_fwd(_ptr(qkv.contiguous()), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(cache_len), _ptr(q),
                                         _ptr(k_cache), _ptr(v_cache), B, num_heads, Dh, k_cache.shape[2], _dt(qkv), _stream()),
            "aki_rope_append_fwd")
    return q


def decode_attn_workspace(B: int, H: int, Dh: int, capacity: int, device) -> torch.Tensor:
    """Zero-filled workspace for decode_attn / decode_attn_fused (allocate once per KV cache and keep passing it)."""
    nbytes = int(L.load().aki_decode_attn_workspace_bytes(B, H, Dh, capacity))
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)


def kv_cache_quant_fp8(src: torch.Tensor, dst: torch.Tensor, scale: torch.Tensor, rows: int) -> None:
    """bf16 K/V rows -> the e4m3 cache, in place: src [..., src_cap, 96] bf16, dst [..., cap, 96] uint8, scale [..., cap] f32 (the same
    leading dims, all contiguous); rows [0, rows) of every (layer, sample, head) slab.  One launch for all layers."""
    _dev(src, dst, scale)
    if src.dtype != torch.bfloat16 or dst.dtype != torch.uint8 or scale.dtype != torch.float32:
        raise AkiError("kv_cache_quant_fp8: bf16 source, uint8 destination, f32 scales")
    if not (src.is_contiguous() and dst.is_contiguous() and scale.is_contiguous()) or src.shape[:-2] != dst.shape[:-2] \
            or scale.shape != dst.shape[:-1]:
        raise AkiError("kv_cache_quant_fp8: contiguous tensors with matching leading dimensions")
    slabs = dst[..., 0, 0].numel()
    L.check(L.load().aki_kv_cache_quant_fp8(_ptr(src), src.shape[-2], _ptr(dst), _ptr(scale), dst.shape[-2], slabs, int(rows), dst.shape[-1],
                                            _dt(src), _stream()), "aki_kv_cache_quant_fp8")


def decode_attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_keys: torch.Tensor, scale: float,
                col_valid_bits: Optional[torch.Tensor] = None, max_keys: int = 0, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B,H,Dh] against the first n_keys[b] rows of the caches [B,H,cap,Dh] -> o [B, H*Dh].
    max_keys: host upper bound of n_keys (0 = capacity); ws: decode_attn_workspace(...) (allocated here if None)."""
    dev = _dev(q, k_cache, v_cache, n_keys, col_valid_bits, ws)
    B, H, Dh = q.shape
    cap = k_cache.shape[2]
    if ws is None:
        ws = decode_attn_workspace(B, H, Dh, cap, dev)
    o = torch.empty((B, H * Dh), dtype=q.dtype, device=dev)
    nw = 0 if col_valid_bits is None else col_valid_bits.shape[1]
    L.check(L.load().aki_decode_attn_fwd(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(o), _ptr(n_keys), _ptr(col_valid_bits), nw,
                                         B, H, Dh, cap, int(max_keys), float(scale), _dt(q), _ptr(ws), ws.numel() * 4, _stream()),
            "aki_decode_attn_fwd")
    return o


def decode_attn_fused(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_len: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, num_heads: int, scale: float, col_valid_bits: Optional[torch.Tensor] = None,
                      max_keys: int = 0, ws: Optional[torch.Tensor] = None, k_scale: Optional[torch.Tensor] = None,
                      v_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode step in one launch: qkv [B, 3*H*Dh] of the new tokens -> RoPE at position cache_len[b], k/v appended at
    row cache_len[b], attention over cache_len[b]+1 keys -> o [B, H*Dh].  f32 (parity path) runs the two plain kernels.
    An e4m3 cache (uint8 k_cache / v_cache, with the f32 row scales k_scale / v_scale [B, H, cap]) runs the fp8-KV twin of the kernel:
    the new k / v are quantised per head and appended, and every key is attended through its quantised copy."""
    dev = _dev(qkv, cos, sin, cache_len, k_cache, v_cache, col_valid_bits, ws, k_scale, v_scale)
    B = qkv.shape[0]
    cap, Dh = k_cache.shape[2], k_cache.shape[3]
    if k_cache.dtype == torch.uint8:
        if k_scale is None or v_scale is None or v_cache.dtype != torch.uint8:
            raise AkiError("an e4m3 KV cache needs uint8 k/v caches and their f32 row scales")
        if ws is None:
            ws = decode_attn_workspace(B, num_heads, Dh, cap, dev)
        o = torch.empty((B, num_heads * Dh), dtype=qkv.dtype, device=dev)
        nw = 0 if col_valid_bits is None else col_valid_bits.shape[1]
        L.check(L.load().aki_decode_attn_fused_fp8kv_fwd(_ptr(qkv.contiguous()), _ptr(cos), _ptr(sin), _ptr(cache_len), _ptr(k_cache),
                                                         _ptr(v_cache), _ptr(k_scale), _ptr(v_scale), _ptr(o), _ptr(col_valid_bits), nw, B,
                                                         num_heads, Dh, cap, int(max_keys), float(scale), _dt(qkv), _ptr(ws), ws.numel() * 4,
                                                         _stream()), "aki_decode_attn_fused_fp8kv_fwd")
        return o
    if qkv.dtype != torch.bfloat16 or Dh != 96:
        q = rope_append(qkv, cos, sin, cache_len, cache_len, k_cache, v_cache, num_heads)
        return decode_attn(q, k_cache, v_cache, cache_len + 1, scale, col_valid_bits, max_keys, ws)
    if ws is None:
        ws = decode_attn_workspace(B, num_heads, Dh, cap, dev)
    o = torch.empty((B, num_heads * Dh), dtype=qkv.dtype, device=dev)
    nw = 0 if col_valid_bits is None else col_valid_bits.shape[1]
    L.check(L.load().aki_decode_attn_fused_fwd(_ptr(qkv.contiguous()), _ptr(cos), _ptr(sin), _ptr(cache_len), _ptr(k_cache),
                                               _ptr(v_cache), _ptr(o), _ptr(col_valid_bits), nw, B, num_heads, Dh, cap,
                                               int(max_keys), float(scale), _dt(qkv), _ptr(ws), ws.numel() * 4, _stream()),
            "aki_decode_attn_fused_fwd")
    return o


def decode_attn_group_workspace(B0: int, N: int, H: int, Dh: int, prefix_cap: int, suffix_cap: int, device) -> torch.Tensor:
    """Zero-filled workspace for decode_attn_group (allocate once per grouped KV cache and keep passing it)."""
    nbytes = int(L.load().aki_decode_attn_group_workspace_bytes(B0, N, H, Dh, prefix_cap, suffix_cap))
    if nbytes <= 0:
        raise AkiError("decode_attn_group: bf16, head_dim 96 and positive sizes")
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)


def decode_attn_group(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_len: torch.Tensor, prefix_len: torch.Tensor,
                      k_prefix: torch.Tensor, v_prefix: torch.Tensor, k_suffix: torch.Tensor, v_suffix: torch.Tensor, num_heads: int,
                      scale: float, col_valid_bits: Optional[torch.Tensor] = None, max_prefix_keys: int = 0, max_suffix_keys: int = 0,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode step of N sampled rows per prompt over ONE copy of the prompt's K/V, in one launch (bf16, head_dim 96):
    qkv [B0*N, 3*H*96] of the new tokens; k_prefix / v_prefix [B0, H, prefix_cap, 96] (read-only), k_suffix / v_suffix [B0*N, H, suffix_cap, 96].
    Row r (sample r // N) attends to prefix rows [0, prefix_len[b]) (filtered by col_valid_bits [B0, nwords]) and to its suffix rows
    [0, cache_len[r] - prefix_len[b]], the last of which is the new token: rotated at position cache_len[r] and appended here.  -> o [B0*N, H*96].
    max_prefix_keys / max_suffix_keys: host bounds that size the grid (0 = the capacities)."""
    dev = _dev(qkv, cos, sin, cache_len, prefix_len, k_prefix, v_prefix, k_suffix, v_suffix, col_valid_bits, ws)
    R, B0 = qkv.shape[0], k_prefix.shape[0]
    pcap, scap, Dh = k_prefix.shape[2], k_suffix.shape[2], k_prefix.shape[3]
    if B0 <= 0 or R % B0 or k_suffix.shape[0] != R or cache_len.shape[0] != R or prefix_len.shape[0] != B0 \
            or qkv.shape[1] != 3 * num_heads * Dh or k_prefix.shape[1] != num_heads or k_suffix.shape[1] != num_heads:
        raise AkiError("decode_attn_group: rows must be samples * N, with one suffix slab and one length per row")
    if col_valid_bits is not None and col_valid_bits.shape[0] != B0:
        raise AkiError("decode_attn_group: col_valid_bits holds one row of words per prompt sample")
    for t in (k_prefix, v_prefix, k_suffix, v_suffix):
        if not t.is_contiguous() or t.dtype != torch.bfloat16:
            raise AkiError("decode_attn_group: contiguous bf16 caches")
    if cache_len.dtype != torch.int32 or prefix_len.dtype != torch.int32:
        raise AkiError("decode_attn_group: int32 lengths")
    N = R // B0
    if ws is None:
        ws = decode_attn_group_workspace(B0, N, num_heads, Dh, pcap, scap, dev)
    o = torch.empty((R, num_heads * Dh), dtype=qkv.dtype, device=dev)
    nw = 0 if col_valid_bits is None else col_valid_bits.shape[1]
    L.check(L.load().aki_decode_attn_group_fwd(_ptr(qkv.contiguous()), _ptr(cos), _ptr(sin), _ptr(cache_len), _ptr(prefix_len), _ptr(k_prefix),
                                               _ptr(v_prefix), _ptr(k_suffix), _ptr(v_suffix), _ptr(o), _ptr(col_valid_bits), nw, B0, N,
                                               num_heads, Dh, pcap, scap, int(max_prefix_keys), int(max_suffix_keys), float(scale), _dt(qkv),
                                               _ptr(ws), ws.numel() * 4, _stream()), "aki_decode_attn_group_fwd")
    return o


def chunk_attn_workspace(B: int, H: int, T: int, Dh: int, device) -> torch.Tensor:
    """The q_rot scratch of chunk_attn (nothing in it outlives a call: allocate once per chunk and pass it to every layer)."""
    nbytes = int(L.load().aki_chunk_attn_workspace_bytes(B, H, T, Dh))
    if nbytes <= 0:
        raise AkiError("chunk_attn: bf16, head_dim 96 and positive sizes")
    return torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)


def chunk_attn(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_len: torch.Tensor, n_new: Optional[torch.Tensor],
               k_cache: torch.Tensor, v_cache: torch.Tensor, num_heads: int, scale: float, col_valid_bits: Optional[torch.Tensor] = None,
               max_new: Optional[int] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T new tokens per sample appended to a KV cache and attended in one pass (bf16, head_dim 96; two launches, chunk_attn.hip):
    qkv [B*T, 3*H*96] un-rotated (row b*T + t = token t of sample b); k_cache / v_cache [B, H, cap, 96].  Token t < n_new[b] is rotated at
    position cache_len[b] + t, its k / v appended at that cache row, and it attends to the cached keys (filtered by col_valid_bits
    [B, nwords]) plus the chunk's tokens 0..t.  -> o [B*T, H*96]; rows t >= n_new[b] are zeros.  n_new: None (every sample brings T
    tokens) or int32 [B]; max_new: host upper bound of n_new (default T), sizes the grid.  cache_len is NOT advanced, and the caller
    guarantees cache_len[b] + n_new[b] <= cap (Phi3ForCausalLM._continue guards it from the cache's host_len)."""
    dev = _dev(qkv, cos, sin, cache_len, n_new, k_cache, v_cache, col_valid_bits, ws)
    if k_cache.dim() != 4 or qkv.dim() != 2:
        raise AkiError("chunk_attn: qkv [B*T, 3*H*Dh] and caches [B, H, cap, Dh]")
    B, H, cap, Dh = k_cache.shape
    R = qkv.shape[0]
    if B <= 0 or R % B or R == 0 or H != num_heads or qkv.shape[1] != 3 * num_heads * Dh or v_cache.shape != k_cache.shape \
            or cache_len.shape != (B,) or (n_new is not None and n_new.shape != (B,)):
        raise AkiError("chunk_attn: rows must be samples * T, with one cache slab and one length per sample")
    if col_valid_bits is not None and col_valid_bits.shape[0] != B:
        raise AkiError("chunk_attn: col_valid_bits holds one row of words per sample")
    for t in (k_cache, v_cache):
        if not t.is_contiguous() or t.dtype != torch.bfloat16:
            raise AkiError("chunk_attn: contiguous bf16 caches")
    if qkv.dtype != torch.bfloat16 or Dh != 96:
        raise AkiError("chunk_attn: bf16 and head_dim 96 only (there is no fallback: take the decode steps instead)")
    if cache_len.dtype != torch.int32 or (n_new is not None and n_new.dtype != torch.int32):
        raise AkiError("chunk_attn: int32 lengths")
    if not cache_len.is_contiguous() or (n_new is not None and not n_new.is_contiguous()):
        raise AkiError("chunk_attn: contiguous lengths")
    for t in (cos, sin):                  # the kernel reads the Dh floats of row cache_len[b] + t < cap
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[0] < cap or t.shape[1] != Dh:
            raise AkiError(f"chunk_attn: cos / sin must be contiguous f32 [>= cap, Dh] = [>= {cap}, {Dh}]")
    if col_valid_bits is not None and (col_valid_bits.dtype != torch.int64 or not col_valid_bits.is_contiguous() or col_valid_bits.dim() != 2):
        raise AkiError("chunk_attn: col_valid_bits must be contiguous int64 words [B, nwords]")
    T = R // B
    max_new = T if max_new is None else int(max_new)
    if not 1 <= max_new <= T:
        raise AkiError(f"chunk_attn: max_new must lie in [1, {T}]")
    lib = L.load()
    if ws is None:
        ws = chunk_attn_workspace(B, H, T, Dh, dev)
    qkv = qkv.contiguous()                # held in a local: the copy, if one is made, lives until the launch is queued
    # the kernel writes the 32-row blocks up to max_new; rows past them are zeros by definition
    o = (torch.empty if (max_new + 31) // 32 * 32 >= T else torch.zeros)((R, H * Dh), dtype=qkv.dtype, device=dev)
    nw = 0 if col_valid_bits is None else col_valid_bits.shape[1]
    L.check(lib.aki_chunk_attn_fwd(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(cache_len), _ptr(n_new), _ptr(k_cache), _ptr(v_cache),
                                   _ptr(o), _ptr(col_valid_bits), nw, B, H, Dh, T, max_new, cap, float(scale), _dt(qkv), _ptr(ws),
                                   ws.numel() * 4, _stream()), "aki_chunk_attn_fwd")
    return o


_CHAIN_LAST = {}                      # device index -> the torch stream of the last chain launch
_CHAIN_LOCK = threading.Lock()


class DecodeChain:
    """The whole decoder stack of a batch-1 decode step as ONE launch (aki_decode_chain_fwd, decode_chain.hip): a device-resident
    table of per-layer pointers + the workspace with the hand-off vectors and arrival counters.  Built once per (model weights,
    KV cache); `step(h_in)` -> the residual stream after the last layer (pre final norm), bit-identical to the per-layer
    launches.  `check()` reads the sticky error word (a device sync): non-zero means a dependency wait gave up."""

    SUPPORTED = dict(d=3072, F=8192, Dh=96)

    FORMATS = {"bf16": L.AKI_DT_BF16, "w8": L.AKI_DT_W8A16, "w4": L.AKI_DT_W4A16}

    def __init__(self, layers, k_caches, v_caches, H: int, Dh: int, d: int, F: int, capacity: int, scale: float, eps: float, device, fmt="bf16",
                 batch: int = 1, w8: Optional[bool] = None):
        """layers: per layer (w_qkv, w_o, w_gate_up, w_down, norm1, norm2, s_qkv, s_o, s_gate_up, s_down) - scales None for bf16.
        fmt: the weight format - "bf16", "w8" (e4m3 weights, an f32 scale per row) or "w4" (MXFP4 as ops.quant_mxfp4 makes it: contiguous
        uint8 nibbles [N, K/2] with contiguous uint8 e8m0 scales [N, K/32] in the scale slots; one sequence only).  False / True = "bf16" / "w8".
        batch 2..8 (bf16): that many sequences per step - the batched chain (16-feature MFMA tiles instead of dot-product rows), bit-identical to
        the per-layer batched launches; k / v caches [batch, H, capacity, Dh]."""
        lib = L.load()
        if w8 is not None:                      # the argument's earlier name
            fmt = bool(w8)
        if isinstance(fmt, bool):
            fmt = "w8" if fmt else "bf16"
        if fmt not in self.FORMATS:
            raise AkiError(f"decode chain: weight format {fmt!r} is not one of {sorted(self.FORMATS)}")
        w8 = fmt == "w8"
        self.batch = int(batch)
        if self.batch > 1 and (fmt != "bf16" or self.batch > 8 or H != 32):
            raise AkiError("decode chain: batches of 2..8 sequences run on bf16 weights with 32 heads")
        self.n_layers = len(layers)
        rows = []
        for (wq, wo, wg, wd, n1, n2, sq, so, sg, sd), k, v in zip(layers, k_caches, v_caches):
            for t_ in (wq, wo, wg, wd):
                if not t_.is_contiguous():
                    raise AkiError("decode chain: weights must be contiguous [N, K]")
            if fmt == "w4":
                # the table holds raw pointers the library cannot inspect (device memory): the layout is checked here
                for t_, s_, K in ((wq, sq, d), (wo, so, H * Dh), (wg, sg, d), (wd, sd, F)):
                    if s_ is None or t_.dtype != torch.uint8 or s_.dtype != torch.uint8 or not s_.is_contiguous() or t_.dim() != 2 \
                            or tuple(t_.shape) != (t_.shape[0], K // 2) or tuple(s_.shape) != (t_.shape[0], K // 32):
                        raise AkiError("decode chain: MXFP4 weights are contiguous uint8 nibbles [N, K/2] with uint8 e8m0 scales [N, K/32]")
            rows.append([wq.data_ptr(), wo.data_ptr(), wg.data_ptr(), wd.data_ptr(), n1.data_ptr(), n2.data_ptr(), k.data_ptr(), v.data_ptr(),
                         _ptr(sq) or 0, _ptr(so) or 0, _ptr(sg) or 0, _ptr(sd) or 0])
        self.keep = (layers, k_caches, v_caches)                      # the table holds raw pointers: keep the tensors alive
        self.key = tuple(r[0] for r in rows) + tuple(r[6] for r in rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)
        assert C.sizeof(L.DecodeChainLayer) == 12 * 8
        nbytes = int(lib.aki_decode_chain_batch_workspace_bytes(self.n_layers, d, H, F, capacity, self.batch))
        if nbytes == 0:
            raise AkiError("decode chain: bad dimensions")
        self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=device)
        off = (-self.ws.data_ptr()) % 256
        self.ws_ptr = self.ws.data_ptr() + off
        self.ws_bytes = nbytes
        self.err_index = (off + int(lib.aki_decode_chain_batch_error_offset(self.n_layers, H, self.batch))) // 4
        self.h_out = torch.empty((self.batch, d), dtype=torch.bfloat16, device=device)
        self.dims = (H, Dh, d, F, capacity)
        self.scale, self.eps, self.w8, self.fmt = float(scale), float(eps), bool(w8), fmt

    def step(self, h_in: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, cache_len: torch.Tensor, col_valid_bits: Optional[torch.Tensor],
             max_keys: int) -> torch.Tensor:
        H, Dh, d, F, cap = self.dims
        if h_in.dtype != torch.bfloat16 or h_in.numel() != self.batch * d or not h_in.is_contiguous():
            raise AkiError("decode chain: h_in must be contiguous bf16 rows [batch, d]")
        if cache_len.numel() != self.batch or (col_valid_bits is not None and col_valid_bits.numel() != self.batch * col_valid_bits.shape[-1]):
            raise AkiError("decode chain: cache_len / col_valid_bits are per sequence")
        if cos.shape[0] < cap or cos.shape[1] != Dh:
            raise AkiError("decode chain: cos/sin tables must cover the cache capacity")
        _dev(h_in, cos, sin, cache_len, col_valid_bits, self.table)
        a = L.DecodeChainArgs(self.table.data_ptr(), _ptr(h_in), _ptr(self.h_out), _ptr(cos), _ptr(sin), _ptr(cache_len), _ptr(col_valid_bits),
                              self.ws_ptr, self.ws_bytes, self.n_layers, 0 if col_valid_bits is None else col_valid_bits.shape[-1], d, H, Dh, F,
                              cap, int(max_keys), self.scale, self.eps, self.FORMATS[self.fmt], self.batch)
        end = _TAP.begin(("decode_chain", self.n_layers)) if (_TAP is not None and _TAP.want(("decode_chain",))) else None
        cur = torch.cuda.current_stream()
        with _CHAIN_LOCK:
            # one chain in flight per device (decode_chain.hip, "Progress"): a launch on another stream than the previous chain launch first
            # lets that stream finish.  Same stream = ordered by the stream; nothing to do (the common case: one comparison).
            last = _CHAIN_LAST.get(cur.device_index)
            if last is not None and last.cuda_stream != cur.cuda_stream and not torch.cuda.is_current_stream_capturing():
                last.synchronize()
            _CHAIN_LAST[cur.device_index] = cur
            L.check(L.load().aki_decode_chain_fwd(C.byref(a), cur.cuda_stream), "aki_decode_chain_fwd")
        if end is not None:
            end.record()
        return self.h_out

    def error_code(self) -> int:
        """The sticky error word (synchronises the device): 0, or (layer << 8 | phase) of a wait that gave up."""
        return int(self.ws.view(torch.int32)[self.err_index].item())

    def check(self) -> None:
        code = self.error_code()
        if code:
            raise AkiError(f"decode chain: a dependency wait gave up (layer {code >> 8}, phase {code & 255}); the step's output is invalid")


def chain_replay_on_current_stream() -> None:
    """A hipGraph that holds a decode-chain launch is about to be replayed on the current stream: apply the same one-chain-in-flight-per-device
    rule as DecodeChain.step does for eager launches (a replay is invisible to it otherwise) - let the stream of the previous chain launch
    finish if it is another one, then record this stream."""
    cur = torch.cuda.current_stream()
    with _CHAIN_LOCK:
        last = _CHAIN_LAST.get(cur.device_index)
        if last is not None and last.cuda_stream != cur.cuda_stream:
            last.synchronize()
        _CHAIN_LAST[cur.device_index] = cur


_NO_WIDE_CONSTRAINT = (None, 0, 0, None, 0)
_NO_ROW_CONSTRAINT = (None, 0, 0, None, 0, None, None)


def check_penalty(name: str, value) -> float:
    """frequency_penalty / presence_penalty: a finite float in [-2, 2] -> the float32 the device reads (slots.check_additive_penalty)."""
    from .slots import check_additive_penalty
    return check_additive_penalty("logits processors", name, value)


def check_min_p(value) -> float:
    """min_p: a float in [0, 1] -> the float32 the device reads (slots.check_min_p)."""
    from .slots import check_min_p as check
    return check("sampler", value)


def _penalty_rows(name: str, processors, frequency_penalty, presence_penalty, B: int, device, min_p=None):
    """The nullable per-row arrays of the *_penalized entry points: (frequency_penalty, presence_penalty, min_p) as given (f32
    contiguous tensors [B] on the logits' device), else a penalised LogitsProcessors' own; None when nothing is set - the call then takes
    the entry point it took before these existed."""
    for nm, x in (("frequency_penalty", frequency_penalty), ("presence_penalty", presence_penalty), ("min_p", min_p)):
        if x is not None and (not torch.is_tensor(x) or x.dtype != torch.float32 or tuple(x.shape) != (B,) or not x.is_contiguous()
                              or x.device != device):
            raise AkiError(f"{name}: {nm} is a contiguous f32 tensor [{B}] on {device}")
    if processors is not None and processors.active and getattr(processors, "penalized", False):
        fq, pr = processors.penalty_rows(B, device)
        frequency_penalty = fq if frequency_penalty is None else frequency_penalty
        presence_penalty = pr if presence_penalty is None else presence_penalty
    if frequency_penalty is None and presence_penalty is None and min_p is None:
        return None
    return frequency_penalty, presence_penalty, min_p


_MIN_P_ROWS = {}


def _min_p_rows(min_p: float, B: int, device) -> Optional[torch.Tensor]:
    """A scalar min_p as the f32 [B] device array the sampler reads (kept per value and shape: a captured graph holds its address);
    None for 0, no filter."""
    v = check_min_p(min_p)
    if v == 0.0:
        return None
    key = (v, int(B), str(device))
    if key not in _MIN_P_ROWS:
        _MIN_P_ROWS[key] = torch.full((int(B),), v, dtype=torch.float32, device=device)
    return _MIN_P_ROWS[key]


class LogitsProcessors:
    """HF `generate`'s logits processors for a decoder-only model called with inputs_embeds only (what src/aki.py:192-207 runs), on the
    device (aki_logits_process / aki_greedy_pick_processed; include/aki_mi355x.h): the processors' input_ids are the GENERATED tokens,
    never the prompt.  In HF's order: repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length (eos ids banned while fewer
    tokens have been generated; min_new_tokens is the same number here), suppress_tokens, begin_suppress_tokens.  The arguments are
    checked here, on the host, and held as device tensors, so one object serves a whole generation (and a captured graph).
    eos_ids: the ids min_length bans; a one-token bad word equal to one of them is dropped, as HF's NoBadWordsLogitsProcessor does.
    constraint (a constraint.BoundConstraint, TokenConstraint.bind's result): a token automaton as the last stage - every token the row's
    state does not allow becomes -inf (the constrained C entry points).  The state history `states()` int32 [rows, steps + 1] belongs to
    this object, one per generation: column 0 holds each row's start state, the picks store the state behind every token they pick, and
    all of them address it by the generated-token index, as they do the token history.
    slot_constraints=True: the picks will be handed a SlotConstraints (one automaton per row, generate_many) - the object is then active
    even with every processor neutral, because the constrained pick scans the f32 scores scratch this object owns.
    frequency_penalty / presence_penalty (the OpenAI definition, in vLLM's place: stage 1b, directly behind the repetition penalty and
    before every ban): for every distinct generated token with c occurrences, score - fl(frequency_penalty * c), then score -
    presence_penalty; finite floats in [-2, 2], 0 is neutral.  They ban nothing, so they compose with a constraint.  With either set the
    object routes to the *_penalized entry points, which take the values as device arrays of one float per row, filled here."""

    def __init__(self, V: int, device, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_length: int = 0, eos_ids=(),
                 suppress_tokens=None, begin_suppress_tokens=None, bad_words_ids=None, constraint=None, slot_constraints: bool = False,
                 frequency_penalty: float = 0.0, presence_penalty: float = 0.0):
        V = int(V)
        self.frequency = check_penalty("frequency_penalty", frequency_penalty)
        self.presence = check_penalty("presence_penalty", presence_penalty)
        self.penalized = bool(self.frequency != 0.0 or self.presence != 0.0)
        self._pen_rows = {}
        if V <= 0:
            raise ValueError(f"logits processors: a vocabulary of {V} columns")
        pen = float(repetition_penalty)
        if not (pen > 0.0 and pen < float("inf")):
            raise ValueError(f"repetition_penalty has to be a strictly positive float, got {repetition_penalty}")
        if int(no_repeat_ngram_size) < 0 or int(min_length) < 0:
            raise ValueError("no_repeat_ngram_size and min_length / min_new_tokens are non-negative integers")
        eos = [int(e) for e in eos_ids]

        def ids(name, x):
            out = [int(i) for i in (x or [])]
            if any(not 0 <= i < V for i in out):
                raise ValueError(f"{name}: every id has to be in [0, {V})")
            return out

        words = []
        for w in (bad_words_ids or []):
            if isinstance(w, int) or len(w) == 0:
                raise ValueError(f"bad_words_ids has to be a list of non-empty lists of token ids, got {bad_words_ids}")
            w = ids("bad_words_ids", w)
            if not (len(w) == 1 and w[0] in eos):
                words.append(w)
        self.V, self.penalty, self.ngram, self.min_length = V, pen, int(no_repeat_ngram_size), int(min_length)
        self.suppress, self.begin_suppress = ids("suppress_tokens", suppress_tokens), ids("begin_suppress_tokens", begin_suppress_tokens)
        self.words = words
        self.active = bool(pen != 1.0 or self.ngram > 0 or words or (self.min_length > 0 and eos) or self.suppress or self.begin_suppress
                           or constraint is not None or slot_constraints or self.penalized)
        if self.active and V > L.AKI_LOGITS_PROCESS_MAX_V:
            raise ValueError(f"logits processors: a vocabulary of {V} is above {L.AKI_LOGITS_PROCESS_MAX_V}")
        dev = torch.device(device)
        if constraint is not None:
            if constraint.V != V:
                raise ValueError(f"the constraint was built for V = {constraint.V}, the logits have {V} columns")
            t_ = constraint.table
            if t_.dtype != torch.int16 or t_.dim() != 2 or t_.shape[0] != constraint.n_states or t_.shape[1] < V or not t_.is_contiguous() \
                    or constraint.row_start.dtype != torch.int32 or t_.device.type != dev.type or constraint.row_start.device != t_.device:
                raise AkiError("logits processors: the constraint's table is contiguous int16 [n_states, >= V] and row_start int32, on the device")
        self.constraint, self._states = constraint, None
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev) if v else None
        self._eos, self._sup, self._bsup = i64(eos), i64(self.suppress), i64(self.begin_suppress)
        self._bad = i64([t for w in words for t in w])
        offs = [0]
        for w in words:
            offs.append(offs[-1] + len(w))
        self._off = torch.tensor(offs, dtype=torch.int32, device=dev) if words else None
        self._scores = None

    def _tail(self):
        n = lambda t: 0 if t is None else t.numel()
        return (self.penalty, self.ngram, self.min_length), (_ptr(self._sup), n(self._sup), _ptr(self._bsup), n(self._bsup), _ptr(self._bad),
                                                            _ptr(self._off), len(self.words), n(self._bad))

    def penalty_rows(self, B: int, device):
        """(frequency_penalty, presence_penalty) as f32 device tensors [B] filled with this object's values, None for a zero one; kept
        per batch size (a captured graph holds their addresses)."""
        key = (int(B), str(torch.device(device)))
        if key not in self._pen_rows:
            row = lambda v: torch.full((int(B),), v, dtype=torch.float32, device=device) if v != 0.0 else None
            self._pen_rows[key] = (row(self.frequency), row(self.presence))
        return self._pen_rows[key]

    def scores(self, B: int, device) -> torch.Tensor:
        """The f32 [B, >= V] scratch the processed greedy pick writes its scores to (kept: a captured graph holds its address)."""
        if self._scores is None or self._scores.shape[0] != B or self._scores.device != torch.device(device):
            self._scores = torch.empty((B, (self.V + 3) // 4 * 4), dtype=torch.float32, device=device)
        return self._scores

    def states(self, rows: int, steps: Optional[int] = None) -> torch.Tensor:
        """The constraint's state history, int32 [rows, steps + 1]: allocated by the first call (which has to name `steps`, the number of
        tokens the generation can pick), column 0 filled with the rows' start states and the rest with -1 (no state: a row is left
        unmasked), then kept for the life of this object - a captured graph holds its address."""
        c = self.constraint
        if c is None:
            raise AkiError("logits processors: states() needs a constraint")
        if self._states is None:
            if steps is None or int(steps) < 0:
                raise AkiError("logits processors: the first states() call names the number of steps")
            if c.rows != int(rows):
                raise ValueError(f"the constraint was bound for {c.rows} rows, the call has {rows}")
            self._states = torch.full((int(rows), int(steps) + 1), -1, dtype=torch.int32, device=c.table.device)
            self._states[:, 0] = c.row_start
        elif self._states.shape[0] != int(rows) or (steps is not None and int(steps) + 1 > self._states.shape[1]):
            raise AkiError(f"logits processors: the state history is {tuple(self._states.shape)}, the call wants {rows} rows and {steps} steps; "
                           "one LogitsProcessors serves one generation")
        return self._states

    def _constraint_args(self, rows: int, steps: Optional[int]):
        """(table, table_ld, n_states, states, states_ld) of the constrained C entry points, or None without a constraint."""
        if self.constraint is None:
            return None
        st, t_ = self.states(rows, steps), self.constraint.table
        return (_ptr(t_), t_.stride(0), self.constraint.n_states, _ptr(st), st.shape[1])

    def advance_states(self, next_ids: torch.Tensor, step: int, done: Optional[torch.Tensor] = None) -> None:
        """For a loop that picks on the host (argmax or sample_next over apply()'s scores; the pick kernels store the state themselves):
        states[:, step + 1] = the state behind next_ids in states[:, step], rows with done[b] keep theirs.  No-op without a constraint."""
        if self.constraint is None or self._states is None or int(step) + 1 >= self._states.shape[1]:
            return
        st, tbl = self._states, self.constraint.table
        cur = st[:, int(step)]
        ok = (cur >= 0) & (next_ids >= 0) & (next_ids < self.V)
        nxt = tbl[cur.clamp(min=0).long(), next_ids.clamp(0, self.V - 1)].to(torch.int32)
        nxt = torch.where(ok, nxt, torch.full_like(nxt, -1))
        st[:, int(step) + 1] = nxt if done is None else torch.where(done.bool(), cur, nxt)

    def apply(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, step: int = 0,
              cache_len: Optional[torch.Tensor] = None, start_len: Optional[torch.Tensor] = None,
              done: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Processed f32 scores [B, V] of bf16 / f32 logits [B, V] (one launch).  The history of row b is tokens[b, :n] (int64 [B, *]) with
        n = step + (cache_len[b] - start_len[b] when cache_len is given); rows with done[b] (uint8) are copied unprocessed.  out may be
        logits itself when they are f32."""
        if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] != self.V:
            raise AkiError(f"logits processors: logits [B, {self.V}] with unit column stride are expected, got {tuple(logits.shape)}")
        B = logits.shape[0]
        dev = _dev(logits, out, tokens, cache_len, start_len, done)
        if out is None:
            out = torch.empty((B, self.V), dtype=torch.float32, device=dev)
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.shape[1] != self.V:
            raise AkiError("logits processors: out is f32 [B, V] with unit column stride")
        for t_, dt in ((tokens, torch.int64), (cache_len, torch.int32), (start_len, torch.int32), (done, torch.uint8)):
            if t_ is not None and (t_.dtype != dt or not t_.is_contiguous()):
                raise AkiError(f"logits processors: a contiguous {dt} tensor is expected, got {t_.dtype}")
        if tokens is not None and (tokens.dim() != 2 or tokens.shape[0] != B):
            raise AkiError("logits processors: tokens is [B, *]")
        if tokens is not None and tokens.shape[1] == 0:
            tokens = None
        head, tail = self._tail()
        args = (_ptr(logits), _dt(logits), B, self.V, logits.stride(0), _ptr(out), out.stride(0), _ptr(tokens),
                0 if tokens is None else tokens.shape[1], _ptr(cache_len), _ptr(start_len), int(step), _ptr(done),
                *head, _ptr(self._eos), 0 if self._eos is None else self._eos.numel(), *tail)
        con = self._constraint_args(B, tokens.shape[1] if tokens is not None else (int(step) + 1 if cache_len is None else None))
        if self.penalized:
            fq, pr = self.penalty_rows(B, dev)
            L.check(L.load().aki_logits_process_penalized(*args, *(con or _NO_WIDE_CONSTRAINT), _ptr(fq), _ptr(pr), _stream()),
                    "aki_logits_process_penalized")
            return out
        if con is not None:
            L.check(L.load().aki_logits_process_constrained(*args, *con, _stream()), "aki_logits_process_constrained")
            return out
        L.check(L.load().aki_logits_process(*args, _stream()), "aki_logits_process")
        return out


class SlotConstraints:
    """One token automaton per ROW, for rows that change hands (generate_many's slots): what the per-row constrained picks take as
    `slot_constraints` (aki_greedy_pick_constrained_rows / aki_sample_pick_rows_constrained).
      pool        int16 [pool rows, ld >= V]: constraint.ConstraintPool.bind's table - the automata one behind the other, states local
      row_base    int32 [slots]: the pool row at which the slot's automaton begins
      row_states  int32 [slots]: its number of states (0: none)
      states      int32 [slots, max_budget + 1]: the slot's state history, addressed by the generated-token index; -1 = no state, the row
                  is left unmasked (an unconstrained request)
    All four are allocated once - a captured step holds their addresses - and `admit` rewrites a slot's entries in place."""

    def __init__(self, pool: torch.Tensor, slots: int, max_budget: int, _parts=None):
        self.pool = pool
        if _parts is not None:
            self.row_base, self.row_states, self.states = _parts
            return
        dev = pool.device
        self.row_base = torch.zeros(int(slots), dtype=torch.int32, device=dev)
        self.row_states = torch.zeros(int(slots), dtype=torch.int32, device=dev)
        self.states = torch.full((int(slots), int(max_budget) + 1), -1, dtype=torch.int32, device=dev)

    def row(self, slot: int) -> "SlotConstraints":
        """One-row views of everything: what a B = 1 pick on the slot's row views takes."""
        s = int(slot)
        return SlotConstraints(self.pool, 1, 0, _parts=(self.row_base[s:s + 1], self.row_states[s:s + 1], self.states[s:s + 1]))

    def admit(self, slot: int, base: int, n: int, start: int) -> None:
        """A new request in `slot`: its history emptied, column 0 = its start state (-1 for an unconstrained request), its table's place.
        Tensor fills only - nothing is copied from the host or reallocated."""
        s = int(slot)
        self.states[s].fill_(-1)
        self.states[s, 0] = int(start)
        self.row_base[s] = int(base)
        self.row_states[s] = int(n)

    def _args(self, name: str, B: int, V: int, device):
        """(table, table_ld, n_states, states, states_ld, row_base, row_states) of the per-row C entry points, checked."""
        t_ = self.pool
        if not torch.is_tensor(t_) or t_.dtype != torch.int16 or t_.dim() != 2 or t_.shape[0] < 1 or t_.shape[1] < V or not t_.is_contiguous() \
                or t_.device != device:
            raise AkiError(f"{name}: slot_constraints.pool is a contiguous int16 tensor [pool rows >= 1, >= {V}] on {device}")
        for nm, x in (("row_base", self.row_base), ("row_states", self.row_states)):
            if not torch.is_tensor(x) or x.dtype != torch.int32 or tuple(x.shape) != (B,) or not x.is_contiguous() or x.device != device:
                raise AkiError(f"{name}: slot_constraints.{nm} is a contiguous int32 tensor [{B}] on {device}")
        st = self.states
        if not torch.is_tensor(st) or st.dtype != torch.int32 or st.dim() != 2 or st.shape[0] != B or st.shape[1] < 1 or not st.is_contiguous() \
                or st.device != device:
            raise AkiError(f"{name}: slot_constraints.states is a contiguous int32 tensor [{B}, >= 1] on {device}")
        return (_ptr(t_), t_.stride(0), t_.shape[0], _ptr(st), st.shape[1], _ptr(self.row_base), _ptr(self.row_states))


class ProcessorSets:
    """One set of logits-processor settings per ROW, for rows that change hands (generate_many's slots): what the per-row picks take as
    `processor_sets` (aki_logits_process_rows / aki_greedy_pick_rows / aki_sample_pick_rows_processed).  The distinct settings of a call
    are a small pool, deduplicated by value and uploaded once:
      keys     the pool on the host: (penalty, ngram, min_len, suppress ids, begin-suppress ids, bad words) per set
               (slots.processor_set_key's values); keys[0] is always the neutral set
      index    {key: its place in the pool}
      sets     int32 [n_sets, 9]: word 0 the penalty's float bits, 1 ngram, 2 min_len, 3..4 / 5..6 the suppress / begin-suppress ranges
               into `ids`, 7..8 the set's range of words in `bad_off`
      ids      int64 [n_ids]: every set's suppress, begin-suppress and bad-word ids, one list behind the other
      bad_off  int32 [n_words + 1]: ascending offsets into `ids`, one bad word between two neighbours
      row_set  int32 [rows]: the set each row is processed with - allocated once, a captured step holds its address, and `admit`
               rewrites a row's entry in place by a tensor fill
    eos_ids: the ids the minimum length bans (the call's).  The object also owns the f32 scores scratch the picks scan."""
    active = True
    constraint = None

    def __init__(self, V: int, device, eos_ids, keys, rows: int):
        V = int(V)
        if V <= 0 or V > L.AKI_LOGITS_PROCESS_MAX_V:
            raise ValueError(f"logits processors: a vocabulary of {V} columns (1..{L.AKI_LOGITS_PROCESS_MAX_V} are served)")
        from .slots import NEUTRAL_SET_KEY
        pool = [NEUTRAL_SET_KEY]
        for k in keys:
            if k not in pool:
                pool.append(k)
        ids, offs, recs = [], [], []
        for pen, ngram, min_len, sup, bsup, _ in pool:  # the plain id lists of every set first ...
            rec = [struct.unpack("<i", struct.pack("<f", float(pen)))[0], int(ngram), int(min_len)]
            for lst in (sup, bsup):
                rec += [len(ids), len(ids) + len(lst)]
                ids += [int(i) for i in lst]
            recs.append(rec)
        for rec, key in zip(recs, pool):                # ... then the words, back to back: a word ends where the next one begins
            rec.append(len(offs))
            for w in key[5]:
                offs.append(len(ids))
                ids += [int(i) for i in w]
            rec.append(len(offs))
        offs.append(len(ids))                           # the last word's end; a pool without words holds this one offset
        if any(not 0 <= i < V for i in ids):
            raise ValueError(f"logits processors: every id has to be in [0, {V})")
        dev = torch.device(device)
        self.V, self.keys, self.index = V, pool, {k: i for i, k in enumerate(pool)}
        self.sets = torch.tensor(recs, dtype=torch.int32, device=dev)
        self.ids = torch.tensor(ids, dtype=torch.int64, device=dev)
        self.bad_off = torch.tensor(offs, dtype=torch.int32, device=dev)
        self.row_set = torch.zeros(int(rows), dtype=torch.int32, device=dev)
        eos = [int(e) for e in eos_ids]
        self._eos = torch.tensor(eos, dtype=torch.int64, device=dev) if eos else None
        self._scratch = {}

    def admit(self, row: int, key) -> None:
        """A new request in `row`: its set, by value.  A tensor fill - nothing is copied from the host or reallocated."""
        self.row_set[int(row)] = self.index[key]

    def row(self, slot: int) -> "ProcessorSets":
        """The one-row view: what a B = 1 pick on the slot's row views takes.  The pool and the scratches are shared."""
        s = int(slot)
        view = ProcessorSets.__new__(ProcessorSets)
        view.__dict__.update(self.__dict__)
        view.row_set = self.row_set[s:s + 1]
        return view

    def scores(self, B: int, device) -> torch.Tensor:
        """The f32 [B, >= V] scratch the per-row picks write the processed scores to, one per batch size (kept: a captured graph holds
        its address; the admit's B = 1 picks use another than the step's)."""
        key = (int(B), str(torch.device(device)))
        if key not in self._scratch:
            self._scratch[key] = torch.empty((int(B), (self.V + 3) // 4 * 4), dtype=torch.float32, device=device)
        return self._scratch[key]

    def _args(self, name: str, B: int, V: int, device):
        """(sets, n_sets, row_set, set_ids, n_set_ids, bad_offsets, n_words) of the per-row C entry points, checked."""
        if V != self.V:
            raise AkiError(f"{name}: the processor sets were built for V = {self.V}, the logits have {V} columns")
        for nm, x, dt in (("sets", self.sets, torch.int32), ("ids", self.ids, torch.int64), ("bad_off", self.bad_off, torch.int32),
                          ("row_set", self.row_set, torch.int32)):
            if not torch.is_tensor(x) or x.dtype != dt or not x.is_contiguous() or x.device != device:
                raise AkiError(f"{name}: processor_sets.{nm} is a contiguous {dt} tensor on {device}")
        if self.sets.dim() != 2 or self.sets.shape[0] < 1 or self.sets.shape[1] != L.AKI_PROCESSOR_SET_WORDS:
            raise AkiError(f"{name}: processor_sets.sets is [n_sets >= 1, {L.AKI_PROCESSOR_SET_WORDS}]")
        if tuple(self.row_set.shape) != (B,) or self.bad_off.numel() < 1:
            raise AkiError(f"{name}: processor_sets.row_set is [{B}] and bad_off holds at least one offset")
        return (_ptr(self.sets), self.sets.shape[0], _ptr(self.row_set), _ptr(self.ids) if self.ids.numel() else None, self.ids.numel(),
                _ptr(self.bad_off), self.bad_off.numel() - 1)

    def apply(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, step: int = 0,
              cache_len: Optional[torch.Tensor] = None, start_len: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
              slot_constraints: Optional["SlotConstraints"] = None, frequency_penalty: Optional[torch.Tensor] = None,
              presence_penalty: Optional[torch.Tensor] = None) -> torch.Tensor:
        """LogitsProcessors.apply with row b processed by set row_set[b] (aki_logits_process_rows, one launch): f32 scores [B, V] of bf16
        / f32 logits.  out=None: a view of the pool's own scratch for this batch size - kept, so a per-step caller allocates nothing, and
        overwritten by the next call of that batch size.  slot_constraints: the rows' automata as the last stage (the state history is
        read, not advanced).  frequency_penalty / presence_penalty: optional f32 tensors [B], one value per row (stage 1b;
        aki_logits_process_rows_penalized)."""
        if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] != self.V:
            raise AkiError(f"logits processors: logits [B, {self.V}] with unit column stride are expected, got {tuple(logits.shape)}")
        B = logits.shape[0]
        dev = _dev(logits, out, tokens, cache_len, start_len, done)
        if out is None:
            out = self.scores(B, dev)[:, :self.V]
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or out.shape[1] != self.V:
            raise AkiError("logits processors: out is f32 [B, V] with unit column stride")
        for t_, dt in ((tokens, torch.int64), (cache_len, torch.int32), (start_len, torch.int32), (done, torch.uint8)):
            if t_ is not None and (t_.dtype != dt or not t_.is_contiguous()):
                raise AkiError(f"logits processors: a contiguous {dt} tensor is expected, got {t_.dtype}")
        if tokens is not None and (tokens.dim() != 2 or tokens.shape[0] != B):
            raise AkiError("logits processors: tokens is [B, *]")
        if tokens is not None and tokens.shape[1] == 0:
            tokens = None
        con = _NO_ROW_CONSTRAINT
        if slot_constraints is not None:
            con = slot_constraints._args("logits processors", B, self.V, dev)
        pen = _penalty_rows("logits processors", None, frequency_penalty, presence_penalty, B, dev)
        fn = "aki_logits_process_rows" if pen is None else "aki_logits_process_rows_penalized"
        L.check(getattr(L.load(), fn)(
            _ptr(logits), _dt(logits), B, self.V, logits.stride(0), _ptr(out), out.stride(0), _ptr(tokens),
            0 if tokens is None else tokens.shape[1], _ptr(cache_len), _ptr(start_len), int(step), _ptr(done), _ptr(self._eos),
            0 if self._eos is None else self._eos.numel(), *self._args("logits processors", B, self.V, dev), *con,
            *(() if pen is None else (_ptr(pen[0]), _ptr(pen[1]))), _stream()), fn)
        return out


def _processor_set_args(name: str, processor_sets, processors, slot_constraints, B: int, V: int, device):
    """(the pool's seven C arguments, the per-row constraint's seven) for a pick with processor_sets=, or None without one.  The sets
    stand in the place of `processors` (they own the scores scratch), so the two exclude each other."""
    if processor_sets is None:
        return None
    if not isinstance(processor_sets, ProcessorSets):
        raise AkiError(f"{name}: processor_sets is an ops.ProcessorSets")
    if processors is not None:
        raise AkiError(f"{name}: processor_sets together with processors: the sets hold every row's settings")
    if slot_constraints is not None and not isinstance(slot_constraints, SlotConstraints):
        raise AkiError(f"{name}: slot_constraints is an ops.SlotConstraints")
    con = (None, 0, 0, None, 0, None, None) if slot_constraints is None else slot_constraints._args(name, B, V, device)
    return processor_sets._args(name, B, V, device), con


def _slot_constraint_args(name: str, slot_constraints, processors, B: int, V: int, device):
    """The per-row constraint's seven C arguments, or None without one.  The pick scans the processors' f32 scratch, so an active
    LogitsProcessors is needed (LogitsProcessors(..., slot_constraints=True) is one); it cannot carry a BoundConstraint of its own."""
    if slot_constraints is None:
        return None
    if not isinstance(slot_constraints, SlotConstraints):
        raise AkiError(f"{name}: slot_constraints is an ops.SlotConstraints")
    if processors is None or not processors.active:
        raise AkiError(f"{name}: slot_constraints needs an active LogitsProcessors (LogitsProcessors(..., slot_constraints=True)) for the scores scratch")
    if processors.constraint is not None:
        raise AkiError(f"{name}: slot_constraints together with a LogitsProcessors that carries a constraint of its own")
    return slot_constraints._args(name, B, V, device)


def greedy_pick(logits: torch.Tensor, next_ids: torch.Tensor, pad_token_id: int = 0, eos_ids: Optional[torch.Tensor] = None,
                done: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, cache_len: Optional[torch.Tensor] = None,
                start_len: Optional[torch.Tensor] = None, advance: bool = False, done_at: Optional[torch.Tensor] = None,
                embed=None, next_embeds: Optional[torch.Tensor] = None, processors: Optional[LogitsProcessors] = None,
                slot_constraints: Optional[SlotConstraints] = None, processor_sets: Optional[ProcessorSets] = None,
                frequency_penalty: Optional[torch.Tensor] = None, presence_penalty: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The step between two decode steps of a greedy `generate` as one launch (aki_greedy_pick; HF GenerationMixin's greedy branch):
    next_ids[b] = pad if done[b] else argmax(logits[b]); tokens[b, t] = next with t = cache_len[b] + advance - start_len[b]; rows whose
    next is an eos id become done (done_at[b] = t); advance: cache_len += 1.  logits: bf16 [B, V] (row stride >= V); next_ids / tokens /
    eos_ids int64; done uint8; cache_len / start_len / done_at int32.  Capturable: no host value is read.
    embed = (weight [rows, d], additional_weight [extra, d] or None, max_original_id) with next_embeds bf16 [B, d]: the picked token's
    embedding row (DecoupledEmbedding's two tables, src/helpers.py:440-492) is written to next_embeds in the same launch - the input of the next
    decode step.
    processors (an active LogitsProcessors): the pick scans the processed scores of the row instead, in the same launch
    (aki_greedy_pick_processed); the history is tokens[b, :t] and the minimum length bans eos_ids.
    slot_constraints (an ops.SlotConstraints, with an active `processors` that carries no constraint of its own): one automaton per row as
    the last processor stage (aki_greedy_pick_constrained_rows) - row b in state s = states[b, t] is masked by pool row row_base[b] + s
    and states[b, t + 1] receives the table entry, a state local to the row's automaton; a row in state -1 is picked unmasked.
    processor_sets (an ops.ProcessorSets, in the place of `processors`): one set of processor settings per row (aki_greedy_pick_rows) - row
    b is processed with the pool's set row_set[b]; slot_constraints composes with it and needs no LogitsProcessors then.
    frequency_penalty / presence_penalty: optional f32 tensors [B], one value per row (stage 1b of the processors; a penalised
    LogitsProcessors brings its own) - with processor_sets aki_greedy_pick_rows_penalized, with processors aki_greedy_pick_penalized."""
    common, emb, processed, con = _pick_front("greedy_pick", logits, next_ids, pad_token_id, eos_ids, done, tokens, cache_len, start_len, advance,
                                              done_at, embed, next_embeds, processors, slot_constraints, processor_sets, scratch=False)
    pen = _penalty_rows("greedy_pick", processors, frequency_penalty, presence_penalty, logits.shape[0], logits.device)
    if pen is not None:
        fn = _penalized_form("greedy_pick", processed, processors, slot_constraints, processor_sets)
        args = (*common, *emb, *processed, *(con or _NO_WIDE_CONSTRAINT), _ptr(pen[0]), _ptr(pen[1]))
    elif processed is None:                 # no processors: the plain forms take no scratch (and no V limit)
        fn, args = ("aki_greedy_pick", common) if embed is None else ("aki_greedy_pick_embed", (*common, *emb))
    else:
        fn = "aki_greedy_pick_rows" if processor_sets is not None else "aki_greedy_pick_constrained_rows" if slot_constraints is not None \
            else "aki_greedy_pick_processed" if con is None else "aki_greedy_pick_constrained"
        args = (*common, *emb, *processed, *(con or ()))
    L.check(getattr(L.load(), fn)(*args, _stream()), fn)
    return next_ids


def _penalized_form(name: str, processed, processors, slot_constraints, processor_sets) -> str:
    """The *_penalized entry point of a pick that carries min_p or a frequency / presence penalty: the per-row form with processor_sets,
    else the call-wide one, which has no per-row constraint."""
    if processed is None:
        raise AkiError(f"{name}: frequency_penalty / presence_penalty need the f32 scores scratch of an active LogitsProcessors or of "
                       "processor_sets")
    if processor_sets is not None:
        return f"aki_{name}_rows_penalized"
    if slot_constraints is not None:
        raise AkiError(f"{name}: min_p / frequency_penalty / presence_penalty with slot_constraints take processor_sets (the per-row form)")
    return f"aki_{name}_penalized"


class DeviceGenerator:
    """The random state of the device sampler (`generate(..., do_sample=True, generator=DeviceGenerator(seed))`, ops.sample_pick): a 64-bit
    `seed` (the Philox key) and an `offset` that every `generate` call takes and bumps by one.  A draw depends on (seed, offset, generated-token
    index, row) only - never on the batch a sample sits in, nor on how often a step is replayed."""

    def __init__(self, seed: int = 0):
        self.manual_seed(seed)

    def manual_seed(self, seed: int) -> "DeviceGenerator":
        self.seed, self.offset = int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        return self

    def next_offset(self) -> int:
        o = self.offset
        self.offset += 1
        return o


def _pick_front(name: str, logits, next_ids, pad_token_id, eos_ids, done, tokens, cache_len, start_len, advance, done_at, embed, next_embeds,
                processors, slot_constraints=None, processor_sets=None, step=0, probs_out=None, scores=None, extra=(), scratch=True):
    """What ops.greedy_pick, ops.sample_pick and ops.sample_pick_rows share: the checks of the pick's tensors and embedding tables, the
    scratch rule and the C arguments in their groups -> (the common 15, the embedding 6, the processed part or None, the constraint's
    arguments or None).  The processed part is the scratch pair followed by the processors' eleven arguments - or, with processor_sets (an
    ops.ProcessorSets, in their place), the pool's seven; the constraint's arguments are then always the per-row seven (NULLs without
    slot_constraints), else slot_constraints' seven, else the five of a constraint the processors carry.
    scratch=False (ops.greedy_pick): without active processors or sets there is no processed part - the plain forms take no scratch and no
    V limit.  extra: further (tensor, dtype) pairs to check."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise AkiError(f"{name} takes bf16 logits [B, V] with unit column stride")
    B, V = logits.shape
    for t_, dt in ((next_ids, torch.int64), (tokens, torch.int64), (eos_ids, torch.int64), (done, torch.uint8), (cache_len, torch.int32),
                   (start_len, torch.int32), (done_at, torch.int32), (probs_out, torch.float32), (scores, torch.float32), *extra):
        if t_ is not None and (t_.dtype != dt or not t_.is_contiguous() or t_.device != logits.device):
            raise AkiError(f"{name}: a {dt} contiguous tensor on {logits.device} is expected, got {t_.dtype} {tuple(t_.shape)}")
    if tokens is not None and (tokens.dim() != 2 or tokens.shape[0] != B):
        raise AkiError(f"{name}: tokens is [B, max_new_tokens]")
    if probs_out is not None and tuple(probs_out.shape) != (B, V):
        raise AkiError(f"{name}: probs_out is f32 [B, V]")
    common = (_ptr(logits), B, V, logits.stride(0), _ptr(eos_ids), 0 if eos_ids is None else eos_ids.numel(), int(pad_token_id), _ptr(done),
              _ptr(next_ids), _ptr(tokens), 0 if tokens is None else tokens.shape[1], _ptr(cache_len), _ptr(start_len), 1 if advance else 0,
              _ptr(done_at))
    emb = (None, None, 0, 0, 0, None)
    if embed is not None:
        w, extra_w, max_orig = embed
        d = w.shape[1]
        for t_ in (w, extra_w, next_embeds):
            if t_ is not None and (t_.dtype != torch.bfloat16 or not t_.is_contiguous() or t_.device != logits.device or t_.shape[-1] != d):
                raise AkiError(f"{name}: embedding tables and next_embeds are contiguous bf16 [*, d] on the logits' device")
        if next_embeds is None or next_embeds.numel() != B * d:
            raise AkiError(f"{name}: next_embeds is [B, d]")
        if w.shape[0] <= max_orig:
            raise AkiError(f"{name}: the embedding table has fewer than max_original_id + 1 rows")
        emb = (_ptr(w), _ptr(extra_w), int(max_orig), 0 if extra_w is None else extra_w.shape[0], d, _ptr(next_embeds))
    sets = _processor_set_args(name, processor_sets, processors, slot_constraints, B, V, logits.device)
    con = None if sets is not None else _slot_constraint_args(name, slot_constraints, processors, B, V, logits.device)
    active = processors is not None and processors.active
    if active and processors.V != V:
        raise AkiError(f"{name}: the processors were built for V = {processors.V}, the logits have {V} columns")
    if not (scratch or active or sets is not None):
        return common, emb, None, None
    if V > L.AKI_LOGITS_PROCESS_MAX_V:
        raise AkiError(f"{name}: a vocabulary of {V} is above {L.AKI_LOGITS_PROCESS_MAX_V}")
    if scores is None:
        scores = processor_sets.scores(B, logits.device) if sets is not None else \
            processors.scores(B, logits.device) if active else _sample_scratch(B, V, logits.device)
    if scores.dim() != 2 or scores.shape[0] != B or scores.shape[1] < V:
        raise AkiError(f"{name}: scores is f32 [B, >= V]")
    if sets is not None:
        proc, con = sets
    else:
        head, tail = processors._tail() if active else ((1.0, 0, 0), (None, 0, None, 0, None, None, 0, 0))
        proc = (*head, *tail)
        if con is None and active:
            con = processors._constraint_args(B, tokens.shape[1] if tokens is not None else (int(step) + 1 if cache_len is None else None))
    return common, emb, (_ptr(scores), scores.stride(0), *proc), con


def sample_pick(logits: torch.Tensor, next_ids: torch.Tensor, pad_token_id: int = 0, eos_ids: Optional[torch.Tensor] = None,
                done: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, cache_len: Optional[torch.Tensor] = None,
                start_len: Optional[torch.Tensor] = None, advance: bool = False, done_at: Optional[torch.Tensor] = None,
                embed=None, next_embeds: Optional[torch.Tensor] = None, processors: Optional[LogitsProcessors] = None, step: int = 0,
                temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, offset: int = 0,
                probs_out: Optional[torch.Tensor] = None, scores: Optional[torch.Tensor] = None, min_p: float = 0.0,
                frequency_penalty: Optional[torch.Tensor] = None, presence_penalty: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.greedy_pick's sibling for `do_sample=True`, one launch (aki_sample_pick): processors, temperature, top-k, top-p and one
    counter-based draw per row, then the same bookkeeping and embedding gather.  The draw of row b is u = Philox4x32-10(key = seed,
    counter = (n, b, offset))[0], n = step + (cache_len[b] + advance - start_len[b] when cache_len is given) - the index tokens[b, n] is
    written at.  probs_out: optional f32 [B, V], the filtered distribution the draw was made from.  scores: the f32 [B, >= V] scratch
    (default: the processors' own, or one kept per shape).  Capturable: no host value is read.
    min_p (HF MinPLogitsWarper, behind top-p): of the tokens top-k and top-p kept, those with exp(y - ymax) >= min_p stay; 0 = no filter.
    frequency_penalty / presence_penalty: optional f32 tensors [B] (a penalised LogitsProcessors brings its own).  With any of the three
    the launch is aki_sample_pick_penalized."""
    if not (float(temperature) > 0.0) or not (0.0 < float(top_p) <= 1.0) or int(top_k) < 0 or int(step) < 0:
        raise ValueError(f"sample_pick: temperature > 0, 0 < top_p <= 1, top_k >= 0 and step >= 0 are expected, got {temperature}, {top_p}, {top_k}, {step}")
    common, emb, processed, con = _pick_front("sample_pick", logits, next_ids, pad_token_id, eos_ids, done, tokens, cache_len, start_len, advance,
                                              done_at, embed, next_embeds, processors, step=step, probs_out=probs_out, scores=scores)
    pen = _penalty_rows("sample_pick", processors, frequency_penalty, presence_penalty, logits.shape[0], logits.device,
                        _min_p_rows(min_p, logits.shape[0], logits.device))
    fn = "aki_sample_pick" if con is None else "aki_sample_pick_constrained"
    tail = ()
    if pen is not None:
        fn, con, tail = "aki_sample_pick_penalized", con or _NO_WIDE_CONSTRAINT, tuple(_ptr(x) for x in pen)
    L.check(getattr(L.load(), fn)(*common, *emb, *processed, int(step), float(temperature), int(top_k), float(top_p),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, _ptr(probs_out),
                                  0 if probs_out is None else probs_out.stride(0), *(con or ()), *tail, _stream()), fn)
    return next_ids


def sample_pick_rows(logits: torch.Tensor, next_ids: torch.Tensor, pad_token_id: int = 0, eos_ids: Optional[torch.Tensor] = None,
                     done: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, cache_len: Optional[torch.Tensor] = None,
                     start_len: Optional[torch.Tensor] = None, advance: bool = False, done_at: Optional[torch.Tensor] = None,
                     embed=None, next_embeds: Optional[torch.Tensor] = None, processors: Optional[LogitsProcessors] = None, step: int = 0,
                     temperature: Optional[torch.Tensor] = None, top_k: Optional[torch.Tensor] = None, top_p: Optional[torch.Tensor] = None,
                     seed: Optional[torch.Tensor] = None, probs_out: Optional[torch.Tensor] = None,
                     scores: Optional[torch.Tensor] = None, slot_constraints: Optional[SlotConstraints] = None,
                     processor_sets: Optional[ProcessorSets] = None, min_p: Optional[torch.Tensor] = None,
                     frequency_penalty: Optional[torch.Tensor] = None, presence_penalty: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.sample_pick with the sampling parameters per row, one launch (aki_sample_pick_rows): `temperature` f32, `top_k` int32, `top_p`
    f32 and `seed` int64 (its bits are the 64-bit Philox key) are contiguous device tensors [B], read by the launch - a captured step
    serves rows whose parameters are rewritten in place.  Row b draws u = Philox4x32-10(key = seed[b], counter = (n, 0, 0, 0))[0], n as
    in ops.sample_pick: the draw of row 0 of a B = 1 ops.sample_pick call with that seed and offset 0, so the stream belongs to the seed and
    not to the row.  A row with top_k[b] == 1 takes ops.greedy_pick's token.  A LogitsProcessors that carries a constraint is refused
    (its row_start is fixed for its life); slot_constraints (an ops.SlotConstraints, as in ops.greedy_pick) gives every row its own
    automaton instead (aki_sample_pick_rows_constrained): the draw is made among the tokens the row's state allows.  The VALUES in the four arrays are not checked here (no host value is read: capturable); whoever writes them validates them
    (temperature > 0, top_k >= 0, 0 < top_p <= 1) - in the kernel a temperature that is not > 0 falls to the greedy token, top_k <= 0 or
    >= V and top_p >= 1 switch their filter off.
    processor_sets (an ops.ProcessorSets, in the place of `processors`): one set of processor settings per row
    (aki_sample_pick_rows_processed); slot_constraints composes with it and needs no LogitsProcessors then.
    min_p, frequency_penalty, presence_penalty: optional f32 tensors [B], one value per row, read by the launch like the four above
    (aki_sample_pick_rows_penalized: the per-row form, so they come with processor_sets - a pool that holds the neutral set alone will
    do).  A min_p[b] outside (0, 1] is no filter, a penalty that is not finite reads as 0."""
    if int(step) < 0:
        raise ValueError(f"sample_pick_rows: step >= 0 is expected, got {step}")
    rows = ((temperature, torch.float32), (top_k, torch.int32), (top_p, torch.float32), (seed, torch.int64))
    if logits.dim() == 2 and any(t_ is None or tuple(t_.shape) != (logits.shape[0],) for t_, _ in rows):
        raise AkiError(f"sample_pick_rows: temperature (f32), top_k (int32), top_p (f32) and seed (int64) are tensors [{logits.shape[0]}]")
    if processors is not None and processors.active and processors.constraint is not None:
        raise AkiError("sample_pick_rows: a LogitsProcessors with a constraint of its own is not taken (no constrained form of that kind); "
                       "pass slot_constraints, or use ops.sample_pick")
    common, emb, processed, con = _pick_front("sample_pick_rows", logits, next_ids, pad_token_id, eos_ids, done, tokens, cache_len, start_len,
                                              advance, done_at, embed, next_embeds, processors, slot_constraints, processor_sets, step=step,
                                              probs_out=probs_out, scores=scores, extra=rows)
    fn = "aki_sample_pick_rows_processed" if processor_sets is not None else \
        "aki_sample_pick_rows" if con is None else "aki_sample_pick_rows_constrained"
    pen = _penalty_rows("sample_pick_rows", processors, frequency_penalty, presence_penalty, logits.shape[0], logits.device, min_p)
    tail = ()
    if pen is not None:
        if processor_sets is None:
            raise AkiError("sample_pick_rows: min_p / frequency_penalty / presence_penalty take processor_sets (the per-row form: "
                           "aki_sample_pick_rows_penalized); a pool that holds the neutral set alone will do")
        fn, tail = "aki_sample_pick_rows_penalized", tuple(_ptr(x) for x in pen)
    L.check(getattr(L.load(), fn)(*common, *emb, *processed, int(step), _ptr(temperature), _ptr(top_k), _ptr(top_p), _ptr(seed), _ptr(probs_out),
                                  0 if probs_out is None else probs_out.stride(0), *(con or ()), *tail, _stream()), fn)
    return next_ids


_SAMPLE_SCRATCH = {}


def _sample_scratch(B: int, V: int, dev) -> torch.Tensor:
    """The sampler's f32 [B, V rounded up to 4] row scratch when no processors own one (kept per shape: a captured graph holds its address)."""
    key = (B, V, str(dev))
    if key not in _SAMPLE_SCRATCH:
        _SAMPLE_SCRATCH[key] = torch.empty((B, (V + 3) // 4 * 4), dtype=torch.float32, device=dev)
    return _SAMPLE_SCRATCH[key]


# ---- beam search on the device (beam.hip) ----------------------------------------------------------------------------------------
BEAM_MAX_K, BEAM_MAX_EOS, KV_BEAM_REORDER_CHUNK = L.AKI_BEAM_MAX_K, L.AKI_BEAM_MAX_EOS, L.AKI_KV_BEAM_REORDER_CHUNK


def beam_logprob(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f32 log-softmax [rows, V] of bf16 / f32 logits [rows, V] (row stride >= V), one launch (aki_beam_logprob): f32 arithmetic in a
    fixed order - the same inputs give the same bits on every run."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise AkiError("beam_logprob takes logits [rows, V] with unit column stride and a row stride >= V")
    rows, V = logits.shape
    dev = _dev(logits, out)
    if out is None:
        out = torch.empty((rows, V), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (rows, V) or out.stride(1) != 1 or out.stride(0) < V:
        raise AkiError("beam_logprob: out is f32 [rows, V] with unit column stride")
    L.check(L.load().aki_beam_logprob(_ptr(logits), _dt(logits), rows, V, logits.stride(0), _ptr(out), out.stride(0), _stream()),
            "aki_beam_logprob")
    return out


# ---- per-token log-probabilities (logprob.hip) -----------------------------------------------------------------------------------
LOGPROB_MAX_TOP, LOGPROB_MAX_V = L.AKI_LOGPROB_MAX_TOP, L.AKI_LOGPROB_MAX_V


def token_logprob(logits: torch.Tensor, ids: Optional[torch.Tensor] = None, top_k: int = 0, skip: Optional[torch.Tensor] = None,
                  step: int = 0, tokens: Optional[torch.Tensor] = None, cache_len: Optional[torch.Tensor] = None,
                  start_len: Optional[torch.Tensor] = None, done_at: Optional[torch.Tensor] = None,
                  out_logprob: Optional[torch.Tensor] = None, out_top_ids: Optional[torch.Tensor] = None,
                  out_top_logprobs: Optional[torch.Tensor] = None):
    """The log-probability of one token per row under the f32 log-softmax of bf16 / f32 logits [rows, V] (row stride >= V), with the
    `top_k` <= LOGPROB_MAX_TOP most likely columns and theirs, one launch (aki_token_logprob; fixed reduction order: the same inputs give
    the same bits on every run).  Returns (logprob f32 [rows, cols], top ids int64 [rows, cols, top_k] or None, top logprobs f32 [rows,
    cols, top_k] or None): the outputs passed in, or new ones of one column (step + 1 columns when a step is given), filled with the
    skipped values.  Row r writes column t = step + (cache_len[r] - start_len[r] when cache_len is given), nothing when t is outside the
    outputs.
    Plain form: `ids` int64 [rows], optional `skip` uint8 [rows] (such rows write logprob 0, ids -1, top logprobs 0) and `step`.
    In-loop form, behind ops.greedy_pick / ops.sample_pick with the same tensors: `tokens` int64 [rows, *] (the token is tokens[r, t]),
    `cache_len` / `start_len` int32 [rows] and `done_at` int32 [rows] (a row that finished before step t is skipped; the step that picked
    its EOS is scored).  Capturable: no host value is read.  An id outside [0, V) gives NaN."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise AkiError("token_logprob takes logits [rows, V] with unit column stride and a row stride >= V")
    rows, V = logits.shape
    top_k, step = int(top_k), int(step)
    if not 0 <= top_k <= LOGPROB_MAX_TOP or step < 0 or not 1 <= V <= LOGPROB_MAX_V or rows < 1:
        raise AkiError(f"token_logprob: 0 <= top_k <= {LOGPROB_MAX_TOP}, step >= 0, rows >= 1 and 1 <= V <= {LOGPROB_MAX_V} are expected")
    dev = _dev(logits, ids, skip, tokens, cache_len, start_len, done_at, out_logprob, out_top_ids, out_top_logprobs)
    _dt(logits)
    if (ids is None) == (tokens is None):
        raise AkiError("token_logprob takes the tokens either as ids [rows] or as tokens [rows, *] (the in-loop form)")
    if (cache_len is None) != (start_len is None):
        raise AkiError("token_logprob: cache_len and start_len go together")
    for t_, dt in ((ids, torch.int64), (tokens, torch.int64), (skip, torch.uint8), (cache_len, torch.int32), (start_len, torch.int32),
                   (done_at, torch.int32)):
        if t_ is not None and (t_.dtype != dt or not t_.is_contiguous()):
            raise AkiError(f"token_logprob: a contiguous {dt} tensor is expected, got {t_.dtype} {tuple(t_.shape)}")
    for t_ in (ids, skip, cache_len, start_len, done_at):
        if t_ is not None and tuple(t_.shape) != (rows,):
            raise AkiError(f"token_logprob: a per-row tensor [{rows}] is expected, got {tuple(t_.shape)}")
    if tokens is not None and (tokens.dim() != 2 or tokens.shape[0] != rows or tokens.shape[1] < 1):
        raise AkiError("token_logprob: tokens is [rows, >= 1]")
    if out_logprob is None:
        cols = tokens.shape[1] if tokens is not None else step + 1
        out_logprob = torch.zeros((rows, cols), dtype=torch.float32, device=dev)
    if out_logprob.dtype != torch.float32 or out_logprob.dim() != 2 or out_logprob.shape[0] != rows or not out_logprob.is_contiguous():
        raise AkiError("token_logprob: out_logprob is contiguous f32 [rows, cols]")
    cols = out_logprob.shape[1]
    if top_k > 0:
        if out_top_ids is None:
            out_top_ids = torch.full((rows, cols, top_k), -1, dtype=torch.int64, device=dev)
        if out_top_logprobs is None:
            out_top_logprobs = torch.zeros((rows, cols, top_k), dtype=torch.float32, device=dev)
        for t_, dt in ((out_top_ids, torch.int64), (out_top_logprobs, torch.float32)):
            if t_.dtype != dt or tuple(t_.shape) != (rows, cols, top_k) or not t_.is_contiguous():
                raise AkiError(f"token_logprob: the top-k outputs are contiguous [rows, cols, top_k] = [{rows}, {cols}, {top_k}], int64 ids and f32 logprobs")
    else:
        out_top_ids = out_top_logprobs = None
    L.check(L.load().aki_token_logprob(_ptr(logits), _dt(logits), rows, V, logits.stride(0), _ptr(ids), _ptr(tokens),
                                       0 if tokens is None else tokens.stride(0), _ptr(cache_len), _ptr(start_len), step, _ptr(skip),
                                       _ptr(done_at), top_k, _ptr(out_logprob), _ptr(out_top_ids), _ptr(out_top_logprobs), cols, cols,
                                       _stream()), "aki_token_logprob")
    return out_logprob, out_top_ids, out_top_logprobs


class BeamState:
    """The device state of one beam search (ops.beam_step), allocated once: running `beam_scores` f32 [B, K] (beam 0 of a sample starts at
    0, the others at -1e9: all beams start identical), the beams' tokens `seqs` int64 [B*K, max_new] (a ping-pong pair: `seqs` is the
    buffer the last step wrote), the hypotheses `hyp_score` f32 [B, K], `hyp_len` int32 [B, K], `hyp_tokens` int64 [B, K, max_new],
    `hyp_count` int32 [B], the samples' `done` flags uint8 [B], and the last step's `next_ids` int64 [B*K] and `parent` int32 [B*K]
    (global rows b*K + beam).  early_stopping: True, False, or anything else ("never"), as HF's BeamSearchScorer reads it."""

    def __init__(self, B: int, K: int, max_new: int, device, eos_ids=(), pad_token_id: int = 0, length_penalty: float = 1.0,
                 early_stopping=False):
        B, K, max_new = int(B), int(K), int(max_new)
        eos = sorted(set(int(e) for e in eos_ids))
        if B < 1 or max_new < 1 or not 1 <= K <= BEAM_MAX_K or len(eos) > BEAM_MAX_EOS:
            raise AkiError(f"BeamState: B >= 1, max_new >= 1, 1 <= K <= {BEAM_MAX_K} and at most {BEAM_MAX_EOS} eos ids are expected")
        dev = torch.device(device)
        self.B, self.K, self.max_new = B, K, max_new
        self.pad_token_id, self.length_penalty = int(pad_token_id), float(length_penalty)
        self.early = 1 if early_stopping is True else (0 if early_stopping is False else 2)
        self.eos = torch.tensor(eos, dtype=torch.int64, device=dev) if eos else None
        self.beam_scores = torch.zeros((B, K), dtype=torch.float32, device=dev)
        self.beam_scores[:, 1:] = -1e9
        self._seqs = [torch.zeros((B * K, max_new), dtype=torch.int64, device=dev) for _ in range(2)]
        self._cur = 0
        self.hyp_score = torch.zeros((B, K), dtype=torch.float32, device=dev)
        self.hyp_len = torch.zeros((B, K), dtype=torch.int32, device=dev)
        self.hyp_tokens = torch.zeros((B, K, max_new), dtype=torch.int64, device=dev)
        self.hyp_count = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.done = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.next_ids = torch.zeros((B * K,), dtype=torch.int64, device=dev)
        self.parent = torch.arange(B * K, dtype=torch.int32, device=dev)

    @property
    def seqs(self) -> torch.Tensor:
        return self._seqs[self._cur]


def beam_step(logp: torch.Tensor, state: BeamState, t: int, last: bool = False) -> BeamState:
    """One step of the search for every sample, one launch (aki_beam_step; the per-token body of AKI._beam_search): the 2K best of
    logp[b*K + k, v] + beam_scores[b, k] ranked by score (exactly equal scores: the lower k*V + v first), the EOS / hypothesis / done
    bookkeeping of HF's BeamSearchScorer, state.seqs re-ordered by parent and extended by token t.  logp: f32 [B*K, V] (row stride >= V).
    last: the closing step.  Capturable: no host value is read."""
    if logp.dtype != torch.float32 or logp.dim() != 2 or logp.stride(1) != 1 or logp.shape[0] != state.B * state.K \
            or logp.stride(0) < logp.shape[1]:
        raise AkiError("beam_step takes f32 log-probabilities [B*K, V] with unit column stride")
    if _dev(logp) != state.beam_scores.device:
        raise AkiError("beam_step: logp and the state are on different devices")
    t = int(t)
    if not 0 <= t < state.max_new:
        raise AkiError(f"beam_step: step {t} is outside [0, {state.max_new})")
    src, dst = state._seqs[state._cur], state._seqs[1 - state._cur]
    L.check(L.load().aki_beam_step(_ptr(logp), logp.stride(0), state.B, state.K, logp.shape[1], t, state.max_new, _ptr(state.beam_scores),
                                   _ptr(src), _ptr(dst), _ptr(state.hyp_score), _ptr(state.hyp_len), _ptr(state.hyp_tokens),
                                   _ptr(state.hyp_count), _ptr(state.done), _ptr(state.next_ids), _ptr(state.parent), _ptr(state.eos),
                                   0 if state.eos is None else state.eos.numel(), state.pad_token_id, state.length_penalty, state.early,
                                   1 if last else 0, _stream()), "aki_beam_step")
    state._cur = 1 - state._cur
    return state


class KVBeamTable:
    """The device table of ops.kv_beam_reorder: the base addresses of the cache tensors [B*K, H, capacity, Dh] (every layer's K and V),
    built once per search.  The tensors are held, so the addresses stay valid."""

    def __init__(self, tensors):
        self.tensors = list(tensors)
        t0 = self.tensors[0]
        for t_ in self.tensors:
            if t_.dim() != 4 or t_.shape != t0.shape or t_.dtype != t0.dtype or not t_.is_contiguous() or not t_.is_cuda or t_.device != t0.device:
                raise AkiError("kv_beam_reorder: contiguous GPU tensors [rows, H, capacity, Dh] of one shape and dtype are expected")
        self.rows, self.H, self.capacity, Dh = t0.shape
        self.row_bytes = Dh * t0.element_size()
        if self.row_bytes % 4 or any(t_.data_ptr() % 16 for t_ in self.tensors):
            raise AkiError("kv_beam_reorder: rows of a multiple of 4 bytes in 16-byte aligned tensors are expected")
        self.table = torch.tensor([t_.data_ptr() for t_ in self.tensors], dtype=torch.int64, device=t0.device)


def kv_beam_reorder(table: KVBeamTable, parent: torch.Tensor, start_len: torch.Tensor, cache_len: torch.Tensor, K: int, pos_lo: int,
                    pos_hi: int) -> None:
    """Beam search's cache re-ordering in place, one launch over all tensors of `table` (aki_kv_beam_reorder):
    t[b*K + n, h, pos, :] = t[parent[b*K + n], h, pos, :] for start_len[row] <= pos < cache_len[row] - the rows written since the prefill; the
    prompt rows, identical across the beams of a sample, never move.  parent / start_len / cache_len: int32 [rows] on the device;
    [pos_lo, pos_hi): host bounds of those positions (they size the grid only).  Samples whose parents are the identity are skipped."""
    K = int(K)
    rows = table.rows
    for t_ in (parent, start_len, cache_len):
        if t_.dtype != torch.int32 or not t_.is_contiguous() or t_.device != table.table.device or t_.numel() != rows:
            raise AkiError("kv_beam_reorder: parent, start_len and cache_len are contiguous int32 [rows] on the cache's device")
    if not 1 <= K <= BEAM_MAX_K or rows % K:
        raise AkiError(f"kv_beam_reorder: 1 <= K <= {BEAM_MAX_K} dividing the cache's {rows} rows is expected")
    pos_lo, pos_hi = max(int(pos_lo), 0), min(int(pos_hi), table.capacity)
    if pos_hi <= pos_lo:
        return
    L.check(L.load().aki_kv_beam_reorder(_ptr(table.table), len(table.tensors), _ptr(parent), _ptr(start_len), _ptr(cache_len), rows // K, K,
                                         table.H, table.capacity, table.row_bytes, pos_lo, pos_hi, _stream()), "aki_kv_beam_reorder")


# ---- in-flight batching (slots.hip) -----------------------------------------------------------------------------------------------
SLOT_MAX_ROWS = L.AKI_SLOT_MAX_ROWS


def kv_slot_admit(src_cache, dst_cache, slot: int) -> None:
    """One prefilled sequence into row `slot` of a larger cache (aki_kv_slot_admit): dst.k[i][slot, :, :len] = src.k[i][0, :, :len], the same
    for v, all layers in one launch, len = src.cache_len[0] read on the device; every other byte of dst stays as it was.  src_cache: an
    AkiKVCache of one sequence [1, H, cap_src, Dh]; dst_cache: one of B rows [B, H, cap_dst, Dh] in the same format (an fp8_e4m3 pair moves
    its f32 scales in a second launch).  Bytes only: nothing is converted.  Rows move as 16-byte vectors when the row bytes and every tensor
    address allow, as 4-byte words otherwise.  dst.cache_len is not touched: the row's state belongs to the caller."""
    slot = int(slot)
    sk, dk = list(src_cache.k) + list(src_cache.v), list(dst_cache.k) + list(dst_cache.v)
    if getattr(src_cache, "group", 1) != 1 or getattr(dst_cache, "group", 1) != 1:
        raise AkiError("kv_slot_admit: neither cache may be grouped (share_prefix)")
    if src_cache.kv_dtype != dst_cache.kv_dtype or len(sk) != len(dk) or not sk:
        raise AkiError("kv_slot_admit: both caches hold the same layers in the same kv_dtype (nothing is converted)")
    s0, d0 = sk[0], dk[0]
    if s0.dim() != 4 or d0.dim() != 4 or s0.shape[0] != 1 or s0.shape[1] != d0.shape[1] or s0.shape[3] != d0.shape[3] or s0.dtype != d0.dtype:
        raise AkiError(f"kv_slot_admit: a source [1, H, cap, Dh] and a destination [B, H, cap, Dh] of one H, Dh and element type are expected, "
                       f"got {tuple(s0.shape)} {s0.dtype} and {tuple(d0.shape)} {d0.dtype}")
    B, H, cap_dst, Dh = d0.shape
    cap_src = s0.shape[2]
    if not 0 <= slot < B:
        raise AkiError(f"kv_slot_admit: slot {slot} is outside the destination's {B} rows")
    host_len = int(src_cache.host_len)
    if not 0 <= host_len <= cap_src or host_len > cap_dst:
        raise AkiError(f"kv_slot_admit: the source holds {host_len} of {cap_src} rows, the destination has room for {cap_dst}")
    ln = src_cache.cache_len
    if ln.dtype != torch.int32 or ln.numel() != 1 or not ln.is_cuda or ln.device != d0.device:
        raise AkiError("kv_slot_admit: the source's cache_len is int32 [1] on the destination's device")

    def launch(src, dst):
        a, b = src[0], dst[0]
        for t_ in src:
            if t_.shape != a.shape or t_.dtype != a.dtype or not t_.is_contiguous() or not t_.is_cuda or t_.device != d0.device:
                raise AkiError("kv_slot_admit: contiguous source tensors of one shape and dtype on the destination's device are expected")
        for t_ in dst:
            if t_.shape != b.shape or t_.dtype != b.dtype or not t_.is_contiguous() or t_.device != d0.device:
                raise AkiError("kv_slot_admit: contiguous destination tensors of one shape and dtype on one device are expected")
        row_bytes = (a.shape[3] if a.dim() == 4 else 1) * a.element_size()
        if row_bytes % 4 or any(t_.data_ptr() % 4 for t_ in src + dst):
            raise AkiError(f"kv_slot_admit: rows of {row_bytes} bytes - a multiple of 4 bytes in 4-byte aligned tensors is expected")
        vec = 16 if row_bytes % 16 == 0 and all(t_.data_ptr() % 16 == 0 for t_ in src + dst) else 4
        table = torch.tensor([t_.data_ptr() for t_ in src + dst], dtype=torch.int64, device=d0.device)
        L.check(L.load().aki_kv_slot_admit(_ptr(table), len(src), _ptr(ln), H, cap_src, cap_dst, B, slot, row_bytes, vec, host_len, _stream()),
                "aki_kv_slot_admit")

    launch(sk, dk)
    if src_cache.k_scale is not None:                 # fp8_e4m3: one f32 scale per (head, position) - [*, H, cap] read as rows of 4 bytes
        ss, ds = list(src_cache.k_scale) + list(src_cache.v_scale), list(dst_cache.k_scale) + list(dst_cache.v_scale)
        if len(ss) != len(sk) or len(ds) != len(dk) or any(t_.shape != s0.shape[:3] for t_ in ss) or any(t_.shape != d0.shape[:3] for t_ in ds):
            raise AkiError("kv_slot_admit: the scales of an fp8_e4m3 cache are [rows, H, capacity] per layer")
        launch(ss, ds)


STOP_MAX_SEQS, STOP_MAX_LEN = L.AKI_STOP_MAX_SEQS, L.AKI_STOP_MAX_LEN


class StopSets:
    """One stop set per ROW (aki_amd/stops.py states the rule): what ops.stop_check and ops.slot_tick(stops=...) take.  The distinct sets of
    a call are a small pool, deduplicated by value and uploaded once (stops.StopPool; set 0 is the empty set):
      ids        int32 [n_ids]: every sequence one behind the other
      seq_off    int32 [n_seqs + 1], set_first int32 [n_sets + 1]: the pool's offsets
      row_set    int32 [rows]: the set each row is checked against; a value outside the pool is the empty set
      stop_hit   int32 [rows]: the index within its set of the sequence that ended the row, -1 for a row that ended otherwise
    row_set and stop_hit are allocated once - a captured step holds their addresses - and `admit` rewrites a row's entries in place."""

    def __init__(self, device, keys, rows: int, _view=None):
        if _view is not None:
            self.__dict__.update(_view)
            return
        from .stops import StopPool
        pool = StopPool(keys)
        dev = torch.device(device)
        self.keys, self.index = pool.keys, pool.index
        self.n_ids, self.n_seqs, self.n_sets = len(pool.ids), pool.n_seqs, pool.n_sets
        self.ids = torch.tensor(pool.ids, dtype=torch.int32, device=dev)
        self.seq_off = torch.tensor(pool.seq_off, dtype=torch.int32, device=dev)
        self.set_first = torch.tensor(pool.set_first, dtype=torch.int32, device=dev)
        self.row_set = torch.zeros(int(rows), dtype=torch.int32, device=dev)
        self.stop_hit = torch.full((int(rows),), -1, dtype=torch.int32, device=dev)

    def admit(self, slot: int, key) -> None:
        """A new request in `slot`: its set, by value, and its hit back to -1.  Tensor fills - nothing is copied from the host or
        reallocated."""
        self.row_set[int(slot)] = self.index[key]
        self.stop_hit[int(slot)] = -1

    def row(self, slot: int) -> "StopSets":
        """One-row views of row_set and stop_hit over the shared pool: what a B = 1 check on the slot's row views takes."""
        s = int(slot)
        return StopSets(None, None, 1, _view=dict(self.__dict__, row_set=self.row_set[s:s + 1], stop_hit=self.stop_hit[s:s + 1]))

    def _args(self, name: str, B: int, device):
        """(stop_hit | ids, n_ids, seq_off, n_seqs, set_first, n_sets, row_set) of the C entry points, checked."""
        for nm, x, n in (("ids", self.ids, self.n_ids), ("seq_off", self.seq_off, self.n_seqs + 1), ("set_first", self.set_first, self.n_sets + 1),
                         ("row_set", self.row_set, B), ("stop_hit", self.stop_hit, B)):
            if not torch.is_tensor(x) or x.dtype != torch.int32 or tuple(x.shape) != (n,) or not x.is_contiguous() or not x.is_cuda \
                    or x.device != device:
                raise AkiError(f"{name}: stops.{nm} is a contiguous int32 GPU tensor [{n}] on {device}")
        return _ptr(self.stop_hit), (_ptr(self.ids) if self.n_ids else None, self.n_ids, _ptr(self.seq_off), self.n_seqs, _ptr(self.set_first),
                                     self.n_sets, _ptr(self.row_set))


def _stop_tokens(name: str, tokens, B: int, device):
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int64 or tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1 \
            or not tokens.is_contiguous() or not tokens.is_cuda or tokens.device != device:
        raise AkiError(f"{name}: tokens is a contiguous int64 GPU tensor [{B}, >= 1] on the rows' device")


def stop_check(tokens: torch.Tensor, cache_len: torch.Tensor, start_len: torch.Tensor, done: torch.Tensor, done_at: torch.Tensor,
               stops: StopSets) -> None:
    """The rows' stop sequences, one launch right behind the pick - and behind ops.token_logprob where there is one (aki_stop_check; one wave
    per row; capturable: no host value is read).  t = cache_len[b] - start_len[b] is the index the pick just wrote.  A live row whose
    generated tokens tokens[b, :t + 1] end with a sequence of its set stops.row_set[b] gets done[b] = 1, done_at[b] = t and
    stops.stop_hit[b] = the lowest-numbered such sequence; a done row, a row with t outside the buffer and a row without a match are not
    touched.  tokens int64 [B, *], done uint8 [B], the others int32 [B]."""
    if not isinstance(stops, StopSets):
        raise AkiError("stop_check: stops is an ops.StopSets")
    B = done.numel() if torch.is_tensor(done) else 0
    for t_, dt in ((done, torch.uint8), (done_at, torch.int32), (cache_len, torch.int32), (start_len, torch.int32)):
        if not torch.is_tensor(t_) or t_.dtype != dt or t_.dim() != 1 or t_.numel() != B or not t_.is_contiguous() or not t_.is_cuda \
                or t_.device != done.device:
            raise AkiError("stop_check: contiguous GPU tensors [B] are expected - done uint8, done_at / cache_len / start_len int32")
    if B < 1:
        raise AkiError("stop_check: at least one row is expected")
    _stop_tokens("stop_check", tokens, B, done.device)
    hit, pool = stops._args("stop_check", B, done.device)
    L.check(L.load().aki_stop_check(_ptr(tokens), tokens.shape[1], _ptr(cache_len), _ptr(start_len), _ptr(done), _ptr(done_at), hit, *pool, B,
                                    _stream()), "aki_stop_check")


def slot_tick(done: torch.Tensor, done_at: torch.Tensor, cache_len: torch.Tensor, start_len: torch.Tensor, limit: torch.Tensor,
              stops: Optional[StopSets] = None, tokens: Optional[torch.Tensor] = None) -> None:
    """The per-row token budget, one launch right behind the pick (aki_slot_tick; capturable: no host value is read).  With generated =
    cache_len[b] - start_len[b] + 1 tokens picked by row b: a live row with generated >= limit[b] gets done[b] = 1 and done_at[b] =
    generated - 1; a done row (done_at >= 0) is parked at cache_len[b] = start_len[b] + done_at[b], so the pad-token steps it is still fed
    overwrite one dead cache row; a live row under its budget is not touched.  done uint8 [B], the others int32 [B], B <= SLOT_MAX_ROWS.
    stops (an ops.StopSets, with the rows' tokens int64 [B, *]): ops.stop_check and this tick in ONE launch (aki_slot_tick_stops), with
    the effect of the two calls one behind the other; without it exactly the call above."""
    B = done.numel()
    for t_, dt in ((done, torch.uint8), (done_at, torch.int32), (cache_len, torch.int32), (start_len, torch.int32), (limit, torch.int32)):
        if t_.dtype != dt or t_.dim() != 1 or t_.numel() != B or not t_.is_contiguous() or not t_.is_cuda or t_.device != done.device:
            raise AkiError(f"slot_tick: contiguous GPU tensors [B] are expected - done uint8, done_at / cache_len / start_len / limit int32; "
                           f"got {t_.dtype} {tuple(t_.shape)}")
    if not 1 <= B <= SLOT_MAX_ROWS:
        raise AkiError(f"slot_tick: 1 <= B <= {SLOT_MAX_ROWS} rows are expected, got {B}")
    if stops is None:
        if tokens is not None:
            raise AkiError("slot_tick: tokens goes with stops")
        L.check(L.load().aki_slot_tick(_ptr(done), _ptr(done_at), _ptr(cache_len), _ptr(start_len), _ptr(limit), B, _stream()), "aki_slot_tick")
        return
    if not isinstance(stops, StopSets):
        raise AkiError("slot_tick: stops is an ops.StopSets")
    _stop_tokens("slot_tick", tokens, B, done.device)
    hit, pool = stops._args("slot_tick", B, done.device)
    L.check(L.load().aki_slot_tick_stops(_ptr(done), _ptr(done_at), _ptr(cache_len), _ptr(start_len), _ptr(limit), _ptr(tokens), tokens.shape[1],
                                         hit, *pool, B, _stream()), "aki_slot_tick_stops")


SKINNY_NORM_FUSED = True       # tools (decode_bench.py --norm-launch): False = the RMSNorm of 2-8 row decode GEMMs as a launch of its own


def decode_linear(x: torch.Tensor, w: torch.Tensor, rms_weight: torch.Tensor, eps: float, act: int = ACT_NONE,
                  bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(rmsnorm(x; rms_weight, eps) W^T + bias) [+ residual] for the few rows of a decode step: one weight-streaming
    launch when x is bf16 with <= 8 rows (one row: the dot-product GEMV; 2-8 rows: the skinny MFMA GEMM, the norm in its prologue),
    otherwise the norm kernel followed by linear()."""
    x2 = _rows2d(x)
    M, K = x2.shape
    n_tiles = ((w.shape[0] // 2 if act == ACT_SWIGLU else w.shape[0]) + 15) // 16
    # 2-8 rows: every workgroup normalises the rows for itself - the 2004 two-wave workgroups of an lm_head-wide output keep the norm launch
    if (x.dtype != torch.bfloat16 or M > 8 or K > (65536 if M == 1 else 8192) or K % 8 or x2.stride(0) % 8 or w.stride(0) % 8
            or (M > 1 and (n_tiles >= 1536 or K % 256 or not SKINNY_NORM_FUSED))):
        return linear(rmsnorm(x, rms_weight, eps), w, bias=bias, residual=residual, act=act)
    dev = _dev(x, w, rms_weight, bias, residual)
    N = w.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty((*x.shape[:-1], n_out), dtype=x.dtype, device=dev)
    o2 = out.view(-1, n_out)
    r2 = None if residual is None else _rows2d(residual)
    a = L.LinearArgs(_ptr(x2), _ptr(w), _ptr(bias), _ptr(r2), _ptr(o2), M, N, K, x2.stride(0), w.stride(0), o2.stride(0),
                     0 if r2 is None else r2.stride(0), 0, act, _dt(x))
    L.check(L.load().aki_decode_linear_fwd(C.byref(a), _ptr(rms_weight), float(eps), _stream()), "aki_decode_linear_fwd")
    return out


# ---- layer loops in one C call (csrc/stack.hip) -------------------------------------------------------------------------
_SCRATCH = {}


def _scratch(nbytes: int, dev) -> torch.Tensor:
    """Uninitialised scratch per (device, stream), 256-byte aligned: launches that use it are stream-ordered."""
    key = (torch.device(dev).index, torch.cuda.current_stream().cuda_stream)
    hit = _SCRATCH.get(key)
    if hit is None or hit.numel() < nbytes + 256:
        hit = _SCRATCH[key] = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=dev)
    return hit


def stack_enabled() -> bool:
    """The one-call layer loops hide the individual launches from the event tap (bench.py brackets single GEMMs): off while one is installed.
    Off under stream capture as well: their scratch buffer is cached across calls and must not come out of a graph's private pool."""
    return _TAP is None and not torch.cuda.is_current_stream_capturing()


def python_must_run_between(layers) -> bool:
    """True when something in Python has to happen inside one of `layers`: a forward (pre-)hook on the layer OR on any of its sub-modules
    (activation capture, adapter wrappers), or an instance-level `forward` override (gradient checkpointing installs one).  The one-call
    layer loops (csrc/stack.hip) never enter Python between layers, so they are only taken when this is False."""
    for ly in layers:
        for m in ly.modules():
            if m._forward_hooks or m._forward_pre_hooks or "forward" in m.__dict__:
                return True
    return False


def params_signature(tensors) -> tuple:
    """(address, in-place version) of every tensor: changes when a parameter is re-allocated (`.to`, `.data = ...`) or written in place
    through torch (`copy_`, an optimizer step).  It signs the OBJECTS it is given: a caller that wants load_state_dict(assign=True) or an
    attribute assignment noticed must pass the module's live parameters (and may add their id()s), or bump a version in its load hooks
    (Phi3Model does the latter, the SigLIP and Perceiver stacks the former).  Writes through raw pointers (this library's trainers) are announced by the
    weight epoch, which callers add themselves.  ~0.25 us per tensor: cheap enough to run before every stacked forward."""
    return tuple((t_.data_ptr(), t_._version) for t_ in tensors)


class LayerTable:
    """A host array of per-layer pointer structs for the stack calls, rebuilt only when a pointer changes."""

    def __init__(self, struct):
        self.struct, self.key, self.arr, self.keep = struct, None, None, None
        self.sig = None                 # the owner's cheap signature of everything the rows were prepared from (see params_signature)

    def get(self, rows):
        """rows: per layer a tuple of tensors / None in the struct's field order."""
        key = tuple(0 if t_ is None else t_.data_ptr() for r in rows for t_ in r)
        if key != self.key:
            n = len(self.struct._fields_)
            arr = (self.struct * len(rows))()
            for i, r in enumerate(rows):
                arr[i] = self.struct(*key[i * n:(i + 1) * n])
            self.key, self.arr, self.keep = key, arr, rows
        return self.arr


def decoder_stack(table_arr, n_layers: int, h: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mask: MaskTable, num_heads: int, head_dim: int,
                  inter: int, scale: float, eps: float, position_ids: Optional[torch.Tensor] = None, kv_capacity: int = 0,
                  dead_rows: int = DEAD_ROWS_UNIFORM):
    """All decoder layers of a bf16 inference forward in ONE call (aki_decoder_stack_fwd): h [B, L, d] raw residual stream -> (h_out, 1/rms of
    its rows).  `table_arr`: LayerTable of L.DecoderLayer (gain-folded w_qkv / w_gate_up, w_o, w_down, KV cache tensors or None)."""
    dev = _dev(h, cos, sin)
    B, Lq, d = h.shape
    if h.dtype != torch.bfloat16 or not h.is_contiguous():
        raise AkiError("decoder_stack: h is a contiguous bf16 [B, L, d] tensor")
    lib = L.load()
    cos = cos.to(torch.float32).reshape(-1, head_dim).contiguous()
    sin = sin.to(torch.float32).reshape(-1, head_dim).contiguous()
    pos = None if position_ids is None else position_ids.to(torch.int32).expand(B, Lq).contiguous()
    M = B * Lq
    out = torch.empty_like(h)
    rstd = torch.empty((M,), dtype=torch.float32, device=dev)
    keep = 1 if kv_capacity else 0
    need = int(lib.aki_decoder_stack_workspace_bytes(B, num_heads, Lq, head_dim, d, inter, keep))
    ws = _scratch(need, dev)
    off = (-ws.data_ptr()) % 256
    sws = _stats_ws(M, d, dev)
    sk = None
    if M <= 2048:
        for K_ in (num_heads * head_dim, inter):          # o_proj, down: one buffer (it only ever grows) serves both
            got = _splitk_ws(M, d, K_, dev)
            sk = sk if got is None else got
    a = L.DecoderStackArgs(table_arr, n_layers, _ptr(h), _ptr(out), _ptr(rstd), _ptr(cos), _ptr(sin), _ptr(pos), cos.shape[0], _ptr(mask.rects),
                           _ptr(mask.col_valid_bits), _ptr(mask.seq_lens), mask.max_rects, B, num_heads, Lq, head_dim, d, inter,
                           int(kv_capacity), float(scale), float(eps), dead_rows, ws.data_ptr() + off, ws.numel() - off, sws.data_ptr(), sws.numel(),
                           None if sk is None else sk.data_ptr(), 0 if sk is None else sk.numel())
    L.check(lib.aki_decoder_stack_fwd(C.byref(a), _stream()), "aki_decoder_stack_fwd")
    return out, RowStats(rstd)


def siglip_stack(table_arr, n_layers: int, h: torch.Tensor, fc1_out: torch.Tensor, heads: int, inter: int, act: int, eps: float,
                 scale: float) -> torch.Tensor:
    """All SigLIP encoder layers of a bf16 inference forward in ONE call (aki_siglip_stack_fwd): h [N, L, E] -> h_out.  `fc1_out` [N*L, Ip]:
    the K-padded fc1 output buffer whose pad columns are zero."""
    dev = _dev(h, fc1_out)
    N, Lq, E = h.shape
    if h.dtype != torch.bfloat16 or not h.is_contiguous() or not fc1_out.is_contiguous():
        raise AkiError("siglip_stack: contiguous bf16 tensors")
    lib = L.load()
    M, Ip = N * Lq, fc1_out.shape[-1]
    out = torch.empty_like(h)
    need = int(lib.aki_siglip_stack_workspace_bytes(N, Lq, E, heads))
    ws = _scratch(need, dev)
    off = (-ws.data_ptr()) % 256
    sws = _stats_ws(M, E, dev)
    sk = None
    if M <= 2048:
        for K_ in (E, Ip):                                # out-proj, fc2
            got = _splitk_ws(M, E, K_, dev)
            sk = sk if got is None else got
    a = L.SiglipStackArgs(table_arr, n_layers, _ptr(h), _ptr(out), _ptr(fc1_out), N, Lq, E, heads, inter, Ip, act, float(eps), float(scale), ws.data_ptr() + off,
                          ws.numel() - off, sws.data_ptr(), sws.numel(), None if sk is None else sk.data_ptr(), 0 if sk is None else sk.numel())
    L.check(lib.aki_siglip_stack_fwd(C.byref(a), _stream()), "aki_siglip_stack_fwd")
    return out


def perceiver_stack(table_arr, n_layers: int, x: torch.Tensor, latents: torch.Tensor, norm_w, norm_b, proj_w, proj_b, heads: int, dim_head: int, d_ff: int,
                    scale: float, eps: float) -> torch.Tensor:
    """The Perceiver connector for ONE (sample, image) pair in one call (aki_perceiver_stack_fwd): x [n1, D], latents [n2, D] -> [n2, D_out]."""
    dev = _dev(x, latents, norm_w, norm_b, proj_w, proj_b)
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or not latents.is_contiguous() or x.dim() != 2 or latents.dim() != 2:
        raise AkiError("perceiver_stack: contiguous bf16 [n, D] tensors")
    lib = L.load()
    n1, D = x.shape
    n2 = latents.shape[0]
    D_out = D if proj_w is None else proj_w.shape[0]
    out = torch.empty((n2, D_out), dtype=x.dtype, device=dev)
    ws = _scratch(int(lib.aki_perceiver_stack_workspace_bytes(n1, n2, D, heads, dim_head, d_ff)), dev)
    off = (-ws.data_ptr()) % 256
    a = L.PerceiverStackArgs(table_arr, n_layers, _ptr(x), _ptr(latents), _ptr(norm_w), _ptr(norm_b), _ptr(proj_w), _ptr(proj_b), _ptr(out), n1, n2, D, heads,
                             dim_head, d_ff, D_out, float(scale), float(eps), ws.data_ptr() + off, ws.numel() - off)
    L.check(lib.aki_perceiver_stack_fwd(C.byref(a), _stream()), "aki_perceiver_stack_fwd")
    return out


# ---- fp8 (e4m3) projections: BASELINE configs[4] -------------------------------------------------------------------
def quant_rows_fp8(x: torch.Tensor, rms_weight: Optional[torch.Tensor] = None, eps: float = 0.0):
    """bf16 rows -> (e4m3 bytes [rows, cols] as uint8, f32 scale per row).  With rms_weight the Phi-3 RMSNorm is applied on
    the way (same rounding points as ops.rmsnorm), i.e. this is `quantize(norm(x))` in one HBM pass."""
    dev = _dev(x, rms_weight)
    if x.dtype != torch.bfloat16:
        raise AkiError("quant_rows_fp8 takes bf16 input")
    x2 = _rows2d(x)
    rows, cols = x2.shape
    q = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    s = torch.empty((rows,), dtype=torch.float32, device=dev)
    L.check(L.load().aki_quant_rows_fp8(_ptr(x2), _ptr(rms_weight), float(eps), _ptr(q), _ptr(s), rows, cols, x2.stride(0),
                                        q.stride(0), _stream()), "aki_quant_rows_fp8")
    return q, s


def linear_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, act: int = ACT_NONE, out_shape=None) -> torch.Tensor:
    """y (bf16) = act((xq * xs) (wq * ws)^T + bias) [+ residual] on the fp8 MFMA path; xq [M,K] / wq [N,K] uint8 (e4m3)."""
    dev = _dev(xq, xs, wq, ws, bias, residual)
    M, K = xq.shape
    N = wq.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty((M, n_out), dtype=torch.bfloat16, device=dev)
    r2 = None if residual is None else _rows2d(residual)
    a = L.LinearArgs(_ptr(xq), _ptr(wq), _ptr(bias), _ptr(r2), _ptr(out), M, N, K, xq.stride(0), wq.stride(0), out.stride(0),
                     0 if r2 is None else r2.stride(0), 0, act, L.AKI_DT_FP8_E4M3, _ptr(xs), _ptr(ws))
    end = _TAP.begin(("linear_fp8", M, N, K, act)) if (_TAP is not None and _TAP.want(("linear_fp8", M, N, K, act))) else None
    L.check(L.load().aki_linear_fwd(C.byref(a), _stream()), "aki_linear_fwd[fp8]")
    if end is not None:
        end.record()
    return out if out_shape is None else out.view(*out_shape)


def mma_attn_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                 table: "MaskTable", B: int, num_heads: int, scale: Optional[float] = None,
                 position_ids: Optional[torch.Tensor] = None, dead_rows: int = DEAD_ROWS_UNIFORM) -> torch.Tensor:
    """Fused MMA op with fp8 QKV projection: xq [B*L, d] e4m3 + scales -> o [B, L, H*Dh] bf16 (RoPE, attention core in bf16)."""
    dev = _dev(xq, xs, wq, ws, cos, sin)
    lib = L.load()
    M, d = xq.shape
    Lq = M // B
    Dh = wq.shape[0] // (3 * num_heads)
    scale = Dh ** -0.5 if scale is None else scale
    o = torch.empty((B, Lq, num_heads * Dh), dtype=torch.bfloat16, device=dev)
    ws_buf = _ws(lib.aki_mma_attn_workspace_bytes(B, num_heads, Lq, Dh, L.AKI_DT_BF16), dev)
    pos = None if position_ids is None else position_ids.to(torch.int32).contiguous()
    a = L.MmaAttnArgs(_ptr(xq), _ptr(wq), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(o), None, _ptr(table.rects),
                      _ptr(table.col_valid_bits), _ptr(table.seq_lens), table.max_rects, B, num_heads, Lq, Dh, d, xq.stride(0),
                      wq.stride(0), cos.shape[0], float(scale), L.AKI_DT_FP8_E4M3, dead_rows, 0, _ptr(xs), _ptr(ws))
    end = _TAP.begin(("mma_attn_fp8", B, num_heads, Lq, Dh)) if (_TAP is not None and _TAP.want(("mma_attn_fp8",))) else None
    L.check(lib.aki_mma_attn_fwd(C.byref(a), _ptr(ws_buf), ws_buf.numel(), _stream()), "aki_mma_attn_fwd[fp8]")
    if end is not None:
        end.record()
    return o


def qkv_rope_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int,
                 num_heads: int, position_ids: Optional[torch.Tensor] = None, k_out: Optional[torch.Tensor] = None,
                 v_out: Optional[torch.Tensor] = None):
    """fp8 QKV projection + RoPE -> bf16 q [B,H,L,Dh], k, v (optionally straight into a KV cache, like qkv_rope)."""
    dev = _dev(xq, xs, wq, ws, cos, sin, k_out, v_out)
    M, d = xq.shape
    Lq = M // B
    Dh = wq.shape[0] // (3 * num_heads)
    cos = cos.to(torch.float32).reshape(-1, Dh).contiguous()
    sin = sin.to(torch.float32).reshape(-1, Dh).contiguous()
    pos = None if position_ids is None else position_ids.to(torch.int32).expand(B, Lq).contiguous()
    q = torch.empty((B, num_heads, Lq, Dh), dtype=torch.bfloat16, device=dev)
    if k_out is None:
        k_out = torch.empty((B, num_heads, Lq, Dh), dtype=torch.bfloat16, device=dev)
        v_out = torch.empty((B, num_heads, Lq, Dh), dtype=torch.bfloat16, device=dev)
    cap = k_out.shape[2]
    if not (k_out.is_contiguous() and v_out.is_contiguous()) or v_out.shape != k_out.shape or cap < Lq:
        raise AkiError("qkv_rope_fp8: bad KV output buffers")
    a = L.MmaAttnArgs(_ptr(xq), _ptr(wq), _ptr(cos), _ptr(sin), _ptr(pos), None, None, None, None, None, 0, B, num_heads, Lq, Dh, d,
                      xq.stride(0), wq.stride(0), cos.shape[0], float(Dh ** -0.5), L.AKI_DT_FP8_E4M3, 0, 0 if cap == Lq else cap,
                      _ptr(xs), _ptr(ws))
    wsb = _ws(256, dev)
    L.check(L.load().aki_qkv_rope_fwd(C.byref(a), _ptr(q), _ptr(k_out), _ptr(v_out), _ptr(wsb), wsb.numel(), _stream()),
            "aki_qkv_rope_fwd[fp8]")
    return q, k_out, v_out


def linear_w8(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, act: int = ACT_NONE, rms_weight: Optional[torch.Tensor] = None,
              eps: float = 0.0) -> torch.Tensor:
    """Weight-only fp8 (decode in the fp8 configuration): x bf16 [M <= 16, K], wq e4m3 [N, K] with one scale per row; optional fused RMSNorm of
    x (rms_weight).  One row: the dot-product GEMV; 2-16 rows: the skinny MFMA GEMM on e4m3 weights (half the bytes of the bf16 one).
    y bf16 [M, N_out]."""
    dev = _dev(x, wq, ws, bias, residual, rms_weight)
    x2 = _rows2d(x)
    M, K = x2.shape
    if M > 16 or x.dtype != torch.bfloat16:
        raise AkiError("linear_w8 serves up to 16 bf16 rows")
    N = wq.shape[0]
    if M > 1 and rms_weight is not None and (M > 8 or K > 8192 or K % 512 or ((N // 2 if act == ACT_SWIGLU else N) + 15) // 16 >= 1536):
        x2 = _rows2d(rmsnorm(x, rms_weight, eps))      # shapes whose rows the GEMM does not normalise itself (wide outputs, more than eight rows)
        rms_weight = None
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty((*x.shape[:-1], n_out), dtype=torch.bfloat16, device=dev)
    o2 = out.view(-1, n_out)
    r2 = None if residual is None else _rows2d(residual)
    a = L.LinearArgs(_ptr(x2), _ptr(wq), _ptr(bias), _ptr(r2), _ptr(o2), M, N, K, x2.stride(0), wq.stride(0), o2.stride(0),
                     0 if r2 is None else r2.stride(0), 0, act, L.AKI_DT_W8A16, None, _ptr(ws))
    lib = L.load()
    if rms_weight is not None:
        L.check(lib.aki_decode_linear_fwd(C.byref(a), _ptr(rms_weight), float(eps), _stream()), "aki_decode_linear_fwd[w8]")
    else:
        L.check(lib.aki_linear_fwd(C.byref(a), _stream()), "aki_linear_fwd[w8]")
    return out


# ---- MXFP4 weight-only decode (csrc/mxfp4.hip): e2m1 nibbles + one e8m0 scale byte per block of 32 k ---------------------------
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quant_mxfp4(w: torch.Tensor):
    """bf16 weight [N, K] (K % 32 == 0, rows 16-byte aligned) -> (wq uint8 [N, K/2], ws uint8 [N, K/32]): OCP MXFP4, the format of
    aki_quant_mxfp4 (include/aki_mi355x.h).  The values must be finite; the caller checks (Phi3ForCausalLM.enable_mxfp4 does)."""
    dev = _dev(w)
    if w.dtype != torch.bfloat16 or w.dim() != 2 or w.stride(1) != 1 or w.shape[1] % 32:
        raise AkiError("quant_mxfp4 takes a bf16 matrix [N, K] with contiguous rows and K a multiple of 32")
    N, K = w.shape
    wq = torch.empty((N, K // 2), dtype=torch.uint8, device=dev)
    ws = torch.empty((N, K // 32), dtype=torch.uint8, device=dev)
    L.check(L.load().aki_quant_mxfp4(_ptr(w), N, K, w.stride(0), _ptr(wq), _ptr(ws), _stream()), "aki_quant_mxfp4")
    return wq, ws


def dequant_mxfp4(wq: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """The bf16 matrix [N, K] that (wq, ws) stand for - exact (e2m1 x 2^e has two significant bits).  A torch expression for tests, tools and
    twin models; the decode kernels never materialise it."""
    N, K2 = wq.shape
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=wq.device)
    nib = torch.stack((wq & 0xF, wq >> 4), dim=-1).reshape(N, K2 * 2).long()
    scale = torch.ldexp(torch.ones((), dtype=torch.float32, device=wq.device), ws.to(torch.int32) - 127)
    return (lut[nib].view(N, -1, 32) * scale.unsqueeze(-1)).reshape(N, K2 * 2).to(torch.bfloat16)


def linear_w4(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, act: int = ACT_NONE, rms_weight: Optional[torch.Tensor] = None,
              eps: float = 0.0, res_row_mod: int = 0) -> torch.Tensor:
    """Weight-only MXFP4 (opt-in decode format): x bf16 [M <= 16, K], wq [N, K/2] nibbles with ws [N, K/32] e8m0 block scales (quant_mxfp4);
    optional fused RMSNorm of x (rms_weight).  One row: the dot-product GEMV; 2-16 rows: the skinny MFMA GEMM on e2m1 weights.  y bf16 [M, N_out].
    2-16 rows of a shape outside the skinny GEMM's gates are served by the GEMV one row at a time; anything else the kernels do not take
    raises AkiError - there is no other route for these weights."""
    dev = _dev(x, wq, ws, bias, residual, rms_weight)
    x2 = _rows2d(x)
    M, K = x2.shape
    if M > 16 or x.dtype != torch.bfloat16 or wq.dtype != torch.uint8 or ws.dtype != torch.uint8:
        raise AkiError("linear_w4 serves up to 16 bf16 rows on uint8 nibbles and scale bytes")
    N = wq.shape[0]
    if wq.shape[1] * 2 != K or tuple(ws.shape) != (N, K // 32) or not ws.is_contiguous() or wq.stride(1) != 1:
        raise AkiError("linear_w4: wq [N, K/2] and a dense ws [N, K/32] for x [M, K]")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if M > 1 and rms_weight is not None and (M > 8 or K > 8192 or K % 512 or (n_out + 15) // 16 >= 1536):
        x2 = _rows2d(rmsnorm(x, rms_weight, eps))      # shapes whose rows the GEMM does not normalise itself (wide outputs, more than eight rows)
        rms_weight = None
    out = torch.empty((*x.shape[:-1], n_out), dtype=torch.bfloat16, device=dev)
    o2 = out.view(-1, n_out)
    r2 = None if residual is None else _rows2d(residual)
    a = L.LinearArgs(_ptr(x2), _ptr(wq), _ptr(bias), _ptr(r2), _ptr(o2), M, N, K, x2.stride(0), wq.stride(0), o2.stride(0),
                     0 if r2 is None else r2.stride(0), int(res_row_mod), act, L.AKI_DT_BF16)
    lib = L.load()
    rc = lib.aki_linear_w4_fwd(C.byref(a), _ptr(ws), _ptr(rms_weight), float(eps), _stream())
    if rc == -2 and M > 1:
        # AKI_ERR_UNSUPPORTED: a shape outside the skinny GEMM's gates (K no multiple of 256, N_out no multiple of 4): the one-row GEMV, row by row
        for m in range(M):
            rr = None if r2 is None else r2[m % res_row_mod if res_row_mod > 0 else m]
            a = L.LinearArgs(_ptr(x2[m]), _ptr(wq), _ptr(bias), _ptr(rr), _ptr(o2[m]), 1, N, K, x2.stride(0), wq.stride(0), o2.stride(0),
                             n_out, 0, act, L.AKI_DT_BF16)
            L.check(lib.aki_linear_w4_fwd(C.byref(a), _ptr(ws), _ptr(rms_weight), float(eps), _stream()), "aki_linear_w4_fwd[row]")
        return out
    L.check(rc, "aki_linear_w4_fwd")
    return out


def pad_k(w: torch.Tensor, mult: int = 64) -> torch.Tensor:
    """Zero-pad the K (last) dimension of a weight to a multiple of `mult` (one-time host-side prep)."""
    K = w.shape[-1]
    Kp = (K + mult - 1) // mult * mult
    if Kp == K:
        return w.contiguous()
    out = torch.zeros(*w.shape[:-1], Kp, dtype=w.dtype, device=w.device)
    out[..., :K] = w
    return out


def patch_embed(pixels: torch.Tensor, w_padded: torch.Tensor, bias: Optional[torch.Tensor], pos: Optional[torch.Tensor],
                patch: int) -> torch.Tensor:
    """pixels [N,3,S,S]; w_padded [E,Kp] = pad_k(conv_weight.reshape(E,-1)); pos [G*G,E] -> [N,G*G,E]."""
    dev = _dev(pixels, w_padded, bias, pos)
    N, _, S, _ = pixels.shape
    E, Kp = w_padded.shape
    G = S // patch
    pixels = pixels.contiguous()
    out = torch.empty((N, G * G, E), dtype=pixels.dtype, device=dev)
    lib = L.load()
    ws = _ws(lib.aki_patch_embed_workspace_bytes(N, S, patch, _dt(pixels)), dev)
    L.check(lib.aki_patch_embed_fwd(_ptr(pixels), _ptr(w_padded), _ptr(bias), _ptr(pos), _ptr(out), N, S, patch, E, Kp,
                                    _dt(pixels), _ptr(ws), ws.numel(), _stream()), "aki_patch_embed_fwd")
    return out


def connector_mlp(x: torch.Tensor, ln_w, ln_b, w1, w2, eps: float = 1e-5) -> torch.Tensor:
    """out = x + W2 gelu(W1 LN(x)) - the Perceiver FeedForward block with its residual (src/helpers.py:32-39,194)."""
    dev = _dev(x, ln_w, ln_b, w1, w2)
    x2 = _rows2d(x).contiguous()
    rows, d = x2.shape
    d_inner = w1.shape[0]
    out = torch.empty_like(x2)
    lib = L.load()
    ws = _ws(lib.aki_connector_mlp_workspace_bytes(rows, d, d_inner, _dt(x)), dev)
    L.check(lib.aki_connector_mlp_fwd(_ptr(x2), _ptr(ln_w), _ptr(ln_b), _ptr(w1), _ptr(w2), _ptr(out), rows, d, d_inner,
                                      float(eps), _dt(x), _ptr(ws), ws.numel(), _stream()), "aki_connector_mlp_fwd")
    return out.reshape(x.shape)


def connector_proj(x: torch.Tensor, ln_w, ln_b, w, b, eps: float = 1e-5) -> torch.Tensor:
    """out = Wp LN(x) + bp (src/helpers.py:196-197)."""
    dev = _dev(x, ln_w, ln_b, w, b)
    x2 = _rows2d(x).contiguous()
    rows, d = x2.shape
    d_out = w.shape[0]
    out = torch.empty((rows, d_out), dtype=x.dtype, device=dev)
    lib = L.load()
    ws = _ws(rows * d * x.element_size() + 256, dev)
    L.check(lib.aki_connector_proj_fwd(_ptr(x2), _ptr(ln_w), _ptr(ln_b), _ptr(w), _ptr(b), _ptr(out), rows, d, d_out,
                                       float(eps), _dt(x), _ptr(ws), ws.numel(), _stream()), "aki_connector_proj_fwd")
    return out.reshape(*x.shape[:-1], d_out)


@dataclass
class SplicePlan:
    """The per-sample splice plan (image count, text span, output length ...) on its way to the host: started early by
    `splice_plan_async`, collected by `splice`."""
    plan: torch.Tensor           # int32 [B, AKI_PLAN_STRIDE] on the device
    host: torch.Tensor           # the same, pinned host memory, valid once `ready` has passed
    ready: "torch.cuda.Event"
    lang_x: torch.Tensor         # the int64 ids the plan was made from
    key: tuple


_PLAN_PINNED = {}


def splice_plan_async(lang_x: torch.Tensor, media_token_id: int, assistant_token_id: int, n_vis_tokens: int) -> SplicePlan:
    """The plan depends on the token ids only, while the splice itself needs the vision tokens - the last thing the vision
    side produces.  Sizing the outputs needs the plan on the HOST: called before the vision tower is issued, the plan kernel and
    its 100-byte copy run ahead of ~8 ms of queued GPU work, and `splice` later waits on an event that has long passed instead
    of draining the stream (0.35 ms of idle GPU per forward at the benchmark shape)."""
    dev = _dev(lang_x)
    B, T = lang_x.shape
    ids = lang_x.to(torch.int64).contiguous()
    plan = torch.empty((B, L.AKI_PLAN_STRIDE), dtype=torch.int32, device=dev)
    L.check(L.load().aki_splice_plan(_ptr(ids), B, T, media_token_id, assistant_token_id, n_vis_tokens, _ptr(plan), _stream()),
            "aki_splice_plan")
    ring = _PLAN_PINNED.setdefault((B, torch.device(dev).index), [[], 0])
    if len(ring[0]) < 4:
        ring[0].append(torch.empty((B, L.AKI_PLAN_STRIDE), dtype=torch.int32).pin_memory())
    host = ring[0][ring[1] % len(ring[0])]
    ring[1] += 1
    host.copy_(plan, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return SplicePlan(plan, host, ev, ids, (lang_x.data_ptr(), lang_x._version, tuple(lang_x.shape), media_token_id, assistant_token_id, n_vis_tokens))


def splice(lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor], labels: Optional[torch.Tensor],
           embed_weight: torch.Tensor, embed_additional: Optional[torch.Tensor], max_original_id: int,
           vision_tokens: torch.Tensor, media_token_id: int, pad_token_id: int, assistant_token_id: int = 32001,
           padding_side: str = "right", max_rects: int = 1, plan: Optional[SplicePlan] = None):
    """Language-stream fusion (src/vlm.py:445-603).  Returns (inputs_embeds, labels_out, MaskTable, plan_host).
    One small device->host copy (the per-sample plan) is needed to size the outputs; `plan` = the result of an earlier
    `splice_plan_async` on the same ids makes that copy free."""
    dev = _dev(lang_x, attention_mask, labels, embed_weight, embed_additional, vision_tokens)
    lib = L.load()
    B, T = lang_x.shape
    if plan is not None and plan.key != (lang_x.data_ptr(), lang_x._version, tuple(lang_x.shape), media_token_id, assistant_token_id,
                                         vision_tokens.shape[2]):
        plan = None                     # made from other ids: plan again
    lang_x = plan.lang_x if plan is not None else lang_x.to(torch.int64).contiguous()
    if attention_mask is not None:
        attention_mask = attention_mask.to(torch.int64).contiguous()
    if labels is not None:
        labels = labels.to(torch.int64).contiguous()
    vision_tokens = vision_tokens.to(embed_weight.dtype).contiguous()
    _, T_img, Nv, d = vision_tokens.shape
    if plan is not None:
        plan.ready.synchronize()
        plan, plan_h = plan.plan, plan.host.clone()
    else:
        plan = torch.empty((B, L.AKI_PLAN_STRIDE), dtype=torch.int32, device=dev)
        L.check(lib.aki_splice_plan(_ptr(lang_x), B, T, media_token_id, assistant_token_id, Nv, _ptr(plan), _stream()),
                "aki_splice_plan")
        plan_h = plan.cpu()
    n_img = plan_h[:, 0]
    if int(n_img.max()) > T_img:
        raise AkiError(f"a sample has {int(n_img.max())} <image> placeholders but vision_x carries only {T_img} images")
    if int(n_img.max()) > max_rects:
        raise AkiError(f"{int(n_img.max())} images in one sample but max_rects={max_rects}")
    L_out = int(plan_h[:, 2].max())
    dt = embed_weight.dtype
    embeds = torch.empty((B, L_out, d), dtype=dt, device=dev)
    labels_out = torch.empty((B, L_out), dtype=torch.int64, device=dev) if labels is not None else None
    mask_1d = torch.empty((B, L_out), dtype=torch.int64, device=dev)
    rects = torch.empty((B, max_rects, 4), dtype=torch.int32, device=dev)
    nw = (L_out + 63) // 64
    bits = torch.empty((B, nw), dtype=torch.int64, device=dev)
    seq_lens = torch.empty((B,), dtype=torch.int32, device=dev)
    a = L.SpliceArgs(_ptr(lang_x), _ptr(attention_mask), _ptr(labels), _ptr(embed_weight), _ptr(embed_additional),
                     _ptr(vision_tokens), _ptr(plan), _ptr(embeds), _ptr(labels_out), _ptr(mask_1d), _ptr(rects),
                     _ptr(bits), _ptr(seq_lens), max_original_id, media_token_id, pad_token_id, B, T, T_img, Nv, d, L_out,
                     max_rects, 1 if padding_side == "left" else 0, _dt(embeds))
    L.check(lib.aki_splice_fwd(C.byref(a), _stream()), "aki_splice_fwd")
    return embeds, labels_out, MaskTable(rects, bits, seq_lens, L_out, mask_1d), plan_h


def mask_to_table(mask: torch.Tensor, max_rects: int = L.AKI_MAX_RECTS, verify: bool = True) -> MaskTable:
    """The reference's LM hand-off type - `attention_mask` (B,1,L,L) 0/1 as returned by `_prepare_inputs_for_forward`
    (src/vlm.py:589-603) - converted on the device into a MaskTable.  The kernels extract a candidate (rectangles from the
    right-of-diagonal row intervals, valid bits from the column-wise OR, seq_lens from the last non-empty row); with
    `verify` the candidate is materialised again and compared with the input bit for bit, so a mask outside the family
    {causal + row-interval rectangles + invalid columns} raises instead of being approximated (one host sync)."""
    dev = _dev(mask)
    if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] != mask.shape[3]:
        raise AkiError(f"mask_to_table: expected (B,1,L,L), got {tuple(mask.shape)}")
    B, _, Lq, _ = mask.shape
    m = mask if mask.dtype == torch.int64 else (mask != 0).to(torch.int64)
    m = m.contiguous()
    lib = L.load()
    rects = torch.empty((B, max_rects, 4), dtype=torch.int32, device=dev)
    bits = torch.empty((B, (Lq + 63) // 64), dtype=torch.int64, device=dev)
    seq_lens = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = _ws(lib.aki_mma_mask_to_table_workspace_bytes(B, Lq), dev)
    L.check(lib.aki_mma_mask_to_table(_ptr(m), B, Lq, max_rects, _ptr(rects), _ptr(bits), _ptr(seq_lens), _ptr(status),
                                      _ptr(ws), ws.numel(), _stream()), "aki_mma_mask_to_table")
    table = MaskTable(rects, bits, seq_lens, Lq)
    if verify:
        st = status.cpu()
        if int(st.max()) != 0:
            b = int(st.argmax())
            raise AkiError(f"dense attention mask: sample {b} needs {int(st[b])} row groups, more than the {max_rects} rectangles "
                           "the MMA kernels take; pass an ops.MaskTable or a causal/padding mask")
        if not torch.equal(mask_dense(table, B), (m != 0).to(torch.int64)):
            raise AkiError("dense attention mask is not of the modality-mutual family (causal triangle + per-row column "
                           "intervals + invalid columns); the MI355X path refuses it rather than approximating it")
    return table


def mask_dense(table: MaskTable, B: int) -> torch.Tensor:
    """The reference's (B,1,L,L) int64 0/1 mask, materialised from the table (bit-exact)."""
    dev = table.rects.device if table.rects is not None else table.col_valid_bits.device
    out = torch.empty((B, 1, table.L, table.L), dtype=torch.int64, device=dev)
    L.check(L.load().aki_mma_mask_dense(_ptr(table.rects), table.max_rects, _ptr(table.col_valid_bits), _ptr(table.seq_lens),
                                        B, table.L, _ptr(out), _stream()), "aki_mma_mask_dense")
    return out

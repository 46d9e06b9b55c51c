"""Attention backward against a float64 reference where every query-key pair counts: every case of tests/attn_bwd_cases.py, in both
input families, through ops.mma_attn_core / ops.attention (o, lse) and train_ops.attn_bwd (attn_delta_kernel, attn_bwd_dkv_kernel,
attn_bwd_dq_kernel), with the 32-row forward core, with the 64-row forward core forced at every length, and once through the
product library at its own boundary L = 1792.  The bar is componentwise and derived in the docstring of attn_bwd_cases.py:
KAPPA 2^-9 M + 2^-8 |ref|, KAPPA = 2.5 (4.5 behind the 64-row forward); tests/test_attn_bwd_cases_cpu.py shows which faults cannot
stay inside it.  The largest err / tol per kernel goes to parity_errors.json through record_parity.

All indices stay inside the allocations: the poisoned guard bands lie outside what the ABI may touch, and the calls that must be
refused are refused on the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_bwd_cases as A
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 4096                      # bf16 elements of poison on either side of an output


def ibits(x: torch.Tensor) -> torch.Tensor:
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


class Job:
    """One case x family: inputs on the device, the mask table, and the float64 reference (computed once per module)."""

    def __init__(self, case, family):
        from aki_amd import ops
        self.case, self.family = case, family
        self.inp = inp = A.make_inputs(case, family)
        self.S = A.reference(inp)
        self.q, self.k, self.v, self.d_o = (t.to(DEV) for t in (inp.q, inp.k, inp.v, inp.d_o))
        self.what = f"{case.id} [{family}]"
        self.table = None
        if case.masked:
            rects = bits = seq = None
            if case.rects is not None:
                ra = np.zeros((case.B, max(len(rs) for rs in case.rects), 4), dtype=np.int32)       # unused entries are all-zero
                for b, rs in enumerate(case.rects):
                    ra[b, :len(rs)] = rs
                rects = torch.from_numpy(ra).to(DEV)
            if case.holes is not None:
                nw = (case.Lk + 63) // 64
                pad = np.zeros((case.B, nw * 64), dtype=bool)
                pad[:, :case.Lk] = case.mask_1d()
                bits = torch.from_numpy(np.packbits(pad.reshape(case.B, nw, 64), axis=-1, bitorder="little").view(np.uint64).reshape(
                    case.B, nw).view(np.int64).copy()).to(DEV)
            if case.seq_lens is not None:
                seq = torch.tensor(list(case.seq_lens), dtype=torch.int32, device=DEV)
            self.table = ops.MaskTable(rects, bits, seq, case.Lq)

    def plain_views(self):
        """q / k / v as ops.attention takes them: [B, L, H, Dh] views (channel stride 1) of the head-major tensors."""
        return tuple(t.permute(0, 2, 1, 3) for t in (self.q, self.k, self.v))

    def forward(self, core="32"):
        from aki_amd import ops, _lib
        c = self.case
        if not c.masked:
            return ops.attention(*self.plain_views(), c.scale, return_lse=True)
        if core == "product":
            return ops.mma_attn_core(self.q, self.k, self.v, self.table, c.scale, return_lse=True)
        with _lib.use_lab_attn(9 if core == "64" else 1):
            o, lse = ops.mma_attn_core(self.q, self.k, self.v, self.table, c.scale, return_lse=True)
            torch.cuda.synchronize()
        return o, lse

    def backward(self, o, lse):
        from aki_amd import train_ops as T
        return T.attn_bwd(self.q, self.k, self.v, o, self.d_o, lse, self.table, self.case.scale)


_JOBS = {}


def job_of(case, family):
    if (case.id, family) not in _JOBS:
        _JOBS[(case.id, family)] = Job(case, family)
    return _JOBS[(case.id, family)]


@pytest.fixture(scope="module", autouse=True)
def _drop_jobs():
    yield
    _JOBS.clear()
    torch.cuda.empty_cache()


ALL = [(c, f) for c in A.CASES for f in A.FAMILIES]
MASKED = [(c, f) for c, f in ALL if c.masked]
_id = lambda p: f"{p[0].id}-{p[1]}"


def compare(job, core, o, lse, dq, dk, dv):
    """Every output against the reference under the derived bar; exact zeros where nothing is seen.  The worst err / tol per kernel is
    printed and recorded before anything is asserted."""
    from conftest import record_parity
    c = job.case
    kap = "64" if core in ("64", "product") else "32"
    torch.cuda.synchronize()
    o = o.float().cpu().numpy().astype(np.float64).reshape(c.B, c.Lq, c.H, c.Dh).transpose(0, 2, 1, 3)
    lse, dq, dk, dv = (t.float().cpu().numpy().astype(np.float64) for t in (lse, dq, dk, dv))
    worst, where, zeros_ok = {}, {}, True
    for b, s in enumerate(job.S):
        got = {"o": o[b][:, s.live], "dq": dq[b], "dk": dk[b], "dv": dv[b]}
        for name, g in got.items():
            ref, tol = getattr(s, name), s.tol(name, kap)
            if name == "o":
                ref, tol = ref[:, s.live], tol[:, s.live]
            err = np.abs(g - ref)
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.where(err > 0, err / np.where(tol > 0, tol, 1e-300), 0.0)
            r = np.where(np.isfinite(err), r, np.inf)
            m = float(r.max()) if r.size else 0.0
            if m >= worst.get(name, -1.0):
                worst[name] = m
                where[name] = (b,) + tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape)) if r.size else (b,)
        el = np.abs(lse[b][:, s.live] - s.lse[:, s.live]) / s.lse_tol(kap)[:, s.live]
        el = np.where(np.isfinite(el), el, np.inf)
        worst["lse"] = max(worst.get("lse", 0.0), float(el.max()) if el.size else 0.0)
        unseen = ~s.vis.any(0)
        zeros_ok = zeros_ok and bool((dq[b][:, ~s.live] == 0).all() and (dk[b][:, unseen] == 0).all() and (dv[b][:, unseen] == 0).all())
    tag = f"{job.what}, {core if c.masked else 'plain'} forward"
    print(f"{tag}: worst err/tol " + ", ".join(f"{k} {v:.3f} at {where.get(k, '')}" for k, v in worst.items()))
    for kernel, names in (("forward o / lse", ("o", "lse")), ("attn_bwd_dq dq", ("dq",)), ("attn_bwd_dkv dk / dv", ("dk", "dv"))):
        w = max(worst[n_] for n_ in names)
        record_parity(f"attention backward, {kernel}: {tag}", BF, w, w, 1.0, f"err/tol <= 1 (KAPPA {A.KAPPA[kap]} 2^-9 M + 2^-8 |ref|)")
    assert zeros_ok, f"{tag}: a gradient of a row that sees nothing, or of a key that nothing sees, is not exactly zero"
    bad = {k: (v, where.get(k)) for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{tag}: outside the derived bar (err/tol, sample and index): {bad}"


def run(job, core):
    o, lse = job.forward(core)
    dq, dk, dv = job.backward(o, lse)
    dq2, dk2, dv2 = job.backward(o, lse)
    torch.cuda.synchronize()
    for a, b_, name in ((dq, dq2, "dq"), (dk, dk2, "dk"), (dv, dv2, "dv")):
        assert torch.equal(ibits(a), ibits(b_)), f"{job.what}: two launches differ in {name}"
    compare(job, core, o, lse, dq, dk, dv)


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_every_case_against_float64(p):
    """The 32-row forward core (masked) or ops.attention (plain), then attn_bwd, as MmaAttnCoreFn / PlainAttnFn do; two launches of the
    backward are bit-equal."""
    run(job_of(*p), "32")


@pytest.mark.parametrize("p", MASKED, ids=_id)
def test_64_row_forward_feeds_the_backward(p):
    """The long-context training route at small shapes: o and lse of the 64-row core (row sums over bf16-rounded p), forced at every
    length through the lab library, into the product library's backward."""
    run(job_of(*p), "64")


@pytest.mark.parametrize("family", A.FAMILIES)
def test_product_library_route_at_its_boundary(family):
    """L = 1792, where the product rule itself hands the forward to the 64-row core; no lab switch."""
    job = Job(A.PRODUCT_CASE, family)
    run(job, "product")


def test_autograd_wrappers_return_what_the_direct_calls_return():
    from aki_amd import train_ops as T
    job = job_of(A.CASE_BY_ID["L129-b2-h1-rect-one-past"], "sentinel")
    c = job.case
    o, lse = job.forward("product")
    want = job.backward(o, lse)
    qg, kg, vg = (t.clone().requires_grad_() for t in (job.q, job.k, job.v))
    og = T.MmaAttnCoreFn.apply(qg, kg, vg, job.table, c.scale)
    og.backward(job.d_o)
    torch.cuda.synchronize()
    assert torch.equal(ibits(og.detach()), ibits(o))
    for g, w, name in zip((qg.grad, kg.grad, vg.grad), want, ("dq", "dk", "dv")):
        assert torch.equal(ibits(g), ibits(w)), f"MmaAttnCoreFn: {name}"
    # PlainAttnFn on strided views: q / k / v as column slices of one wider projection output each
    job = job_of(A.CASE_BY_ID["plain-d64-b2-h3-129x257"], "sentinel")
    c = job.case
    o, lse = job.forward()
    want = job.backward(o, lse)
    leaves = []
    views = []
    for t in job.plain_views():                                               # [B, L, H, Dh] inside [B, L, 2 * H * Dh + 64]
        wide = torch.full((c.B, t.shape[1], 2 * c.H * c.Dh + 64), float("nan"), dtype=BF, device=DEV)
        wide[:, :, 64:64 + c.H * c.Dh] = t.reshape(c.B, t.shape[1], c.H * c.Dh)
        wide.requires_grad_()
        leaves.append(wide)
        views.append(wide[:, :, 64:64 + c.H * c.Dh].view(c.B, t.shape[1], c.H, c.Dh))
    og = T.PlainAttnFn.apply(*views, c.scale)
    og.backward(job.d_o)
    torch.cuda.synchronize()
    assert torch.equal(ibits(og.detach()), ibits(o))
    for leaf, w, name in zip(leaves, want, ("dq", "dk", "dv")):
        g = leaf.grad[:, :, 64:64 + c.H * c.Dh].reshape(c.B, -1, c.H, c.Dh).permute(0, 2, 1, 3)
        assert torch.equal(ibits(g.contiguous()), ibits(w)), f"PlainAttnFn: {name}"
        assert bool((leaf.grad[:, :, :64] == 0).all()) and bool((leaf.grad[:, :, 64 + c.H * c.Dh:] == 0).all())


def raw_attn_bwd(job, q, k, v, o, d_o, lse, dq, dk, dv, ws, ws_bytes=None, masked=None, Lq=None, Lk=None, Dh=None):
    """aki_attn_bwd on caller-owned buffers; returns the status."""
    from aki_amd import _lib as L
    from aki_amd.ops import _ptr, _stream
    c, t = job.case, job.table
    masked = c.masked if masked is None else masked
    a = L.AttnBwdArgs(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(d_o), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv),
                      _ptr(t.rects) if (masked and t) else None, t.max_rects if (masked and t) else 0,
                      _ptr(t.col_valid_bits) if (masked and t) else None, _ptr(t.seq_lens) if (masked and t) else None,
                      1 if masked else 0, c.B, c.H, Lq or c.Lq, Lk or c.Lk, Dh or c.Dh, float(c.scale), L.AKI_DT_BF16)
    return L.load().aki_attn_bwd(C.byref(a), _ptr(ws), ws.numel() * ws.element_size() if ws_bytes is None else ws_bytes, _stream())


def _followed_by_nan(t, rows=64):
    """A copy of t at the front of a buffer whose tail is NaN rows: a read past the tensor taken for data turns the output NaN."""
    big = torch.full((t.numel() + rows * t.shape[-1],), float("nan"), dtype=t.dtype, device=DEV)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape)


def _in_poison(shape):
    n_ = int(np.prod(shape))
    big = torch.full((n_ + 2 * GUARD,), float("nan"), dtype=BF, device=DEV)
    ibits(big).fill_(0x5A5A)
    return big, big[GUARD:GUARD + n_].view(shape)


@pytest.mark.parametrize("cid", ["L129-b2-h1-rect-one-past", "L33-b3-h2-ragged-17-32-33", "plain-d64-b2-h3-129x257", "plain-d96-b1-h3-33x31"])
def test_outputs_stay_inside_their_buffers_and_inputs_are_not_read_past_their_end(cid):
    from aki_amd import _lib as L
    job = job_of(A.CASE_BY_ID[cid], "diffuse")
    c = job.case
    o, lse = job.forward("product")
    want = job.backward(o, lse)
    q, k, v, d_o, o2 = (_followed_by_nan(t) for t in (job.q, job.k, job.v, job.d_o, o))
    lse2 = _followed_by_nan(lse)
    outs = [_in_poison(s) for s in (job.q.shape, job.k.shape, job.v.shape)]
    nbytes = L.load().aki_attn_bwd_workspace_bytes(c.B, c.H, c.Lq)
    wsbig = torch.full((nbytes // 4 + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ws = wsbig[GUARD:GUARD + nbytes // 4]
    rc = raw_attn_bwd(job, q, k, v, o2, d_o, lse2, outs[0][1], outs[1][1], outs[2][1], ws)
    torch.cuda.synchronize()
    assert rc == 0
    for (big, view), w, name in zip(outs, want, ("dq", "dk", "dv")):
        assert torch.equal(ibits(view), ibits(w)), f"{cid}: {name} differs when the inputs are followed by NaN rows"
        assert bool((ibits(big[:GUARD]) == 0x5A5A).all()) and bool((ibits(big[GUARD + view.numel():]) == 0x5A5A).all()), f"{cid}: bytes outside {name} changed"
    assert bool((wsbig[:GUARD] == 0x5A5A5A5A).all()) and bool((wsbig[GUARD + ws.numel():] == 0x5A5A5A5A).all()), f"{cid}: bytes outside the workspace changed"


def test_calls_the_abi_must_refuse_are_refused():
    """Masked with Lq != Lk, head_dim 72 and a short workspace return the ABI's error codes before anything is launched."""
    from aki_amd import _lib as L, train_ops as T
    from aki_amd._lib import AkiError
    job = job_of(A.CASE_BY_ID["L33-b3-h2-ragged-17-32-33"], "diffuse")
    c = job.case
    o, lse = job.forward("product")
    outs = [_in_poison(s) for s in (job.q.shape, job.k.shape, job.v.shape)]
    nbytes = L.load().aki_attn_bwd_workspace_bytes(c.B, c.H, c.Lq)
    assert nbytes == c.B * c.H * c.Lq * 4
    ws = torch.zeros((nbytes // 4,), dtype=torch.int32, device=DEV)
    args = (job, job.q, job.k, job.v, o, job.d_o, lse, outs[0][1], outs[1][1], outs[2][1], ws)
    assert raw_attn_bwd(*args, ws_bytes=nbytes - 4) == -4                      # AKI_ERR_WORKSPACE
    assert raw_attn_bwd(*args, Lk=c.Lk - 1) == -1                              # AKI_ERR_INVALID_ARG: masked needs Lq == Lk
    assert raw_attn_bwd(*args, Dh=72) == -2                                    # AKI_ERR_UNSUPPORTED
    assert raw_attn_bwd(*args, masked=False, Dh=72) == -2
    torch.cuda.synchronize()
    for big, _ in outs:
        assert bool((ibits(big) == 0x5A5A).all()), "a refused call wrote to an output"
    with pytest.raises(AkiError):
        T.attn_bwd(job.q, job.k[:, :, :-1], job.v[:, :, :-1], o, job.d_o, lse, job.table, c.scale)
    assert raw_attn_bwd(*args) == 0
    torch.cuda.synchronize()

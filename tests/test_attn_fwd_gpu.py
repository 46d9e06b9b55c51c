"""Attention forward against a float64 reference where every key counts, at the lengths the 64-row core exists for: every case of
tests/attn_fwd_cases.py, in each of its input families, through the 32-row core forced (L <= 2100), the 64-row core's shipped build
forced, its every-tile-exact build (seam and rising cases), the product library without a lab switch (L >= 1791; it must return the bits
of the core its rule names) and ops.attention at every head_dim attn_nc_bf16 exports (72, 32, 64, 96), in every layout of
attn_fwd_cases.layouts(): head-major tensors, SigLIP's three views of one [B, L, 3, H, Dh] buffer and the Perceiver's q plus two views
of one [B, Lk, 2, H, Dh] buffer, with adversarial rows behind key Lk - 1 and an adversarial leading sample.  o - live and dead rows,
under both dead-row conventions where the case asks for it - and lse are compared elementwise under the bar derived in the docstring
of attn_fwd_cases.py; tests/test_attn_fwd_cases_cpu.py shows which faults cannot stay inside it.  Every route runs twice and must give
equal bits, and so must the layouts of one case: the same arithmetic on the same values.  The largest err / tol per kernel goes to
parity_errors.json through record_parity.

Nothing here leaves the allocations or provokes a fault: the rising case past 2^64 is the kernel's defined second walk of a rank, the
views are checked against what attn_nc_bf16 refuses and against their buffers' ends before a launch, and the refusals at the end of the
module are calls that return a status (or raise) before anything is launched."""
import ctypes
import numpy as np
import pytest
import torch

import attn_fwd_cases as F
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LAB = {"32": 1, "64": 9, "164": 164}
KERNEL = {"32": "32-row core", "64": "64-row core, shipped", "164": "64-row core, every tile exact", "product": "product rule", "plain": "attn_nc"}


def ibits(x: torch.Tensor) -> torch.Tensor:
    return x.view({2: torch.int16, 4: torch.int32}[x.element_size()])


class Job:
    """One case x family on the device; the float64 reference is the module-level cache of attn_fwd_cases."""

    def __init__(self, case, family):
        from aki_amd import ops
        self.case, self.family = case, family
        self.ref = F.reference(case, family)
        inp = self.ref.inp
        self.q, self.k, self.v = (t.to(DEV) for t in (inp.q, inp.k, inp.v))
        self.what = f"{case.id} [{family}]"
        self.table = None
        self._placed = {}
        if case.masked:
            self.table = ops.MaskTable.from_host(case.rect_table(), case.mask_1d(), case.seq_lens, DEV)

    def views(self, layout):
        """q, k, v of the plain route in this layout: views of buffers that live on the device as long as the job does."""
        if layout not in self._placed:
            placed = F.place(self.ref.inp, layout)
            bufs = {name: t.to(DEV) for name, t in placed.bufs.items()}
            views = placed.views(bufs)
            F.check_views(placed, views)
            self._placed[layout] = (bufs, views)
        return self._placed[layout][1]

    def run(self, route, dead_rows=1, kv=None, layout="heads"):
        from aki_amd import ops, _lib
        c = self.case
        k, v = (self.k, self.v) if kv is None else kv
        if route == "plain":
            out = ops.attention(*self.views(layout), c.scale, return_lse=True)
        elif route == "product":
            out = ops.mma_attn_core(self.q, k, v, self.table, c.scale, dead_rows=dead_rows, return_lse=True)
        else:
            with _lib.use_lab_attn(LAB[route]):
                out = ops.mma_attn_core(self.q, k, v, self.table, c.scale, dead_rows=dead_rows, return_lse=True)
                torch.cuda.synchronize()                                          # inside: the switch goes back when the block ends
            return out
        torch.cuda.synchronize()
        return out


_JOBS = {}


def job_of(case, family):
    if (case.id, family) not in _JOBS:
        _JOBS.clear()                                                             # one case's tensors on the device at a time
        _JOBS[(case.id, family)] = Job(case, family)
    return _JOBS[(case.id, family)]


@pytest.fixture(scope="module", autouse=True)
def _drop_jobs():
    yield
    _JOBS.clear()
    F._REFS.clear()
    torch.cuda.empty_cache()


def compare(job, route, dead_rows, o, lse, layout="heads"):
    """o (every row) and lse against the reference under the derived bar; the worst err / tol is printed and recorded before anything is asserted."""
    from conftest import record_parity
    c = job.case
    core = F.product_core(c) if route == "product" else "32" if route in ("32", "plain") else "64"
    o = o.float().cpu().numpy().astype(np.float64).reshape(c.B, c.Lq, c.H, c.Dh).transpose(0, 2, 1, 3)
    lse = lse.float().cpu().numpy().astype(np.float64)
    worst, report, pattern_ok = {"o": 0.0, "lse": 0.0}, {}, True
    for b in range(c.B):
        want, _, _, live = job.ref.expected(b, dead_rows)
        t_o, t_l = job.ref.tol(b, core, dead_rows)
        err = np.abs(o[b] - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err > 0, err / np.where(t_o > 0, t_o, 1e-300), 0.0)
        r = np.where(np.isfinite(err), r, np.inf)
        if r.max() >= worst["o"]:
            h, row, d = (int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
            worst["o"] = float(r.max())
            report["o"] = dict(sample=b, head=h, row=row, feature=d, got=o[b][h, row, d], want=want[h, row, d], err=err[h, row, d], tol=t_o[h, row, d])
        pat = F.lse_pattern(c, b, dead_rows)
        pattern_ok = pattern_ok and bool(np.isfinite(lse[b][:, pat]).all() and (lse[b][:, ~pat] == -np.inf).all())
        rl = np.abs(lse[b][:, live] - job.ref.S[b].lse[:, live]) / t_l[:, live]
        rl = np.where(np.isfinite(rl), rl, np.inf)
        if rl.size and rl.max() >= worst["lse"]:
            h, i = (int(x) for x in np.unravel_index(int(rl.argmax()), rl.shape))
            row = int(np.flatnonzero(live)[i])
            worst["lse"] = float(rl.max())
            report["lse"] = dict(sample=b, head=h, row=row, got=lse[b][h, row], want=job.ref.S[b].lse[h, row],
                                 err=abs(lse[b][h, row] - job.ref.S[b].lse[h, row]), tol=t_l[h, row])
    tag = f"{job.what}, {KERNEL[route]}, dead_rows {dead_rows}" + ("" if layout == "heads" else f", layout {layout}")
    print(f"{tag}: worst err/tol o {worst['o']:.3f}, lse {worst['lse']:.3f}")
    w = max(worst.values())
    kernel = f"{KERNEL['plain']} d{c.Dh}" if route == "plain" else KERNEL[route]
    record_parity(f"attention forward, {kernel}: {tag}", BF, w, w, 1.0, f"err/tol <= 1 ((KAPPA {F.KAPPA[core]} + 2 n 2^-15) 2^-9 M + 2^-8 |ref|)")
    assert pattern_ok, f"{tag}: lse is not -inf exactly on the rows whose row sum is zero"
    bad = {k: report[k] for k, v_ in worst.items() if not v_ <= 1.0}
    assert not bad, f"{tag}: outside the derived bar: {bad}"


def run(job, route, dead_rows, layout="heads"):
    o, lse = job.run(route, dead_rows, layout=layout)
    o, lse = o.clone(), lse.clone()
    o2, lse2 = job.run(route, dead_rows, layout=layout)
    assert torch.equal(ibits(o), ibits(o2)) and torch.equal(ibits(lse), ibits(lse2)), f"{job.what}, {route}: two launches differ"
    if route == "product":
        o3, lse3 = job.run(F.product_core(job.case), dead_rows)
        assert torch.equal(ibits(o), ibits(o3)) and torch.equal(ibits(lse), ibits(lse3)), f"{job.what}: the product library did not pick the core its rule names"
    compare(job, route, dead_rows, o, lse, layout)


# (the masked routes take head-major tensors by their ABI: the layout axis is the plain route's)
PARAMS = [(c, f, r, d, l) for c in F.CASES for f in F.families(c) for r in F.routes(c) for d in F.dead_conventions(c) for l in (F.layouts(c) or ("heads",))]


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: f"{p[0].id}-{p[1]}-{p[2]}-dead{p[3]}" + ("" if p[4] == "heads" else f"-{p[4]}"))
def test_every_route_against_float64(p):
    case, family, route, dead_rows, layout = p
    run(job_of(case, family), route, dead_rows, layout)


@pytest.mark.parametrize("p", [(c, f) for c in F.CASES if not c.masked for f in F.families(c)], ids=lambda p: f"{p[0].id}-{p[1]}")
def test_layouts_of_a_case_give_equal_bits(p):
    """The same values behind other strides, other bases and in front of adversarial rows: the same arithmetic, so the same bits.  A
    difference is an address bug (or a read of something the call does not name), whatever the bar says."""
    case, family = p
    job = job_of(case, family)
    o0, lse0 = (t.clone() for t in job.run("plain"))
    for layout in F.layouts(case)[1:]:
        o, lse = job.run("plain", layout=layout)
        assert torch.equal(ibits(o), ibits(o0)) and torch.equal(ibits(lse), ibits(lse0)), f"{job.what}: layout {layout} and head-major tensors give different bits"


@pytest.mark.parametrize("family", F.families(F.CASE_BY_ID[F.KV_CACHE_CASE]))
def test_kv_cache_views_across_the_seam(family):
    """K / V handed over as KV-cache views: capacity > L, the tail NaN.  Rows past L must never be read as data - under the strong bar, at
    L = 4097: the last tile (tile 64) holds one key and would hold 63 NaN rows of the cache, and the second head starts at capacity * 96."""
    case = F.CASE_BY_ID[F.KV_CACHE_CASE]
    job = job_of(case, family)
    cap = case.Lk + 64 + 37
    kv = []
    for t in (job.k, job.v):
        big = torch.full((case.B, case.H, cap, case.Dh), float("nan"), device=DEV, dtype=BF)
        big[:, :, :case.Lk] = t
        kv.append(big)
    o, lse = job.run("product", 1, kv)
    o0, lse0 = job.run("product", 1)
    assert torch.equal(ibits(o), ibits(o0)) and torch.equal(ibits(lse), ibits(lse0)), "a KV cache with spare capacity changes the result"
    compare(job, "product", 1, o, lse)


# ---- what aki_attn_fwd and ops.attention refuse: a status or an exception before any launch, and an output nobody touched ---------------
UNSUPPORTED, ALIGNMENT = -2, -3                # aki_status of include/aki_mi355x.h


def _attn_call(q, k, v, o, Dh, strides=None):
    """aki_attn_fwd itself on q [B, Lq, H, .] / k, v [B, Lk, H, .] views with a head_dim and strides of the caller's choosing."""
    from aki_amd import _lib
    B, Lq, H, _ = q.shape
    st = strides or [(t.stride(0), t.stride(2), t.stride(1)) for t in (q, k, v)]
    a = _lib.AttnArgs(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), *st[0], *st[1], *st[2], B, H, Lq, k.shape[1], Dh, float(Dh) ** -0.5,
                      _lib.AKI_DT_BF16, None)
    ws = torch.empty(B * H * Dh * 4 + 256, dtype=torch.uint8, device=DEV)
    rc = _lib.load().aki_attn_fwd(ctypes.byref(a), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_refusals_return_their_status_and_leave_the_output_alone():
    from aki_amd import ops, _lib
    B, L, H = 1, 40, 2
    g = torch.Generator(device="cpu").manual_seed(5)
    buf = torch.randn(B, L, 3, H, 96, generator=g).to(BF).to(DEV)               # room for every head_dim and stride named below
    fill = torch.full((B, L, H * 96), float("nan"), dtype=BF, device=DEV)
    q, k, v = (buf[:, :, i] for i in range(3))
    for what, want, Dh, strides in (
            ("head_dim 80", UNSUPPORTED, 80, None),
            ("a token stride of Dh + 4", ALIGNMENT, 72, [(q.stride(0), q.stride(2), 72 + 4)] * 3),
            ("a k token stride of Dh + 4 alone", ALIGNMENT, 64, [(q.stride(0), q.stride(2), q.stride(1)), (q.stride(0), q.stride(2), 64 + 4), (q.stride(0), q.stride(2), q.stride(1))])):
        o = fill.clone()
        rc = _attn_call(q, k, v, o, Dh, strides)
        assert rc == want, f"{what}: status {rc}, expected {want}"
        assert torch.equal(ibits(o), ibits(fill)), f"{what}: a refused call wrote to the output"
    # a channel stride other than 1 has no field in aki_attn_args: ops.attention refuses it before it allocates or launches anything
    wide = torch.randn(B, L, H, 2 * 64, generator=g).to(BF).to(DEV)
    with pytest.raises(_lib.AkiError, match="channel stride"):
        ops.attention(wide[..., ::2], k[..., :64], v[..., :64], 64 ** -0.5)
    with pytest.raises(_lib.AkiError, match="channel stride"):
        ops.attention(q[..., :64], k[..., :64], wide[..., ::2], 64 ** -0.5)


def test_f32_queries_longer_than_the_keys_are_refused_by_name():
    """The f32 parity kernel is square: ops.attention pads shorter queries to Lk rows and says so where it cannot (the table's 33 x 31)."""
    from aki_amd import ops, _lib
    g = torch.Generator(device="cpu").manual_seed(6)
    q, k, v = (torch.randn(1, n_, 3, 32, generator=g).to(DEV) for n_ in (33, 31, 31))
    with pytest.raises(_lib.AkiError, match="Lq <= Lk"):
        ops.attention(q, k, v, 32 ** -0.5)
    o = ops.attention(q[:, :31], k, v, 32 ** -0.5)                                # the same call inside the limit runs
    assert o.shape == (1, 31, 96) and bool(torch.isfinite(o).all())

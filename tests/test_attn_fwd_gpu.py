"""Attention forward against a float64 reference where every key counts, at the lengths the 64-row core exists for: every case of
tests/attn_fwd_cases.py, in each of its input families, through the 32-row core forced (L <= 2100), the 64-row core's shipped build
forced, its every-tile-exact build (seam and rising cases), the product library without a lab switch (L >= 1791; it must return the bits
of the core its rule names) and ops.attention at head_dim 72 and 32.  o - live and dead rows, under both dead-row conventions where
the case asks for it - and lse are compared elementwise under the bar derived in the docstring of attn_fwd_cases.py;
tests/test_attn_fwd_cases_cpu.py shows which faults cannot stay inside it.  Every route runs twice and must give equal bits.  The
largest err / tol per kernel goes to parity_errors.json through record_parity.

Nothing here leaves the allocations or provokes a fault: the rising case past 2^64 is the kernel's defined second walk of a rank."""
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
        if case.masked:
            self.table = ops.MaskTable.from_host(case.rect_table(), case.mask_1d(), case.seq_lens, DEV)

    def run(self, route, dead_rows=1, kv=None):
        from aki_amd import ops, _lib
        c = self.case
        k, v = (self.k, self.v) if kv is None else kv
        if route == "plain":
            out = ops.attention(*(t.permute(0, 2, 1, 3) for t in (self.q, k, v)), c.scale, return_lse=True)
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


def compare(job, route, dead_rows, o, lse):
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
    tag = f"{job.what}, {KERNEL[route]}, dead_rows {dead_rows}"
    print(f"{tag}: worst err/tol o {worst['o']:.3f}, lse {worst['lse']:.3f}")
    w = max(worst.values())
    kernel = f"{KERNEL['plain']} d{c.Dh}" if route == "plain" else KERNEL[route]
    record_parity(f"attention forward, {kernel}: {tag}", BF, w, w, 1.0, f"err/tol <= 1 ((KAPPA {F.KAPPA[core]} + 2 n 2^-15) 2^-9 M + 2^-8 |ref|)")
    assert pattern_ok, f"{tag}: lse is not -inf exactly on the rows whose row sum is zero"
    bad = {k: report[k] for k, v_ in worst.items() if not v_ <= 1.0}
    assert not bad, f"{tag}: outside the derived bar: {bad}"


def run(job, route, dead_rows):
    o, lse = job.run(route, dead_rows)
    o, lse = o.clone(), lse.clone()
    o2, lse2 = job.run(route, dead_rows)
    assert torch.equal(ibits(o), ibits(o2)) and torch.equal(ibits(lse), ibits(lse2)), f"{job.what}, {route}: two launches differ"
    if route == "product":
        o3, lse3 = job.run(F.product_core(job.case), dead_rows)
        assert torch.equal(ibits(o), ibits(o3)) and torch.equal(ibits(lse), ibits(lse3)), f"{job.what}: the product library did not pick the core its rule names"
    compare(job, route, dead_rows, o, lse)


PARAMS = [(c, f, r, d) for c in F.CASES for f in F.families(c) for r in F.routes(c) for d in F.dead_conventions(c)]


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: f"{p[0].id}-{p[1]}-{p[2]}-dead{p[3]}")
def test_every_route_against_float64(p):
    case, family, route, dead_rows = p
    run(job_of(case, family), route, dead_rows)


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

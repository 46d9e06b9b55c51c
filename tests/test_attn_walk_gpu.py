"""Attention forward against a float64 reference where a persistent workgroup walks several ranks of its (batch, head) pair: every case of
tests/attn_walk_cases.py, in each of its input families, through each of its routes (the 32-row core forced, the 64-row core's shipped
build forced, its every-tile-exact build, the product library without a lab switch - which must return the bits of the core its rule
names) and under each dead-row convention the case asks for.  o - every row of every head, dead rows included - and lse are compared
elementwise under the bar derived in attn_fwd_cases.py, unchanged; the H heads of a case are HB = 2 base heads per sample with V scaled by
a sign and a power of two (attn_walk_cases.py, "Replicated heads"), so the float64 reference is made once per base head.  Every route runs
twice and must give equal bits.  The largest err / tol per kernel goes to parity_errors.json through record_parity.

The structural properties of the table (which rank follows which) are claimed for 256 compute units; here the plan is recomputed for the
device's count and every case must still have a workgroup that walks two ranks or more.

Nothing here leaves the allocations or provokes a fault: the rising family past 2^64 is the kernel's defined second walk of a rank."""
import numpy as np
import pytest
import torch

import attn_walk_cases as W
from test_attn_fwd_gpu import ibits, LAB, KERNEL
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


class Job:
    """One case x family on the device; the float64 reference is the module-level cache of attn_walk_cases."""

    def __init__(self, case, family):
        from aki_amd import ops
        self.case, self.family = case, family
        self.ref = W.reference(case, family)
        self.q, self.k, self.v = (t.to(DEV) for t in W.expand(self.ref.inp, case))
        self.what = f"{case.id} [{family}]"
        self.table = ops.MaskTable.from_host(case.rect_table(), case.mask_1d(), case.seq_lens, DEV)

    def run(self, route, dead_rows=1):
        from aki_amd import ops, _lib
        c = self.case
        if route == "product":
            out = ops.mma_attn_core(self.q, self.k, self.v, self.table, c.scale, dead_rows=dead_rows, return_lse=True)
            torch.cuda.synchronize()
            return out
        with _lib.use_lab_attn(LAB[route]):
            out = ops.mma_attn_core(self.q, self.k, self.v, self.table, c.scale, dead_rows=dead_rows, return_lse=True)
            torch.cuda.synchronize()                                              # inside: the switch goes back when the block ends
        return out


_JOBS = {}


def job_of(case, family):
    if (case.id, family) not in _JOBS:
        _JOBS.clear()                                                             # one case's tensors on the device at a time
        torch.cuda.empty_cache()
        _JOBS[(case.id, family)] = Job(case, family)
    return _JOBS[(case.id, family)]


@pytest.fixture(scope="module", autouse=True)
def _drop_jobs():
    yield
    _JOBS.clear()
    W._REFS.clear()
    torch.cuda.empty_cache()


def compare(job, route, dead_rows, o, lse):
    """o (every row of every head) and lse against the reference under the derived bar; the worst err / tol is printed and recorded before
    anything is asserted."""
    from conftest import record_parity
    c = job.case
    core = W.core_of(c, route)
    o = o.float().cpu().numpy().astype(np.float64).reshape(c.B, c.Lq, c.H, c.Dh).transpose(0, 2, 1, 3)
    lse = lse.float().cpu().numpy().astype(np.float64)
    worst, report, pattern_ok = {"o": 0.0, "lse": 0.0}, {}, True
    for b in range(c.B):
        want, t_o, want_l, t_l, live = job.ref.expected(b, core, dead_rows)
        err = np.abs(o[b] - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err > 0, err / np.where(t_o > 0, t_o, 1e-300), 0.0)
        r = np.where(np.isfinite(err), r, np.inf)
        if r.max() >= worst["o"]:
            h, row, d = (int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
            worst["o"] = float(r.max())
            report["o"] = dict(sample=b, head=h, row=row, feature=d, got=o[b][h, row, d], want=want[h, row, d], err=err[h, row, d], tol=t_o[h, row, d])
        pat = W.lse_pattern(c, b, dead_rows)
        pattern_ok = pattern_ok and bool(np.isfinite(lse[b][:, pat]).all() and (lse[b][:, ~pat] == -np.inf).all())
        rl = np.abs(lse[b][:, live] - want_l[:, live]) / t_l[:, live]
        rl = np.where(np.isfinite(rl), rl, np.inf)
        if rl.size and rl.max() >= worst["lse"]:
            h, i = (int(x) for x in np.unravel_index(int(rl.argmax()), rl.shape))
            row = int(np.flatnonzero(live)[i])
            worst["lse"] = float(rl.max())
            report["lse"] = dict(sample=b, head=h, row=row, got=lse[b][h, row], want=want_l[h, row], err=abs(lse[b][h, row] - want_l[h, row]), tol=t_l[h, row])
    tag = f"{job.what}, {KERNEL[route]}, dead_rows {dead_rows}"
    print(f"{tag}: worst err/tol o {worst['o']:.3f}, lse {worst['lse']:.3f}")
    w = max(worst.values())
    record_parity(f"attention forward, several ranks per workgroup, {KERNEL[route]}: {tag}", BF, w, w, 1.0,
                  f"err/tol <= 1 ((KAPPA {W.KAPPA[core]} + 2 n 2^-15) 2^-9 M + 2^-8 |ref|)")
    assert pattern_ok, f"{tag}: lse is not -inf exactly on the rows whose row sum is zero"
    bad = {k: report[k] for k, v_ in worst.items() if not v_ <= 1.0}
    assert not bad, f"{tag}: outside the derived bar: {bad}"


def run(job, route, dead_rows):
    o, lse = job.run(route, dead_rows)
    o, lse = o.clone(), lse.clone()
    o2, lse2 = job.run(route, dead_rows)
    assert torch.equal(ibits(o), ibits(o2)) and torch.equal(ibits(lse), ibits(lse2)), f"{job.what}, {route}: two launches differ"
    if route == "product":
        o3, lse3 = job.run(W.product_core(job.case), dead_rows)
        assert torch.equal(ibits(o), ibits(o3)) and torch.equal(ibits(lse), ibits(lse3)), f"{job.what}: the product library did not pick the core its rule names"
    compare(job, route, dead_rows, o, lse)


PARAMS = [(c, f, r, d) for c in W.CASES for f in W.families(c) for r in W.routes(c) for d in W.dead_conventions(c)]


@pytest.mark.parametrize("p", PARAMS, ids=lambda p: f"{p[0].id}-{p[1]}-{p[2]}-dead{p[3]}")
def test_every_walk_against_float64(p):
    case, family, route, dead_rows = p
    run(job_of(case, family), route, dead_rows)


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_every_case_still_walks_several_ranks_on_this_device(case):
    """Fewer compute units only lower `splits`, so a case that walks several ranks at 256 compute units does so on any smaller device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for core in W.cores(case):
        for dr in W.dead_conventions(case):
            pl = W.walk_plan(case, core, cus, dr)
            assert max(len(w) for w in pl.walks) >= 2, f"{case.id}, {core}-row core: no workgroup walks a second rank with {cus} compute units"
            assert max(len(w) for w in pl.walks) == W.ranks_per_workgroup(case.B, case.H, case.Lq, core, cus)


def test_32_row_core_ranks_per_workgroup_are_invisible():
    """The 32-row counterpart of test_mma_attn_core_dispatch_grouping_is_invisible.  The benchmark shape with all-distinct N(0, 1) heads: the full
    launch (256 pairs: splits 2, every workgroup walks three ranks) against the same heads run two at a time (16 pairs: splits = nqt, one rank
    per workgroup).  How a pair is cut into ranks does not depend on splits, so any differing bit in o or lse is a hand-over fault."""
    from aki_amd import ops
    case = W.CASE_BY_ID["bench-655"]
    B, H, L = case.B, case.H, case.Lq
    assert W.ranks_per_workgroup(B, H, L, "32") == 3 and W.ranks_per_workgroup(B, 2, L, "32") == 1 and W.product_core(case) == "32"
    g = torch.Generator(device="cpu").manual_seed(655)
    q, k, v = (torch.randn(B, H, L, 96, generator=g).to(BF).to(DEV) for _ in range(3))
    table = ops.MaskTable.from_host(case.rect_table(), case.mask_1d(), case.seq_lens, DEV)
    for dead_rows in (1, 0):
        o, lse = ops.mma_attn_core(q, k, v, table, case.scale, dead_rows=dead_rows, return_lse=True)
        o = o.reshape(B, L, H, 96)
        for h in range(0, H, 2):
            o2, lse2 = ops.mma_attn_core(*(t[:, h:h + 2].contiguous() for t in (q, k, v)), table, case.scale, dead_rows=dead_rows, return_lse=True)
            assert torch.equal(ibits(o[:, :, h:h + 2].contiguous()), ibits(o2.reshape(B, L, 2, 96))), f"heads {h}, {h + 1}: o differs between three ranks and one rank per workgroup"
            assert torch.equal(ibits(lse[:, h:h + 2].contiguous()), ibits(lse2)), f"heads {h}, {h + 1}: lse differs between three ranks and one rank per workgroup"

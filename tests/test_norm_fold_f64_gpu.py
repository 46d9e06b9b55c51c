"""The GEMM's row statistics and its folded-norm epilogue against float64: every case of tests/norm_fold_cases.py once on the device, under
the bars derived there (tests/test_norm_fold_cases_cpu.py shows which faults cannot stay inside them).

Producer cases: the launch with stats_out stores the bits of the same launch without it, the statistics of the y it stored are inside their
bars (mean, and 1 / rstd^2 - see the case module), the NaN-filled elements around the statistics vectors and the guard elements around the
output survive, the counter areas of ops._STATS_WS and ops._SPLITK_WS read zero again, and a second launch on the same workspace gives the same
bits.  Consumer cases: ops.linear with row_scale [+ row_shift + col_shift] on exact operands against rs (x w'^T - mu c) [+ bias -> act]
[+ res].  Chained cases: a producer's statistics into a consumer against norm-then-linear of the stored intermediate.  Operands are views
into NaN-filled buffers; every launch's route is the one the table names.  No retries and no soak (tests/test_norm_fold_gpu.py keeps that)."""
import numpy as np
import pytest
import torch

import norm_fold_cases as F
from test_gemm_routes_gpu import Guarded, _counters_zero, _nan_vec, _nan_view
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = {}
_ids = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for fam, (w, what) in sorted(WORST.items()):
        print(f"worst err/bar norm fold [{fam}]: {w:.3f} on {what}")
    torch.cuda.empty_cache()


def _ops():
    from aki_amd import ops
    return ops


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def record(fam, what, worst):
    from conftest import record_parity
    if worst >= WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (worst, what)
    print(f"{what} [{fam}]: err/bar {worst:.3f}")
    record_parity(f"norm fold [{fam}]: {what}", torch.float32 if fam.startswith("producer") else BF, worst, worst, 1.0, "err/bar <= 1 (norm_fold_cases.py)")


class StatVec:
    """An f32 [M] vector inside a NaN-filled buffer, itself NaN until the launch writes it."""
    PAD = 4

    def __init__(self, M):
        self.buf = torch.full((M + 2 * self.PAD,), float("nan"), dtype=torch.float32, device=DEV)
        self.view = self.buf[self.PAD:self.PAD + M]

    def assert_guard(self, what):
        outside = torch.cat([self.buf[:self.PAD], self.buf[self.PAD + self.view.numel():]])
        assert bool(torch.isnan(outside).all()), f"{what}: elements outside [0, M) of a statistics vector were written"


def _residual(res):
    """The residual 16-byte aligned with a row stride that is a multiple of 8, NaN around it (16-byte loads exist when n_out % 8 == 0)."""
    M, n = res.shape
    buf = torch.full((M + 2, (n + 7) // 8 * 8 + 16), float("nan"), dtype=BF, device=DEV)
    v = buf[1:1 + M, 8:8 + n]
    v.copy_(res)
    assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0
    return v


def _expect_log(lib, want, what, also=None):
    from aki_amd import _lib
    got = _lib.gemm_log(lib, cap=16)
    assert got == want or got == also, f"{what}: launched {got}, the table says {want}"


@pytest.mark.parametrize("c", F.PRODUCER, ids=_ids(F.PRODUCER))
def test_producer_case(c):
    from aki_amd import _lib
    ops = _ops()
    inp = F.producer_inputs(c)
    kw = dict(act=c.act)
    x = _nan_view(inp.x)
    if "w2" in c.epi:
        r0 = F.w2_row0(c.N)
        w, kw["w2"], kw["w2_row0"] = _nan_view(inp.w[:r0]), _nan_view(inp.w[r0:]), r0
    else:
        w = _nan_view(inp.w)
    if inp.bias is not None:
        kw["bias"] = _nan_vec(inp.bias.to(DEV))
    if inp.res is not None:
        kw["residual"] = _residual(inp.res)
    if inp.rs is not None:
        kw["row_scale"] = _nan_vec(inp.rs.to(DEV))
    if inp.mu is not None:
        kw["row_shift"], kw["col_shift"] = _nan_vec(inp.mu.to(DEV)), _nan_vec(inp.col.to(DEV))
    gemm_plain = c.M > 16 or inp.rs is not None or "w2" in c.epi        # <= 16 rows without statistics: the decode linears, not this GEMM
    assert gemm_plain or c.exact, "a case of <= 16 rows is bit-comparable with its plain launch only through the residual"
    outs = [Guarded(c.M, c.N, 8) for _ in range(3)]
    stats = [(StatVec(c.M), StatVec(c.M) if c.ln else None) for _ in range(2)]
    with _lib.use_lab(c.mode) as lib:
        lib.aki_lab_gemm_log_reset()
        ops.linear(x, w, out=outs[0].view, **kw)
        for out, (rstd, mean) in zip(outs[1:], stats):
            st = ops.RowStats(rstd.view, mean.view if mean is not None else None)
            ops.linear(x, w, out=out.view, stats_out=st, stats_eps=c.eps, **kw)
        torch.cuda.synchronize()
        _expect_log(lib, c.records * 3, c.id, also=None if gemm_plain else c.records * 2)
    for i, out in enumerate(outs):
        out.assert_guard(f"{c.id}: output of launch {i}")
    assert torch.equal(outs[1].view, outs[0].view), f"{c.id}: the statistics epilogue changed the GEMM's output"
    y = host(outs[1].view)
    assert np.isfinite(y).all()
    if c.exact:
        assert np.array_equal(y, F.f64(inp.res)), f"{c.id}: x = 0 must store the residual bit for bit"
    ref = F.producer_reference(c, y)
    rstd, mean = stats[0]
    for sv in (rstd, mean):
        if sv is not None:
            sv.assert_guard(c.id)
    got = F.producer_ratio(ref, host(mean.view) if c.ln else None, host(rstd.view))
    record(f"producer {c.family} {'ln' if c.ln else 'rms'}", c.id, got.worst)
    if c.ln and c.family.startswith("offset-"):          # measured beside the assertion: what the header's accuracy sentence speaks of
        print(f"{c.id}: worst relative error of the device's rstd {np.abs(host(rstd.view) * np.sqrt(ref.v) - 1.0).max():.2e}")
    m_bad = int(np.argmax(np.maximum(got.mean, got.v)))
    assert got.worst <= 1.0, (f"{c.id}: row {m_bad}: mean err/bar {got.mean[m_bad]:.3g}, 1/rstd^2 err/bar {got.v[m_bad]:.3g} "
                              f"(device mean {host(mean.view)[m_bad] if c.ln else 0.0!r}, rstd {host(rstd.view)[m_bad]!r}; reference mean {ref.mean[m_bad]!r}, "
                              f"v {ref.v[m_bad]!r}); {int((np.maximum(got.mean, got.v) > 1).sum())} of {c.M} rows outside")
    _counters_zero(c.id)
    assert torch.equal(outs[2].view, outs[1].view), f"{c.id}: the second launch's output differs"
    rstd2, mean2 = stats[1]
    assert torch.equal(rstd2.view.view(torch.int32), rstd.view.view(torch.int32)), f"{c.id}: rstd of a second launch on the same workspace differs"
    if c.ln:
        assert torch.equal(mean2.view.view(torch.int32), mean.view.view(torch.int32)), f"{c.id}: mean of a second launch on the same workspace differs"
        mean2.assert_guard(c.id + ", second launch")
    rstd2.assert_guard(c.id + ", second launch")


def _consumer_launch(c, inp, lib_mode):
    from aki_amd import _lib
    ops = _ops()
    kw = dict(act=c.act, row_scale=_nan_vec(inp.rs.to(DEV)))
    if c.ln:
        kw["row_shift"], kw["col_shift"] = _nan_vec(inp.mu.to(DEV)), _nan_vec(inp.col.to(DEV))
    if inp.bias is not None:
        kw["bias"] = _nan_vec(inp.bias.to(DEV))
    if inp.res is not None:
        kw["residual"] = _residual(inp.res)
    out = Guarded(c.M, c.N, 8)
    with _lib.use_lab(lib_mode) as lib:
        lib.aki_lab_gemm_log_reset()
        ops.linear(_nan_view(inp.x), _nan_view(inp.w), out=out.view, **kw)
        torch.cuda.synchronize()
        _expect_log(lib, c.records, c.id)
    out.assert_guard(c.id)
    return host(out.view)


@pytest.mark.parametrize("c", F.CONSUMER, ids=_ids(F.CONSUMER))
def test_consumer_case(c):
    inp = F.consumer_inputs(c)
    ref = F.consumer_reference(c, inp)
    got = _consumer_launch(c, inp, c.mode)
    r = ref.ratio(got)
    at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
    record(f"consumer {c.epi} {c.family}", c.id, float(r.max()))
    assert r.max() <= 1.0, f"{c.id}: {int((r > 1).sum())} of {r.size} elements outside the bar, worst err/tol {r.max():.3g} at {at}: got {got[at]!r}, want {ref.x[at]!r}"


@pytest.mark.parametrize("c", F.CHAINED, ids=_ids(F.CHAINED))
def test_chained_case(c):
    from aki_amd import _lib
    ops = _ops()
    inp = F.chain_inputs(c)
    wf, bfold, col = F.chain_fold(c, inp)
    rstd, mean = StatVec(c.M), StatVec(c.M) if c.ln else None
    st = ops.RowStats(rstd.view, mean.view if c.ln else None)
    y1 = Guarded(c.M, c.N1, 8)
    y2 = Guarded(c.M, c.N2, 8)
    kw = dict(row_scale=st.rstd)
    if c.ln:
        kw.update(row_shift=st.mean, col_shift=_nan_vec(col.to(DEV)), bias=_nan_vec(bfold.to(DEV)))
    with _lib.use_lab(0) as lib:
        lib.aki_lab_gemm_log_reset()
        ops.linear(_nan_view(inp.x0), _nan_view(inp.w0), bias=_nan_vec(inp.b0.to(DEV)), residual=_residual(inp.r0), out=y1.view, stats_out=st, stats_eps=c.eps)
        ops.linear(y1.view, _nan_view(wf), out=y2.view, **kw)
        torch.cuda.synchronize()
        _expect_log(lib, F.chain_records(c), c.id)
    y1.assert_guard(c.id + ": intermediate")
    y2.assert_guard(c.id)
    rstd.assert_guard(c.id)
    stored = host(y1.view)
    pc = F.NS(cfg=F.CFG[F.CHAIN_TILE], ln=c.ln, eps=c.eps, cfg_of_row=lambda m: F.CFG[F.CHAIN_TILE])
    pr = F.producer_ratio(F.producer_reference(pc, stored), host(mean.view) if c.ln else None, host(rstd.view))
    record("chain producer", c.id, pr.worst)
    assert pr.worst <= 1.0, f"{c.id}: the producer's statistics: mean err/bar {pr.mean.max():.3g}, 1/rstd^2 err/bar {pr.v.max():.3g}"
    ref = F.chain_reference(c, stored, wf, bfold)
    got = host(y2.view)
    r = ref.ratio(got)
    at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
    record("chain", c.id, float(r.max()))
    assert r.max() <= 1.0, f"{c.id}: {int((r > 1).sum())} of {r.size} elements outside the bar, worst err/tol {r.max():.3g} at {at}: got {got[at]!r}, want {ref.x[at]!r}"
    _counters_zero(c.id)

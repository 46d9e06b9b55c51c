"""The case table of the folded normalisation (tests/norm_fold_cases.py) checked on the CPU: the tile configurations parsed out of
gemm_bf16.hip, every structural edge reached (computed from those constants), every route the one the lab library's dry run shows, every
reference against float64 torch, a plain float32 restatement of the kernel's summation order inside every producer bar, a plain float32
GEMM + epilogue inside every consumer bar, every mutation visible, and the conditions on the inputs."""
import functools

import numpy as np
import pytest
import torch

import gemm_routes as R
import norm_fold_cases as F
from train_kernel_cases import BF, EPS, MIN_RATIO, bf, f64

_ids = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module")
def lab():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    lib = _lib.load_lab()
    lib.aki_lab_set_gemm_tile(0)
    yield lib
    lib.aki_lab_set_gemm_tile(0)
    lib.aki_lab_set_gemm_dry_run(0)
    lib.aki_lab_gemm_log_reset()


@functools.lru_cache(maxsize=4)
def _pin(cid):
    c = F.PRODUCER_BY_ID[cid]
    inp = F.producer_inputs(c)
    return inp, F.stored_model(c, inp)


# ---- constants and structure ---------------------------------------------------------------------------------------------------------
def test_tile_configurations_are_the_ones_the_table_was_written_for():
    got = {k: (c.CH, c.pipes) for k, c in F.CFG.items()}
    assert got == F.EXPECTED_CONFIGS, f"gemm_bf16.hip now reaches {got}"
    used = {(F.CFG[name].NF, F.CFG[name].NT, F.CFG[name].WN, F.CFG[name].WM, F.CFG[name].NST, pipe, F.CFG[name].SK)
            for c in F.PRODUCER for name, pipe, _, _, _ in c.launches}
    assert used == F.kernel_constants().reach, f"instantiations without a producer case: {sorted(F.kernel_constants().reach - used)}"
    for c in F.CFG.values():
        assert c.lane == 4 * c.NF and c.WN == 2 and c.CH >= 8


def _reach(cfg):
    """What the planner lets a configuration reach: (largest M, largest n_out, smallest n_out)."""
    if cfg.SK:
        return (256 if cfg.BM == 64 else 1024), F.SPLITK_MAX_N, 4
    if cfg.name == "64x128-ring4":
        return 128, 128 * 128, 4
    if cfg.name == "128x128-ring4":
        return 128, 256 * 128, 128 * 128 + 4
    return 1 << 20, 1 << 20, 4


@pytest.mark.parametrize("name", sorted(F.EXPECTED_CONFIGS))
def test_every_structural_edge_is_reached(name):
    cfg = F.CFG[name]
    cases = [c for c in F.PRODUCER if c.launches[0][0] == name and len(c.launches) == 1]
    max_m, max_n, min_n = _reach(cfg)
    slots = {F.slots_of(cfg, c.N) for c in cases}
    tails = {c.N % 64 for c in cases}
    have = lambda pred: any(pred(c) for c in cases)
    if min_n <= cfg.BN:
        assert have(lambda c: c.N <= cfg.BN), "one tile column"
    one, two = F.slot_edges(cfg)
    if two // cfg.WN * cfg.BN - cfg.BN < max_n and F.slots_of(cfg, min_n) <= two:
        assert one in slots and two in slots, f"slots {one} (one pass) and {two} (second pass); CH = {cfg.CH}"
        assert two - cfg.CH in (1, 2)
        spikes = {c.arg for c in cases if c.family == "spike" and F.slots_of(cfg, c.N) == two}
        assert spikes == set(F.SPIKES), f"spike positions {spikes}"
    elif F.slots_of(cfg, min_n) > two:
        assert min(slots) == F.slots_of(cfg, min_n) and min(slots) > 2 * cfg.CH, "the smallest launch of the ring takes three passes"
        assert have(lambda c: c.family == "spike" and c.arg == "ch")
    else:
        assert F.slots_of(cfg, max_n) <= cfg.CH, "one pass only"
    # (the 128-feature ring shares its epilogue paths with the two-stage 128x128 tile: one tail there)
    assert ({60} if name == "128x128-ring4" else {4, 8, 20, 60}) <= tails, f"n_out % 64: {sorted(tails)}"
    assert have(lambda c: c.N % 8 == 4), "p.wide off"
    if max_m >= cfg.BM + 1 and not (cfg.SK and cfg.BM == 96):
        assert have(lambda c: c.M < cfg.BM), "M < BM"
    if max_m > cfg.BM:
        assert have(lambda c: c.M > cfg.BM and c.M % cfg.BM == 1) and have(lambda c: c.M > cfg.BM and c.M % cfg.BM == cfg.BM - 1), "M % BM in {1, BM - 1}"
    else:
        assert have(lambda c: c.M == 1) and have(lambda c: c.M == cfg.BM - 1 or c.M == cfg.BM), "one panel: M = 1, BM - 1 or BM"
    if max_m > F.GM * cfg.BM:
        assert have(lambda c: (c.M + cfg.BM - 1) // cfg.BM > F.GM and ((c.M + cfg.BM - 1) // cfg.BM) % F.GM), "more than GM row panels, a short last group"
    else:
        assert max((c.M + cfg.BM - 1) // cfg.BM for c in cases) == (max_m + cfg.BM - 1) // cfg.BM or max_m == 128, "as many panels as the planner allows"
    assert have(lambda c: c.M % cfg.BM > 48 or c.M >= cfg.BM), "rows 48..63 of a panel"


def test_table_covers_the_other_routes_and_epilogues():
    ids = set(F.PRODUCER_BY_ID)
    plan2 = [c for c in F.PRODUCER if len(c.launches) == 2]
    assert len(plan2) >= 2 and all(c.launches[1][4] == c.launches[0][3] and c.launches[1][4] % 256 == 0 for c in plan2)
    assert {c.launches[1][0] for c in plan2} == {"64x128-ring4", "128x128"}
    assert any(c.cfg.SK and c.launches[0][2] > 1 for c in F.PRODUCER)
    epis = {c.epi for c in F.PRODUCER}
    for e in ((), ("bias",), ("residual",), ("bias", "residual"), ("bias", "gelu"), ("fold-rms",), ("fold-ln", "bias"), ("w2",)):
        assert frozenset(e) in epis, e
    assert {c.family for c in F.PRODUCER} == {"plain", "offset-4", "offset-32", "offset-128", "constant", "zero", "spike", "zero-sum", "row-ladder"}
    assert any(c.launches[0][1] == 6 for c in F.PRODUCER) and "epi-interior-residual" in ids
    for fam in F.LN_FAMILIES:             # these families are about the mean and s2 / n - mean^2: an RMS launch computes neither
        ln_cases = [c for c in F.PRODUCER if c.family == fam and c.ln]
        assert ln_cases, f"{fam}: no LayerNorm case"
        if fam != "constant":
            assert any(F.slots_of(c.cfg, c.N) == F.slot_edges(c.cfg)[1] for c in ln_cases), f"{fam}: no LayerNorm case at the second-pass edge"
    assert sum(c.family == "offset-128" and c.ln for c in F.PRODUCER) >= 5
    assert any(c.family.startswith("offset-") and not c.ln for c in F.PRODUCER), "an offset row under RMSNorm, for the LN formula on an RMS case"
    assert {c.K for c in F.CONSUMER} == {64, 256, 1152}
    assert {c.epi for c in F.CONSUMER} == {"rms", "rms-swiglu", "ln", "ln-bias", "ln-gelu", "ln-res"}
    assert {c.mode for c in F.CONSUMER} == {0, 1, 2, 3, 5}
    assert {c.family for c in F.CONSUMER} == {"x0", "x4", "x32", "wmean", "ladder"}
    assert [(c.ln, c.ratio) for c in F.CHAINED] == [(True, 0.0), (True, 4.0), (True, 32.0), (False, 0.0)]
    for muts, by_id in ((F.PRODUCER_MUTATIONS, F.PRODUCER_BY_ID), (F.CONSUMER_MUTATIONS, F.CONSUMER_BY_ID)):
        for mut, pairs in muts.items():
            assert pairs and all(cid in by_id for cid, _ in pairs), mut
    assert {a for _, a in F.PRODUCER_MUTATIONS["slot-dropped"]} == {"first", "last", "ch-1", "ch"}
    kinds = {F.PRODUCER_BY_ID[cid].ln for cid, _ in F.PRODUCER_MUTATIONS["other-norm"]}
    assert kinds == {True, False}, "the RMS formula on an LN case and the reverse"
    assert {m for m in F.PRODUCER_MUTATIONS} >= {"n-padded-64", "n-padded-bn"}


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
def _dry(lab, mode, route):
    lab.aki_lab_set_gemm_tile(mode)
    try:
        return R.dry_run(lab, route)
    finally:
        lab.aki_lab_set_gemm_tile(0)


@pytest.mark.parametrize("c", F.PRODUCER + F.CONSUMER, ids=_ids(F.PRODUCER + F.CONSUMER))
def test_case_reaches_its_launches(lab, c):
    got = _dry(lab, c.mode, c.route())
    assert got == c.records, f"{c.id}: planned {got}, the table says {c.records}"
    if isinstance(c, F.PCase):
        for name, pipe, ks, rows, first in c.launches:
            assert rows > 0 and first + rows <= c.M and pipe in F.CFG[name].pipes
        assert 64 <= c.K <= 256 or (c.cfg.SK and c.K == F.SPLITK_MIN_K), "K stays small wherever the route allows"


@pytest.mark.parametrize("c", F.CHAINED, ids=_ids(F.CHAINED))
def test_chain_routes(lab, c):
    cfg = F.CFG[F.CHAIN_TILE]
    tile = (cfg.NF, cfg.NT, cfg.WN, cfg.WM)
    prod = R.Route(c.id, "linear", (c.M, c.N1, c.K1), (), opts=dict(bias=True, residual=True, stats="ln" if c.ln else "rms"))
    cons = R.Route(c.id, "linear", (c.M, c.N2, c.N1), (), opts=dict(bias=c.ln, fold="ln" if c.ln else "rms"))
    for route, want in zip((prod, cons), F.chain_records(c)):
        got = _dry(lab, 0, route)
        assert got == [want] and got[0][:4] == tile, got


# ---- producer: conditions, reference, the float32 restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.PRODUCER, ids=_ids(F.PRODUCER))
def test_producer_inputs_reference_and_f32_restatement(c):
    inp, y = _pin(c.id)
    assert np.isfinite(y).all() and float((y * y).sum(1).max()) < 2.0 ** 100
    assert c.M > 16 or c.exact, "<= 16 rows: the plain launch is a decode linear, bit-comparable only through the residual"
    if c.exact:
        assert not f64(inp.x).any() and np.array_equal(y, f64(inp.res)), "a steered family stores its residual bit for bit"
    ref = F.producer_reference(c, y)
    # against float64 torch: the normalised row is what layer_norm / RMSNorm give
    yt = torch.from_numpy(y)
    eps = float(np.float32(c.eps))
    want = torch.nn.functional.layer_norm(yt, (c.N,), eps=eps) if c.ln else yt * torch.rsqrt((yt * yt).mean(-1, keepdim=True) + eps)
    mine = (y - ref.mean[:, None]) / np.sqrt(ref.v)[:, None]
    assert np.abs(mine - want.numpy()).max() <= 1e-9 * max(1.0, float(np.abs(mine).max()))
    if c.family == "zero":
        assert (ref.v[0::2] == eps).all() and (ref.bar_mean[0::2] == 0).all()
    if c.family == "constant":
        assert (np.abs(ref.v - eps) <= 1e-12 * (y[:, 0] ** 2)).all()
    if c.family == "zero-sum":
        assert (ref.mean == 0).all()
    if c.family.startswith("offset-") and c.ln:
        r = np.abs(ref.mean) / np.sqrt(ref.v)
        lo, hi = (0.9, 1.1) if c.N >= 1024 and c.M >= 8 else (0.6, 1.6)          # (a single row of 60 values has a sample deviation off by 10 to 25 %)
        assert lo * float(c.family[7:]) < np.median(r) < hi * float(c.family[7:])
    mean, rstd = F.producer_f32(c, y)
    worst = F.producer_ratio(ref, mean, rstd)
    assert worst.worst <= 1.0, f"{c.id}: the float32 restatement misses the bar: mean {worst.mean.max():.3g}, v {worst.v.max():.3g}"


def test_rstd_error_grows_with_the_square_of_mean_over_std():
    """The figures of the module docstring: the restated-f32 rstd against float64 by mean / std, each inside the bound of the K's."""
    lines = []
    for N in (1152, 3072):
        got = F.rstd_error_by_ratio(N)
        lines.append(f"N = {N}:  " + "  ".join(f"{r}: {got[r][0]:.1e} (bound {got[r][1]:.1e})" for r in F.RATIOS))
        for r in F.RATIOS:
            assert got[r][0] <= got[r][1], (N, r, got[r])
        assert got[128][0] > 100 * got[0][0] and got[0][0] < 3e-7
        assert got[16][0] > 3e-5 / 4, "the old rtol = 3e-5 is of the order of the error at 16 standard deviations"
    print("\nworst relative error of the restated-f32 rstd by mean/std\n" + "\n".join(lines))


# ---- producer mutations ------------------------------------------------------------------------------------------------------------------
PM = [(mut, cid, arg) for mut, pairs in F.PRODUCER_MUTATIONS.items() for cid, arg in pairs]


@pytest.mark.parametrize("mut,cid,arg", PM, ids=[f"{m}-{c}-{a}" for m, c, a in PM])
def test_producer_mutation_is_visible(mut, cid, arg):
    c = F.PRODUCER_BY_ID[cid]
    inp, y = _pin(cid)
    ref = F.producer_reference(c, y)
    mean, rstd = F.producer_mutant(c, inp, mut, arg)
    got = F.producer_ratio(ref, mean, rstd)
    assert got.worst >= MIN_RATIO, f"{mut} on {cid} ({arg}): worst err / bar {got.worst:.3g}"
    if mut == "clamp-removed":
        assert np.isnan(rstd).any(), "without the clamp a constant row's variance goes negative: NaN"
    if mut == "slot-dropped" and c.family == "spike":
        s = F.named_slot(c, arg)
        rows = [m for m in range(c.M) if m % 8 == 0]
        assert F.spike_feature(c, c.arg) // c.cfg.slot_w == s and all(got.v[m] >= MIN_RATIO for m in rows)


@pytest.mark.parametrize("cid", sorted({c.id for c in F.PRODUCER if c.family == "spike"}))
def test_every_slot_is_visible_alone(cid):
    """Dropping any one slot moves the row that carries its spike out of the bar."""
    c = F.PRODUCER_BY_ID[cid]
    inp, y = _pin(cid)
    ref = F.producer_reference(c, y)
    slots = F.slots_of(c.cfg, c.N)
    seen = set()
    n, eps = c.N, float(np.float32(c.eps))
    for m in range(c.M):
        s = int(np.argmax(y[m])) // c.cfg.slot_w
        if s in seen:
            continue
        y2 = y[m:m + 1].copy()
        y2[:, s * c.cfg.slot_w:(s + 1) * c.cfg.slot_w] = 0.0
        mean, rstd = F._stats64(y2, n, c.ln, eps)
        one = F.NS(mean=ref.mean[m:m + 1], v=ref.v[m:m + 1], bar_mean=ref.bar_mean[m:m + 1], bar_v=ref.bar_v[m:m + 1], ln=ref.ln)
        assert F.producer_ratio(one, mean, rstd).v[0] >= MIN_RATIO, (cid, m, s)
        seen.add(s)
    assert len(seen) >= min(slots, c.M - (c.M + 7) // 8), f"{cid}: {len(seen)} of {slots} slots carry a spike"


# ---- consumer --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _cin(cid):
    c = F.CONSUMER_BY_ID[cid]
    inp = F.consumer_inputs(c)
    return inp, F.consumer_reference(c, inp)


def _consumer_f32(c, inp):
    """A plain float32 torch implementation in the kernel's order of operations, cast once."""
    acc = inp.x.float() @ inp.w.float().t()
    v = (acc - inp.mu[:, None] * inp.col[None, :]) * inp.rs[:, None] if c.ln else acc * inp.rs[:, None]
    if c.swiglu:
        g, u = v[:, :c.N], v[:, c.N:]
        return f64((u * (g * torch.sigmoid(g))).to(BF))
    if inp.bias is not None:
        v = v + inp.bias.float()
    if c.act == F.ACT_GELU_TANH:
        v = torch.nn.functional.gelu(v, approximate="tanh")
    if inp.res is not None:
        v = v + inp.res.float()
    return f64(v.to(BF))


@pytest.mark.parametrize("c", F.CONSUMER, ids=_ids(F.CONSUMER))
def test_consumer_reference_torch_and_f32(c):
    inp, ref = _cin(c.id)
    assert np.isfinite(ref.x).all() and ref.ok.all()
    x = inp.x.double()
    if c.family != "ladder":                  # rs, mu, c are the row's own statistics there: the fold IS norm-then-linear
        normed = torch.nn.functional.layer_norm(x, (c.K,), eps=1e-6) if c.ln else x * inp.rs.double()[:, None]
        v = normed @ inp.w.double().t()
        if c.swiglu:
            v = v[:, c.N:] * torch.nn.functional.silu(v[:, :c.N])
        if inp.bias is not None:
            v = v + inp.bias.double()
        if c.act == F.ACT_GELU_TANH:
            v = torch.nn.functional.gelu(v, approximate="tanh")
        if inp.res is not None:
            v = v + inp.res.double()
        # rs, mu and c are f32 roundings of the float64 statistics: 2^-24 relative each on the terms they multiply
        slack = 8 * EPS * (f64(inp.rs)[:, None] * (np.abs(f64(inp.x)) @ np.abs(f64(inp.w)).T + (np.abs(f64(inp.mu))[:, None] * np.abs(f64(inp.col))[None, :] if c.ln else 0)))
        if c.swiglu:
            slack = 4 * (slack[:, :c.N] + slack[:, c.N:]) * (1 + np.abs(ref.x))
        assert (np.abs(v.numpy() - ref.x) <= slack + 1e-9).all(), f"{c.id}: the reference is not norm-then-linear"
    if c.ln and c.family in ("x32", "wmean"):
        shift = np.abs(f64(inp.mu)[:, None] * f64(inp.col)[None, :]) * f64(inp.rs)[:, None]
        assert np.median(shift / (np.abs(ref.x) + 1e-30)) > 4, "mu c is many times the result"
    assert (f64(inp.mu) > 0).any() and (f64(inp.mu) < 0).any() and (f64(inp.col) > 0).any() and (f64(inp.col) < 0).any() if c.ln else True
    w = ref.worst(_consumer_f32(c, inp))
    assert w <= 1.0, f"{c.id}: a plain float32 implementation misses the bar: {w:.3g}"


CM = [(mut, cid) for mut, pairs in F.CONSUMER_MUTATIONS.items() for cid, _ in pairs]


@pytest.mark.parametrize("mut,cid", CM, ids=[f"{m}-{c}" for m, c in CM])
def test_consumer_mutation_is_visible(mut, cid):
    c = F.CONSUMER_BY_ID[cid]
    inp, ref = _cin(cid)
    got = F.consumer_reference(c, inp, mut=mut).x
    assert ref.worst(f64(bf(got))) >= MIN_RATIO, f"{mut} on {cid}: worst err / tol {ref.worst(f64(bf(got))):.3g}"


# ---- chained ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.CHAINED, ids=_ids(F.CHAINED))
def test_chain_reference_host_fold_and_f32(c):
    inp = F.chain_inputs(c)
    y1 = f64(bf(f64(inp.x0) @ f64(inp.w0).T + f64(inp.b0)[None, :] + f64(inp.r0)))
    wf, bfold, col = F.chain_fold(c, inp)
    ref = F.chain_reference(c, y1, wf, bfold)
    if c.ln:
        mu, sd = y1.mean(1), y1.std(1)
        if c.ratio:
            assert 0.8 * c.ratio < np.median(np.abs(mu) / sd) < 1.25 * c.ratio
        want, dcol = F.chain_col_bar(wf)
        assert col.dtype == torch.float32 and (np.abs(f64(col) - want) <= dcol).all(), "fold_layernorm's c is not the row sums of the ROUNDED w'"
        unrounded = (f64(inp.w) * f64(inp.gamma)[None, :]).sum(1)
        assert (np.abs(unrounded - want) > dcol).any(), "the check tells the rounded sums from the unrounded ones"
    # float64 torch norm + linear with the unrounded fold: apart by the rounding of w' and b' (2^-9 relative per term) and no more
    t = F.chain_torch(c, y1, inp)
    st = F.producer_reference(F.NS(cfg=F.CFG[F.CHAIN_TILE], ln=c.ln, eps=c.eps, cfg_of_row=lambda m: F.CFG[F.CHAIN_TILE]), y1)
    normed = np.abs(y1 - st.mean[:, None]) / np.sqrt(st.v)[:, None]
    slack = 2.0 ** -8 * (normed @ np.abs(f64(wf)).T) + (2.0 ** -8 * np.abs(f64(bfold))[None, :] if c.ln else 0.0)
    assert (np.abs(t - ref.x) <= slack + 1e-9).all(), f"{c.id}: the reference is not norm-then-linear"
    # the restated float32 producer into a float32 consumer: inside the chain's bar
    cfg = F.CFG[F.CHAIN_TILE]
    mean, rstd = F.kernel_stats_f32(cfg, y1.astype(np.float32), c.ln, c.eps)
    acc = torch.from_numpy(y1).float() @ wf.float().t()
    rs = torch.from_numpy(rstd)[:, None]
    v = (acc - torch.from_numpy(mean)[:, None] * col[None, :]) * rs + bfold.float() if c.ln else acc * rs
    w = ref.worst(f64(v.to(BF)))
    assert w <= 1.0, f"{c.id}: float32 producer + consumer misses the chain's bar: {w:.3g}"

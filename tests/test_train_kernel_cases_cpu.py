"""The case table of tests/train_kernel_cases.py checked on the CPU: every float64 reference against float64 torch autograd (or
torch.optim.AdamW), every structural edge of the kernels reached (from the constants parsed out of train_kernels.hip), every mutation
of the reference visible at MIN_RATIO (or at its derived cap), and a plain float32 torch implementation of each documented formula
inside the bar on every case - the guard against a bar nobody could meet."""
import numpy as np
import pytest
import torch

import train_kernel_cases as T

K = T.kernel_constants()
_ids = lambda cs: [c.id for c in cs]


def agree(ref, auto, what, rel=1e-10):
    """|reference - autograd| <= rel * M componentwise (M = the reference's own sum of |terms|)."""
    for name, a in auto.items():
        o = ref[name]
        with np.errstate(invalid="ignore"):
            bad = np.abs(o.x - a) > rel * o.M + 1e-300
        bad &= o.ok & np.isfinite(a)
        assert not bad.any(), f"{what}: {name} differs from float64 autograd at {np.argwhere(bad)[:3].tolist()}"


def inside(ref, got, what):
    for name, g in got.items():
        w = ref[name].worst(g)
        assert w <= 1.0, f"{what}: the float32 implementation's {name} is at {w:.3f} of the bar"


def worst_ratio(ref, mutated):
    return max(ref[n].worst(mutated[n].x) for n in mutated if isinstance(mutated[n], T.Out) and n in ref)


# ---- the bar itself ------------------------------------------------------------------------------------------------------------------
def test_half_an_ulp_is_the_smallest_bar_one_cast_meets():
    """The bf16 cast of the float64 reference itself - no arithmetic error at all - exceeds 2^-9 |x| on a large share of the elements
    and never exceeds half an ulp of its binade."""
    x = np.abs(T.rng_of("cast").standard_normal(4096)) + 0.01
    err = np.abs(T.f64(T.bf(x)) - x)
    assert (err > 2.0 ** -9 * x).mean() > 0.1
    assert (err <= 2.0 ** -8 * T.hb(x)).all()
    o = T.Out(x, x, 0.0)
    assert o.worst(T.f64(T.bf(x))) <= 1.0 and (o.tol() <= 2.0 ** -8 * x + T.FLOOR).all() and (o.tol() > 2.0 ** -9 * x).all()


# ---- norm ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.NORM_CASES, ids=_ids(T.NORM_CASES))
def test_norm_reference_and_float32(c):
    for fam in T.norm_families(c.rms):
        for with_dres in (False, True):
            inp = T.norm_inputs(c, fam, with_dres)
            ref = T.norm_reference(c, inp)
            if with_dres:
                agree(ref, T.norm_autograd(c, inp), f"{c} [{fam}]")
            inside(ref, T.norm_f32(c, inp), f"{c} [{fam}, dres {with_dres}]")


def test_norm_families_are_what_the_docstring_says():
    c = T.CASE_BY_ID[("norm", "ln-r33-c1152")]
    off = T.norm_inputs(c, "offset", False)
    x = T.f64(off.x)
    assert (np.abs(x.mean(1)) > 50 * x.std(1)).all()
    sm = T.norm_inputs(c, "small", False)
    x, dy, w = T.f64(sm.x), T.f64(sm.dy), T.f64(sm.w)
    assert 0.1 * T.NORM_EPS < (x * x).mean() < 10 * T.NORM_EPS
    assert (np.abs((dy * w).sum(0)) == np.abs(dy * w).sum(0)).all() and (np.abs(x.sum(0)) == np.abs(x).sum(0)).all()


def test_norm_and_fold_edges_are_reached():
    assert K["MAXC"] == 2 and K["NORM_BWD_GROUPS"] == 512 and K["FOLD_COLS"] == 16, "re-aim the norm cases at the new constants"
    cols = {c.cols for c in T.NORM_CASES}
    top = K["MAXC"] * 256 * 8
    assert top in cols and top // 2 in cols and top // 2 + 8 in cols and 8 in cols         # last chunk of slot 0, first of slot 1, the maximum
    assert T.NORM_REFUSED_COLS[0] == top + 8 and T.NORM_REFUSED_COLS[1] % 8
    assert any(c % K["FOLD_COLS"] for c in cols)                                           # a fold workgroup with idle columns
    G = K["NORM_BWD_GROUPS"]
    for cn in (8, 2056):
        for rms in (True, False):
            rows = {c.rows for c in T.NORM_CASES if c.cols == cn and c.rms == rms}
            for edge in (16, 32, 48):                                                      # g + 16 < G: every exit of the fold's loop
                assert {edge - 1, edge, edge + 1} <= rows
            assert {1, G - 1, G, G + 1, 2 * G + 1} <= rows                                 # second and third row of workgroup 0, prefetch past the end
    assert any(c.accumulate for c in T.NORM_CASES)


NORM_MUT = [(m, cid) for m, cids in T.MUTATIONS["norm"].items() for cid in cids]


@pytest.mark.parametrize("m", list(T.MUTATIONS["norm"]))
def test_norm_mutations_are_visible(m):
    need = T.CAPPED.get(("norm", m), T.MIN_RATIO)
    best = 0.0
    for cid in T.MUTATIONS["norm"][m]:
        c = T.CASE_BY_ID[("norm", cid)]
        for fam in T.norm_families(c.rms):
            inp = T.norm_inputs(c, fam, True)
            best = max(best, worst_ratio(T.norm_reference(c, inp), T.norm_reference(c, inp, m)))
    print(f"norm {m}: {best:.2f}")
    assert best >= need, f"norm mutation {m} reaches only {best:.2f} of the bar"


# ---- colsum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.COLSUM_CASES, ids=_ids(T.COLSUM_CASES))
def test_colsum_reference_and_float32(c):
    for fam in T.COLSUM_FAMILIES:
        inp = T.colsum_inputs(c, fam)
        ref = T.colsum_reference(c, inp)
        want = inp.x.to(torch.float64).sum(0) + (inp.out0.to(torch.float64) if c.accumulate else 0)
        agree(ref, {"out": want.numpy()}, f"{c} [{fam}]")
        inside(ref, T.colsum_f32(c, inp), f"{c} [{fam}]")


def test_colsum_edges_are_reached():
    rows, cols = {c.rows for c in T.COLSUM_CASES}, {c.cols for c in T.COLSUM_CASES}
    assert {1, 31, 32, 33, 2048, 2049, 2081} <= rows and {8, 24, 64, 72, 1152} <= cols
    assert T.colsum_G(2048) == 64 and T.colsum_G(2049) == 64 and T.colsum_G(33) == 2       # the 64-group cap and one row past it
    assert any(c.ld > c.cols for c in T.COLSUM_CASES) and any(c.accumulate for c in T.COLSUM_CASES)
    assert any(cn % K["FOLD_COLS"] for cn in cols) and any(cn % 64 for cn in cols)


@pytest.mark.parametrize("m", list(T.MUTATIONS["colsum"]))
def test_colsum_mutations_are_visible(m):
    best = 0.0
    for cid in T.MUTATIONS["colsum"][m]:
        c = T.CASE_BY_ID[("colsum", cid)]
        for fam in T.COLSUM_FAMILIES:
            inp = T.colsum_inputs(c, fam)
            best = max(best, worst_ratio(T.colsum_reference(c, inp), T.colsum_reference(c, inp, m)))
    assert best >= T.MIN_RATIO, f"colsum mutation {m} reaches only {best:.2f} of the bar"


# ---- swiglu / gelu -------------------------------------------------------------------------------------------------------------------
def test_every_finite_bf16_value_is_in_the_exhaustive_inputs():
    v = T.all_finite_bf16()
    assert v.numel() == 65280 and torch.isfinite(v.float()).all() and len(set(v.view(torch.int16).tolist())) == 65280
    assert K["EW_GRID"] == 8192 and 2049 * (8192 // 8) > K["EW_GRID"] * 256 >= 2048 * (8192 // 8)   # (2049, 8192): one row past the grid cap


@pytest.mark.parametrize("partner", T.PARTNERS, ids=str)
def test_swiglu_reference_float32_and_mutations(partner):
    inp = T.exhaustive_inputs("swiglu", partner)
    g, u, da = T.f64(inp.val), T.f64(inp.a), T.f64(inp.b)
    fwd, bwd = T.swiglu_reference(g, u), T.swiglu_reference(g, u, da)
    auto = T.swiglu_autograd(g, u, da)
    agree({**fwd, **bwd}, auto, f"swiglu [{partner}]")
    inside(fwd, T.swiglu_f32(inp.val, inp.a), f"swiglu fwd [{partner}]")
    inside(bwd, T.swiglu_f32(inp.val, inp.a, inp.b), f"swiglu bwd [{partner}]")
    assert worst_ratio(bwd, T.swiglu_reference(g, u, da, "silu-without-g(1-s)")) >= T.MIN_RATIO
    assert worst_ratio(fwd, T.swiglu_reference(g, u, mut="halves-swapped")) >= T.MIN_RATIO
    assert worst_ratio(bwd, T.swiglu_reference(g, u, da, "halves-swapped")) >= T.MIN_RATIO


def test_swiglu_shape_cases_reference_and_float32():
    for rows, F in T.SWIGLU_SHAPES:
        inp = T.swiglu_shape_inputs(rows, F)
        g, u, da = T.f64(inp.gu[:, :F]), T.f64(inp.gu[:, F:]), T.f64(inp.da)
        ref = {**T.swiglu_reference(g, u), **T.swiglu_reference(g, u, da)}
        agree(ref, T.swiglu_autograd(g, u, da), f"swiglu {rows}x{F}")
        inside(ref, {**T.swiglu_f32(inp.gu[:, :F], inp.gu[:, F:]), **T.swiglu_f32(inp.gu[:, :F], inp.gu[:, F:], inp.da)}, f"swiglu {rows}x{F}")


@pytest.mark.parametrize("partner", T.PARTNERS, ids=str)
def test_gelu_reference_float32_and_mutations(partner):
    inp = T.exhaustive_inputs("gelu", partner)
    x, dy = T.f64(inp.val), T.f64(inp.a)
    fwd, bwd = T.gelu_reference(x), T.gelu_reference(x, dy)
    agree({**fwd, **bwd}, T.gelu_autograd(x, dy), f"gelu [{partner}]")
    inside(fwd, T.gelu_f32(inp.val), f"gelu fwd [{partner}]")
    inside(bwd, T.gelu_f32(inp.val, inp.a), f"gelu bwd [{partner}]")
    assert worst_ratio(fwd, T.gelu_reference(x, mut="tanh-form")) >= T.MIN_RATIO
    assert worst_ratio(bwd, T.gelu_reference(x, dy, "x-pdf-dropped")) >= T.MIN_RATIO
    assert T.GELU_REFUSED_N % 8 and all(n % 8 == 0 for n in T.GELU_N) and max(T.GELU_N) > 8 * 256


# ---- rope ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.ROPE_CASES, ids=_ids(T.ROPE_CASES))
def test_rope_reference_and_float32(c):
    for table in T.ROPE_TABLES:
        inp = T.rope_inputs(c, table)
        ref = T.rope_reference(c, inp)
        agree(ref, T.rope_autograd(c, inp), f"{c} [{table}]")
        got = T.rope_f32(c, inp)
        inside({"dqk": ref["dqk"]}, {"dqk": got["dqk"]}, f"{c} [{table}]")
        assert np.array_equal(got["dv"], ref["dv"].x)


def test_rope_edges_are_reached():
    for Dh in T.ROPE_DH:
        mc, ms = T.rope_table(59, Dh, "real")
        assert mc.dtype == np.float32 and mc.shape == (59, Dh)
        assert np.array_equal(mc[:, :Dh // 2], mc[:, Dh // 2:])
        sc, ss = T.rope_table(59, Dh, "synthetic")
        assert (sc[:, :Dh // 2] != sc[:, Dh // 2:]).all() and (ss[:, :Dh // 2] != ss[:, Dh // 2:]).all()
    assert T.ROPE_REFUSED_DH % 16 and all(d % 16 == 0 for d in T.ROPE_DH)
    for c in T.ROPE_CASES:
        if c.pos:
            p = T.rope_inputs(c, "real").pos.numpy()
            assert p.max() >= c.L and p.max() < c.L + T.ROPE_EXTRA and (p[0] != p[1]).any()
            assert c.L == 1 or (np.diff(p[0]) < 0).any()


@pytest.mark.parametrize("m", list(T.MUTATIONS["rope"]))
def test_rope_mutations_are_visible(m):
    best, on_real = 0.0, 0.0
    for cid in T.MUTATIONS["rope"][m]:
        c = T.CASE_BY_ID[("rope", cid)]
        for table in T.ROPE_TABLES:
            inp = T.rope_inputs(c, table)
            r = worst_ratio({"dqk": T.rope_reference(c, inp)["dqk"]}, {"dqk": T.rope_reference(c, inp, m)["dqk"]})
            best = max(best, r)
            on_real = max(on_real, r) if table == "real" else on_real
    assert best >= T.MIN_RATIO, f"rope mutation {m} reaches only {best:.2f} of the bar"
    if "in-place-of-" in m and "[half+d]" in m:
        assert on_real == 0.0, "a wrong-half index is invisible on the real table: the synthetic one is what catches it"


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CE_CASES, ids=_ids(T.CE_CASES))
def test_ce_reference_and_float32(c):
    for fam in T.CE_FAMILIES:
        inp = T.ce_inputs(c, fam)
        ref = T.ce_reference(c, inp)
        agree(ref, T.ce_autograd(c, inp), f"{c} [{fam}]")
        got = T.ce_f32(c, inp)
        assert int(got.pop("n_valid")[0]) == int(ref["n_valid"].x[0])
        inside(ref, got, f"{c} [{fam}]")
        assert (ref["grad"].x[ref["ignored"]] == 0).all() and (ref["loss_rows"].x[ref["ignored"]] == 0).all()


def test_ce_edges_are_reached():
    Vs = {c.V for c in T.CE_CASES}
    assert {511, 512, 513} <= Vs and 2 in Vs and any(v > 2 * 512 for v in Vs) and any(v % 2 for v in Vs)      # the 512-column stride of a thread's passes
    assert any(c.ld > (c.V + 7) // 8 * 8 for c in T.CE_CASES) and any(c.gscale != 1.0 for c in T.CE_CASES)
    seen = set()
    for c in T.CE_CASES:
        inp = T.ce_inputs(c, "diffuse")
        lab = inp.labels.numpy()
        tg = T.ce_targets(c, inp.labels)
        if (tg == -100).all():
            seen.add("n_valid=0")
        if c.L > 1:
            nxt = lab[:, 1:]
            seen |= {"col0"} if (nxt == 0).any() else set()
            seen |= {"last-odd"} if (c.V % 2 and (nxt == c.V - 1).any()) else set()
            seen |= {"-100"} if (nxt == -100).any() else set()
            seen |= {">=V"} if (nxt >= c.V).any() else set()
        assert (T.f64(inp.logits[..., c.V:].view(torch.int16)) == T.CE_POISON).all()
    assert seen == {"n_valid=0", "col0", "last-odd", "-100", ">=V"}, seen
    assert any(c.L == 1 for c in T.CE_CASES) and any(c.labels == "none" for c in T.CE_CASES)
    pk = T.ce_inputs(T.CE_CASES[0], "peaked")
    assert (T.f64(pk.logits[..., :T.CE_CASES[0].V]).max(-1) > 70).all()
    assert T.f64(T.ce_inputs(T.CE_CASES[0], "shifted").logits[..., :2]).min() > 88.8       # exp overflows f32 without the max subtraction


@pytest.mark.parametrize("m", list(T.MUTATIONS["ce"]))
def test_ce_mutations_are_visible(m):
    best = 0.0
    for cid in T.MUTATIONS["ce"][m]:
        c = T.CASE_BY_ID[("ce", cid)]
        for fam in T.CE_FAMILIES:
            inp = T.ce_inputs(c, fam)
            ref, mu = T.ce_reference(c, inp), T.ce_reference(c, inp, m)
            r = max(ref[n].worst(mu[n].x) for n in ("loss_rows", "grad", "loss"))
            if int(mu["n_valid"].x[0]) != int(ref["n_valid"].x[0]):
                r = np.inf
            best = max(best, r)
    assert best >= T.MIN_RATIO, f"ce mutation {m} reaches only {best:.2f} of the bar"


# ---- grad_sqnorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.SQNORM_CASES, ids=_ids(T.SQNORM_CASES))
def test_sqnorm_reference_and_float32(c):
    inp = T.sqnorm_inputs(c)
    ref = T.sqnorm_reference(c, inp)
    want = float((inp.g.to(torch.float64) ** 2).sum()) + (float(inp.out0) if c.accumulate else 0.0)
    agree(ref, {"out": np.array([want])}, str(c))
    inside(ref, T.sqnorm_f32(c, inp), str(c))


def test_sqnorm_edges_and_mutations():
    assert K["SQNORM_GROUPS"] == 1024
    ns = {c.n for c in T.SQNORM_CASES}
    assert max(ns) // 8 > K["SQNORM_GROUPS"] * 256 and 8 in ns and any(n // 8 < 256 for n in ns) and T.SQNORM_REFUSED_N % 8
    for m, cids in T.MUTATIONS["sqnorm"].items():
        best = 0.0
        for cid in cids:
            c = T.CASE_BY_ID[("sqnorm", cid)]
            inp = T.sqnorm_inputs(c)
            best = max(best, worst_ratio(T.sqnorm_reference(c, inp), T.sqnorm_reference(c, inp, m)))
        assert best >= T.MIN_RATIO, f"sqnorm mutation {m} reaches only {best:.2f} of the bar"


# ---- adamw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.ADAMW_CASES, ids=_ids(T.ADAMW_CASES))
def test_adamw_reference_and_float32(c):
    inp = T.adamw_inputs(c)                                                                # the grid-cap case: one period, a slice of it
    ref = T.adamw_reference(c, inp)
    agree(ref, T.adamw_torch(c, inp), str(c))
    inside(ref, T.adamw_f32(c, inp), str(c))
    norm = float(np.sqrt(inp.sqnorm)) * c.gscale
    assert {"off": c.max_norm == 0, "active": norm > 1.01, "inactive": 0.4 < norm < 0.6, "barely": 1.0 < norm < 1.2}[c.clip]
    g = T.f64(inp.g)
    assert g[0] == 0 and g[1] == 0 and abs(g[2]) > 0 and (c.clip in ("inactive", "barely") or abs(g[2]) == 2.0 ** -60) and T.f64(inp.v)[0] == 0


def test_adamw_edges_are_reached():
    cs = [c for c in T.ADAMW_CASES if c.reps == 1]
    for key, vals in (("g32", {False, True}), ("gscale", {1.0, 0.25}), ("max_norm", {0.0, 1.0}), ("clip", {"off", "active", "inactive", "barely"}),
                      ("wd", {0.0, 0.1}), ("step", set(T.ADAMW_STEPS)), ("n", {8, 8 * 257})):
        assert {getattr(c, key) for c in cs} == vals, key
    big = [c for c in T.ADAMW_CASES if c.reps > 1]
    assert len(big) == 1 and big[0].n // 8 > K["EW_GRID"] * 256 and big[0].n == T.ADAMW_PERIOD * big[0].reps
    for N, Kk in T.ADAMW_T_SHAPES:
        assert Kk % 4 == 0
    assert {(N % 64 == 0, Kk % 64 == 0) for N, Kk in T.ADAMW_T_SHAPES} >= {(True, True), (False, False)}
    assert any(N > 64 for N, _ in T.ADAMW_T_SHAPES) and any(Kk > 128 for _, Kk in T.ADAMW_T_SHAPES)


@pytest.mark.parametrize("m", list(T.MUTATIONS["adamw"]))
def test_adamw_mutations_are_visible(m):
    need = T.CAPPED.get(("adamw", m), T.MIN_RATIO)
    best = 0.0
    for cid in T.MUTATIONS["adamw"][m]:
        c = T.CASE_BY_ID[("adamw", cid)]
        inp = T.adamw_inputs(c)
        best = max(best, worst_ratio(T.adamw_reference(c, inp), T.adamw_reference(c, inp, m)))
    print(f"adamw {m}: {best:.2f}")
    assert best >= need, f"adamw mutation {m} reaches only {best:.2f} of the bar"
    if ("adamw", m) in T.CAPPED:
        assert best < T.MIN_RATIO, "no longer capped: move it out of CAPPED"


def test_every_mutation_the_table_names_has_cases():
    for kernel, muts in T.MUTATIONS.items():
        for m, cids in muts.items():
            for cid in cids or ():
                assert (kernel, cid) in T.CASE_BY_ID, f"{kernel} mutation {m}: no case {cid}"
    for kernel, m in T.CAPPED:
        assert m in T.MUTATIONS[kernel] and 1.0 < T.CAPPED[(kernel, m)] < T.MIN_RATIO

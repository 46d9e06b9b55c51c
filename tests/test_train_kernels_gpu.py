"""The row and elementwise kernels of the training step against float64, element by element: every case of tests/train_kernel_cases.py
on the device, under the componentwise bar derived in that module's docstring (tests/test_train_kernel_cases_cpu.py shows which faults
cannot stay inside it).  Outputs that are copies or are defined by other outputs are compared bit for bit.  The largest err / tol per
kernel and output goes to the session's parity log through record_parity and is printed when the module ends.

Where a train_ops wrapper cannot express a pitch, an output view or an accumulate flag the library entry is called with the arguments
the wrapper passes.  All indices stay inside the allocations; refused calls are refused on the host before any launch."""
import numpy as np
import pytest
import torch

import train_kernel_cases as T
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON = 0x5A5A
WORST = {}
_ids = lambda cs: [c.id for c in cs]


def ibits(x):
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def poisoned(*shape, dtype=BF):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    ibits(t).fill_(POISON if t.element_size() == 2 else 0x5A5A5A5A)
    return t


def is_poison(t):
    return bool((ibits(t) == (POISON if t.element_size() == 2 else 0x5A5A5A5A)).all())


def in_wide(t, left=8):
    """t [R, C] as a column slice of a wider poisoned buffer (row pitch above C, 16-byte aligned)."""
    R, Cn = t.shape
    wide = poisoned(R, T.pitch(Cn), dtype=t.dtype)
    wide[:, left:left + Cn] = t.to(DEV)
    return wide, wide[:, left:left + Cn]


def lib():
    from aki_amd import _lib as L
    return L, L.load()


def P(t):
    from aki_amd.ops import _ptr
    return _ptr(t)


def S():
    from aki_amd.ops import _stream
    return _stream()


def host(t):
    torch.cuda.synchronize()
    return t.detach().to("cpu").to(torch.float64).numpy()


def check(kernel, what, ref, got):
    """got: name -> device tensor (or array).  Records and prints the worst err / tol of every output, then asserts."""
    from conftest import record_parity
    bad = {}
    for name, g in got.items():
        o = ref[name]
        g = host(g) if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64)
        g = g.reshape(o.x.shape)
        if o.kind == "exact":
            if not np.array_equal(g, o.x):
                bad[name] = "not bit for bit"
            continue
        r = o.ratio(g)
        w = float(r.max()) if r.size else 0.0
        at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape)) if r.size else ()
        key = f"{kernel} {name}"
        WORST[key] = max(WORST.get(key, 0.0), w)
        print(f"{what}: {name} err/tol {w:.3f} at {at}")
        record_parity(f"{kernel} {name}: {what}", BF if o.kind == "bf16" else torch.float32, w, w, 1.0, "err/tol <= 1 (train_kernel_cases.py)")
        if not w <= 1.0:
            bad[name] = (w, at, float(g[at]), float(o.x[at]))
    assert not bad, f"{what}: outside the derived bar (err/tol, index, got, want): {bad}"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for key, w in sorted(WORST.items()):
        print(f"worst err/tol {key}: {w:.3f}")
    torch.cuda.empty_cache()


# ---- norm_bwd ------------------------------------------------------------------------------------------------------------------------
def raw_norm_bwd(c, x, w, dy, dres, dx, dw, db, cols=None, accumulate=0):
    L, l = lib()
    cols = c.cols if cols is None else cols
    nbytes = l.aki_norm_bwd_workspace_bytes(cols)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=DEV)
    return l.aki_norm_bwd(1 if c.rms else 0, P(x), P(w), P(dy), P(dres), P(dx), P(dw), P(db), c.rows, cols, x.stride(0), dy.stride(0),
                          0 if dres is None else dres.stride(0), dx.stride(0), float(T.NORM_EPS), accumulate, L.AKI_DT_BF16, P(ws),
                          ws.numel() * 4, S())


@pytest.mark.parametrize("c", T.NORM_CASES, ids=_ids(T.NORM_CASES))
def test_norm_backward(c):
    """x, dy and dres are column slices of wider buffers; dw / db are views into one poisoned flat buffer whose neighbours stay
    untouched; accumulate = 1 goes through the library entry onto non-zero bf16 dw / db."""
    from aki_amd import train_ops as TO
    for fam in T.norm_families(c.rms):
        for with_dres in (False, True):
            inp = T.norm_inputs(c, fam, with_dres)
            ref = T.norm_reference(c, inp)
            (_, x), (_, dy) = in_wide(inp.x), in_wide(inp.dy, 16)
            dres = in_wide(inp.dres)[1] if with_dres else None
            flat = poisoned(2 * c.cols + 48)
            dw, db = flat[16:16 + c.cols], flat[32 + c.cols:32 + 2 * c.cols]
            w = inp.w.to(DEV)
            if c.accumulate:
                dw.copy_(inp.dw0)
                db.copy_(inp.db0)
                dxw, dx = in_wide(torch.zeros(c.rows, c.cols, dtype=BF))
                assert raw_norm_bwd(c, x, w, dy, dres, dx, dw, None if c.rms else db, accumulate=1) == 0
                torch.cuda.synchronize()
                assert is_poison(dxw[:, :8]) and is_poison(dxw[:, 8 + c.cols:])
            else:
                dx, dw_, db_ = TO.norm_bwd(c.rms, x, w, dy, T.NORM_EPS, need_db=not c.rms, dw_out=dw, db_out=None if c.rms else db, dres=dres)
                assert dw_.data_ptr() == dw.data_ptr()
            got = {"dx": dx, "dw": dw}
            if not c.rms:
                got["db"] = db
            check(f"norm_bwd<{'RMS' if c.rms else 'LN'}>", f"{c} [{fam}, dres {with_dres}]", ref, got)
            rest = [flat[:16], flat[16 + c.cols:32 + c.cols], flat[32 + 2 * c.cols:]] + ([db] if c.rms and not c.accumulate else [])
            assert all(is_poison(t) for t in rest), f"{c}: bytes beside dw / db changed"


@pytest.mark.parametrize("cols", T.NORM_REFUSED_COLS)
def test_norm_backward_refuses_what_it_cannot_do(cols):
    c = T.Case("norm", "refused", rms=True, rows=3, cols=cols, accumulate=False)
    x, dy, w = (torch.ones(3, 4112, dtype=BF, device=DEV) for _ in range(3))
    dx, dw = poisoned(3, 4112), poisoned(4112)
    assert raw_norm_bwd(c, x, w[0], dy, None, dx, dw, None, cols=cols) == -2               # AKI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert is_poison(dx) and is_poison(dw)


# ---- colsum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.COLSUM_CASES, ids=_ids(T.COLSUM_CASES))
def test_colsum(c):
    from aki_amd import train_ops as TO
    L, l = lib()
    for fam in T.COLSUM_FAMILIES:
        inp = T.colsum_inputs(c, fam)
        ref = T.colsum_reference(c, inp)
        x = in_wide(inp.x)[1] if c.ld > c.cols else inp.x.to(DEV)
        assert x.stride(0) == c.ld
        if c.accumulate:
            flat = poisoned(c.cols + 32)
            out = flat[16:16 + c.cols]
            out.copy_(inp.out0)
            nbytes = l.aki_colsum_workspace_bytes(c.cols)
            ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=DEV)
            assert l.aki_colsum(P(x), P(out), c.rows, c.cols, x.stride(0), 1, L.AKI_DT_BF16, P(ws), nbytes, S()) == 0
            torch.cuda.synchronize()
            assert is_poison(flat[:16]) and is_poison(flat[16 + c.cols:])
        else:
            out = TO.colsum(x)
        check("colsum", f"{c} [{fam}]", ref, {"out": out})


# ---- swiglu / gelu -------------------------------------------------------------------------------------------------------------------
def _swiglu_run(g, u, da, F, what, padded=False):
    """g, u, da: flat bf16 CPU tensors of rows * F elements -> forward and backward through the wrappers (dense) or the library entry
    (pitches above the widths, poisoned padding)."""
    from aki_amd import train_ops as TO
    L, l = lib()
    rows = g.numel() // F
    gu = torch.cat([g.view(rows, F), u.view(rows, F)], 1)
    d2 = da.view(rows, F)
    ref = {**T.swiglu_reference(T.f64(g), T.f64(u)), **T.swiglu_reference(T.f64(g), T.f64(u), T.f64(da))}
    if not padded:
        gud, dad = gu.to(DEV), d2.to(DEV)
        a, dgu = TO.swiglu_fwd(gud), TO.swiglu_bwd(gud, dad)
    else:
        gud, dad = in_wide(gu)[1], in_wide(d2)[1]
        aw, dw_ = poisoned(rows, T.pitch(F)), poisoned(rows, T.pitch(2 * F))
        a, dgu = aw[:, 8:8 + F], dw_[:, 16:16 + 2 * F]
        assert l.aki_swiglu_fwd(P(gud), P(a), rows, F, gud.stride(0), a.stride(0), L.AKI_DT_BF16, S()) == 0
        assert l.aki_swiglu_bwd(P(gud), P(dad), P(dgu), rows, F, gud.stride(0), dad.stride(0), dgu.stride(0), L.AKI_DT_BF16, S()) == 0
        torch.cuda.synchronize()
        assert is_poison(aw[:, :8]) and is_poison(aw[:, 8 + F:]) and is_poison(dw_[:, :16]) and is_poison(dw_[:, 16 + 2 * F:]), f"{what}: padding written"
    check("swiglu_fwd", what, ref, {"a": a.reshape(-1)})
    check("swiglu_bwd", what, ref, {"dg": dgu[:, :F].reshape(-1), "du": dgu[:, F:].reshape(-1)})


@pytest.mark.parametrize("partner", T.PARTNERS, ids=str)
def test_swiglu_every_finite_bf16_gate(partner):
    inp = T.exhaustive_inputs("swiglu", partner)
    _swiglu_run(inp.val, inp.a, inp.b, 64, f"swiglu every gate [{partner}]")


@pytest.mark.parametrize("shape", T.SWIGLU_SHAPES + ("padded",), ids=str)
def test_swiglu_shapes(shape):
    rows, F = (3, 24) if shape == "padded" else shape
    inp = T.swiglu_shape_inputs(rows, F)
    _swiglu_run(inp.gu[:, :F].reshape(-1), inp.gu[:, F:].reshape(-1), inp.da.reshape(-1), F, f"swiglu {shape}", padded=shape == "padded")


def test_swiglu_one_row_past_the_grid_cap():
    """(2049, 8192): 2049 * 1024 chunks against 8192 * 256 threads - the grid-stride second pass.  The reference is computed on the
    rows both passes touch."""
    from aki_amd import train_ops as TO
    rows, F = 2049, 8192
    assert rows * (F // 8) > T.kernel_constants()["EW_GRID"] * 256
    g = torch.Generator().manual_seed(7)
    gu = (2.0 * torch.randn(rows, 2 * F, generator=g)).to(BF)
    da = torch.randn(rows, F, generator=g).to(BF)
    gud, dad = gu.to(DEV), da.to(DEV)
    a, dgu = TO.swiglu_fwd(gud), TO.swiglu_bwd(gud, dad)
    sel = [0, 1, 1023, 2047, 2048]
    gs, us, ds = T.f64(gu[sel, :F]), T.f64(gu[sel, F:]), T.f64(da[sel])
    ref = {**T.swiglu_reference(gs, us), **T.swiglu_reference(gs, us, ds)}
    check("swiglu_fwd", "swiglu (2049, 8192)", ref, {"a": a[sel]})
    check("swiglu_bwd", "swiglu (2049, 8192)", ref, {"dg": dgu[sel, :F], "du": dgu[sel, F:]})
    want = T.swiglu_f32(gu[:, :F], gu[:, F:])["a"]                                        # every element, against float32 torch, loosely:
    assert np.abs(host(a) - want).max() <= 2.0 ** -6 * np.abs(want).max()                  # nothing skipped between the two passes


@pytest.mark.parametrize("partner", T.PARTNERS, ids=str)
def test_gelu_every_finite_bf16_value(partner):
    from aki_amd import train_ops as TO
    inp = T.exhaustive_inputs("gelu", partner)
    x, dy = inp.val.to(DEV), inp.a.to(DEV)
    ref = {**T.gelu_reference(T.f64(inp.val)), **T.gelu_reference(T.f64(inp.val), T.f64(inp.a))}
    check("gelu<0>", f"gelu every value [{partner}]", ref, {"y": TO.gelu_fwd(x)})
    check("gelu<1>", f"gelu every value [{partner}]", ref, {"dx": TO.gelu_bwd(x, dy)})


def test_gelu_sizes_and_refusal():
    from aki_amd import train_ops as TO
    L, l = lib()
    for n in T.GELU_N:
        g = T.rng_of("gelu", n)
        x, dy = T.bf(2.0 * g.standard_normal(n)), T.bf(g.standard_normal(n))
        ref = {**T.gelu_reference(T.f64(x)), **T.gelu_reference(T.f64(x), T.f64(dy))}
        check("gelu<0>", f"gelu n={n}", ref, {"y": TO.gelu_fwd(x.to(DEV))})
        check("gelu<1>", f"gelu n={n}", ref, {"dx": TO.gelu_bwd(x.to(DEV), dy.to(DEV))})
    x, out = torch.ones(16, dtype=BF, device=DEV), poisoned(16)
    assert l.aki_gelu_fwd(P(x), P(out), T.GELU_REFUSED_N, L.AKI_DT_BF16, S()) == -2
    assert l.aki_gelu_bwd(P(x), P(x), P(out), T.GELU_REFUSED_N, L.AKI_DT_BF16, S()) == -2
    torch.cuda.synchronize()
    assert is_poison(out)


# ---- rope ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.ROPE_CASES, ids=_ids(T.ROPE_CASES))
def test_rope_backward_merge(c):
    from aki_amd import train_ops as TO
    for table in T.ROPE_TABLES:
        inp = T.rope_inputs(c, table)
        ref = T.rope_reference(c, inp)
        out = TO.rope_bwd_merge(inp.dq.to(DEV), inp.dk.to(DEV), inp.dv.to(DEV), inp.cos.to(DEV), inp.sin.to(DEV),
                                None if inp.pos is None else inp.pos.to(DEV))
        n = 2 * c.H * c.Dh
        check("rope_bwd_merge", f"{c} [{table}]", ref, {"dqk": out[..., :n], "dv": out[..., n:]})


def test_rope_backward_merge_refuses_head_dim_24():
    L, l = lib()
    t = torch.ones(2, 1, 4, 24, dtype=BF, device=DEV)
    cs = torch.ones(4, 24, device=DEV)
    out = poisoned(2, 4, 72)
    assert l.aki_rope_bwd_merge(P(t), P(t), P(t), P(cs), P(cs), None, P(out), 2, 1, 4, T.ROPE_REFUSED_DH, L.AKI_DT_BF16, S()) == -2
    torch.cuda.synchronize()
    assert is_poison(out)


# ---- cross-entropy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CE_CASES, ids=_ids(T.CE_CASES))
def test_cross_entropy(c):
    """ce_loss without and with the gradient (which overwrites the logits), then ce_rows on the same rows: bit for bit the same
    loss rows and gradients.  Columns V..ld keep their poison."""
    from aki_amd import train_ops as TO
    L, l = lib()
    rows = c.B * c.L
    for fam in T.CE_FAMILIES:
        inp = T.ce_inputs(c, fam)
        ref = T.ce_reference(c, inp)
        what = f"{c} [{fam}]"
        labels = inp.labels.to(DEV)
        buf = inp.logits.to(DEV)
        loss0, nv0 = TO.ce_loss(buf, labels, c.V, gscale=c.gscale, want_grad=False)
        torch.cuda.synchronize()
        assert torch.equal(ibits(buf.cpu()), ibits(inp.logits)), f"{what}: the logits changed without want_grad"
        # with the gradient, through the entry the wrapper calls (it returns the mean only; the rows are compared too)
        lr = torch.empty((rows,), dtype=torch.float32, device=DEV)
        nv = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        assert l.aki_ce_loss_fwd_bwd(P(buf), P(labels), P(nv), P(lr), P(buf), c.B, c.L, c.V, c.ld, c.ld, float(c.gscale), L.AKI_DT_BF16, S()) == 0
        buf2 = inp.logits.to(DEV)
        loss1, nv1 = TO.ce_loss(buf2, labels, c.V, gscale=c.gscale, want_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(ibits(buf), ibits(buf2)) and int(nv) == int(nv0) == int(nv1) and float(loss0) == float(loss1)
        g = buf.reshape(rows, c.ld)
        assert is_poison(g[:, c.V:]), f"{what}: columns V..ld written"
        check("ce_fwd_bwd<0>", what, ref, {"n_valid": nv, "loss_rows": lr, "loss": loss1.reshape(1), "grad": g[:, :c.V]})
        ign = torch.from_numpy(ref["ignored"]).to(DEV)
        assert bool((ibits(g[:, :c.V])[ign] == 0).all()) and bool((ibits(lr)[ign] == 0).all()), f"{what}: ignored rows are not exactly zero"
        if int(nv) == 0:
            assert float(loss1) == 0.0 and bool((ibits(g[:, :c.V]) == 0).all())
        assert bool(torch.isfinite(g[:, :c.V].float()).all()) and bool(torch.isfinite(lr).all())
        # ce_rows on the whole batch as one chunk
        tgt = torch.from_numpy(T.ce_targets(c, inp.labels)).to(DEV)
        buf3 = inp.logits.to(DEV).reshape(rows, c.ld)
        lr3 = torch.empty_like(lr)
        assert l.aki_ce_rows_fwd_bwd(P(buf3), P(tgt), P(nv), P(lr3), P(buf3), rows, c.V, c.ld, c.ld, float(c.gscale), L.AKI_DT_BF16, S()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ibits(lr3), ibits(lr)) and torch.equal(ibits(buf3), ibits(g)), f"{what}: ce_rows differs from ce_loss"
        if c.gscale == 1.0:
            buf4 = inp.logits.to(DEV).reshape(rows, c.ld)
            lr4 = TO.ce_rows(buf4, tgt, nv, c.V, want_grad=True)
            torch.cuda.synchronize()
            assert torch.equal(ibits(lr4), ibits(lr)) and torch.equal(ibits(buf4), ibits(g))


# ---- grad_sqnorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.SQNORM_CASES, ids=_ids(T.SQNORM_CASES))
def test_grad_sqnorm(c):
    from aki_amd import train_ops as TO
    inp = T.sqnorm_inputs(c)
    out = torch.full((1,), float(inp.out0) if c.accumulate else float("nan"), device=DEV)
    TO.grad_sqnorm(inp.g.to(DEV), out, accumulate=c.accumulate)
    check(f"grad_sqnorm<{'f32' if c.g32 else 'bf16'}>", str(c), T.sqnorm_reference(c, inp), {"out": out})


def test_grad_sqnorm_refuses_n_12():
    L, l = lib()
    g = torch.ones(16, dtype=BF, device=DEV)
    out = torch.full((1,), 5.0, device=DEV)
    ws = torch.empty((l.aki_grad_sqnorm_workspace_bytes() // 4,), dtype=torch.int32, device=DEV)
    assert l.aki_grad_sqnorm(P(g), T.SQNORM_REFUSED_N, P(out), 0, L.AKI_DT_BF16, P(ws), ws.numel() * 4, S()) == -2
    assert float(out) == 5.0


# ---- adamw ---------------------------------------------------------------------------------------------------------------------------
def _adamw_call(c, inp, reps=1, t_shape=None):
    from aki_amd import train_ops as TO
    p, m, v, g = (t.repeat(reps).to(DEV) for t in (inp.p, inp.m, inp.v, inp.g))
    w16 = poisoned(p.numel())
    sq = torch.tensor([inp.sqnorm], dtype=torch.float32, device=DEV)
    h = T.ADAMW_HYPER
    if t_shape is None:
        TO.adamw_step(p, m, v, g, w16, sq, c.max_norm, c.gscale, h["lr"], h["beta1"], h["beta2"], h["eps"], c.wd, c.step)
        return p, m, v, w16
    N, Kk = t_shape
    wT = poisoned(Kk, (N + 63) // 64 * 64)
    TO.adamw_step_t(p, m, v, g, w16, wT, N, Kk, sq, c.max_norm, c.gscale, h["lr"], h["beta1"], h["beta2"], h["eps"], c.wd, c.step)
    return p, m, v, w16, wT


@pytest.mark.parametrize("c", T.ADAMW_CASES, ids=_ids(T.ADAMW_CASES))
def test_adamw_step(c):
    inp = T.adamw_inputs(c)
    ref = T.adamw_reference(c, inp)
    p, m, v, w16 = _adamw_call(c, inp, c.reps)
    torch.cuda.synchronize()
    assert torch.equal(ibits(w16), ibits(p.to(BF))), f"{c}: w16 is not bf16(p)"
    if c.reps > 1:                                                                         # every period equals the first, bit for bit
        for t in (p, m, v):
            assert torch.equal(ibits(t.view(c.reps, -1)), ibits(t[:T.ADAMW_PERIOD].expand(c.reps, -1))), f"{c}: periods differ"
        p, m, v = (t[-T.ADAMW_PERIOD:] for t in (p, m, v))                                 # the last one holds the grid-stride second pass
    check(f"adamw<{'f32' if c.g32 else 'bf16'}>", str(c), ref, {"p": p, "m": m, "v": v})


@pytest.mark.parametrize("g32", (False, True), ids=("bf16", "f32"))
@pytest.mark.parametrize("shape", T.ADAMW_T_SHAPES, ids=str)
def test_adamw_step_t(shape, g32):
    """p, m, v, w16 bit for bit those of adamw_step on the same inputs; wT = w16^T, padding columns zero."""
    N, Kk = shape
    c = T.Case("adamw", f"t-{N}x{Kk}", n=N * Kk, g32=g32, gscale=0.25, clip="active", max_norm=1.0, wd=0.1, step=2, reps=1)
    inp = T.adamw_inputs(c, n=N * Kk)
    n, pad = N * Kk, -(N * Kk) % 8                                                         # adamw_step takes multiples of 8: pad its copy
    inp8 = T.NS(**{k: torch.cat([getattr(inp, k), torch.zeros(pad, dtype=getattr(inp, k).dtype)]) for k in ("p", "m", "v", "g")}, sqnorm=inp.sqnorm)
    a = _adamw_call(c, inp8)
    b = _adamw_call(c, inp, t_shape=shape)
    torch.cuda.synchronize()
    for x, y, name in zip(a, b, ("p", "m", "v", "w16")):
        assert torch.equal(ibits(x[:n]), ibits(y)), f"adamw_step_t {shape}: {name} differs from adamw_step"
    wT = b[4]
    assert torch.equal(ibits(wT[:, :N]), ibits(b[3].view(N, Kk).t().contiguous())), f"adamw_step_t {shape}: wT is not w16^T"
    assert bool((ibits(wT[:, N:]) == 0).all()), f"adamw_step_t {shape}: padding columns are not zero"
    check(f"adamw_t<{'f32' if g32 else 'bf16'}>", str(c), T.adamw_reference(c, inp), {"p": b[0], "m": b[1], "v": b[2]})

"""aki_gemm_tn against float64, every contraction row: every case of tests/gemm_tn_cases.py on the device in all input families - bit for bit
in the exact family, under the derived componentwise bar in the diffuse ones (tests/test_gemm_tn_cases_cpu.py shows which faults cannot
stay inside them).  Operands are views into NaN-filled buffers, outputs views into guard-filled ones; every launch is repeated and
must reproduce its bits.  Then train_ops._tn_ok against the launch's own conditions, the three delivery forms of train_ops._wgrad, and a
weight gradient taken from consecutive row chunks.  All indices stay inside the allocations: the case near 4 GiB owns every row its last
K-step can name, with or without a 32-bit wrap."""
import numpy as np
import pytest
import torch

import gemm_tn_cases as G
from test_kernels_gpu import DEV
from test_train_kernels_gpu import P, S, host, ibits, lib

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
UNSUPPORTED = -2
WORST = {}
_ids = lambda cs: [c.id for c in cs]


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for fam, (w, what) in sorted(WORST.items()):
        print(f"worst err/tol gemm_tn [{fam}]: {w:.3f} on {what}")
    torch.cuda.empty_cache()


def place(t, ld, col0, row0, below):
    """t [Kc, n] as rows row0.. and columns col0.. of a [row0 + Kc + below, ld] buffer of NaN."""
    Kc, n = t.shape
    buf = torch.full((row0 + Kc + below, ld), float("nan"), dtype=BF, device=DEV)
    view = buf[row0:row0 + Kc, col0:col0 + n]
    view.copy_(t)
    return view


def place_case(c, inp):
    oa, ob = G.OPERANDS[c.la], G.OPERANDS[c.lb]
    a = place(inp.a, c.lda, oa["col0"], oa["row0"], oa["below"])
    b = place(inp.b, c.ldb, ob["col0"], ob["row0"], ob["below"])
    assert a.stride(0) == c.lda and b.stride(0) == c.ldb and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    return a, b


class GuardedOut:
    """An [I, J] view with row stride ldc, `off` elements into a flat buffer filled with G.GUARD."""

    def __init__(self, I, J, ldc, off):
        self.flat = torch.empty(((I + 2) * ldc + 16,), dtype=torch.int16, device=DEV)
        self.view = self.flat.view(BF).as_strided((I, J), (ldc, 1), off)
        idx = off + torch.arange(I, device=DEV)[:, None] * ldc + torch.arange(J, device=DEV)[None]
        self.outside = torch.ones(self.flat.shape, dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        self.reset()

    def reset(self):
        self.flat.fill_(G.GUARD)

    def assert_guard(self, what):
        bad = int((self.flat[self.outside] != G.GUARD).sum())
        assert bad == 0, f"{what}: {bad} elements outside the output view were written"


def check(c, fam, ref, got, note=""):
    """Prints and records the worst err / tol of the case, then asserts the family's bar."""
    from conftest import record_parity
    what = f"{c} [{fam}]"
    r = ref.ratio(got)
    w = float(r.max())
    at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape))
    bar = G.bar_of(fam)
    shown = 0.0 if w == 0 else (w if bar == "diffuse" else float("inf"))
    if shown >= WORST.get(bar, (-1.0, ""))[0]:
        WORST[bar] = (shown, what)
    print(f"{what}: err/tol {shown:.3f} at {at}")
    record_parity(f"gemm_tn: {what}", BF, shown, shown, 1.0, "bit for bit" if bar == "exact" else "err/tol <= 1 (gemm_tn_cases.py)")
    wrong = int((r > 1.0).sum())
    assert w <= 1.0, f"{what}: {wrong} of {r.size} elements outside the bar, worst err/tol {shown:.3g} at {at}: got {got[at]!r}, want {ref.x[at]!r}{note}"


def run(c, fam, a, b, inp, note=lambda got, ref: ""):
    from aki_amd import train_ops as TO
    ref = G.reference(c, inp, fam)
    out = GuardedOut(c.I, c.J, c.ldc, c.c_off)
    assert out.view.stride(0) == c.ldc and (out.view.data_ptr() % 16 == 0 and c.ldc % 8 == 0) == c.wide
    TO.gemm_tn(a, b, out=out.view)
    got = host(out.view)
    first = out.view.clone()
    out.assert_guard(f"{c} [{fam}]")
    check(c, fam, ref, got, note(got, ref))
    out.reset()
    TO.gemm_tn(a, b, out=out.view)
    torch.cuda.synchronize()
    assert torch.equal(ibits(out.view), ibits(first)), f"{c} [{fam}]: the second launch differs from the first"
    out.assert_guard(f"{c} [{fam}], second launch")


@pytest.mark.parametrize("c", G.SMALL_CASES, ids=_ids(G.SMALL_CASES))
def test_gemm_tn_case(c):
    for fam in G.FAMILIES:
        inp = G.inputs(c, fam)
        a, b = place_case(c, inp)
        run(c, fam, a, b, inp)


def test_gemm_tn_padding_row_past_4_gib():
    """The case near 4 GiB and its refusal twin on one buffer, filled once and freed here.  The exact family tells the three possible
    behaviours of the range check apart: zeros (exact), the row behind the view (+ P_TAIL^2), the wrapped offset (+ P_WRAP^2).
    On gfx950 the row comes back as zeros: the check compares voffset + soffset with the descriptor's size without wrapping at 2^32."""
    from aki_amd import train_ops as TO
    L, l = lib()
    c, twin = G.CASE_BY_ID["near-4g"], G.CASE_BY_ID["near-4g-twin"]
    rows = 1 + G.kernel_constants()["TN_BK"] * c.nk
    buf = None
    try:
        buf = torch.empty((rows, G.LD_BIG), dtype=BF, device=DEV)
        buf.fill_(G.P_WRAP)
        buf[1 + c.Kc:].fill_(G.P_TAIL)
        a, b = buf[1:1 + c.Kc, G.shared_cols("a"):G.shared_cols("a") + c.I], buf[1:1 + c.Kc, G.shared_cols("b"):G.shared_cols("b") + c.J]
        assert TO._tn_ok(a, b) and ((c.Kc - 1) * a.stride(0) + c.I) * 2 == c.span_a

        def note(got, ref):
            d = np.unique(got - ref.x)
            return (f"; every output is off by {d.tolist()}: {G.P_TAIL ** 2} = the padding row was read behind the view, "
                    f"{G.P_WRAP ** 2} = at the wrapped 32-bit offset") if d.size <= 2 else ""
        for fam in G.FAMILIES:
            inp = G.inputs(c, fam)
            a.copy_(inp.a)
            b.copy_(inp.b)
            run(c, fam, a, b, inp, note)
        a2, b2 = buf[1:1 + twin.Kc, 8:8 + twin.I], buf[1:1 + twin.Kc, 24:24 + twin.J]
        out = GuardedOut(twin.I, twin.J, twin.ldc, twin.c_off)
        assert not TO._tn_ok(a2, b2)
        assert l.aki_gemm_tn(P(a2), P(b2), P(out.view), twin.Kc, twin.I, twin.J, a2.stride(0), b2.stride(0), twin.ldc, L.AKI_DT_BF16, S()) == UNSUPPORTED
        torch.cuda.synchronize()
        out.assert_guard("near-4g-twin")
        assert bool((ibits(out.view) == G.GUARD).all())
    finally:
        del buf
        torch.cuda.empty_cache()


# what, Kc, I, J, lda, ldb, ldc, element offsets of a, b, c, operands addressable, output addressable
LAYOUTS = (
    ("plain", 64, 16, 16, 16, 16, 16, 0, 0, 0, True, True),
    ("I = 4", 64, 4, 16, 8, 16, 16, 0, 0, 0, False, True),
    ("I = 12", 64, 12, 16, 16, 16, 16, 0, 0, 0, False, True),
    ("J = 4", 64, 16, 4, 16, 8, 8, 0, 0, 0, False, True),
    ("J = 12", 64, 16, 12, 16, 16, 16, 0, 0, 0, False, True),
    ("lda = 12", 64, 8, 16, 12, 16, 16, 0, 0, 0, False, True),
    ("ldb = 12", 64, 16, 8, 16, 12, 8, 0, 0, 0, False, True),
    ("lda = 24", 64, 8, 16, 24, 16, 16, 0, 0, 0, True, True),
    ("a at 8 bytes", 64, 16, 16, 24, 16, 16, 4, 0, 0, False, True),
    ("b at 8 bytes", 64, 16, 16, 16, 24, 16, 0, 4, 0, False, True),
    ("a at 16 bytes", 64, 16, 16, 24, 16, 16, 8, 0, 0, True, True),
    ("ldc = 18", 64, 16, 16, 16, 16, 18, 0, 0, 0, True, False),
    ("ldc = 20", 64, 16, 16, 16, 16, 20, 0, 0, 0, True, True),
    ("c at 4 bytes", 64, 16, 16, 16, 16, 24, 0, 0, 2, True, False),
    ("c at 8 bytes", 64, 16, 16, 16, 16, 24, 0, 0, 4, True, True),
)


@pytest.mark.parametrize("lay", LAYOUTS, ids=[x[0] for x in LAYOUTS])
def test_tn_ok_is_what_the_launch_accepts(lay):
    """_tn_ok(a, b) is True exactly when aki_gemm_tn accepts the operands (into an output it can address); an output it cannot address is
    refused as well, and _wgrad then copies (test_wgrad_delivery_forms).  A refused call writes nothing, an accepted one the product."""
    from aki_amd import train_ops as TO
    L, l = lib()
    what, Kc, I, J, lda, ldb, ldc, ao, bo, co, ab_ok, c_ok = lay
    src = G.inputs(G.Case("layout", Kc, 16, 16), "exact")
    fa, fb = (torch.zeros((Kc * 24 + 16,), dtype=BF, device=DEV) for _ in range(2))
    a, b = fa.as_strided((Kc, I), (lda, 1), ao), fb.as_strided((Kc, J), (ldb, 1), bo)
    a.copy_(src.a[:, :I])
    b.copy_(src.b[:, :J])
    out = GuardedOut(I, J, ldc, ldc + co)
    status = l.aki_gemm_tn(P(a), P(b), P(out.view), Kc, I, J, lda, ldb, ldc, L.AKI_DT_BF16, S())
    torch.cuda.synchronize()
    assert TO._tn_ok(a, b) == ab_ok, what
    assert status == (0 if ab_ok and c_ok else UNSUPPORTED), f"{what}: status {status}"
    if c_ok:
        assert TO._tn_ok(a, b) == (status == 0), what
    out.assert_guard(what)
    if status == 0:
        assert np.array_equal(host(out.view), G.f64(src.a[:, :I]).T @ G.f64(src.b[:, :J])), what
    else:
        assert bool((ibits(out.view) == G.GUARD).all()), f"{what}: a refused call wrote"


def test_wgrad_delivery_forms(monkeypatch):
    """_wgrad on the exact family: straight into the target, gemm_tn + copy_ for a target the kernel cannot address, two transposes + the
    forward GEMM for operands _tn_ok refuses - the same bits, the reference's, every time."""
    from aki_amd import train_ops as TO
    calls = []
    real_tn, real_tr = TO.gemm_tn, TO.transpose
    monkeypatch.setattr(TO, "gemm_tn", lambda a, b, out=None: (calls.append("tn-direct" if out is not None else "tn-fresh"), real_tn(a, b, out=out))[1])
    monkeypatch.setattr(TO, "transpose", lambda *x, **k: (calls.append("transpose"), real_tr(*x, **k))[1])
    c = G.Case("delivery", 100, 136, 264, "cols", "rows")
    inp = G.inputs(c, "exact")
    want = G.reference(c, inp, "exact").x
    a, b = place_case(c, inp)
    a8 = place(inp.a, c.I + 8, 4, 1, 64)                                   # the same operand at an 8-byte address
    assert TO._tn_ok(a, b) and not TO._tn_ok(a8, b) and a8.data_ptr() % 16 == 8
    J = c.J
    forms = (("direct, wide", a, (J + 24, J + 32), ["tn-direct"]), ("direct, narrow", a, (J + 4, J + 4), ["tn-direct"]),
             ("copy, ldc % 4 != 0", a, (J + 2, J + 2), ["tn-fresh"]), ("copy, target at 4 bytes", a, (J + 4, J + 6), ["tn-fresh"]),
             ("fresh tensor", a, None, ["tn-fresh"]), ("transposes into the target", a8, (J + 24, J + 32), ["transpose", "transpose"]),
             ("transposes, fresh tensor", a8, None, ["transpose", "transpose"]))
    for what, aa, lay, trace in forms:
        del calls[:]
        if lay is None:
            got = TO._wgrad(None, aa, b)
        else:
            out = GuardedOut(c.I, J, *lay)
            param = G.NS(_aki_grad=out.view)
            assert TO._wgrad(param, aa, b) is None and param._aki_grad_live
            out.assert_guard(what)
            got = out.view
        assert calls == trace, f"{what}: took {calls}"
        assert np.array_equal(host(got), want), f"{what}: not the reference's bits"


def test_wgrad_from_row_chunks():
    """dW from three consecutive row chunks of one dY and one X, the chunk length no multiple of the K-step: the rows behind a chunk are the
    next chunk's data (behind the last one, further finite rows), and every chunk's product is exact."""
    from aki_amd import train_ops as TO
    chunk, I, J = 100, 136, 264
    BK = G.kernel_constants()["TN_BK"]
    assert chunk % BK
    src = G.inputs(G.Case("chunks", 3 * chunk + BK, I, J), "exact")
    dy, x = src.a.to(DEV), src.b.to(DEV)
    total = np.zeros((I, J))
    for r0 in range(0, 3 * chunk, chunk):
        a, b = dy[r0:r0 + chunk], x[r0:r0 + chunk]
        assert TO._tn_ok(a, b)
        out = GuardedOut(I, J, J, J)
        TO.gemm_tn(a, b, out=out.view)
        want = G.f64(src.a[r0:r0 + chunk]).T @ G.f64(src.b[r0:r0 + chunk])
        got = host(out.view)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"rows {r0}..{r0 + chunk}: {len(bad)} elements differ, first at {bad[0].tolist()}"
        out.assert_guard(f"rows {r0}..")
        total += got
    assert np.array_equal(total, G.f64(src.a[:3 * chunk]).T @ G.f64(src.b[:3 * chunk]))

"""The small forward kernels against float64, element by element: every case of tests/fwd_row_cases.py on the device - RMSNorm and
LayerNorm forward (bf16 and f32), the row statistics, both fp8 quantisers and rope_append - under the bars derived in that module's
docstring (tests/test_fwd_row_cases_cpu.py shows which faults cannot stay inside them).  Every padded or out-of-range region must keep
its poison bit for bit.  The largest err / bar per kernel and output goes to the session's parity log through record_parity and is
printed when the module ends.

Where ops.py cannot express an argument (ldy != cols, a padded ldq, a missing bias) the library entry is called with the arguments
the wrapper passes.  All indices stay inside the allocations; refused calls are refused on the host before any launch."""
import numpy as np
import pytest
import torch

import fwd_row_cases as T
from test_kernels_gpu import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = {}
_ids = lambda cs: [c.id for c in cs]
POISON = {1: T.Q_POISON, 2: 0x5A5A, 4: T.S_POISON}
ERR_UNSUPPORTED, ERR_ALIGNMENT = -2, -3                 # include/aki_mi355x.h


def ibits(x):
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def poisoned(*shape, dtype=BF):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    ibits(t).fill_(POISON[t.element_size()])
    return t


def is_poison(t):
    return bool((ibits(t) == POISON[t.element_size()]).all())


def widened(t, ld):
    """t [R, C] as the leading columns of a poisoned [R, ld] buffer -> (buffer, view)."""
    wide = poisoned(t.shape[0], ld, dtype=t.dtype)
    wide[:, :t.shape[1]] = t.to(DEV)
    return wide, wide[:, :t.shape[1]]


def lib():
    from aki_amd import _lib as L
    return L, L.load()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def host(t):
    torch.cuda.synchronize()
    return t.detach().to("cpu").to(torch.float64).numpy()


def record(key, what, w, dtype=BF):
    from conftest import record_parity
    WORST[key] = max(WORST.get(key, 0.0), w)
    record_parity(f"{key}: {what}", dtype, w, w, 1.0, "err/bar <= 1 (fwd_row_cases.py)")


def check(kernel, what, ref, got):
    """got: name -> device tensor.  Records and prints the worst err / tol of every output, then asserts."""
    bad = {}
    for name, g in got.items():
        o = ref[name]
        g = host(g).reshape(o.x.shape)
        if o.kind == "exact":
            if not np.array_equal(g, o.x):
                bad[name] = "not bit for bit"
            continue
        r = o.ratio(g)
        w = float(r.max()) if r.size else 0.0
        at = tuple(int(i) for i in np.unravel_index(int(r.argmax()), r.shape)) if r.size else ()
        print(f"{what}: {name} err/tol {w:.3f} at {at}")
        record(f"{kernel} {name}", what, w, BF if o.kind == "bf16" else torch.float32)
        if not w <= 1.0:
            bad[name] = (w, at, float(g[at]), float(o.x[at]))
    assert not bad, f"{what}: outside the derived bar (err/tol, index, got, want): {bad}"


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for key, w in sorted(WORST.items()):
        print(f"worst err/bar {key}: {w:.3f}")
    torch.cuda.empty_cache()


# ---- norms ---------------------------------------------------------------------------------------------------------------------------
def raw_norm(c, x, w, b, y, cols=None, ldx=None):
    L, l = lib()
    cols = c.cols if cols is None else cols
    ldx = x.stride(0) if ldx is None else ldx
    dt = L.AKI_DT_F32 if c.f32 else L.AKI_DT_BF16
    if c.mode == "rms":
        return l.aki_rmsnorm_fwd(P(x), P(w), P(y), c.rows, cols, ldx, y.stride(0), T.NORM_EPS, dt, S())
    return l.aki_layernorm_fwd(P(x), P(w), P(b), P(y), c.rows, cols, ldx, y.stride(0), T.NORM_EPS, dt, S())


NORM_Y_CASES = T.CASES["norm_bf16"] + T.CASES["norm_f32"]


@pytest.mark.parametrize("c", NORM_Y_CASES, ids=[repr(c) for c in NORM_Y_CASES])
def test_norm_forward(c):
    """x and y sit in poisoned buffers of pitch ldx and ldy; columns cols..ldy of y keep their poison; an all-zero row gives exact
    zeros (RMS) or exactly the bias (LN); a LayerNorm without bias passes a null pointer."""
    for fam in T.NORM_FAMILIES:
        inp = T.norm_inputs(c, fam)
        ref = T.norm_reference(c, inp)
        _, x = widened(inp["x"], c.ldx)
        yw = poisoned(c.rows, c.ldy, dtype=inp["x"].dtype)
        y = yw[:, :c.cols]
        b = None if inp["b"] is None else inp["b"].to(DEV)
        assert raw_norm(c, x, inp["w"].to(DEV), b, y) == 0
        torch.cuda.synchronize()
        assert is_poison(yw[:, c.cols:]), f"{c} [{fam}]: columns cols..ldy of y were written"
        check(f"{c.kernel}<{'RMS' if c.mode == 'rms' else 'LN'}>", f"{c} [{fam}]", ref, {"y": y})
        for r in ref["zero_rows"]:
            want = torch.zeros(c.cols, dtype=y.dtype) if inp["b"] is None else inp["b"]
            assert torch.equal(y[r].cpu().float(), want.float()), f"{c} [{fam}]: the all-zero row {r} is not exact"


@pytest.mark.parametrize("what", T.NORM_REJECTED)
@pytest.mark.parametrize("mode", ("rms", "ln"))
def test_norm_bf16_rejections_write_nothing(mode, what):
    """cols above the register limit, cols or ldx no multiple of 8 and a pointer off the 16-byte grid return the error code before any
    launch; y keeps its poison.  The buffers are large enough for the shape that is refused."""
    cols, ldx, off = {"cols-8200": (8200, 8200, 0), "cols-12": (12, 16, 0), "ldx-2060": (2056, 2060, 0), "x-misaligned": (2056, 2064, 4)}[what]
    c = T.Case("norm_bf16", what, mode=mode, rows=T.ROWS, cols=cols, f32=False)
    g = T.rng_of("rejected", what)
    flat = T.bf(g.standard_normal(T.ROWS * ldx + 8)).to(DEV)
    x = flat[off:off + T.ROWS * ldx].view(T.ROWS, ldx)
    w, b = (T.bf(g.standard_normal(cols + 8)).to(DEV)[:cols] for _ in range(2))
    y = poisoned(T.ROWS, (cols + 15) // 16 * 16)
    rc = raw_norm(c, x, w, b if mode == "ln" else None, y, cols=cols, ldx=ldx)
    torch.cuda.synchronize()
    assert rc == (ERR_ALIGNMENT if what == "x-misaligned" else ERR_UNSUPPORTED), f"{what}: returned {rc}"
    assert is_poison(y)


@pytest.mark.parametrize("c", T.CASES["row_stats"], ids=_ids(T.CASES["row_stats"]))
def test_row_stats(c):
    """rstd (and mean) of rows of pitch ldx, the loop stride of 2048 columns crossed up to eight times; entries >= rows keep their poison."""
    L, l = lib()
    for fam in T.NORM_FAMILIES:
        inp = T.norm_inputs(c, fam)
        ref = T.norm_reference(c, inp)
        _, x = widened(inp["x"], c.ldx)
        rstd, mean = poisoned(c.rows + 3, dtype=torch.float32), poisoned(c.rows + 3, dtype=torch.float32)
        ln = c.mode == "ln"
        assert l.aki_row_stats(P(x), c.rows, c.cols, c.ldx, T.NORM_EPS, P(rstd), P(mean) if ln else None, L.AKI_DT_BF16, S()) == 0
        torch.cuda.synchronize()
        assert is_poison(rstd[c.rows:]) and is_poison(mean[c.rows if ln else 0:])
        got = {"rstd": rstd[:c.rows]}
        if ln:
            got["mean"] = mean[:c.rows]
        check(f"row_stats<{c.mode}>", f"{c} [{fam}]", ref, got)


# ---- fp8 quantisers ------------------------------------------------------------------------------------------------------------------
def judge(kernel, what, ref, s, q):
    """s [rows] f32, q [rows, cols] uint8 of the device against the scale bar and the admissible bytes."""
    torch.cuda.synchronize()
    s, q = s.cpu().numpy().astype(np.float64), q.cpu().numpy()
    sr = ref.scale_ratio(s)
    br = ref.byte_ratio(s, q)
    bad = ref.bad_bytes(s, q)
    print(f"{what}: scale err/bar {sr.max():.3f}, byte err/bar {br.max():.3f}, inadmissible bytes {int(bad.sum())} of {bad.size}, "
          f"elements with a choice {int((ref.choices(s) > 1).sum())}")
    record(f"{kernel} scale", what, float(sr.max()), torch.float32)
    record(f"{kernel} bytes", what, float(br.max()), torch.uint8)
    assert sr.max() <= 1.0, f"{what}: scale of row {int(sr.argmax())} at {sr.max():.3f} of its bar ({s[int(sr.argmax())]!r})"
    at = np.argwhere(bad)[:4].tolist()
    assert not bad.any(), f"{what}: {int(bad.sum())} inadmissible bytes, first at {at}: got {[hex(int(q[tuple(i)])) for i in at]}, " \
                          f"admissible {[sorted({hex(int(v)) for v in ref.admissible(s)[(slice(None),) + tuple(i)]}) for i in at]}"


@pytest.mark.parametrize("c", T.QUANT_CASES, ids=_ids(T.QUANT_CASES))
def test_quant_rows_fp8(c):
    """x of pitch ldx, q of pitch ldq; columns cols..ldq of q and the scales past the last row keep their poison."""
    _, l = lib()
    for fam in T.families_of(c):
        inp = T.quant_inputs(c, fam)
        ref = T.QuantRef(c, inp)
        rows = inp["x"].shape[0]
        _, x = widened(inp["x"], c.ldx)
        qw = poisoned(rows, c.ldq, dtype=torch.uint8)
        s = poisoned(rows + 3, dtype=torch.float32)
        w = None if inp["w"] is None else inp["w"].to(DEV)
        assert l.aki_quant_rows_fp8(P(x), P(w), T.NORM_EPS, P(qw), P(s), rows, c.cols, c.ldx, c.ldq, S()) == 0
        torch.cuda.synchronize()
        assert is_poison(qw[:, c.cols:]) and is_poison(s[rows:]), f"{c} [{fam}]: padding written"
        if fam == "ties":
            assert (ref.choices(host(s[:rows])) == 1).all()
        judge(f"quant_rows_fp8<{c.mode}>", f"{c} [{fam}]", ref, s[:rows], qw[:, :c.cols])


@pytest.mark.parametrize("c", T.KV_CASES, ids=_ids(T.KV_CASES))
def test_kv_cache_quant_fp8(c):
    """Blocks of 16 rows over one to four slabs, a partial last block, different capacities; rows >= rows of every slab keep their
    poison in the cache and in the scales; on the tie family exactly one byte per element is admissible (as for quant_rows)."""
    from aki_amd import ops
    for fam in T.KV_FAMILIES:
        inp = T.kv_inputs(c, fam)
        ref = T.QuantRef(c, inp)
        dst = poisoned(c.slabs, c.dst_cap, T.KV_DH, dtype=torch.uint8)
        s = poisoned(c.slabs, c.dst_cap, dtype=torch.float32)
        ops.kv_cache_quant_fp8(inp["x"].to(DEV), dst, s, c.rows)
        torch.cuda.synchronize()
        assert is_poison(dst[:, c.rows:]) and is_poison(s[:, c.rows:]), f"{c} [{fam}]: rows past `rows` written"
        if fam == "ties":
            assert (ref.choices(host(s[:, :c.rows]).reshape(-1)) == 1).all()
        judge("kv_cache_quant_fp8", f"{c} [{fam}]", ref, s[:, :c.rows].reshape(-1), dst[:, :c.rows].reshape(-1, T.KV_DH))


# ---- rope_append ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.ROPE_CASES, ids=_ids(T.ROPE_CASES))
def test_rope_append(c):
    """pos != cache_len, H * Dh below, above and at multiples of the 256-thread block; q and k under the bar, v bit for bit, every other
    element of both caches bit-identical to its poison."""
    from aki_amd import ops
    inp = T.rope_inputs(c)
    ref = T.rope_reference(c, inp)
    dt = torch.float32 if c.f32 else BF
    kc, vc = poisoned(c.B, c.H, c.cap, c.Dh, dtype=dt), poisoned(c.B, c.H, c.cap, c.Dh, dtype=dt)
    q = ops.rope_append(inp["qkv"].to(DEV), inp["cos"].to(DEV), inp["sin"].to(DEV), inp["pos"].to(DEV), inp["cache_len"].to(DEV), kc, vc, c.H)
    torch.cuda.synchronize()
    at = inp["cache_len"].long()
    idx = torch.arange(c.B)
    k_new, v_new = kc.cpu()[idx, :, at], vc.cpu()[idx, :, at]                       # [B, H, Dh]
    check(f"rope_append<{'f32' if c.f32 else 'bf16'}>", repr(c), ref, {"q": q, "k": k_new, "v": v_new})
    for cache in (kc, vc):
        rest = ibits(cache.cpu().clone())
        rest[idx, :, at] = POISON[cache.element_size()]
        assert bool((rest == POISON[cache.element_size()]).all()), f"{c}: a cache element outside the appended row changed"

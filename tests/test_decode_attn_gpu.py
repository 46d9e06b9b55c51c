"""Decode attention against a float64 reference where every key counts: every case of tests/decode_attn_cases.py, in both input
families, through the four kernels a generated token can take - decode_attn_split_kernel<false> (ops.decode_attn, bf16),
decode_attn_kernel<float, 96> (ops.decode_attn, f32), decode_attn_split_kernel<true> (ops.decode_attn_fused, bf16) and
decode_attn_split_fp8kv_kernel (ops.decode_attn_fused on an e4m3 cache).  The bar is the project's own (check: bf16
2e-3 max(1, max|ref|) + 2^-8 |ref|, f32 2e-5 max(1, max|ref|)), applied per sample so that one sample's large output does not widen
another's tolerance.  tests/test_decode_attn_cases_cpu.py shows that no single missing key, leaked mask column, dropped tile or item,
or wrong merge weight stays within that bar on these inputs.

All indices stay inside the allocations: lens[b] < cap, the cos / sin tables have cap rows, the mask words are read only below
nwords, and the workspaces are at least as large as the launch asks (a shorter one is refused on the host before any launch)."""
import numpy as np
import pytest
import torch

import decode_attn_cases as D
from test_kernels_gpu import check, DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON = 0x5A5A5A5A
GUARD = 1024                      # int32 words of poison on either side of a workspace


class Job:
    """One case x family on the device: the poisoned caches before the step, the new tokens' qkv, and the float64 reference."""

    def __init__(self, case, family):
        self.case, self.family = case, family
        self.inp = inp = D.make_inputs(case, family)
        self.ref = D.reference(case, inp)
        self.k, self.v, self.qkv = inp.k.to(DEV), inp.v.to(DEV), inp.qkv.to(DEV)
        self.cos, self.sin = torch.from_numpy(inp.cos).to(DEV), torch.from_numpy(inp.sin).to(DEV)
        self.lens = torch.tensor(case.lens, dtype=torch.int32, device=DEV)
        bits = case.bits()
        self.bits = None if bits is None else torch.from_numpy(bits).to(DEV)
        self.k_new, self.v_new, self.k_new64 = D.appended_rows(inp)
        self.what = f"{case.id} [{family}]"

    def appended(self, dtype):
        """The caches after the append, as rope_append leaves them: the reference's own rotation of k in row lens[b]."""
        k, v = self.k.clone(), self.v.clone()
        for b, ln in enumerate(self.case.lens):
            k[b, :, ln] = torch.from_numpy(self.k_new[b]).to(DEV).to(BF)
            v[b, :, ln] = torch.from_numpy(self.v_new[b]).to(DEV).to(BF)
        return k.to(dtype), v.to(dtype)


@pytest.fixture(scope="module", params=[(c, f) for c in D.CASES for f in D.FAMILIES], ids=lambda p: f"{p[0].id}-{p[1]}")
def job(request):
    j = Job(*request.param)
    yield j
    del j
    torch.cuda.empty_cache()


def ibits(x: torch.Tensor) -> torch.Tensor:
    """Integer view: bit-for-bit comparisons that see NaN poison as well."""
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def guarded_workspace(case):
    """A zero-filled workspace of the documented size, handed in as a slice of a larger poisoned buffer."""
    from aki_amd import ops
    words = ops.decode_attn_workspace(case.B, case.H, D.DH, case.cap, DEV).numel()
    big = torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device=DEV)
    ws = big[GUARD:GUARD + words]
    ws.zero_()
    return big, ws


def check_workspace_after(case, big, ws, what):
    torch.cuda.synchronize()
    assert bool((big[:GUARD] == POISON).all()) and bool((big[GUARD + ws.numel():] == POISON).all()), f"{what}: bytes outside the workspace changed"
    assert int(ws[: case.B * case.H].abs().sum()) == 0, f"{what}: arrival counters not re-armed"


def run_launches(job, launch, what):
    """The launch twice through one workspace at max_keys = max(lens) + 1 (the counters re-arm; the same bits), then at max_keys = 0
    (the whole capacity, what a captured step uses: trailing empty items, the same bits again)."""
    case = job.case
    eager, full = case.max_keys_options()
    big, ws = guarded_workspace(case)
    o1 = launch(eager, ws).clone()
    o2 = launch(eager, ws).clone()
    check_workspace_after(case, big, ws, what)
    o3 = launch(full, ws).clone()
    check_workspace_after(case, big, ws, what)
    assert torch.equal(ibits(o1), ibits(o2)), f"{what}: the second pass through the workspace differs from the first"
    assert torch.equal(ibits(o1), ibits(o3)), f"{what}: max_keys = 0 and max_keys = {eager} differ"
    return o1


def check_rows(got: torch.Tensor, want: np.ndarray, dtype, what):
    """check() per sample; the worst err / tol of the sample travels in the name of the comparison (-> parity_errors.json)."""
    got = got.detach().float().cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(want.shape[0]):
        mx = max(1.0, float(np.abs(want[b]).max()))
        tol = 2e-3 * mx + 2.0 ** -8 * np.abs(want[b]) if dtype == BF else 2e-5 * mx + 0 * want[b]
        ratio = float((np.abs(got[b] - want[b]) / tol).max())
        worst = max(worst, ratio) if np.isfinite(ratio) else float("inf")
        check(got[b], want[b], dtype, f"{what} sample {b} (worst err/tol {ratio:.3f})", scale_atol=2.0)
    print(f"{what}: worst err/tol {worst:.3f}")


def test_split_kernel_bf16(job):
    """ops.decode_attn, bf16: decode_attn_split_kernel<false> on the appended caches, q rotated by the reference."""
    from aki_amd import ops
    k, v = job.appended(BF)
    k0, v0 = k.clone(), v.clone()
    q = torch.from_numpy(D.rotated_q(job.inp)).to(DEV).to(BF)
    got = run_launches(job, lambda mk, ws: ops.decode_attn(q, k, v, job.lens + 1, D.SCALE, job.bits, mk, ws), f"decode_attn bf16 {job.what}")
    assert torch.equal(ibits(k), ibits(k0)) and torch.equal(ibits(v), ibits(v0)), "decode_attn wrote to the caches"
    check_rows(got, job.ref, BF, f"decode_attn bf16 {job.what}")


def test_plain_kernel_f32(job):
    """ops.decode_attn, f32: decode_attn_kernel<float, 96> on the same (bf16-valued) rows."""
    from aki_amd import ops
    k, v = job.appended(torch.float32)
    q = torch.from_numpy(D.rotated_q(job.inp)).to(DEV)
    o1 = ops.decode_attn(q, k, v, job.lens + 1, D.SCALE, job.bits)
    o2 = ops.decode_attn(q, k, v, job.lens + 1, D.SCALE, job.bits, max(job.case.lens) + 1)
    torch.cuda.synchronize()
    assert torch.equal(ibits(o1), ibits(o2)), "decode_attn f32: two launches differ"
    check_rows(o1, job.ref, torch.float32, f"decode_attn f32 {job.what}")


def test_fused_kernel_bf16(job):
    """ops.decode_attn_fused, bf16: decode_attn_split_kernel<true> - RoPE, append and attention in one launch."""
    from aki_amd import ops
    case = job.case
    k, v = job.k.clone(), job.v.clone()

    def launch(mk, ws):
        k.copy_(job.k); v.copy_(job.v)
        return ops.decode_attn_fused(job.qkv, job.cos, job.sin, job.lens, k, v, case.H, D.SCALE, job.bits, mk, ws)

    got = run_launches(job, launch, f"decode_attn_fused bf16 {job.what}")
    # the appended rows: k within one bf16 ulp of the float64 rotation and bit-identical to rope_append's, v a bit-exact copy
    k2, v2 = job.k.clone(), job.v.clone()
    ops.rope_append(job.qkv, job.cos, job.sin, job.lens, job.lens, k2, v2, case.H)
    torch.cuda.synchronize()
    assert torch.equal(ibits(k), ibits(k2)) and torch.equal(ibits(v), ibits(v2)), "the caches differ from those rope_append leaves"
    want_k, want_v = job.k.clone(), job.v.clone()
    raw_v = job.qkv.view(case.B, 3, case.H, D.DH)[:, 2]
    for b, ln in enumerate(case.lens):
        got_k = k[b, :, ln].float().cpu().numpy().astype(np.float64)
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(job.k_new64[b]), 2.0 ** -126))) - 7)
        assert (np.abs(got_k - job.k_new64[b]) <= ulp).all(), f"appended k row of sample {b} is more than one bf16 ulp off the f64 rotation"
        assert torch.equal(ibits(v[b, :, ln]), ibits(raw_v[b])), f"appended v row of sample {b} is not a copy"
        want_k[b, :, ln], want_v[b, :, ln] = k[b, :, ln], v[b, :, ln]
    assert torch.equal(ibits(k), ibits(want_k)) and torch.equal(ibits(v), ibits(want_v)), "a cache element outside the appended rows changed"
    check_rows(got, job.ref, BF, f"decode_attn_fused bf16 {job.what}")


def _fp8_caches(job):
    """The e4m3 cache holding the quantised rows of the bf16 one (host rule: ref_quant); rows at and past the append position are
    unwritten cache: NaN bytes and NaN scales."""
    k8, ks = D.ref_quant(job.inp.k.float())
    v8, vs = D.ref_quant(job.inp.v.float())
    for b, ln in enumerate(job.case.lens):
        k8[b, :, ln:] = 0x7F
        v8[b, :, ln:] = 0xFF
        ks[b, :, ln:] = float("nan")
        vs[b, :, ln:] = float("nan")
    return tuple(a.contiguous().to(DEV) for a in (k8, v8, ks, vs))


def test_fused_kernel_fp8_cache(job):
    """ops.decode_attn_fused on an e4m3 cache: decode_attn_split_fp8kv_kernel, against its own stored rows."""
    from aki_amd import ops
    case = job.case
    k0, v0, ks0, vs0 = _fp8_caches(job)
    k8, v8, ks, vs = k0.clone(), v0.clone(), ks0.clone(), vs0.clone()

    def launch(mk, ws):
        k8.copy_(k0); v8.copy_(v0); ks.copy_(ks0); vs.copy_(vs0)
        return ops.decode_attn_fused(job.qkv, job.cos, job.sin, job.lens, k8, v8, case.H, D.SCALE, job.bits, mk, ws, ks, vs)

    got = run_launches(job, launch, f"decode_attn_fused fp8-KV {job.what}")
    want = [a.clone() for a in (k0, v0, ks0, vs0)]
    for b, ln in enumerate(case.lens):          # the appended rows: the documented quantisation of the bf16-rounded rotated k and of v
        qk, sk = D.ref_quant(torch.from_numpy(job.k_new[b]))
        qv, sv = D.ref_quant(torch.from_numpy(job.v_new[b]))
        assert torch.equal(k8[b, :, ln].cpu(), qk) and torch.equal(ks[b, :, ln].cpu(), sk), f"appended k row of sample {b}"
        assert torch.equal(v8[b, :, ln].cpu(), qv) and torch.equal(vs[b, :, ln].cpu(), sv), f"appended v row of sample {b}"
        for w, a in zip(want, (k8, v8, ks, vs)):
            w[b, :, ln] = a[b, :, ln]
    for w, a, name in zip(want, (k8, v8, ks, vs), ("k bytes", "v bytes", "k scales", "v scales")):
        assert torch.equal(ibits(a), ibits(w)), f"{name}: an element outside the appended rows changed"
    stored = (D.deq(k8.cpu(), ks.cpu()), D.deq(v8.cpu(), vs.cpu()))
    check_rows(got, D.reference(case, job.inp, "fp8", stored), BF, f"decode_attn_fused fp8-KV {job.what}")


def test_a_workspace_one_item_short_is_refused(job):
    """Every split launch asks for the counters + S partials per (sample, head), S from plan(): exactly that is accepted, one item
    less raises AkiError (on the host, before any launch)."""
    from aki_amd import ops
    from aki_amd._lib import AkiError
    case = job.case
    k, v = job.appended(BF)
    q = torch.from_numpy(D.rotated_q(job.inp)).to(DEV).to(BF)
    k0, v0, ks0, vs0 = _fp8_caches(job)
    kf, vf = job.k.clone(), job.v.clone()
    calls = {
        "decode_attn": lambda mk, ws: ops.decode_attn(q, k, v, job.lens + 1, D.SCALE, job.bits, mk, ws),
        "decode_attn_fused": lambda mk, ws: ops.decode_attn_fused(job.qkv, job.cos, job.sin, job.lens, kf, vf, case.H, D.SCALE, job.bits, mk, ws),
        "decode_attn_fused fp8-KV": lambda mk, ws: ops.decode_attn_fused(job.qkv, job.cos, job.sin, job.lens, k0, v0, case.H, D.SCALE, job.bits,
                                                                         mk, ws, ks0, vs0),
    }
    for mk in case.max_keys_options():
        S = D.plan(case.B, case.H, case.cap, mk)[0]
        words = D.workspace_bytes_needed(case.B, case.H, S) // 4
        big = torch.full((words + 2 * GUARD,), POISON, dtype=torch.int32, device=DEV)
        ws = big[GUARD:GUARD + words]
        ws.zero_()
        for name, call in calls.items():
            with pytest.raises(AkiError):
                call(mk, ws[: words - 104])
            out = call(mk, ws)                  # exactly what plan() says is enough
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out.float()).all()), name
            assert bool((big[:GUARD] == POISON).all()) and bool((big[GUARD + words:] == POISON).all()), f"{name}: bytes outside the workspace changed"

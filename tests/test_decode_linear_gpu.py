"""Every case x input family of tests/decode_linear_cases.py on the device, against the float64 reference under the derived bar.

Each call goes through the C ABI (aki_linear_fwd / aki_decode_linear_fwd) with raw pointers: aki_amd.ops re-routes some shapes before
the ABI sees them (ops.decode_linear sends them to rmsnorm + linear) and has no res_row_mod or padded leading dimensions on the decode
entry points, and the ABI's own routing is what is under test.  Per case and family: the product library's result against the
reference (largest err / tol and its index printed and recorded before anything is asserted); the lab library's route log equal to
the table's records, so the route believed to have run is the route that ran; the lab launch and a second product launch bit-equal
to the first; the output inside poisoned guard rows, padded ldy columns keeping their poison; x, w, scales, bias, residual and gain
each followed by NaN inside the same allocation, so that a read past a tensor that is taken for data turns the output NaN while every
index stays inside an allocation.  Refused calls return their status and leave the output's poison intact.

The decode chain and the batched chain run the same kernels' phases and are tested bit-identical to these per-layer calls
(tests/test_decode_gpu.py); nothing new is needed for them."""
import numpy as np
import pytest
import torch

import decode_linear_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = D.GUARD_ROWS


@pytest.fixture(scope="module")
def libs():
    from aki_amd import _lib
    lab = _lib.load_lab()
    lab.aki_lab_set_gemm_tile(0)
    lab.aki_lab_set_decode_dry_run(0)
    lab.aki_lab_set_gemm_dry_run(0)
    lab.aki_lab_decode_log_reset()
    lab.aki_lab_gemm_log_reset()
    yield _lib.load(), lab
    lab.aki_lab_decode_log_reset()
    lab.aki_lab_gemm_log_reset()


def _padded(t, rows, ld, fill):
    """t [r, c] -> a [rows, ld] buffer filled with `fill` holding t in its top-left corner."""
    buf = torch.full((rows, ld), fill, dtype=t.dtype) if t.dtype != torch.uint8 else torch.full((rows, ld), 0x7F, dtype=torch.uint8)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.to(DEV)


def device_buffers(case, inp):
    """The operands with NaN (e4m3: 0x7f) behind every tensor and in every pad column; y: NaN everywhere."""
    M, N, K = case.shape
    ld = D.lds(case)
    nan = float("nan")
    b = D.NS()
    b.x = _padded(inp.x, M + G, ld.ldx, nan)
    b.w = _padded(inp.wq if case.w8 else inp.w, N + G, ld.ldw, nan)
    b.ws = torch.cat([inp.ws, torch.full((8,), nan)]).to(DEV) if case.w8 else None
    b.bias = torch.cat([inp.bias, torch.full((8,), nan, dtype=D.BF)]).to(DEV) if inp.bias is not None else None
    b.res = _padded(inp.res, max(ld.res_rows, 1) + G, ld.ldr, nan) if inp.res is not None else None
    b.gain = torch.cat([inp.gain, torch.full((8,), nan, dtype=D.BF)]).to(DEV) if inp.gain is not None else None
    return b


def launch(lib, case, b):
    """One call on a fresh, poisoned output buffer; returns (status, the whole buffer as float64 [G + M + G, ldy], its raw bits)."""
    M = case.shape[0]
    ld = D.lds(case)
    y = torch.full((G + M + G, ld.ldy), float("nan"), dtype=D.BF, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()
    args = D.make_args(case, ptr(b.x), ptr(b.w), ptr(b.bias), ptr(b.res), y.data_ptr() + G * ld.ldy * 2, ptr(b.ws))
    rc = D.call(lib, case, args, ptr(b.gain), torch.cuda.current_stream().cuda_stream)
    if rc == -5:                      # AKI_ERR_LAUNCH: nothing more is started on a device that has just failed a launch
        pytest.exit(f"{case.id}: the launch failed (status -5)", returncode=3)
    torch.cuda.synchronize()
    return rc, y.cpu().to(D.F64).numpy(), y.cpu().view(torch.int16).numpy()


@pytest.mark.parametrize("cid", D.RUN_IDS)
def test_case_against_float64(libs, cid):
    from aki_amd import _lib
    from conftest import record_parity
    lib, lab = libs
    case = D.by_id(cid)
    failures = []
    for family in D.families(case):
        inp = D.inputs(case, family)
        ref = D.reference(case, inp)
        b = device_buffers(case, inp)
        rc, got, bits = launch(lib, case, b)
        assert rc == 0, f"{cid} / {family}: status {rc}"
        r, at = D.worst(ref, got)
        err = np.nan_to_num(np.abs(got[G:G + case.shape[0], :case.n_out] - ref.y), nan=np.inf)
        print(f"\n{cid} / {family}: worst err / tol {r:.3f} at (row, feature) {at}; max err {err.max():.4g}; ties {ref.tie_share:.4%}")
        record_parity(f"decode linear {cid} / {family} vs float64 (err / tol {r:.3f})", torch.bfloat16, float(err.max()), float(err.mean()),
                      float(np.abs(ref.y).max()), "err <= half_ulp + KAPPA 2^-24 M(y) (tests/decode_linear_cases.py)")
        if not r <= 1.0:
            failures.append(f"{family}: err / tol {r:.3f} at {at}")
        if family == "one-hot" and not case.epilogue:
            want = D.one_hot_expected(case, inp).view(torch.int16).numpy()
            if not np.array_equal(bits[G:G + case.shape[0], :case.n_out], want):
                failures.append("one-hot: y is not w[n, k_m] bit for bit")
        lab.aki_lab_decode_log_reset()
        rc2, _, bits2 = launch(lab, case, b)
        records = _lib.decode_log(lab)
        lab.aki_lab_decode_log_reset()
        assert rc2 == 0 and records == list(case.expect), f"{cid} / {family}: the lab library logged {records}, the table says {list(case.expect)}"
        rc3, _, bits3 = launch(lib, case, b)
        assert rc3 == 0
        if not (np.array_equal(bits, bits2) and np.array_equal(bits, bits3)):
            failures.append(f"{family}: two launches (or the lab twin) differ bitwise")
    assert not failures, f"{cid}: " + "; ".join(failures)


@pytest.mark.parametrize("cid", [c.id for c in D.CASES if c.status != D.OK])
def test_refusal_returns_its_status_and_leaves_the_output_alone(libs, cid):
    lib, lab = libs
    case = D.by_id(cid)
    M, N, K = case.shape
    ld = D.lds(case)
    inp = D.NS(x=torch.ones((M, K), dtype=D.BF), w=torch.ones((N, K), dtype=D.BF), wq=torch.full((N, K), 0x38, dtype=torch.uint8),
               ws=torch.ones(N), bias=None, res=None, gain=torch.ones(K, dtype=D.BF) if case.norm else None)
    b = device_buffers(case, inp)
    lab.aki_lab_decode_log_reset()         # the lab library is shared by the whole session: earlier tests leave their launches in its logs
    lab.aki_lab_gemm_log_reset()
    for which in (lib, lab):
        rc, got, _ = launch(which, case, b)
        assert rc == case.status, f"{cid}: status {rc}, expected {case.status}"
        assert np.isnan(got).all(), f"{cid}: a refused call wrote to the output"
    assert lab.aki_lab_decode_log(None, 0) == 0 and lab.aki_lab_gemm_log(None, 0) == 0, f"{cid}: a refused call logged a launch"


def test_beyond_the_lds_limit_the_mfma_gemm_runs(libs):
    """The one shape of the table that leaves the decode kernels: its result is held to the same float64 reference (product only)."""
    from aki_amd import _lib
    lib, lab = libs
    case = next(c for c in D.CASES if c.gemm)
    M, N, K = case.shape
    rng = D.rng_of("beyond", case.id)
    inp = D.NS(x=D.bf(np.abs(rng.standard_normal((M, K)))), w=D.bf(np.abs(rng.standard_normal((N, K))) / K), wq=None, ws=None, bias=None, res=None, gain=None)
    b = device_buffers(case, inp)
    lab.aki_lab_decode_log_reset()
    lab.aki_lab_gemm_log_reset()
    rc, got, _ = launch(lab, case, b)
    assert rc == 0 and lab.aki_lab_decode_log(None, 0) == 0 and len(_lib.gemm_log(lab)) == 1
    lab.aki_lab_gemm_log_reset()
    y = D.f64(inp.x) @ D.f64(inp.w).T
    tol = 2.0 ** -8 * D.hb(np.abs(y)) + (K // 32 + 8) * D.EPS * np.abs(y) + D.FLOOR       # one rounding per 16x16x32 MFMA of the K loop
    out = got[G:G + M, :N]
    print(f"\n{case.id}: worst err / tol {(np.abs(out - y) / tol).max():.3f}")
    assert (np.abs(out - y) <= tol).all() and np.isnan(got[:G]).all() and np.isnan(got[G + M:]).all()

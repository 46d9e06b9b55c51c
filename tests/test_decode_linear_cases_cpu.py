"""The decode-linear planner and the case table of tests/decode_linear_cases.py without a GPU: every case reaches exactly its records in
dry-run mode (the lab library's route log, on fake pointers that are never dereferenced) and every refusal returns its status and logs
nothing; the cases cover every instantiation of the three kernel templates the product library exports; every structural corner is
reached; every mutation of the float64 reference is visible at MIN_RATIO; a plain float32 torch implementation stays inside every bar;
the share of normalised operands near a bf16 tie stays under the cap."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import decode_linear_cases as D


@pytest.fixture(scope="module")
def lab():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    lib = _lib.load_lab()
    yield lib
    lib.aki_lab_set_decode_dry_run(0)
    lib.aki_lab_set_gemm_dry_run(0)
    lib.aki_lab_decode_log_reset()
    lib.aki_lab_gemm_log_reset()


def _fmt(records):
    from aki_amd import _lib
    return "\n".join("  " + ", ".join(f"{k}={v}" for k, v in zip(_lib.DECODE_LOG_FIELDS, r)) for r in records) or "  (none)"


@pytest.mark.parametrize("cid", D.CASE_IDS)
def test_case_reaches_its_records(lab, cid):
    case = D.by_id(cid)
    rc, got, gemm = D.dry_run(lab, case)
    assert rc == case.status, f"{cid}: status {rc}, expected {case.status}"
    assert got == list(case.expect), f"{cid}: planned\n{_fmt(got)}\nexpected\n{_fmt(case.expect)}"
    assert bool(gemm) == case.gemm, f"{cid}: the MFMA GEMM's log shows {gemm}"
    if case.status != D.OK:
        assert not got and not gemm, f"{cid}: a refusal must log nothing"
    assert lab.aki_lab_decode_log(None, 0) == 0, "dry_run must leave the log empty"


def test_decode_log_counts_every_launch_and_resets(lab):
    from aki_amd import _lib
    case = D.by_id("skinny-ks4-m3")
    lab.aki_lab_set_decode_dry_run(1)
    try:
        lab.aki_lab_decode_log_reset()
        for _ in range(3):
            assert D.call(lab, case, D.make_args(case, *(D._fake(i) for i in range(1, 7))), D._fake(7)) == 0
        assert lab.aki_lab_decode_log(None, 0) == 3
        assert _lib.decode_log(lab, cap=4) == list(case.expect) * 3
        with pytest.raises(_lib.AkiError):
            _lib.decode_log(lab, cap=2)
        lab.aki_lab_decode_log_reset()
        assert lab.aki_lab_decode_log(None, 0) == 0
    finally:
        lab.aki_lab_set_decode_dry_run(0)
        lab.aki_lab_decode_log_reset()


def _nm():
    for tool in ("llvm-nm", "/opt/rocm/llvm/bin/llvm-nm", "nm"):
        path = shutil.which(tool) or (tool if os.path.isabs(tool) and os.path.exists(tool) else None)
        if path:
            return path
    pytest.fail("no nm / llvm-nm on this machine")


def product_instantiations():
    from aki_amd import _lib
    out = subprocess.run([_nm(), "-C", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set()
    for m in re.finditer(r"aki::(gemv_bf16_kernel|skinny_gemm_bf16_kernel|skinny_gemm_w8_kernel)<([^>]*)>\(aki::GemvParams\)", out):
        args = [a.strip() for a in m.group(2).split(",")]
        found.add((m.group(1), tuple(1 if a == "true" else 0 if a == "false" else int(a) for a in args)))
    return found


# Instantiations removed by this table's first run: gemv_bf16_kernel<3..8, false, 4> sat behind a run-time `M <= 2` on a template constant in
# launch_gemv (now `if constexpr`).  None is left that the planner cannot reach, so the list of named exceptions is empty.
UNREACHABLE = {}
REMOVED = [("gemv_bf16_kernel", (m, 0, 4, 0)) for m in range(3, 9)]


def test_cases_cover_every_product_instantiation(lab):
    have = product_instantiations()
    covered = {D.kernel_of(r) for c in D.CASES for r in c.expect}
    per = {name: (len({k for k in have if k[0] == name}), len({k for k in covered if k[0] == name}))
           for name in ("gemv_bf16_kernel", "skinny_gemm_bf16_kernel", "skinny_gemm_w8_kernel")}
    print(f"\ndecode-linear table: {len(D.CASES)} cases; product instantiations exported / covered: {per}; "
          f"named unreachable: {sorted(UNREACHABLE)}; removed from the library: {REMOVED}")
    assert len(have) >= 40, f"only {len(have)} symbols of the three templates found: did the symbols survive the link?"
    assert covered - have == set(), f"cases name kernels the product library does not have: {sorted(covered - have)}"
    assert have - covered - set(UNREACHABLE) == set(), f"product kernels no case reaches: {sorted(have - covered - set(UNREACHABLE))}"
    assert not set(REMOVED) & have, "an instantiation listed as removed is back in the library"


def test_every_structural_corner_is_reached():
    corners = D.corners()
    missing = [name for name, ids in corners.items() if not ids]
    print(f"\n{len(corners)} structural corners, each reached by at least one case")
    assert not missing, f"corners no case reaches (retune the table in tests/decode_linear_cases.py): {missing}"


_REF = {}


def ref_of(cid, family):
    """(inputs, unmutated reference) computed once per (case, family) and shared."""
    key = (cid, family)
    if key not in _REF:
        case = D.by_id(cid)
        inp = D.inputs(case, family)
        _REF[key] = (inp, D.reference(case, inp))
    return _REF[key]


@pytest.mark.parametrize("cid", D.RUN_IDS)
def test_float32_implementation_sits_inside_the_bar_and_ties_are_rare(cid):
    case = D.by_id(cid)
    for family in D.families(case):
        inp, ref = ref_of(cid, family)
        got = D.f32_impl(case, inp)
        r, at = D.worst(ref, D.image_of(case, got.to(D.F64).numpy()))
        assert r <= 1.0, f"{cid} / {family}: the float32 implementation is at {r:.3f} of the bar at {at}"
        assert ref.tie_share <= D.TIE_CAP, f"{cid} / {family}: {ref.tie_share:.4%} of the normalised operands sit near a bf16 tie"
        if family == "one-hot" and not case.epilogue:
            want = D.one_hot_expected(case, inp)
            assert np.array_equal(D._bf16_round(ref.y), want.to(D.F64).numpy()), f"{cid}: the reference is not w[n, k_m] bit for bit"
        _REF.pop((cid, family), None) if case.shape[1] * case.shape[2] > (1 << 22) else None


@pytest.mark.parametrize("mut", sorted(D.MUTATIONS))
def test_mutation_is_visible(mut):
    best = {}
    for cid, family in D.MUTATIONS[mut]:
        case = D.by_id(cid)
        inp, ref = ref_of(cid, family)
        wrong = D.reference(case, inp, mut=mut)
        r, at = D.worst(ref, wrong.image)
        best[(cid, family)] = r
        need = D.CAPPED.get(mut, D.MIN_RATIO)
        assert r >= need, f"{mut} on {cid} / {family}: only {r:.2f} x the bar (at {at}); needed {need}"
    print(f"\n{mut}: " + ", ".join(f"{c}/{f} {r:.3g}x" for (c, f), r in best.items()))

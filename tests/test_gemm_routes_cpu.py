"""The GEMM planner without a GPU: every entry of tests/gemm_routes.py reaches exactly its expected launches (the lab library's route
log in dry-run mode, on fake pointers that are never dereferenced), the entries cover every gemm_bf16_kernel instantiation of the
product library, and the split-K fallbacks (workspace too small or misaligned, row_shift) hold."""
import os
import re
import shutil
import subprocess

import pytest

import gemm_routes as R


@pytest.fixture(scope="module")
def lab():
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib
    lib = _lib.load_lab()
    lib.aki_lab_set_gemm_tile(0)
    yield lib
    lib.aki_lab_set_gemm_dry_run(0)
    lib.aki_lab_gemm_log_reset()


def _fmt(records):
    return "\n".join("  " + ", ".join(f"{k}={v}" for k, v in zip(("NF", "NT", "WN", "WM", "EPI", "ACT", "FP8", "NST", "PIPE", "SK", "ksplit", "M",
                                                                       "m_offset", "grid"), r)) for r in records)


@pytest.mark.parametrize("rid", R.ROUTE_IDS)
def test_route_reaches_its_launches(lab, rid):
    route = R.by_id(rid)
    got = R.dry_run(lab, route)
    assert got == list(route.expect), f"{rid}: planned\n{_fmt(got)}\nexpected\n{_fmt(route.expect)}"
    if route.opt("residual"):
        got8 = R.dry_run(lab, route, res8=True)
        want8 = list(route.expect_res8 or route.expect)
        assert got8 == want8, f"{rid} (residual 8-byte aligned): planned\n{_fmt(got8)}\nexpected\n{_fmt(want8)}"
    assert lab.aki_lab_gemm_log(None, 0) == 0, "dry_run must leave the log empty"


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
    for m in re.finditer(r"aki::gemm_bf16_kernel<([^>]*)>\(aki::GemmParams\)", out):
        args = [a.strip() for a in m.group(1).split(",")]
        found.add(tuple(1 if a == "true" else 0 if a == "false" else int(a) for a in args))
    return found


def test_routes_cover_every_product_instantiation(lab):
    """A kernel added to the planner without a route entry (or an entry whose kernel left the library) fails here.  The host
    symbols are the launchable set: the device code also holds the 64-feature four-stage QKV kernel, which launch_small names but
    never launches (its 64-feature branch excludes EPI_QKV_ROPE8 at run time), and the optimiser drops that host stub."""
    have = product_instantiations()
    covered = {R.kernel_of(r) for route in R.ROUTES for r in route.expect + (route.expect_res8 or ())}
    print(f"\nroute table: {len(R.ROUTES)} entries cover {len(covered)} gemm_bf16_kernel instantiations; "
          f"the product library exports {len(have)}")
    assert len(have) >= 30, f"only {len(have)} gemm_bf16_kernel symbols found: did the symbols survive the link?"
    assert covered - have == set(), f"route entries name kernels the product library does not have: {sorted(covered - have)}"
    assert have - covered == set(), f"product kernels no route entry reaches: {sorted(have - covered)}"


SPLITK = [r for r in R.ROUTES if r.uses_splitk]


@pytest.mark.parametrize("rid", [r.id for r in SPLITK])
def test_splitk_falls_back_when_the_workspace_does_not_fit(lab, rid):
    route = R.by_id(rid)
    M, N, K = route.shape
    need = lab.aki_linear_splitk_workspace_bytes(M, N, K)
    assert need > 0
    split = R.dry_run(lab, route, splitk_bytes=need)
    assert split == list(route.expect), "the exact workspace size must be enough"
    for what, kw in (("one byte short", dict(splitk_bytes=need - 1)), ("tickets only", dict(splitk_bytes=64 << 10)),
                     ("128-byte aligned", dict(splitk_bytes=need + 256, splitk_offset=128)), ("none", dict(splitk_bytes=0))):
        got = R.dry_run(lab, route, **kw)
        assert len(got) == 1 and got[0][9] == 0 and got[0][10] == 1, f"{rid}, workspace {what}: {_fmt(got)}"
        assert got[0][11] == M and got[0][12] == 0


@pytest.mark.parametrize("rid", [r.id for r in SPLITK])
def test_row_shift_never_takes_splitk(lab, rid):
    route = R.by_id(rid)
    opts = dict(route.opts, fold="ln")
    opts.pop("stats", None)
    got = R.dry_run(lab, R.Route(rid + "+row_shift", route.entry, route.shape, (), opts))
    assert got and all(r[9] == 0 and r[10] == 1 for r in got), _fmt(got)
    opts["fold"] = "rms"       # row_scale alone keeps the split
    assert R.dry_run(lab, R.Route(rid + "+row_scale", route.entry, route.shape, (), opts)) == list(route.expect)


def test_gemm_log_counts_every_launch_and_resets(lab):
    pair = R.by_id("plan2-ring64-row-mod")
    lab.aki_lab_set_gemm_dry_run(1)
    try:
        lab.aki_lab_gemm_log_reset()
        for _ in range(3):
            assert R._call(lab, pair, None, 0, False) == 0
        from aki_amd import _lib
        assert lab.aki_lab_gemm_log(None, 0) == 6
        assert _lib.gemm_log(lab, cap=8) == list(pair.expect) * 3
        with pytest.raises(_lib.AkiError):
            _lib.gemm_log(lab, cap=4)
        lab.aki_lab_gemm_log_reset()
        assert lab.aki_lab_gemm_log(None, 0) == 0
    finally:
        lab.aki_lab_set_gemm_dry_run(0)
        lab.aki_lab_gemm_log_reset()

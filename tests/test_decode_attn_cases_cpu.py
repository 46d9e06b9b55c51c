"""The decode attention case table (tests/decode_attn_cases.py) is checked here, without a GPU: every corner of the launch plan is
reached by a case, and every mutation of the float64 reference - a key left out, a masked column let in, a tile or an item dropped,
a merge weight taken from the neighbouring item, RoPE one position early, the appended row taken from the stale cache - moves at
least one output element of the sample by MIN_RATIO = 8 times the tolerance the GPU test grants at that element, in the input family
meant to catch it.  This is a condition on the inputs, not a measurement of the kernels: a kernel with one of these faults cannot
pass tests/test_decode_attn_gpu.py.  Run with -s to see, per case, (S, T), the smallest ratio and the corners reached."""
import numpy as np
import pytest

import decode_attn_cases as D


def test_plan_restates_the_launch_arithmetic():
    assert D.dec_items() > 0
    items = D.dec_items()
    # T from the capacity, S from max_keys; max_keys = 0 or past the capacity means the capacity
    assert D.plan(1, 32, 64, 0) == (1, 1) and D.plan(1, 32, 64, 1) == (1, 1) and D.plan(1, 32, 64, 1000) == (1, 1)
    B, H, cap = 8, 32, 1100
    T = -(-B * H * 18 // items)
    assert D.plan(B, H, cap, 0) == (-(-18 // T), T) and D.plan(B, H, cap, 193) == (-(-4 // T), T)
    assert D.plan(2, 2, 4200, 4097) == (65, 1) or items != 2048


def test_every_corner_of_the_plan_is_reached_by_a_case():
    reached = {}
    for c in D.CASES:
        P = D.properties(c)
        S_full, T = D.plan(c.B, c.H, c.cap, 0)
        S_eager = D.plan(c.B, c.H, c.cap, max(c.lens) + 1)[0]
        print(f"{c.id}: T = {T}, S = {S_eager} (max_keys = max(lens) + 1) / {S_full} (max_keys = 0): {', '.join(sorted(P))}")
        for p in P:
            reached.setdefault(p, c.id)
        for part in c.id.split("-"):                        # the plan named in the id is the plan the launch takes
            if part[0] == "T" and part[1:].isdigit():
                assert int(part[1:]) == T, f"{c.id}: T = {T}"
            if part[0] == "S" and part[1:].isdigit():
                assert int(part[1:]) in (S_full, S_eager), f"{c.id}: S = {S_eager} / {S_full}"
    missing = [p for p in D.REQUIRED if p not in reached]
    assert not missing, f"no case reaches: {missing}"
    # the two max_keys options must differ somewhere in S (trailing empty items), or the bit-identity check compares a launch with itself
    assert any(D.plan(c.B, c.H, c.cap, 0)[0] != D.plan(c.B, c.H, c.cap, max(c.lens) + 1)[0] for c in D.CASES)


def test_inputs_are_finite_where_cached_and_poisoned_past_the_append_position():
    c = D.CASE_BY_ID["b4-h2-cap320-T1-S5-lens64-65-319-200-leftpad64-hole-across-word-whole-word"]
    for fam in D.FAMILIES:
        inp = D.make_inputs(c, fam)
        for b, ln in enumerate(c.lens):
            assert bool(inp.k[b, :, :ln].float().isfinite().all()) and bool(inp.v[b, :, :ln].float().isfinite().all())
            assert bool(inp.k[b, :, ln:].float().isnan().all()) and bool(inp.v[b, :, ln:].float().isnan().all())
        assert bool(inp.qkv.float().isfinite().all())
        ref = D.reference(c, inp)
        assert np.isfinite(ref).all() and 0.05 < np.abs(ref).max() < 100
    # sentinel family: the sentinels hold most of the mass, about equally; masked columns would outweigh all of them
    b = 1
    t = D.sample_terms(inp, b)
    share = t.kw[:, inp.sent[b]] / t.kw.sum(1, keepdims=True)
    assert share.sum(1).min() > 0.85 and share.max() / share.min() < 1.5
    assert (t.w[:, 58:65] > 20 * t.kw.max(1, keepdims=True)).all() and float(inp.v[b, :, 58:65].float().min()) == D.MASKED_V


def test_a_row_without_a_visible_key_is_zeros_in_the_reference():
    c = D.CASE_BY_ID["b2-h2-cap128-T1-S2-lens70-5-no-visible-key-all-before-masked"]
    for fam in D.FAMILIES:
        inp = D.make_inputs(c, fam)
        ref = D.reference(c, inp)
        assert (ref[0] == 0).all()
        # everything before the new token masked: the output is the new v row
        assert np.allclose(ref[1], D.appended_rows(inp)[1][1].reshape(-1).astype(np.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_every_mutation_of_the_reference_clears_the_bar_eight_times(case):
    inps = {fam: D.make_inputs(case, fam) for fam in D.FAMILIES}
    applied = set()
    for view in D.VIEWS:
        worst = {}
        for b in range(case.B):
            R = {fam: D.mutation_ratios(inps[fam], b, view) for fam in D.FAMILIES}
            for name, (meant, _) in D.MUTATIONS.items():
                assert R["diffuse"][name].keys() == R["sentinel"][name].keys(), "applicability is a rule of the table, not of the draw"
                for label in R["diffuse"][name]:
                    r = max(R[fam][name][label] for fam in D.FAMILIES) if meant == "either" else R[meant][name][label]
                    if name not in worst or r < worst[name][0]:
                        worst[name] = (r, b, label)
                    applied.add(name)
        low = min(worst, key=lambda k: worst[k][0])
        print(f"{case.id} [{view}] (S, T) = {D.plan(case.B, case.H, case.cap, 0)}: smallest ratio {worst[low][0]:.1f} ({low}: sample "
              f"{worst[low][1]}, {worst[low][2]}); " + ", ".join(f"{k} {v[0]:.0f}" for k, v in sorted(worst.items())))
        bad = {k: v for k, v in worst.items() if not v[0] >= D.MIN_RATIO}
        assert not bad, f"{case.id} [{view}]: mutations the inputs would let through: {bad}"
    assert {"n_keys-1", "drop-sentinel", "stale-v"} <= applied


def test_every_mutation_applies_to_some_case():
    # cheap: applicability only needs small cases; the large ones are covered by the parametrised test above
    seen = set()
    for c in D.CASES:
        if c.B * c.H * c.cap > 40000:
            continue
        inp = D.make_inputs(c, "sentinel")
        for b in range(c.B):
            seen |= {k for k, v in D.mutation_ratios(inp, b, "bf16").items() if v}
    assert seen == set(D.MUTATIONS), set(D.MUTATIONS) - seen


def test_report_the_same_mutations_on_the_old_inputs():
    """Reported, not asserted: q, K, V ~ N(0, 1) (K, V ~ 2 N(0, 1) for the fp8 sweep), the lengths of
    test_decode_attn_fused_vs_two_kernels and of the fp8 n_keys sweep, hole 3:7.  Worst element's error as a multiple of its
    tolerance, minimum over four seeds - the table in the module docstring of decode_attn_cases.py in numbers."""
    H = 4
    for kv_scale, lengths in ((1.0, (18, 201, 299, 64, 656, 4101)), (2.0, (65, 655, 4096))):
        for n in lengths:
            res = {}
            for seed in range(4):
                rng = np.random.default_rng(1000 * n + seed)
                q = D.bf16(rng.standard_normal((H, D.DH))).astype(np.float64)
                K = D.bf16(rng.standard_normal((H, n, D.DH)) * kv_scale).astype(np.float64)
                V = D.bf16(rng.standard_normal((H, n, D.DH)) * kv_scale).astype(np.float64)
                keep = np.ones(n, dtype=bool)
                keep[3:7] = False
                t = D.Terms(q, K, V, keep)
                ref = t.out()
                tol = D.tolerance(ref)
                muts = {"new token's key left out": t.with_columns([n - 1], -1)[0], "one key in the middle left out": t.with_columns([n // 2], -1)[0],
                        "mask ignored": D.Terms(q, K, V, np.ones(n, dtype=bool)).out(), "first tile left out": t.without_groups(1)[0],
                        "bf16 rounding of the output": D.bf16(ref).astype(np.float64)}
                for k, o in muts.items():
                    res.setdefault(k, []).append(float((np.abs(o - ref) / tol).max()))
            print(f"N(0,1) x {kv_scale:g}, n = {n}: " + ", ".join(f"{k} {min(v):.2f}" for k, v in res.items()))

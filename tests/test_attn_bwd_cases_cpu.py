"""The attention-backward case table (tests/attn_bwd_cases.py) is checked here, without a GPU: the closed-form float64 reference
agrees with float64 autograd on every case, every named corner is reached by a case, the derived bar is attainable (the reference
rounded to bf16 stays inside it), and every mutation of the reference moves some output element by MIN_RATIO = 8 times its
tolerance in at least one case and family (the one mutation the bar itself caps - see the module docstring - by CAPPED).  This is a
condition on the inputs, not a measurement of the kernels.  Run with -s to see the ratios."""
import numpy as np
import pytest

import attn_bwd_cases as A

MUTATION_MAX_L = 340          # the mutation table is evaluated on the cases up to this length: every corner exists there


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case, family):
        key = (case.id, family)
        if key not in cache:
            inp = A.make_inputs(case, family)
            cache[key] = (inp, A.reference(inp))
        return cache[key]
    return get


@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_reference_against_float64_autograd_and_its_own_bar(case, refs):
    for family in A.FAMILIES:
        inp, S = refs(case, family)
        for b, s in enumerate(S):
            o, dq, dk, dv = A.autograd_f64(inp, b)
            for name, want in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
                got = getattr(s, name)
                assert np.isfinite(got).all()
                assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), f"{case.id} [{family}] sample {b}: {name}"
                # the bar is attainable: a bf16 round trip of the exact result stays inside it
                assert (np.abs(A.bf16(got).astype(np.float64) - got) <= s.tol(name)).all(), f"{case.id} [{family}] sample {b}: {name} after a bf16 round trip"
            # rows that see nothing and keys that nothing sees have exactly zero gradient
            assert (s.dq[:, ~s.live] == 0).all() and (s.dk[:, ~s.vis.any(0)] == 0).all() and (s.dv[:, ~s.vis.any(0)] == 0).all()
            assert s.score_terms() <= A.MAX_SCORE_TERMS, f"{case.id} [{family}]: scores too large for the e_P term of the derivation"


def test_every_named_corner_is_reached_by_a_case():
    reached = {}
    for c in A.CASES:
        assert c.why
        assert 1 <= c.B <= 3 and 1 <= c.H <= 3
        for p in A.properties(c):
            reached.setdefault(p, c.id)
    missing = [p for p in A.REQUIRED if p not in reached]
    assert not missing, f"no case reaches: {missing}"
    assert sum(c.B != c.H for c in A.CASES) > len(A.CASES) // 2
    assert max(c.Lq for c in A.CASES) <= 700 and max(c.Lk for c in A.CASES) <= 900
    # a workgroup with no needed tile at all: a query block and a key block wholly at or past seq_len
    c = A.CASE_BY_ID["L257-b3-h2-two-rects-above-diagonal-empty-blocks"]
    assert not c.visible(2)[A.BLK:].any() and not c.visible(2)[:, A.BLK:].any()
    # the tile sizes the table is aimed at are the kernels'
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aki_amd", "csrc", "attn_bwd_bf16.hip")).read()
    assert "kb0 + wave * 32 + l31" in src and "* 128;" in src and "t * 32 + 31 >= kb0" in src and "t * 32 <= q0 + 127" in src


def test_sentinels_hold_their_rows_and_forbidden_pairs_would_dominate(refs):
    c = A.CASE_BY_ID["L333-b2-h3-four-and-eight-rects-ragged"]
    inp, S = refs(c, "sentinel")
    for b, s in enumerate(S):
        rows = sorted({r for r, _ in inp.pairs[b]})
        share = np.zeros((c.H, len(rows)))
        for i, r in enumerate(rows):
            cols = [k for rr, k in inp.pairs[b] if rr == r]
            share[:, i] = s.P[:, r, cols].sum(-1)
        assert np.median(share) > 0.8 and share.min() > 0.2, (b, share.min(), np.median(share))
        assert inp.forbidden[b]
        for r, k in inp.forbidden[b]:
            assert not s.vis[r, k]
            if s.live[r]:
                assert (np.exp(s.s[:, r, k] - s.lse[:, r]) > 0.3).all(), (r, k)     # a leak would take a quarter of the row's mass or more
            assert float(inp.v[b, :, k].float().min()) == A.FORBIDDEN_V


def test_every_mutation_is_visible_in_some_case_and_family(refs):
    best = {n: (0.0, "") for n in A.MUTATIONS}
    for c in A.CASES:
        if max(c.Lq, c.Lk) > MUTATION_MAX_L:
            continue
        for family in A.FAMILIES:
            inp, S = refs(c, family)
            for b, s in enumerate(S):
                for name, res in A.mutation_ratios(s, inp).items():
                    for label, r in res.items():
                        if r > best[name][0]:
                            best[name] = (r, f"{c.id} [{family}] sample {b}: {label}")
    for name, (r, where) in sorted(best.items()):
        print(f"{name}: {r:.1f}  ({where})")
    bad = {n: v for n, v in best.items() if not v[0] >= A.CAPPED.get(n, A.MIN_RATIO)}
    assert not bad, f"mutations the inputs would let through: {bad}"


def test_edge_mutations_are_visible_in_every_case_they_apply_to(refs):
    """The single-pair faults at a case's own edges - the diagonal, each rectangle edge moved by one either way, row seq_len - 1, row
    seq_len, a hole's edge columns - clear MIN_RATIO in EVERY case that has that edge (in the sentinel or the diffuse family), not
    just in one: each case's edges sit at different offsets inside the tiles."""
    names = ("diagonal-excluded", "row_lo+1", "row_hi-1", "col_lo+1", "col_hi-1", "col_hi+1", "row_hi+1", "row-seq_len-1-skipped",
             "row-seq_len-included", "hole-edge-visible", "column-after-hole-hidden")
    for c in A.CASES:
        if max(c.Lq, c.Lk) > MUTATION_MAX_L or not c.masked:
            continue
        per = {}
        for family in A.FAMILIES:
            inp, S = refs(c, family)
            for b, s in enumerate(S):
                for name, res in A.mutation_ratios(s, inp, names).items():
                    for label, r in res.items():
                        per[(name, b, label)] = max(per.get((name, b, label), 0.0), r)
        bad = {k: v for k, v in per.items() if not v >= A.MIN_RATIO}
        assert not bad, f"{c.id}: {bad}"

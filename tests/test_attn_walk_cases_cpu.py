"""The multi-rank case table of the attention forward (tests/attn_walk_cases.py) is checked here, without a GPU: walk_plan restates the
launchers (it agrees with ranks_per_workgroup and with the geometry the table is aimed at), every required hand-over property is reached by
a case and the two that the decomposition excludes are shown to be excluded, the replicated-heads identity is exact, the distinct pair
counts stay under the cap, the sentinel keys reach the tiles a rank re-issues, the rising family's ranks fail and pass where the table
says, and every mutation of the reference leaves the bar by MIN_RATIO on every case it applies to (or is listed in CAPPED with its reason).
A condition on the table, not a measurement of the kernels.  Run with -s to see the ratios."""

import numpy as np
import pytest
import torch

import attn_bwd_cases as A
import attn_fwd_cases as F
import attn_walk_cases as W

_INP = {}


def inputs(case, family):
    if (case.id, family) not in _INP:
        _INP[(case.id, family)] = W.make_inputs(case, family)
    return _INP[(case.id, family)]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _INP.clear()
    W._REFS.clear()


def test_walk_plan_agrees_with_ranks_per_workgroup_and_covers_every_block_once():
    for case in W.CASES:
        for core in ("32", "64"):
            for cus in (256, 304, 128, 64, 8):
                for dr in (1, 0):
                    pl = W.walk_plan(case, core, cus, dr)
                    assert max(len(w) for w in pl.walks) == W.ranks_per_workgroup(case.B, case.H, case.Lq, core, cus), (case.id, core, cus)
                    assert sorted(g for w in pl.walks for g in w) == list(range(pl.nqt)), "the snake visits every rank of a pair once"
                    for b in range(case.B):
                        blocks = sorted(bl for r in pl.ranks[b] for bl in r.blocks if bl >= 0)
                        assert blocks == list(range((case.Lq + 31) // 32)), "every 32-row block belongs to one rank"
    # fewer compute units only lower splits: ranks per workgroup never shrink
    for case in W.CASES:
        for core in W.cores(case):
            n = [max(len(w) for w in W.walk_plan(case, core, cus).walks) for cus in (304, 256, 208, 128, 64)]
            assert n == sorted(n), (case.id, n)


def test_geometry_the_table_is_aimed_at():
    """nqt, splits, group_bh and the walks of every case at 256 compute units, re-derived from walk_plan."""
    g = lambda cid, core: W.walk_plan(W.CASE_BY_ID[cid], core)
    geo = lambda pl: (pl.nqt, pl.splits, pl.group_bh, pl.last_group, sorted(len(w) for w in pl.walks))
    assert geo(g("bench-655", "32")) == (6, 2, 256, 256, [3, 3]) and g("bench-655", "32").walks == [[0, 3, 4], [1, 2, 5]]
    assert geo(g("bench-655", "64")) == (3, 1, 256, 256, [3])
    assert geo(g("uneven-655", "32")) == (6, 4, 128, 128, [1, 1, 2, 2])
    assert geo(g("short-group-655", "32")) == (6, 2, 256, 8, [3, 3])
    assert geo(g("one-split-200", "32")) == (2, 1, 512, 512, [2])
    kc = W.WC
    lo, hi = W.CASE_BY_ID[f"below-min-{kc['MIN_L'] - 1}"], W.CASE_BY_ID[f"min-{kc['MIN_L']}"]
    assert W.product_core(lo) == "32" and W.product_core(hi) == "64" and W.routes(lo) == W.routes(hi) == ("product",)
    assert geo(W.walk_plan(lo, "32")) == (14, 8, 64, 64, [1, 1, 2, 2, 2, 2, 2, 2]) and W.walk_plan(lo, "32").sched and (lo.Lq + 31) // 32 == 56
    assert geo(W.walk_plan(hi, "64")) == (7, 3, 88, 8, [2, 2, 3])
    assert geo(g("rise-1856", "64")) == (8, 3, 88, 8, [2, 3, 3]) and g("rise-1856", "64").walks == [[0, 5, 6], [1, 4, 7], [2, 3]]
    p = g("position-4160", "64")
    assert geo(p) == (17, 16, 16, 16, [1] * 15 + [2]) and not p.sched and p.walks[15] == [15, 16]
    assert p.ranks[0][16].blocks == tuple(range(8)) and p.ranks[0][15].blocks == tuple(range(8, 16)) and p.ranks[0][0].blocks == (128, 129) + (-1,) * 6
    # block extents and the ranking on hand-checked samples of the benchmark mask (32-row core)
    c = W.CASE_BY_ID["bench-655"]
    p1, p0 = W.walk_plan(c, "32", dead_rows=1), W.walk_plan(c, "32", dead_rows=0)
    assert p1.ranks[0][0].blocks == (20, 19, 4, 3) and p1.ranks[0][0].ext == (655, 640, 638, 638) and [r.jend for r in p1.ranks[0]] == [11, 10, 9, 7, 5, 3]
    assert p1.ranks[0][5].blocks == (5, -1, -1, -1)
    # sample 3: no rectangle, seq_len 512: under the uniform convention the blocks of rows >= 512 walk all L columns, later block first
    assert p1.ranks[3][0].blocks == (20, 19, 18, 17) and p1.ranks[3][0].ext == (655,) * 4 and p1.ranks[3][1].blocks == (16, 15, 14, 13) and p1.ranks[3][1].ext[:2] == (655, 512)
    assert p0.ranks[3][0].ext == (655, 640, 608, 576) and p0.ranks[3][5].blocks == (0, -1, -1, -1) and p0.ranks[3][5].jend == 1
    for case in W.CASES:
        assert case.why and case.Dh == 96 and case.H % W.HB == 0 and case.H // W.HB <= len(W.SCALES)
        assert W.distinct_pairs(case) <= W.MAX_PAIRS, f"{case.id}: {W.distinct_pairs(case)} distinct query-key pairs"
    assert len(set(W.SCALES)) == len(W.SCALES) == 16


def test_every_required_property_is_reached_and_the_excluded_ones_are_excluded():
    reached = {}
    for c in W.CASES:
        for p in W.properties(c):
            reached.setdefault(p, c.id)
    for p in W.REQUIRED:
        print(f"{p}: {reached.get(p)}")
    missing = [p for p in W.REQUIRED if p not in reached]
    assert not missing, f"no case reaches: {missing}"
    assert not set(W.UNREACHABLE) & set(reached) and not set(W.UNREACHABLE) & set(W.REQUIRED)
    # why the two cannot be reached: a ranked walk never grows, and in position order a rank of one or two tiles is the pair's last
    for c in W.CASES:
        for core in ("32", "64"):
            for dr in (1, 0):
                pl = W.walk_plan(c, core, dead_rows=dr)
                for b in range(c.B):
                    je = [r.jend for r in pl.ranks[b]]
                    if pl.sched:
                        assert je == sorted(je, reverse=True), (c.id, core, je)
                    else:
                        assert all(j > 2 for j in je[:-1]), (c.id, core, je)
    # the rising table against itself: every walk of the case is classified
    c = W.CASE_BY_ID["rise-1856"]
    assert {"rise:fail->pass", "rise:pass->fail", "rise:fail->fail", "rise:failing-last-rank"} <= W.rise_patterns(c)


def test_replicated_heads_are_exactly_a_scaled_base_reference():
    """o = s 2^e o_base, tol = 2^e tol_base, lse = lse_base with max |diff| = 0 in float64, against a reference computed for all H heads."""
    case = A._m("identity-100", 2, 8, 100, [[(6, 40, 40, 90)], [W.Z]], [[(50, 55)], [(0, 3), (80, 100)]], [100, 80], why="small")
    for family in ("diffuse", "sentinel"):
        ref = W.Reference(case, family)
        q, k, v = W.expand(ref.inp, case)
        for h in range(case.H):
            assert torch.equal(q[:, h], ref.inp.q[:, h % W.HB]) and torch.equal(k[:, h], ref.inp.k[:, h % W.HB])
        assert len({(h % W.HB, W.SCALES[h // W.HB]) for h in range(case.H)}) == case.H
        direct = F.Reference(F.Inputs(case, family, q, k, v, ref.inp.pairs, ref.inp.forbidden))
        dead = False
        for b in range(case.B):
            for dr in (1, 0):
                for core in ("32", "64"):
                    o, t_o, lse, t_l, live = ref.expected(b, core, dr)
                    o_d, _, _, live_d = direct.expected(b, dr)
                    td_o, td_l = direct.tol(b, core, dr)
                    assert np.array_equal(live, live_d)
                    assert np.abs(o - o_d).max() == 0.0 and np.abs(t_o - td_o).max() == 0.0, (family, b, dr, core)
                    assert np.array_equal(lse, direct.S[b].lse) and np.abs(t_l - td_l).max() == 0.0
            dead = dead or bool((~live).any())
        assert dead, "the identity is checked on dead rows too"


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_sentinel_keys_reach_the_tiles_a_rank_reissues(case):
    """Every 32-row block of every later-walked rank holds sentinel keys on both sides of the edges of tiles 0, 1, 2 and in the last tile of its
    rank's stream, as far as rows of the block see them; and the inputs meet the conditions of the bar's derivation."""
    inp = inputs(case, "sentinel")
    bc = inp.case
    for b in range(case.B):
        vis = F.vis_of(bc, b)
        pairs = set(inp.pairs[b])
        _, _, reached = W.walk_pairs(case, b)
        targets = W.walk_targets(case, b)
        assert targets, "a case without a later-walked rank"
        for bl, keys in targets.items():
            rows = [r for r in range(32 * bl, min(32 * bl + 32, case.seq_len(b))) if vis[r].any()]
            for kx in keys:
                if isinstance(kx, tuple):
                    t = kx[1]
                    if any(vis[r, 64 * t:64 * t + 64].any() for r in rows):
                        assert kx in reached.get(bl, ()), (case.id, b, bl, kx)
                        assert any((r, c) in pairs for r in range(32 * bl, 32 * bl + 32) for c in range(64 * t, min(64 * t + 64, case.Lk)))
                elif any(vis[r, kx] for r in rows):
                    assert kx in reached.get(bl, ()), (case.id, b, bl, kx)
                    assert any((r, kx) in pairs for r in range(32 * bl, 32 * bl + 32))
        rows = sorted({r for r, _ in inp.pairs[b]} | {r for r, _ in inp.forbidden[b]})
        R = F.forward_rows(inp, b, rows)
        assert R.terms <= F.MAX_SCORE_TERMS, f"{case.id} sample {b}: sum |q k| scale = {R.terms:.1f}"
        at = {r: i for i, r in enumerate(rows)}
        q, k = inp.q[b].double().numpy(), inp.k[b].double().numpy()
        share = []
        for r in sorted({r for r, _ in inp.pairs[b]}):
            cols = [c for rr, c in inp.pairs[b] if rr == r]
            assert len(cols) + sum(rr == r for rr, _ in inp.forbidden[b]) <= W.MAX_TARGETS
            s = np.einsum("hd,hkd->hk", q[:, r], k[:, cols]) * bc.scale
            share.append(np.exp(s - R.lse[:, at[r], None]).sum(-1))
        share = np.array(share)
        assert np.median(share) > 0.8 and share.min() > 0.2, (case.id, b, share.min(), np.median(share))
        for r, c in inp.forbidden[b]:
            assert not vis[r, c] and float(inp.v[b, :, c].float().min()) == F.FORBIDDEN_V
    d = inputs(case, "diffuse")
    for b in range(case.B):
        assert F.forward_rows(d, b, list(range(0, case.Lq, 97))).terms <= F.MAX_SCORE_TERMS


def test_rising_ranks_fail_and_pass_where_the_table_says():
    """From the float64 scores, with the first tile's maximum as reference: a rank "fails" when some row sum is >= 2^64 (required here: >= 2^68),
    "passes" when all are < 2^60; the walks then hold fail -> pass, pass -> fail, fail -> fail and a failing last rank.  The lifted keys lie beyond
    the first tile of every lifted row, and the three +-2^x keys of the first tile hold a checkable share of M_o on the lifted rows."""
    kc = W.WC
    case = W.CASE_BY_ID["rise-1856"]
    par = W.RISE[case.id]
    inp = inputs(case, "rising")
    pl = W.walk_plan(case, "64")
    assert par["band"][0] >= 64 and par["lift"] == 72.0 and par["min_row"] >= par["band"][1] + 64
    seen = set()
    for b in range(case.B):
        R = F.forward_rows(inp, b)
        excess = (R.lse - R.m0) / np.log(2.0)                                     # [HB, L] log2 of the row sum against the first tile's maximum
        assert np.isfinite(excess).all()
        v = inp.v[b].double().numpy()
        for hb_ in range(W.HB):
            rows = W.rise_rows(case, b, hb_)
            assert len(rows) and rows.min() >= par["min_row"]
            assert (inp.q[b, hb_, :, -1].float().numpy() != 0).nonzero()[0].tolist() == rows.tolist()
            fails = {}
            for r in pl.ranks[b]:
                rr = np.concatenate([np.arange(32 * bl, min(32 * bl + 32, case.Lq)) for bl in r.blocks if bl >= 0])
                e = excess[hb_, rr].max()
                assert e >= kc["SUM_LOG2"] + 4 or e < kc["SUM_LOG2"] - 4, (b, hb_, r.g, e)
                fails[r.g] = e >= kc["SUM_LOG2"]
            assert {g for g, f in fails.items() if f} == set(par["fail"][b][hb_]), (b, hb_, fails)
            for w in pl.walks:
                seen.update(f"{'fail' if fails[a] else 'pass'}->{'fail' if fails[c] else 'pass'}" for a, c in zip(w, w[1:]))
                if fails[w[-1]]:
                    seen.add("failing-last-rank")
            sent = list(W.RISE_SENT)
            q, k = inp.q[b, hb_].double().numpy(), inp.k[b, hb_].double().numpy()
            s = (q[rows] @ k[sent].T) * inp.case.scale
            share = (np.exp(s - R.lse[hb_, rows, None]) * np.abs(v[hb_, sent, 0])).sum(-1) / R.M[hb_, rows, 0]
            print(f"{case.id} sample {b} base head {hb_}: first-tile share median {np.median(share):.2f}, 5th percentile {np.percentile(share, 5):.2f}")
            assert 0.3 <= np.median(share) <= 0.7 and np.percentile(share, 5) >= 0.1
    assert {"fail->pass", "pass->fail", "fail->fail", "failing-last-rank"} <= seen, seen


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_every_mutation_is_visible_on_every_case_it_applies_to(case):
    best = {}
    for family in W.families(case):
        ctx = W.Ctx(case, family, inputs(case, family))
        for b in range(min(case.B, 4)):                                           # (the masks of the 655 cases repeat from sample 4 on)
            for core in W.cores(case):
                for name, res in W.mutation_ratios(ctx, b, core).items():
                    for label, r in res.items():
                        best[name] = max(best.get(name, 0.0), r)
    for name, r in sorted(best.items()):
        print(f"{case.id}: {name}: {r:.1f}" + (f"  (capped: {W.CAPPED[name][1]})" if name in W.CAPPED else ""))
    need = set(W.MUTATIONS) - ({n for n in W.MUTATIONS if n.startswith("rising:")} if case.id not in W.RISE else set())
    assert need <= set(best), f"{case.id}: found no place for: {sorted(need - set(best))}"
    bad = {k: v for k, v in best.items() if not v >= (W.CAPPED[k][0] if k in W.CAPPED else W.MIN_RATIO)}
    assert not bad, f"{case.id}: mutations the inputs would let through: {bad}"
    for k in W.CAPPED:
        if k in best:
            assert best[k] < W.MIN_RATIO, f"{k} is visible after all ({best[k]:.1f}): take it out of CAPPED"

"""The case table of tests/gemm_tn_cases.py checked on the CPU: every structural edge of aki_gemm_tn reached (from the constants parsed out of
gemm_tn_bf16.hip), the exact family exact, every mutation of the reference outside the bar, a plain float32 product inside both bars, and
every case but the refusal twin admitted by train_ops._tn_ok.  Nothing of the near-4g case is allocated beyond its compact operands."""
import numpy as np
import pytest

import gemm_tn_cases as G

K = G.kernel_constants()
_ids = lambda cs: [c.id for c in cs]


def test_constants_are_the_ones_the_table_was_aimed_at():
    assert K == dict(TN_BI=256, TN_BJ=256, TN_BK=64, GM=8, UNROLL_AHEAD=7, UNROLL=6, FULL_AHEAD=2, A_RING=3, B_RING=2), f"re-aim the cases: {K}"


def test_step_counts_and_loop_structure_are_reached():
    nks = {c.nk for c in G.STEP_CASES}
    assert nks == {1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14} and all(c.I == K["TN_BI"] and c.J == K["TN_BJ"] for c in G.STEP_CASES)
    assert {c.nk % K["UNROLL"] for c in G.RUN_CASES if c.nk > K["UNROLL_AHEAD"]} == set(range(K["UNROLL"]))
    count = lambda nk: tuple(G.loops(nk, K).count(w) for w in ("unrolled", "full", "last"))
    assert count(1) == (0, 0, 1) and count(2) == (0, 0, 2)                  # nk = 2: stage_a(1, 1) is the last stage, no FULL step
    for nk in (4, 6, 7):                                                    # the run-time loops alone, aslot all the way round
        u, f, l = count(nk)
        assert u == 0 and f + l == nk >= K["A_RING"] + 1 and f >= 2
    assert count(7) == (0, 5, 2) and count(8) == (6, 0, 2)                  # the last nk without, the first with the unrolled block
    assert count(9) == (6, 1, 2) and count(13) == (6, 5, 2) and count(14) == (12, 0, 2)
    for nk in range(1, 40):
        assert len(G.loops(nk, K)) == nk
    assert max(c.Kc for c in G.SMALL_CASES) <= 896


def test_k_tails_are_reached():
    assert {c.Kc % K["TN_BK"] for c in G.RUN_CASES} >= {0, 1, 8, 32, 33, 63}
    assert {1, 63, 64} <= {c.Kc for c in G.RUN_CASES}


def test_tile_tails_and_mapping_are_reached():
    sizes = {8, 16, 120, 136, 248, 256, 264, 520}
    assert sizes <= {c.I for c in G.RUN_CASES} and sizes <= {c.J for c in G.RUN_CASES}
    assert any(c.I < 16 and c.J > K["TN_BJ"] for c in G.RUN_CASES) and any(c.J < 16 and c.I > K["TN_BI"] for c in G.RUN_CASES)
    grids = {c.grid for c in G.RUN_CASES}
    assert {1, 2, 7, 8, 9} <= grids and any(g >> 3 >= 2 and g & 7 not in (0, 1) for g in grids)
    shapes = {(c.tiles_i, c.tiles_j) for c in G.RUN_CASES}
    assert {9, 11} <= {s[0] for s in shapes if s[1] == 1} | {s[0] for s in shapes if s[1] == 3}
    assert any(s[0] in (9, 11) and s[1] == 1 for s in shapes) and any(s[0] in (9, 11) and s[1] == 3 for s in shapes)
    assert all(c.Kc <= 72 for c in G.RUN_CASES if c.id.startswith("grid"))
    for g in grids:                                                        # the remap and the tile decode are bijections onto the tiles
        assert sorted(G.xcd_remap(b, g) for b in range(g)) == list(range(g))
    for c in G.RUN_CASES:
        tiles = {G.tile_of(t, c.tiles_i, c.tiles_j, K["GM"]) for t in range(c.grid)}
        assert tiles == {(i, j) for i in range(c.tiles_i) for j in range(c.tiles_j)}, c


def test_store_paths_and_layouts_are_reached():
    full = lambda c: c.I % K["TN_BI"] == 0 and c.J % K["TN_BJ"] == 0
    seen = {(c.wide, c.ldc > c.J, full(c)) for c in G.SMALL_CASES}
    assert seen == {(w, p, f) for w in (False, True) for p in (False, True) for f in (False, True)}
    narrow = [c for c in G.SMALL_CASES if not c.wide]
    assert any(c.ldc % 8 for c in narrow) and any(c.ldc % 8 == 0 and (c.c_off * 2) % 16 == 8 for c in narrow)
    for c in G.SMALL_CASES:
        assert c.ldc % 4 == 0 and (c.c_off * 2) % 8 == 0 and c.ldc >= c.J
        for name in (c.la, c.lb):
            o = G.OPERANDS[name]
            assert o["col0"] % 8 == 0 and o["pad"] % 8 == 0 and o["row0"] >= 1 and o["below"] >= K["TN_BK"] and o["pad"] >= o["col0"]
    pairs = {(c.la, c.lb) for c in G.SMALL_CASES}
    kind = lambda n: n.rstrip("16")
    assert {(kind(a), kind(b)) for a, b in pairs} >= {(x, y) for x in ("whole", "cols", "rows") for y in ("whole", "cols", "rows")}


def test_the_case_near_4_gib_is_where_it_should_be():
    c, twin = G.CASE_BY_ID["near-4g"], G.CASE_BY_ID["near-4g-twin"]
    BK = K["TN_BK"]
    assert c.lda == c.ldb == G.LD_BIG and G.LD_BIG & (G.LD_BIG - 1) and G.LD_BIG % 8 == 0
    assert (1 << 32) - 8192 < c.span_a < 1 << 32 and c.span_b == c.span_a and not c.refused
    assert BK * c.nk * c.lda * 2 > 1 << 32 and c.Kc % BK
    assert twin.Kc == c.Kc + 1 and twin.span_a >= 1 << 32 and twin.refused
    for r in range(c.Kc, BK * c.nk):                                        # the wrapped offsets point at P_WRAP: rows of data, beside both views
        assert r * c.lda * 2 >= 1 << 32
        for which in "ab":
            row, col = G.wrap_target(c, which, r)
            assert 1 <= row <= c.Kc and col + 8 <= G.LD_BIG and all(col + 8 <= G.shared_cols(w) or col >= G.shared_cols(w) + 8 for w in "ab")
    assert G.shared_cols("a") % 8 == 0 and G.shared_cols("b") % 8 == 0


class Layout:
    """What _tn_ok reads of a tensor."""

    def __init__(self, rows, cols, ld, byte_offset):
        self.shape, self._ld, self._ptr = (rows, cols), ld, 4096 + byte_offset

    def stride(self, d):
        return (self._ld, 1)[d]

    def data_ptr(self):
        return self._ptr


def test_tn_ok_admits_every_case_but_the_twin():
    from aki_amd import train_ops as TO
    for c in G.CASES:
        if c.shared:
            a, b = (Layout(c.Kc, n, G.LD_BIG, (G.LD_BIG + G.shared_cols(w)) * 2) for n, w in ((c.I, "a"), (c.J, "b")))
        else:
            oa, ob = G.OPERANDS[c.la], G.OPERANDS[c.lb]
            a = Layout(c.Kc, c.I, c.lda, (oa["row0"] * c.lda + oa["col0"]) * 2)
            b = Layout(c.Kc, c.J, c.ldb, (ob["row0"] * c.ldb + ob["col0"]) * 2)
        assert TO._tn_ok(a, b) == (not c.refused), c
    assert [c.id for c in G.CASES if c.refused] == ["near-4g-twin"]


@pytest.mark.parametrize("c", G.RUN_CASES, ids=_ids(G.RUN_CASES))
def test_exact_family_is_exact_and_float32_is_inside_both_bars(c):
    for fam in G.FAMILIES:
        inp = G.inputs(c, fam)
        ref = G.reference(c, inp, fam)
        a, b = G.f64(inp.a), G.f64(inp.b)
        if fam == "exact":
            assert set(np.unique(a)) <= {-1.0, 0.0, 1.0} and np.abs(ref.x).max() <= G.EXACT_MAX
            assert a.any(1).all() and b.any(1).all(), f"{c}: a contraction row that cannot be seen"
            assert 0.4 < np.abs(a).mean() < 0.7 or c.I <= 16
            assert (ref.tol() == 0).all()
            assert np.array_equal(G.product_f32(inp), ref.x), f"{c}: the float32 product is not exact"
        else:
            if fam == "one-sign":
                assert np.array_equal(ref.M, np.abs(ref.x))
            w = ref.worst(G.product_f32(inp))
            assert w <= 1.0, f"{c} [{fam}]: the float32 product is at {w:.3f} of the bar"


@pytest.mark.parametrize("m", list(G.MUTATIONS))
def test_mutations_break_the_bar(m):
    bar, pairs = G.MUTATIONS[m]
    assert pairs
    fams = [f for f in G.FAMILIES if G.bar_of(f) == bar]
    cache = {}
    for cid, arg in pairs:
        c = G.CASE_BY_ID[cid]
        best = 0.0
        for fam in fams:
            if (cid, fam) not in cache:
                inp = G.inputs(c, fam)
                cache[(cid, fam)] = (inp, G.reference(c, inp, fam))
            inp, ref = cache[(cid, fam)]
            best = max(best, ref.worst(G.mutate(c, inp, m, arg)))
        print(f"{m} on {cid}{'' if arg is None else f' [{arg}]'}: {best:.3g} of the bar")
        assert best >= G.MIN_RATIO, f"mutation {m} on {cid} [{arg}] reaches only {best:.2f} of the bar"


def test_stale_slots_are_tried_in_every_loop_and_every_row_class_is_dropped():
    BK = K["TN_BK"]
    for mut, depth in (("stale-a", K["A_RING"]), ("stale-b", K["B_RING"])):
        seen = {G.loops(G.CASE_BY_ID[cid].nk, K)[kt] for cid, kt in G.MUTATIONS[mut][1]}
        assert seen == {"unrolled", "full", "last"}, (mut, seen)
        assert all(kt >= depth for _, kt in G.MUTATIONS[mut][1])
    for c in G.STEP_CASES:
        rows = {r for cid, r in G.MUTATIONS["drop-row"][1] if cid == c.id}
        want = {0, 3, 4, 7, 8, 31, 32, 63} | {BK * k for k in range(1, c.nk)} | {c.Kc - 1, BK * (c.nk - 1)}
        assert rows == {r for r in want if r < c.Kc}, c
    assert any(G.CASE_BY_ID[cid].shared for cid, _ in G.MUTATIONS["k-tail-leak"][1])

"""The attention-forward case table (tests/attn_fwd_cases.py) is checked here, without a GPU: the row-blocked float64 reference agrees
with a dense float64 softmax and with attn_bwd_cases.Sample, every named corner is reached by a case, the inputs meet the conditions the
derivation of the bar assumes (score-term sums, the rising family's margins to 2^64 on both sides, sentinel shares), every
mutation of the reference moves some compared element by MIN_RATIO = 8 times its tolerance, in some family, on every case it applies
to, and so does every mutation of the address rule in every layout of the plain route.  A condition on the table, not a measurement of the kernels.  Run with -s to see the ratios."""
import numpy as np
import pytest
import torch

import attn_bwd_cases as A
import attn_fwd_cases as F

MASKED = [c for c in F.CASES if c.masked]
_INP = {}


def inputs(case, family):
    if (case.id, family) not in _INP:
        _INP[(case.id, family)] = F.make_inputs(case, family)
    return _INP[(case.id, family)]


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    _INP.clear()
    F._REFS.clear()


@pytest.mark.parametrize("case", [c for c in F.CASES if max(c.Lq, c.Lk) <= 700], ids=lambda c: c.id)
def test_blocked_reference_equals_a_dense_float64_softmax(case):
    for family in F.families(case):
        ref = F.reference(case, family)
        for b, s in enumerate(ref.S):
            o, lse = F.dense_f64(ref.inp, b)
            assert np.abs(s.o - o).max() <= 1e-12 * max(1.0, np.abs(o).max()), (case.id, family, b)
            assert np.abs(s.lse - lse).max() <= 1e-12 * max(1.0, np.abs(lse).max())
            assert s.terms <= F.MAX_SCORE_TERMS, f"{case.id} [{family}]: scores too large for the e_P term of the derivation"
            # the bar is attainable: a bf16 round trip of the exact result stays inside it
            assert (np.abs(F.bf16(s.o).astype(np.float64) - s.o) <= ref.tol(b, "32")[0]).all()


def test_blocked_reference_equals_the_backward_suites_sample_on_a_shared_case(monkeypatch):
    case = A.CASE_BY_ID["L333-b2-h3-four-and-eight-rects-ragged"]
    inp = A.make_inputs(case, "sentinel")
    monkeypatch.setattr(F, "ROWS_PER_BLOCK", 100)                                # four blocks, the last one partial
    for b, S in enumerate(A.reference(inp)):
        R = F.forward_rows(inp, b)
        assert (R.n > 0).tolist() == S.live.tolist()
        assert np.abs(R.o - S.o).max() <= 1e-12 * np.abs(S.o).max() and np.abs(R.M - S.M_o).max() <= 1e-12 * S.M_o.max()
        assert (R.lse[:, ~S.live] == -np.inf).all() and np.abs(R.lse[:, S.live] - S.lse[:, S.live]).max() <= 1e-12 * np.abs(S.lse[:, S.live]).max()
        assert abs(R.terms - S.score_terms()) <= 1e-9
        # a subset of rows under a changed visibility is the dense result of that visibility
        rows = np.array([0, 5, 131, 259, 332])
        vis = case.visible(b, seq_of=(b + 1) % case.B)[rows]
        R2 = F.forward_rows(inp, b, rows, vis)
        with np.errstate(invalid="ignore"):
            P = np.where(vis[None], np.exp(S.s[:, rows] - np.where(vis[None], S.s[:, rows], -np.inf).max(-1, keepdims=True)), 0.0)
        l = P.sum(-1, keepdims=True)
        want = np.where(l > 0, P / np.where(l > 0, l, 1.0), 0.0) @ S.v
        assert np.abs(R2.o - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_every_named_corner_is_reached_by_a_case():
    kc = F.kernel_constants()
    # the lengths aimed at AKI_ATTN64_MIN_L and kSchedMax are made from them; the seam cases sit on the 64-row core's own limits
    assert 32 * kc["SCHED64"] == F.SEAM == 64 * F.TILE, f"the 64-row core's ranked-block limit left the seam of its mask windows: re-aim the 4096 / 4097 cases ({kc})"
    reached = {}
    for c in F.CASES:
        assert c.why
        assert c.H <= 2 or max(c.Lq, c.Lk) <= 2048
        assert c.Dh == (96 if c.masked else c.Dh) and (c.masked or c.Dh in (72, 32, 64, 96))
        for p in F.properties(c):
            reached.setdefault(p, c.id)
    missing = [p for p in F.REQUIRED if p not in reached]
    assert not missing, f"no case reaches: {missing}"
    # routes: every masked case through the shipped 64-row build; the 32-row core up to 2100 rows; the every-tile-exact build on the seam and
    # rising cases; the product rule from one row below its boundary
    for c in MASKED:
        r = F.routes(c)
        assert "64" in r and ("32" in r) == (c.Lq <= 2100 and c.id not in F.RISING) and ("164" in r) == (c.Lq > F.SEAM or c.id in F.RISING)
        assert ("product" in r) == (c.Lq >= kc["MIN_L"] - 1)
    assert F.product_core(F.CASES[0]) == "32" and F.product_core(F.CASES[1]) == "64"
    kv = F.CASE_BY_ID[F.KV_CACHE_CASE]
    assert kv.Lq > F.SEAM and kv.Lq % 64 != 0 and kv.B * kv.H > 1              # a partial last tile past the seam, a head stride that counts
    assert sorted(F.dead_conventions(F.CASE_BY_ID["L2300-b2-h2-ragged-mid-tile-and-tile-edge"])) == [0, 1]
    # the zero convention reaches both cores
    assert any(0 in F.dead_conventions(c) and "32" in F.routes(c) for c in MASKED) and any(0 in F.dead_conventions(c) and "64" in F.routes(c) for c in MASKED)
    # no case makes a persistent workgroup walk a second rank (module docstring); the many-heads shape of test_attn64_gpu.py does
    for c in MASKED:
        assert all(F.ranks_per_workgroup(c.B, c.H, c.Lq, "64" if r != "32" else "32") == 1 for r in F.routes(c)), c.id
    assert F.ranks_per_workgroup(1, 32, 4096, "64") == 2 and F.ranks_per_workgroup(2, 32, 4096, "64") == 4
    assert F.ranks_per_workgroup(3, 2, 4096, "64") == 1 and F.ranks_per_workgroup(1, 18, 4096, "64") == 2


def test_dead_rows_and_their_lse_pattern():
    c = F.CASE_BY_ID["L2300-b2-h2-ragged-mid-tile-and-tile-edge"]
    ref = F.reference(c, "sentinel")
    for b in range(c.B):
        Ls = c.seq_len(b)
        o1, M1, n1, live = ref.expected(b, 1)
        o0, M0, _, _ = ref.expected(b, 0)
        assert not live[Ls:].any() and live[:Ls].all()
        v = ref.inp.v[b].double().numpy()
        assert np.allclose(o1[:, Ls:], v.mean(1)[:, None]) and np.allclose(M1[:, Ls:], np.abs(v).mean(1)[:, None]) and (n1[Ls:] == c.Lk).all()
        assert (o0[:, Ls:] == 0).all() and (M0[:, Ls:] == 0).all() and (ref.tol(b, "64", 0)[0][:, Ls:] == 0).all()
        assert (ref.S[b].lse[:, Ls:] == -np.inf).all()
        assert F.lse_pattern(c, b, 1).all() and (F.lse_pattern(c, b, 0) == live).all()
    c = F.CASE_BY_ID["L1856-b2-h1-leftpad-137-and-195-hole-later"]
    for b, pad in enumerate((137, 195)):                                          # rows inside seq_len that see nothing: -inf under both conventions
        for dr in (0, 1):
            pat = F.lse_pattern(c, b, dr)
            assert not pat[:pad].any() and pat[pad:].all()


@pytest.mark.parametrize("case", MASKED + [c for c in F.CASES if not c.masked and c.Lk >= 257], ids=lambda c: c.id)
def test_inputs_meet_the_conditions_of_the_derivation(case):
    """Score-term sums <= 64 outside the rising family; sentinels hold their rows and a leak would dominate; the rising family's row sums
    against the first tile's maximum keep a margin of 2^4 to the kernel's 2^64 on either side and its first tile a checkable share."""
    kc = F.kernel_constants()
    for family in F.families(case):
        inp = inputs(case, family)
        for b in range(case.B):
            if family == "rising":
                R = F.forward_rows(inp, b)
                rows = np.arange(F.RISE_KEY + 64, case.Lq)
                excess = (R.lse[:, rows] - R.m0[:, rows]) / np.log(2.0)           # log2 of the row sum against the first tile's maximum
                assert np.isfinite(excess).all()
                if F.RISING[case.id] < kc["SUM_LOG2"]:
                    assert ((R.lse - R.m0) / np.log(2.0)).max() <= kc["SUM_LOG2"] - 4, "a row sum too close to 2^64: the rank might be walked again"
                    assert excess.min() >= 30, "the later tiles do not beat the first tile's maximum"
                else:
                    assert excess.min() >= kc["SUM_LOG2"] + 4, "a lifted row's sum too close to 2^64: the rank might stay blind"
                    early = (R.lse[:, :F.RISE_KEY - 256] - R.m0[:, :F.RISE_KEY - 256]) / np.log(2.0)
                    assert early[:, 160:].max() <= 20, "the ranks ahead of the lift must stay blind"
                v = inp.v[b].double().numpy()
                sent = list(F.RISE_SENT)
                q, k = inp.q[b].double().numpy(), inp.k[b].double().numpy()
                s = np.einsum("hqd,hkd->hqk", q[:, rows], k[:, sent]) * case.scale
                share = (np.exp(s - R.lse[:, rows, None]) * np.abs(v[:, sent, 0])[:, None]).sum(-1) / R.M[:, rows, 0]
                print(f"{case.id}: first-tile share median {np.median(share):.2f}, 5th percentile {np.percentile(share, 5):.2f}, v = 2^{np.log2(abs(v[0, sent[0], 0])):.0f}")
                assert 0.3 <= np.median(share) <= 0.7 and np.percentile(share, 5) >= 0.1
                continue
            rows = sorted({r for r, _ in inp.pairs[b]} | {r for r, _ in inp.forbidden[b]}) if family == "sentinel" else list(range(0, case.Lq, 97))
            R = F.forward_rows(inp, b, rows)
            assert R.terms <= F.MAX_SCORE_TERMS, f"{case.id} [{family}] sample {b}: sum |q k| scale = {R.terms:.1f}"
            if family != "sentinel":
                continue
            at = {r: i for i, r in enumerate(rows)}
            q, k = inp.q[b].double().numpy(), inp.k[b].double().numpy()
            share = []
            for r in sorted({r for r, _ in inp.pairs[b]}):
                cols = [c for rr, c in inp.pairs[b] if rr == r]
                assert len(cols) + sum(rr == r for rr, _ in inp.forbidden[b]) <= F.max_targets(case)
                s = np.einsum("hd,hkd->hk", q[:, r], k[:, cols]) * case.scale
                share.append(np.exp(s - R.lse[:, at[r], None]).sum(-1))
            share = np.array(share)
            assert np.median(share) > 0.8 and share.min() > 0.2, (case.id, b, share.min(), np.median(share))
            assert inp.forbidden[b] or not case.masked
            for r, c in inp.forbidden[b]:
                assert not F.vis_of(case, b)[r, c] and float(inp.v[b, :, c].float().min()) == F.FORBIDDEN_V
                if np.isfinite(R.lse[:, at[r]]).all():
                    s = np.einsum("hd,hd->h", q[:, r], k[:, c]) * case.scale
                    assert (np.exp(s - R.lse[:, at[r]]) > 0.3).all(), (r, c)     # a leak would take a quarter of the row's mass or more


PLAIN = [c for c in F.CASES if not c.masked]


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c.id)
def test_layouts_hold_the_same_values_where_the_product_puts_them(case):
    """Every layout of the plain route gives back the inputs bit for bit through the kernel's address rule; the strides are SigLIP's and
    the Perceiver's; what the call does not name is adversarial; nothing is placed where attn_nc_bf16 would refuse it."""
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.Dh
    assert F.layouts(case) == (F.LAYOUTS if Lq == Lk else ("heads", "heads+spare", "q+kv"))
    for family in F.families(case):
        inp = inputs(case, family)
        for layout in F.layouts(case):
            P = F.place(inp, layout)
            q, k, v = P.views()
            F.check_views(P, (q, k, v))
            assert q.shape == (B, Lq, H, D) and k.shape == v.shape == (B, Lk, H, D)
            assert all(torch.equal(a, b_) for a, b_ in zip(F.gather(P), (inp.q, inp.k, inp.v))), (case.id, family, layout)
            assert all(torch.equal(a.permute(0, 2, 1, 3), b_) for a, b_ in zip((q, k, v), (inp.q, inp.k, inp.v)))
            rows = Lk + (F.SPARE if layout != "heads" else 0)
            if layout in ("heads", "heads+spare"):
                assert k.stride() == v.stride() == (H * rows * D, D, rows * D, 1) and q.stride() == (H * Lq * D, D, Lq * D, 1)
            elif layout == "qkv":
                assert q.stride() == k.stride() == v.stride() == (rows * 3 * H * D, 3 * H * D, D, 1)
                assert k.storage_offset() - q.storage_offset() == v.storage_offset() - k.storage_offset() == H * D
            else:
                assert q.stride() == (Lq * H * D, H * D, D, 1) and k.stride() == v.stride() == (rows * 2 * H * D, 2 * H * D, D, 1)
                assert v.storage_offset() - k.storage_offset() == H * D
            if layout == "heads":
                assert P.lead == 0 and k.storage_offset() == 0
                continue
            assert P.lead == (B > 1) and (B == 1 or k.storage_offset() // k.stride(0) == 1)
            assert B == 1 or k.stride(0) != Lk * k.stride(1)                     # the batch stride is not the product of the view's sizes
            # behind key Lk - 1: SPARE rows with the forbidden value, row Lk at LEVEL + LIFT against the last row's q (sentinel family)
            kf, vf = (F.gather(P, "keys-past-Lk-visible")[i] for i in (1, 2))
            assert kf.shape[2] == Lk + F.SPARE > Lk + F.TILE and F.SPARE % F.TILE and (vf[:, :, Lk:].float() == F.FORBIDDEN_V).all()
            if family == "sentinel":
                s = (inp.q[:, :, Lq - 1].double() * kf[:, :, Lk].double()).sum(-1) * case.scale
                assert (s - (np.log(100.0 * Lk) + F.LIFT)).abs().max() <= 0.1, (case.id, layout, s)
            if B > 1:                                                            # the leading sample: sample 0's keys under the forbidden value
                lead_v = P.bufs["v"][0, :, :Lk] if layout == "heads+spare" else P.bufs["qkv" if layout == "qkv" else "kv"][0, :Lk, -1]
                assert (lead_v.float() == F.FORBIDDEN_V).all()


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_every_mutation_is_visible_on_every_case_it_applies_to(case):
    assert len(F.CAPPED) <= 1 and not set(F.CAPPED) & set(F.PER_KEY)
    best = {}
    for family in F.families(case):
        inp = inputs(case, family)
        for b in range(case.B):
            for dr in F.dead_conventions(case):
                for name, res in F.mutation_ratios(inp, b, dead_rows=dr).items():
                    for label, r in res.items():
                        key = (name, b, label.split(":")[0] if family == "rising" else label)
                        best[key] = max(best.get(key, 0.0), r)
    got = {k[0] for k in best}                                                   # (the layout mutations below have a need-list of their own)
    for layout in F.layouts(case):                                               # the plain route: a gather that misreads the buffers
        seen = set()
        for family in F.families(case):
            for name, res in F.layout_mutation_ratios(inputs(case, family), layout).items():
                seen.add(name)
                for b, r in res.items():
                    best[(name, b, layout)] = max(best.get((name, b, layout), 0.0), r)
        want = {"head-h-reads-head-h+1"} if case.H > 1 else set()
        want |= {"batch-stride-ignored"} if case.B > 1 else set()
        want |= {"keys-past-Lk-visible", "one-key-past-Lk-visible"} if layout != "heads" else set()
        want |= {"v-read-from-k-slot"} if layout in ("qkv", "q+kv") else set()
        assert seen == want, f"{case.id} [{layout}]: layout mutations {sorted(seen)}, expected {sorted(want)}"
    for (name, b, label), r in sorted(best.items()):
        print(f"{case.id} sample {b}: {name}: {r:.1f}  ({label})")
    bad = {k: v for k, v in best.items() if not v >= F.CAPPED.get(k[0], F.MIN_RATIO)}
    assert not bad, f"{case.id}: mutations the inputs would let through: {bad}"
    if case.id in F.RISING:
        assert got == set(F.RISING_MUTATIONS)
        return
    need = {"key-dropped:below-tile-edge", "key-dropped:above-tile-edge"}
    if any(F.vis_of(case, b)[:, case.Lk - 1].any() for b in range(case.B)):
        need |= {"key-dropped:last-key"}
    if case.masked:
        need |= {"key-dropped:rect-last-column", "key-leaked:col_hi", "key-leaked:after-diagonal", "tile-dropped:first-of-rank", "rows-r-and-r+32-swapped"}
        if any(case.valid(b)[:64].any() for b in range(case.B)):
            need |= {"lse-against-first-tile"}
        if case.Lq > F.SEAM:
            need |= {"tile-dropped:tile-64"}
            if all(case.valid(b)[F.SEAM - 1:F.SEAM + 1].all() for b in range(case.B)):             # (L = 5000 has its hole there)
                need |= {"key-dropped:4095", "key-dropped:4096"}
        if case.holes and any(case.holes):
            need |= {"key-leaked:in-hole"}
        if case.seq_lens:
            need |= {"key-leaked:row-seq_len", "seq_len-of-other-sample", "dead-rows-mean-over-valid-only"}
        if case.B > 1:
            need |= {"rects-of-other-sample"}
            if any((case.visible(b, valid_of=(b + 1) % case.B) != F.vis_of(case, b)).any() for b in range(case.B)):
                need |= {"bits-of-other-sample"}
    elif case.Lk < 257:
        need = {"key-dropped:last-key"}
    assert need <= got, f"{case.id}: found no edge for: {sorted(need - got)}"

"""The device sampler's case table, checked with the reference alone (tests/sampling_cases.py; no GPU)."""
import numpy as np
import pytest
import torch

import sampling_cases as S


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()                                    # cross-compiles for gfx950 without a GPU
    from aki_amd import _lib
    return _lib.load()


def test_philox_known_answers():
    for ctr, key, want in S.PHILOX_KAT:
        assert S.philox4x32_10(ctr, key) == want, (ctr, key)
    for n, b, o, seed in ((0, 0, 0, 0), (7, 3, 21, S.SEED), (0xFFFFFFFF, 0xFFFFFFFF, (1 << 64) - 1, (1 << 64) - 1), (24, 7, 1 << 20, 5)):
        want = S.philox4x32_10((n, b, o & 0xFFFFFFFF, o >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
        assert int(S.philox_word0(n, b, o, seed)) == want
    u = S.uniform(*S.draws())
    assert u.shape == (len(S.OFFSETS), S.STEPS, S.ROWS) and u.size >= 2000 and 0.0 < u.min() and u.max() < 1.0
    assert len(np.unique(u)) > 0.99 * u.size


def test_the_table_covers_what_it_should():
    cs = S.cases()
    assert len({c.name for c in cs}) == len(cs)
    main = [c for c in cs if c.kind == "normal" and not c.processed and c.V == S.V_MAIN]
    assert {(c.sigma, c.T, c.k, c.p) for c in main} == {(s, T, k, p) for s in (2.0, 4.0) for T in (0.7, 1.0, 1.3) for k in (0, 1, 50, 1000)
                                                         for p in (1.0, 0.9, 0.5, 1e-6)}
    assert any(c.V % 8 for c in cs) and any(c.processed and c.V % 8 for c in cs) and sum(c.processed for c in cs) >= 8
    assert any(c.kind == "neg_inf" for c in cs)
    ties = [c for c in cs if c.kind == "ties" and 0 < c.k]
    assert ties
    for c in ties:                                          # the top-k threshold is a value several tokens share
        r = S.reference(c, mutation=None)
        y = np.sort(r.y)[::-1]
        assert (r.y == y[c.k - 1]).sum() > 1 and S.reference(S.Case(c.name, c.V, c.sigma, c.T, c.k, 1.0, c.kind, salt=c.salt)).kept.sum() > c.k


@pytest.mark.parametrize("c", S.cases(), ids=lambda c: c.name)
def test_conditions_on_the_inputs(c):
    ok, f = S.conditions_hold(c)
    assert ok, f
    assert f["gap"] > S.DELTA and f["mean_gap"] <= S.MAX_MEAN_GAP
    if f["kept"] <= 1000:
        assert f["multi"] <= 0.02, f
    elif not c.filtered:
        assert f["multi"] <= 0.15, f
    r = S.reference(c)
    assert r.kept[np.argmax(r.y)] and abs(r.probs.sum() - 1.0) < 1e-12
    # the reference's own draw is accepted, for every draw
    u = S.uniform(*S.draws(c))
    assert S.accepted(r, S.reference_tokens(r, u), u).all()


@pytest.mark.parametrize("c", S.cases(), ids=lambda c: c.name)
def test_f32_in_the_kernels_order_is_within_half_delta(c):
    r = S.reference(c)
    err = np.abs(S.f32_cdf_in_kernel_order(r) - r.cdf).max()
    assert err <= S.DELTA / 2, err


@pytest.mark.parametrize("c", S.cases(), ids=lambda c: c.name)
def test_kept_set_is_transformers_support(c):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on the case's (processed) scores.  HF's top-p sorts, so where several
    tokens share the value of the last kept class it keeps an arbitrary part of them; the reference keeps equal values together.  The two
    sets are equal outside that one class, and equal altogether when the class holds one token."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = S.processed_scores(c, S.logits(c))
    sc = torch.from_numpy(x)[None].clone()
    ids = torch.zeros((1, 1), dtype=torch.long)
    if c.T != 1.0:
        sc = TemperatureLogitsWarper(float(c.T))(ids, sc)
    if c.k > 0:
        sc = TopKLogitsWarper(min(c.k, c.V))(ids, sc)
    if c.p < 1.0:
        sc = TopPLogitsWarper(float(c.p))(ids, sc)
    hf = torch.isfinite(sc[0]).numpy()
    r = S.reference(c, x)
    finite = np.isfinite(r.y)
    ours = r.kept & finite
    if c.p < 1.0 and r.boundary_multiplicity > 1:
        edge = r.y == r.y[ours].min()
        assert (hf & ~edge == ours & ~edge).all() and (hf & edge).sum() >= 1 and not (hf & ~ours).any()
    else:
        assert (hf == ours).all(), (hf.sum(), ours.sum())


def test_hf_support_is_exact_on_enough_cases():
    exact = [c for c in S.cases() if c.p < 1.0 and S.reference(c).boundary_multiplicity == 1]
    assert len(exact) >= 20, len(exact)


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_mutation_is_rejected(mutation):
    """A reference with the defect draws tokens the acceptance test refuses in at least half of the draws of at least one case."""
    worst = 0.0
    for c in S.cases():
        if c.k == 1:
            continue
        u = S.uniform(*S.draws(c))
        r = S.reference(c)
        rej = 1.0 - S.accepted(r, S.mutated_tokens(c, mutation), u).mean()
        worst = max(worst, rej)
        if worst >= 0.5:
            return
    raise AssertionError(f"{mutation}: rejected in at most {worst:.3f} of a case's draws")


def test_host_side_validation_of_the_c_entry(lib):
    """aki_sample_pick refuses bad sampling parameters and a misaligned scratch on the host: an error code, nothing launched."""
    from aki_amd import _lib as L
    assert "aki_sample_pick" in L.SIGNATURES and lib.aki_abi_version() == 17
    P = 4096                                               # a non-null, 16-byte aligned address; never dereferenced on these paths

    def call(T=1.0, k=0, p=1.0, scores=P, ld_scores=64, step=0, penalty=1.0):
        return lib.aki_sample_pick(P, 2, 64, 64, None, 0, 0, None, P, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, scores, ld_scores,
                                   penalty, 0, 0, None, 0, None, 0, None, None, 0, 0, step, T, k, p, 1, 0, None, 0, None)

    for bad in (dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(p=0.0), dict(p=1.5), dict(k=-1), dict(scores=None), dict(ld_scores=60),
                dict(step=-1), dict(penalty=0.0)):
        assert call(**bad) == -1, bad
    assert call(scores=P + 4) < 0 and call(ld_scores=66) < 0        # alignment

"""Per-request sampling in generate_many, the parts that need no GPU: the row table of tests/many_sampling_cases.py checked with the
reference alone (the cap on ambiguous draws, the two mutations of the seed rule), slots.request_seed against a restatement,
RequestParams validation and generate_many's request parsing."""
import types

import numpy as np
import pytest
import torch

import many_sampling_cases as M
import sampling_cases as S


def test_row_table_is_what_it_should_be():
    table = M.rows()
    assert [(c.sigma, c.T, c.k, c.p) for c, _ in table[:5]] == [(2.0, 0.7, 0, 1.0), (2.0, 1.0, 1, 1.0), (2.0, 1.3, 50, 0.9),
                                                                (4.0, 0.7, 1000, 0.5), (2.0, 1.0, 0, 0.9)]
    assert all(c.V == S.V_SMALL for c, _ in table) and S.V_SMALL % 8 == 3
    assert table[5][0] is table[0][0] and table[5][1] == table[0][1]
    seeds = [s for _, s in table[:5]]
    assert len(set(seeds)) == 5 and all(0 <= s < 1 << 64 for s in seeds)
    assert max(seeds) >= 1 << 63, "no seed uses the top bit: the int64 reinterpretation would not be exercised"
    T, k, p, seed = M.param_arrays(table)
    assert (T.dtype, k.dtype, p.dtype, seed.dtype) == (np.float32, np.int32, np.float32, np.int64)
    assert [int(s) & M.MASK64 for s in seed] == [s for _, s in table]


def test_the_share_of_ambiguous_draws_stays_under_the_cap():
    """The cap is a condition on the inputs: with it, `accepted` pins almost every device token to one id."""
    for r, (c, seed) in enumerate(M.rows()):
        ok, facts = S.conditions_hold(c)
        assert ok, (r, facts)
        u = M.draws(seed)
        assert u.shape == (M.STEPS,) and 0.0 < u.min() and u.max() < 1.0
        share = M.multi_share(c, u)
        print(f"row {r}: kept {int(M.reference(c).kept.sum())}, ambiguous share {share:.4f}, top-p gap {M.reference(c).boundary_gap:.3g}")
        assert share <= M.MULTI_CAP, (r, share)
        assert M.reference(c).boundary_gap > 8 * S.DELTA
    for r, (c, seed) in enumerate(M.main_rows()):
        share = M.multi_share(c, M.draws(seed, M.MAIN_STEPS))
        print(f"V_MAIN row {r}: kept {int(M.reference(c).kept.sum())}, ambiguous share {share:.4f}")
        assert share <= (M.MAIN_UNFILTERED_CAP if not c.filtered else M.MULTI_CAP), (r, share)


def test_the_draw_is_philox_with_the_rows_seed_and_no_row_index():
    for r, (c, seed) in enumerate(M.rows()):
        u = M.draws(seed)
        for n in (0, 1, 17, 255):
            x0 = S.philox4x32_10((n, 0, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
            assert u[n] == ((x0 >> 8) + 0.5) * 2.0 ** -24
    # it is the scalar sampler's draw for row 0, offset 0: what a batch-1 generate with DeviceGenerator(seed) draws first
    seed = M.rows()[2][1]
    assert np.array_equal(M.draws(seed), S.uniform(np.arange(M.STEPS), 0, 0, seed=seed))


@pytest.mark.parametrize("mutation", ["row_index_in_counter", "row_0_seed_for_every_row"])
def test_a_wrong_seed_rule_is_caught(mutation):
    """A sampler that keys the draw by the row index (the scalar kernel's counter), or uses one seed for all rows, draws other tokens:
    `accepted` rejects more than half of them on the rows 2, 4 and 5 (row 5: only the counter mutation - it shares row 0's seed)."""
    table = M.rows()
    checked = 0
    for r in (2, 4, 5):
        c, seed = table[r]
        if mutation == "row_0_seed_for_every_row" and seed == table[0][1]:
            continue
        ref = M.reference(c)
        wrong_u = M.draws(seed, row=r) if mutation == "row_index_in_counter" else M.draws(table[0][1])
        wrong_tok = S.reference_tokens(ref, wrong_u)
        right_u = M.draws(seed)
        assert S.accepted(ref, S.reference_tokens(ref, right_u), right_u).all()
        rejected = 1.0 - float(S.accepted(ref, wrong_tok, right_u).mean())
        assert rejected > 0.5, (mutation, r, rejected)
        checked += 1
    assert checked >= 2


def test_request_seed():
    from aki_amd.slots import philox4x32_10, request_seed
    for ctr, key, want in S.PHILOX_KAT:
        assert philox4x32_10(ctr, key) == want
    for seed, off, r in ((0, 0, 0), (S.SEED, 0, 3), (S.SEED, 1, 3), ((1 << 64) - 1, (1 << 40) + 5, 63), (5, 7, 1 << 20)):
        w = S.philox4x32_10((r, 0, off & 0xFFFFFFFF, off >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert request_seed(seed, off, r) == w[0] | (w[1] << 32)
        assert 0 <= request_seed(seed, off, r) < 1 << 64
    for off in (0, 1):
        assert len({request_seed(S.SEED, off, r) for r in range(64)}) == 64
    for r in range(64):
        a, b = request_seed(S.SEED, 0, r), request_seed(S.SEED, 1, r)
        assert a & 0xFFFFFFFF != b & 0xFFFFFFFF and a >> 32 != b >> 32
    assert {request_seed(S.SEED, 0, r) for r in range(64)}.isdisjoint(request_seed(S.SEED, 1, r) for r in range(64))


BAD_PARAMS = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5),
              dict(top_p=float("nan")), dict(top_k=-1), dict(logprobs=True, top_logprobs=-1), dict(logprobs=True, top_logprobs=9),
              dict(top_logprobs=2), dict(seed=-1), dict(seed=1 << 64)]


def _stub():
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: [7])


@pytest.mark.parametrize("bad", BAD_PARAMS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_request_params_are_validated_on_the_host_with_the_request_index(bad):
    import aki_amd
    from aki_amd import ops
    from aki_amd.aki import AKI, _many_requests, _parse_many_kwargs
    assert ops.LOGPROB_MAX_TOP == 8
    ids = torch.zeros((1, 3), dtype=torch.long)
    good = aki_amd.RequestParams(do_sample=True, temperature=0.7, top_k=8, top_p=0.9, seed=(1 << 64) - 1, logprobs=True, top_logprobs=8)
    assert _many_requests([(None, ids, 4, good)], 5)[0][3] is good
    rp = aki_amd.RequestParams(do_sample=True, **bad)
    with pytest.raises(ValueError, match="request 1"):
        _many_requests([(None, ids, 4, good), (None, ids, 4, rp)], 5)
    with pytest.raises(ValueError, match="request 1"):            # through the public entry, before the model is touched (the stub has none)
        AKI.generate_many(_stub(), [(None, ids), (None, ids, None, rp)], slots=2)
    with pytest.raises(ValueError, match="params"):               # the default is checked as well
        _parse_many_kwargs({"params": rp}, 0, lambda: [])


def test_request_parsing_and_the_new_keywords():
    import aki_amd
    from aki_amd.aki import AKI, _many_requests, _many_seeds, _parse_many_kwargs
    from aki_amd.slots import request_seed
    ids = torch.zeros((1, 3), dtype=torch.long)
    plain, samp = aki_amd.RequestParams(), aki_amd.RequestParams(do_sample=True, top_k=8)
    assert plain == aki_amd.RequestParams(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=None, logprobs=False, top_logprobs=0)
    own = aki_amd.RequestParams(do_sample=True, seed=77)
    reqs = _many_requests([(None, ids), (None, ids, 9), (None, ids, None, own), (None, ids, 2, None)], 5, samp)
    assert [r[2] for r in reqs] == [5, 9, 5, 2]                   # a 4-tuple with a None budget takes the default
    assert [r[3] for r in reqs] == [samp, samp, own, samp]        # params= supplies the default, None in the tuple as well
    assert [r[3] for r in _many_requests([(None, ids), (None, ids, 3)], 5)] == [plain, plain]
    with pytest.raises(ValueError, match="request 0"):
        _many_requests([(None, ids, 3, dict(do_sample=True))], 5)
    with pytest.raises(ValueError, match="request 0"):
        _many_requests([(None, ids, 3, samp, 1)], 5)
    # the keywords
    opt = _parse_many_kwargs({"params": samp, "generator": aki_amd.DeviceGenerator(3)}, 0, lambda: [])
    assert opt.params is samp and opt.generator.seed == 3
    assert _parse_many_kwargs({}, 0, lambda: []).params == plain and _parse_many_kwargs({}, 0, lambda: []).generator is None
    for bad in (torch.Generator(), 5):
        with pytest.raises(ValueError, match="generator"):
            _parse_many_kwargs({"generator": bad}, 0, lambda: [])
        with pytest.raises(ValueError, match="generator"):
            AKI.generate_many(_stub(), [(None, ids)], generator=bad)
    with pytest.raises(ValueError, match="params"):
        _parse_many_kwargs({"params": dict(do_sample=True)}, 0, lambda: [])
    # the refusals name RequestParams and keep the keyword
    for kw in ("do_sample", "output_logprobs"):
        with pytest.raises(NotImplementedError, match=kw) as e:
            _parse_many_kwargs({kw: True}, 0, lambda: [])
        assert "RequestParams" in str(e.value)
    # seeds: own seeds as they are, derived ones by position; the generator's offset is bumped once per call, sampled or not
    g = aki_amd.DeviceGenerator(S.SEED)
    assert _many_seeds(reqs, g) == [request_seed(S.SEED, 0, 0), request_seed(S.SEED, 0, 1), 77, request_seed(S.SEED, 0, 3)] and g.offset == 1
    assert _many_seeds(reqs, g)[3] == request_seed(S.SEED, 1, 3) and g.offset == 2
    assert _many_seeds(_many_requests([(None, ids)], 5), g) == [None] and g.offset == 3
    # without a generator: 64 bits from torch's CPU default generator - reproducible by torch.manual_seed, different from call to call
    torch.manual_seed(11)
    a, b = _many_seeds(reqs, None), _many_seeds(reqs, None)
    torch.manual_seed(11)
    assert _many_seeds(reqs, None) == a and a != b and a[2] == 77
    state = torch.get_rng_state()
    _many_seeds(_many_requests([(None, ids), (None, ids, 3, own)], 5), None)       # nothing to derive: torch's generator is left alone
    assert torch.equal(torch.get_rng_state(), state)
    # an empty queue still bumps the generator
    stub, g = _stub(), aki_amd.DeviceGenerator(1)
    assert AKI.generate_many(stub, [], slots=4, generator=g) == [] and g.offset == 1


def test_sample_pick_rows_is_declared_and_refuses_bad_arguments_on_the_host():
    """aki_sample_pick_rows: exported, and null arrays, B < 1 and a vocabulary above the limit are error codes with nothing launched."""
    import __graft_entry__ as ge
    ge.build()                                    # cross-compiles for gfx950 without a GPU
    from aki_amd import _lib as L, ops
    assert callable(ops.sample_pick_rows) and "aki_sample_pick_rows" in L.SIGNATURES
    lib = L.load()
    assert lib.aki_abi_version() == 17
    P = 4096                                      # a non-null, 16-byte aligned address; never dereferenced on these paths

    def call(B=2, V=64, T=P, k=P, p=P, seed=P, logits=P, ids=P, scores=P):
        return lib.aki_sample_pick_rows(logits, B, V, V, None, 0, 0, None, ids, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, scores, V,
                                        1.0, 0, 0, None, 0, None, 0, None, None, 0, 0, 0, T, k, p, seed, None, 0, None)

    bad = [call(T=None), call(k=None), call(p=None), call(seed=None), call(B=0), call(V=L.AKI_LOGITS_PROCESS_MAX_V + 4), call(logits=None),
           call(ids=None), call(scores=None)]
    assert all(rc == -1 for rc in bad), bad
    assert call(scores=P + 4) < 0                 # alignment

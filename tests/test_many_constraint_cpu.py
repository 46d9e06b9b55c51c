"""Per-request token constraints in generate_many, the parts that need no GPU: the layout of constraint.ConstraintPool, the refusals
generate_many raises on the host (each names its request, before any device call), and the numpy reference of
tests/many_constraint_cases.py against tests/constraint_cases.py."""
import types

import numpy as np
import pytest
import torch

import constraint_cases as CC
import many_constraint_cases as MC
from aki_amd.constraint import DEFAULT_MAX_TABLE_BYTES, MAX_STATES, ConstraintPool, TokenConstraint
from aki_amd.slots import RequestParams


# ---- the pool's layout --------------------------------------------------------------------------------------------------------------------
def test_pool_keeps_every_members_table_as_it_is():
    V = 64
    a, b, c = MC.members(V)
    pool = ConstraintPool(MC.EOS, [a, None, b, a, c, b], V)
    assert pool.members == [a, b, c], "identical objects are stored once, in the order of their first request"
    sizes = [a.n_states, b.n_states, c.n_states]
    assert pool.total_states == sum(sizes) and pool.nbytes == sum(sizes) * 64 * 2
    bases = [0, sizes[0], sizes[0] + sizes[1]]                  # cumulative
    assert pool.base == [bases[0], 0, bases[1], bases[0], bases[2], bases[1]]
    assert pool.n_states == [sizes[0], 0, sizes[1], sizes[0], sizes[2], sizes[1]]
    assert pool.start == [0, -1, 0, 0, 0, 0]
    table = pool.table()
    assert table.shape == (sum(sizes), V)
    for m, base in zip((a, b, c), bases):
        own = m.with_eos(MC.EOS)
        assert np.array_equal(table[base:base + m.n_states], own), "a member's slice is its with_eos table, not renumbered"
        assert int(own.max()) < m.n_states
    # an equal but distinct object is another member
    a2 = MC.members(V)[0]
    assert ConstraintPool(MC.EOS, [a, a2], V).total_states == 2 * a.n_states
    # no constrained request at all
    empty = ConstraintPool(MC.EOS, [None, None], V)
    assert not empty.constrained and empty.total_states == 0 and empty.nbytes == 0 and empty.start == [-1, -1]
    with pytest.raises(ValueError):
        empty.bind("cpu")


def test_pool_pads_the_row_stride_and_uploads_int16():
    V = 1003
    a, b, c = MC.members(V)
    pool = ConstraintPool(MC.EOS, [b, c], V)
    assert pool.ld == 1008 and pool.nbytes == (b.n_states + c.n_states) * 1008 * 2
    t = pool.bind("cpu")
    assert t.dtype == torch.int16 and tuple(t.shape) == (pool.total_states, 1008) and t.is_contiguous()
    assert np.array_equal(t[:, :V].numpy().astype(np.int32), pool.table()) and bool((t[:, V:] == -1).all())


def test_the_state_limit_holds_per_constraint_and_the_byte_cap_for_the_pool():
    V = 8
    # n states in a ring on token 1
    ring = lambda n: TokenConstraint.from_table(np.where(np.arange(V)[None, :] == 1, (np.arange(n)[:, None] + 1) % n, -1), np.zeros(n, bool), 0)
    big1, big2 = ring(20000), ring(20000)
    pool = ConstraintPool((), [big1, big2], V)                  # 40000 states: more than one int16 number space, no renumbering needed
    assert pool.total_states == 40000 and pool.base == [0, 20000] and int(pool.table().max()) == 19999
    assert MAX_STATES == 32767
    with pytest.raises(ValueError, match="32767"):
        ring(32768)                                             # a member cannot even be built
    grown = ring(4)                                             # ... and one that grew behind the constructor's back is refused by the pool
    grown.next_state, grown.accepting = np.zeros((32768, V), np.int32), np.zeros(32768, bool)
    with pytest.raises(ValueError, match=r"request 1.*32767"):
        ConstraintPool((), [None, grown], V)
    need = 40000 * 8 * 2
    with pytest.raises(ValueError, match=str(need)):
        ConstraintPool((), [big1, big2], V, max_table_bytes=need - 1)
    assert ConstraintPool((), [big1, big2], V, max_table_bytes=need).nbytes == need <= DEFAULT_MAX_TABLE_BYTES


def test_pool_refusals_name_the_first_request_that_uses_the_constraint():
    V = 64
    a, b, c = MC.members(V)
    two = TokenConstraint.from_table(np.zeros((2, V), np.int64), [True, True], [0, 1])
    edge = TokenConstraint.from_choices([[MC.EOS[0], 5]], V)    # an eos id used as a transition
    dead = TokenConstraint.from_choices([[5, 6]], V)            # its leaf accepts, but without an eos id nothing is allowed there
    for cons, eos, who, what in (([a, object()], MC.EOS, "request 1", "TokenConstraint"),
                                 ([None, a, two, two], MC.EOS, "request 2", "start states"),
                                 ([a, None, MC.members(V + 1)[1]], MC.EOS, "request 2", "built for V"),
                                 ([None, None, None, edge, edge], MC.EOS, "request 3", "ordinary transition"),
                                 ([b, dead], (), "request 1", "allows no token")):
        with pytest.raises(ValueError, match=f"{who}.*{what}"):
            ConstraintPool(eos, cons, V)


# ---- RequestParams and generate_many's host refusals -------------------------------------------------------------------------------------
def test_request_params_check_the_constraint():
    V = 64
    a = MC.members(V)[0]
    assert RequestParams().constraint is None
    assert RequestParams(constraint=a).check(3, 5).constraint is a
    with pytest.raises(ValueError, match="request 3.*TokenConstraint"):
        RequestParams(constraint="abc").check(3, 5)
    two = TokenConstraint.from_table(np.zeros((2, V), np.int64), [True, True], [0, 1])
    with pytest.raises(ValueError, match="request 4.*2 start states"):
        RequestParams(constraint=two).check(4, 5)


V_STUB = 64


def _stub(dtype=torch.bfloat16):
    """Just enough of a model for generate_many's host half; anything that would be device work raises."""
    def boom(*a, **kw):
        raise AssertionError("device work before the refusal")

    lm = types.SimpleNamespace(get_output_embeddings=lambda: types.SimpleNamespace(out_features=V_STUB),
                               get_input_embeddings=lambda: types.SimpleNamespace(weight=torch.zeros(1, dtype=dtype)),
                               decode_step=boom, config=None, model=None)
    return types.SimpleNamespace(pad_token_id=0, default_eos_token_ids=lambda: list(MC.EOS), lang_model=lm, _prefill_request=boom,
                                 _generate_one=boom, generate=boom, media_token_id=63, num_tokens_per_vis=4)


def _requests(params):
    ids = torch.tensor([[1, 5, 6]], dtype=torch.long)
    return [(None, ids, 4, p) for p in params]


@pytest.mark.parametrize("slots", [3, 1])
def test_generate_many_refuses_on_the_host_and_names_the_request(slots):
    from aki_amd.aki import AKI
    a, b, c = MC.members(V_STUB)
    plain = RequestParams()
    two = TokenConstraint.from_table(np.zeros((2, V_STUB), np.int64), [True, True], [0, 1])
    edge = TokenConstraint.from_choices([[MC.EOS[0], 5]], V_STUB)
    dead = TokenConstraint.from_choices([[5, 6]], V_STUB)
    wide = MC.members(V_STUB + 8)[0]
    cases = [([plain, RequestParams(constraint=5)], {}, "request 1.*TokenConstraint"),
             ([plain, plain, RequestParams(constraint=two)], {}, "request 2.*start states"),
             ([RequestParams(constraint=a), RequestParams(constraint=wide)], {}, "request 1.*built for V = 72"),
             ([plain, RequestParams(constraint=edge)], {}, "request 1.*ordinary transition"),
             ([RequestParams(constraint=b), plain, RequestParams(constraint=dead)], dict(eos_token_id=[]), "request 2.*allows no token")]
    for banning in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[7]]), dict(min_length=2), dict(min_new_tokens=2),
                    dict(suppress_tokens=[9]), dict(begin_suppress_tokens=[9])):
        cases.append(([plain, RequestParams(constraint=a)], banning, f"request 1.*{next(iter(banning))}"))
    for params, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            AKI.generate_many(_stub(), _requests(params), slots=slots, **kw)
    # CPU tensors (or an f32 model) have no device pick: refused as a sampled request is
    with pytest.raises(ValueError, match="request 1.*bf16"):
        AKI.generate_many(_stub(), _requests([plain, RequestParams(constraint=a)]), slots=slots)
    with pytest.raises(ValueError, match="request 0.*bf16"):
        AKI.generate_many(_stub(torch.float32), _requests([RequestParams(constraint=a), plain]), slots=slots)
    # the call-wide keyword stays refused, and says where a constraint goes
    with pytest.raises(NotImplementedError, match="constraint.*RequestParams"):
        AKI.generate_many(_stub(), _requests([plain]), slots=slots, constraint=a)


def test_new_entry_points_validate_on_the_host():
    """Exported, and null arrays or an empty pool are error codes with nothing launched."""
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib as L, ops
    lib = L.load()
    assert "aki_greedy_pick_constrained_rows" in L.SIGNATURES and "aki_sample_pick_rows_constrained" in L.SIGNATURES
    assert callable(ops.SlotConstraints) and lib.aki_abi_version() == 17
    buf = np.zeros(4096, dtype=np.int64)
    P = buf.ctypes.data

    def greedy(table=P, n_states=4, states=P, row_base=P, row_states=P, table_ld=64, states_ld=2):
        return lib.aki_greedy_pick_constrained_rows(P, 2, 64, 64, None, 0, 0, None, P, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, P, 64,
                                                    1.0, 0, 0, None, 0, None, 0, None, None, 0, 0, table, table_ld, n_states, states, states_ld,
                                                    row_base, row_states, None)

    def sample(table=P, n_states=4, states=P, row_base=P, row_states=P):
        return lib.aki_sample_pick_rows_constrained(P, 2, 64, 64, None, 0, 0, None, P, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, P, 64,
                                                    1.0, 0, 0, None, 0, None, 0, None, None, 0, 0, 0, P, P, P, P, None, 0, table, 64, n_states,
                                                    states, 2, row_base, row_states, None)

    for fn in (greedy, sample):
        for bad in (dict(table=None), dict(states=None), dict(row_base=None), dict(row_states=None), dict(n_states=0)):
            assert fn(**bad) == -1, (fn.__name__, bad)
    assert greedy(table_ld=63) == -1 and greedy(states_ld=0) == -1


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_the_pool_reference_agrees_with_the_single_table_reference(case):
    """constraint_cases.greedy on its own cases, against the pool reference with the case's table placed behind another one."""
    c = TokenConstraint.from_choices(case.choices, case.V)
    table = c.with_eos(case.eos)
    front = MC.cycle(case.V, 3, 10, 2).with_eos(())
    pool = np.concatenate([front, table], axis=0)
    base, n = front.shape[0], table.shape[0]
    rng = np.random.Generator(np.random.PCG64(case.V))
    for trial in range(4):
        scores = rng.standard_normal((7, case.V)).astype(np.float32)
        scores[:, ::5] = np.round(scores[:, ::5])               # ties: the lowest id wins in both
        want = CC.greedy(table, 0, scores, case.eos, MC.PAD)
        assert MC.greedy(pool, base, n, 0, scores, case.eos, MC.PAD) == want, trial
        assert MC.walk(pool, base, n, 0, want[0][:3]) == CC.walk(table, 0, want[0][:3])
    for s in range(n):
        assert np.array_equal(MC.mask(pool, base, n, s), CC.mask(table, s))
    # outside the row's table: untouched, next state -1 - even where the pool has a row at that place
    assert MC.mask(pool, 0, 3, 3) is None and MC.mask(pool, base, n, n) is None and MC.mask(pool, base, n, -1) is None
    x = rng.standard_normal(case.V)
    assert MC.pick(pool, 0, 3, 3, x) == (int(np.argmax(x)), -1) and MC.pick(pool, base, n, 0, x, done=True) == (MC.PAD, 0)


def test_the_row_table_puts_the_free_argmax_outside_every_allowed_set():
    for V in (8, 1000, 32067):
        tables = [m.with_eos(MC.EOS) for m in MC.members(V)]
        pool, placed = MC.place(tables)
        x = MC.row_scores(V, pool, placed)
        kinds = [mem for mem, *_ in MC.ROWS]
        assert kinds.count(0) == 3 and kinds.count(1) == 1 and kinds.count(2) == 1 and kinds.count(None) == 1
        assert MC.ROWS[0][1] != MC.ROWS[1][1] and sum(done for *_, done in MC.ROWS) == 1
        for b, ((mem, s, t, done), (base, n)) in enumerate(zip(MC.ROWS, placed)):
            m = MC.mask(pool, base, n, s)
            assert t + 1 < MC.HISTORY
            if mem is None:
                assert m is None
            else:
                assert m.any() and not m[int(np.argmax(x[b]))], (V, b)


def test_the_request_pattern_hands_a_slot_from_a_constrained_request_to_a_free_one_and_back():
    served = MC.slot_history()
    assert sorted(r for s in served for r in s) == list(range(7))
    kinds = [[MC.PATTERN[r] is not None for r in s] for s in served]
    assert any(any(k[i] and not k[i + 1] and k[i + 2] for i in range(len(k) - 2)) for k in kinds), (served, kinds)
    cons = MC.request_constraints(32064)
    assert cons[0] is cons[4] and cons[1] is cons[6] and cons[3] is None and cons[5] is None
    pool = ConstraintPool((), cons, 32064)
    assert len(pool.members) == 3 and pool.total_states == 4 + 3 + 5
    for ch, c in zip(MC.CHOICES, MC.choice_constraints(32064)):
        assert len(c.starts) == 1 and all(len(x) + 1 < MC.CHOICE_BUDGET for x in ch)

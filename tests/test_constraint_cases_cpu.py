"""Constrained decoding on the host (aki_amd/constraint.py, the `constraint` keyword of _parse_generate_kwargs) and the reference of
tests/constraint_cases.py against the installed transformers.  No GPU."""
import numpy as np
import pytest
import torch

import constraint_cases as CC
from aki_amd.constraint import MAX_STATES, TokenConstraint


def test_importable_from_the_package_without_the_library():
    import aki_amd
    assert aki_amd.TokenConstraint is TokenConstraint


def test_trie_shape_and_acceptance():
    c = TokenConstraint.from_choices([[5, 6, 7], [5, 6, 8], [9]], 16)
    # states: 0 -5-> 1 -6-> 2 -7-> 3, 2 -8-> 4, 0 -9-> 5
    assert c.n_states == 6 and c.V == 16 and c.starts == [0]
    assert c.next_state[0, 5] == 1 and c.next_state[1, 6] == 2 and c.next_state[2, 7] == 3 and c.next_state[2, 8] == 4 and c.next_state[0, 9] == 5
    assert int((c.next_state >= 0).sum()) == 5
    assert c.accepting.tolist() == [False, False, False, True, True, True]


def test_a_choice_may_be_a_prefix_of_another_and_equal_choices_collapse():
    c = TokenConstraint.from_choices([[5, 6], [5, 6, 7], [5, 6]], 16)
    assert c.n_states == 4 and c.accepting.tolist() == [False, False, True, True]
    t = c.with_eos([2])
    assert sorted(np.flatnonzero(t[2] >= 0).tolist()) == [2, 7]        # in the prefix's end: stop, or go on to the longer choice
    assert np.flatnonzero(t[3] >= 0).tolist() == [2] and t[3, 2] == 3 and t[2, 2] == 2
    assert (t[0] >= 0).sum() == 1 and t[0, 2] == -1


def test_from_table_and_union_offsets():
    a = TokenConstraint.from_choices([[1], [2, 3]], 8)            # 4 states
    b = TokenConstraint.from_choices([[4, 4]], 8)                 # 3 states
    nxt = np.full((2, 8), -1)
    nxt[0, 7], nxt[1, 7] = 1, 1
    c = TokenConstraint.from_table(nxt, [False, True], start=0)   # 7+
    u = TokenConstraint.union([a, b, c])
    assert u.n_states == 9 and u.starts == [0, 4, 7] and u.V == 8
    assert np.array_equal(u.next_state[:4], a.next_state)
    assert np.array_equal(u.next_state[4:7], np.where(b.next_state >= 0, b.next_state + 4, -1))
    assert np.array_equal(u.next_state[7:], np.where(c.next_state >= 0, c.next_state + 7, -1))
    assert u.accepting.tolist() == a.accepting.tolist() + b.accepting.tolist() + [False, True]
    t = u.with_eos([0])
    assert CC.legal(t, 4, [4, 4, 0, 0]) and not CC.legal(t, 4, [1]) and CC.legal(t, 0, [2, 3, 0]) and CC.legal(t, 7, [7, 7, 7, 0])
    with pytest.raises(ValueError):
        TokenConstraint.union([a, TokenConstraint.from_choices([[1]], 9)])
    with pytest.raises(ValueError):
        TokenConstraint.union([])


def test_bind_eos_columns_and_device_table():
    c = TokenConstraint.from_choices([[5], [6, 7]], 13)
    b = c.bind([2, 3], "cpu", rows_start=[0, 0, 0])
    assert b.table.dtype == torch.int16 and b.table.is_contiguous() and b.table.shape == (4, 16) and b.V == 13 and b.n_states == 4
    assert b.table.stride(0) * 2 % 16 == 0                         # every row 16-byte aligned
    assert b.row_start.dtype == torch.int32 and b.row_start.tolist() == [0, 0, 0] and b.rows == 3
    t = b.table[:, :13].numpy()
    assert np.array_equal(t, c.with_eos([2, 3])) and (b.table[:, 13:] == -1).all()
    for s in range(4):
        for e in (2, 3):
            assert t[s, e] == (s if c.accepting[s] else -1)
    assert c.bind([2], "cpu").row_start.tolist() == [0]


@pytest.mark.parametrize("bad", [[], None, [[]], [[1], []], [3], [[1, 99]], [[-1]]])
def test_from_choices_refuses(bad):
    with pytest.raises(ValueError):
        TokenConstraint.from_choices(bad, 16)


def test_value_errors_of_tables_and_bind():
    c = TokenConstraint.from_choices([[5], [6, 7]], 16)
    with pytest.raises(ValueError, match="ordinary transition"):
        c.with_eos([5])                                            # eos used as an edge
    with pytest.raises(ValueError, match="ordinary transition"):
        c.bind([7], "cpu")
    with pytest.raises(ValueError, match="allows no token"):
        c.bind([], "cpu")                                          # an accepting leaf and no eos id: a dead end
    nxt = np.full((3, 8), -1)
    nxt[0, 1], nxt[0, 2] = 1, 2                                    # state 2: not accepting, no edge
    dead = TokenConstraint.from_table(nxt, [False, True, False])
    with pytest.raises(ValueError, match="state 2"):
        dead.bind([0], "cpu")
    nxt[0, 2] = -1                                                 # ... and fine once it cannot be reached
    assert TokenConstraint.from_table(nxt, [False, True, False]).bind([0], "cpu").n_states == 3
    with pytest.raises(ValueError, match="max_table_bytes"):
        c.bind([2], "cpu", max_table_bytes=c.n_states * 16 * 2 - 1)
    assert c.bind([2], "cpu", max_table_bytes=c.n_states * 16 * 2).n_states == c.n_states
    with pytest.raises(ValueError):
        c.bind([16], "cpu")                                        # eos outside [0, V)
    with pytest.raises(ValueError):
        c.bind([2], "cpu", rows_start=[4])
    with pytest.raises(ValueError):
        TokenConstraint.from_table(np.full((MAX_STATES + 1, 1), 0), np.ones(MAX_STATES + 1, bool))
    with pytest.raises(ValueError):
        TokenConstraint.from_table(np.full((2, 4), 2), [True, True])            # a transition to a state that does not exist
    with pytest.raises(ValueError):
        TokenConstraint.from_table(np.full((2, 4), -1), [True])
    with pytest.raises(ValueError):
        TokenConstraint.from_table(np.full((2, 4), -1), [True, True], start=2)


def test_v_mismatch_is_refused_by_the_processors():
    from aki_amd import ops
    b = TokenConstraint.from_choices([[5]], 16).bind([2], "cpu")
    with pytest.raises(ValueError, match="built for V = 16"):
        ops.LogitsProcessors(17, "cpu", constraint=b)
    p = ops.LogitsProcessors(16, "cpu", constraint=b)
    assert p.active
    assert not ops.LogitsProcessors(16, "cpu").active and not ops.LogitsProcessors(16, "cpu", 1.0, 0, 0, (2,), [], [], []).active
    st = p.states(1, 4)
    assert st.shape == (1, 5) and st.dtype == torch.int32 and st[0].tolist() == [0, -1, -1, -1, -1] and p.states(1) is st
    with pytest.raises(ValueError):
        ops.LogitsProcessors(16, "cpu", constraint=b).states(2, 4)


@pytest.mark.parametrize("c", CC.CASES, ids=lambda c: c.name)
def test_reference_mask_equals_transformers_prefix_constrained(c):
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    tc = TokenConstraint.from_choices(c.choices, c.V)
    table = tc.with_eos(c.eos)
    hf = PrefixConstrainedLogitsProcessor(CC.allowed_fn(table, 0), 1)
    g = torch.Generator().manual_seed(len(c.name))
    hs = CC.histories(c, table, 0)
    assert [len(h) for h in hs] == [0, 1, 3]
    for h in hs:
        scores = torch.randn((1, c.V), generator=g)
        want = hf(torch.tensor([h], dtype=torch.long), scores.clone())[0]
        s = CC.walk(table, 0, h)[-1]
        assert s >= 0
        got = torch.where(torch.from_numpy(CC.mask(table, s)), scores[0], torch.full_like(scores[0], float("-inf")))
        assert torch.equal(got, want), (c.name, h)
        assert int(torch.isfinite(got).sum()) >= 1


def test_reference_greedy_walks_the_automaton():
    c = CC.CASES[1]
    table = TokenConstraint.from_choices(c.choices, c.V).with_eos(c.eos)
    sc = np.zeros((6, c.V), np.float32)
    sc[:, 40] = 9.0                                                # the free argmax is never allowed
    sc[0, 9], sc[0, 5] = 1.0, 2.0
    sc[2, 2], sc[2, 7] = 1.0, 3.0                                  # behind (5, 6): go on to 7 rather than stop
    toks, states, done_at = CC.greedy(table, 0, sc, c.eos, pad=0)
    assert toks == [5, 6, 7, 2, 0, 0] and done_at == 3 and states[:5] == CC.walk(table, 0, toks[:4]) and states[5:] == [states[4]] * 2
    assert CC.legal(table, 0, toks[:4])


def _parse(**kw):
    from aki_amd.aki import _parse_generate_kwargs
    return _parse_generate_kwargs(dict(kw), 0, lambda: [2], False, batch=3)


def test_parse_generate_kwargs_refusals():
    c = TokenConstraint.from_choices([[5], [6, 7]], 32)
    assert _parse(constraint=c).constraint is c and _parse().constraint is None
    assert len(_parse(constraint=[c, c, c], repetition_penalty=1.3).constraint) == 3
    with pytest.raises(NotImplementedError):
        _parse(constraint=c, num_beams=2)
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4]]), dict(min_length=2), dict(min_new_tokens=2), dict(suppress_tokens=[4]),
               dict(begin_suppress_tokens=[4])):
        with pytest.raises(ValueError, match="constraint together with"):
            _parse(constraint=c, **kw)
    assert _parse(constraint=c, no_repeat_ngram_size=0, bad_words_ids=[], min_new_tokens=0, suppress_tokens=None).constraint is c
    with pytest.raises(ValueError, match="batch of 3"):
        _parse(constraint=[c, c])
    with pytest.raises(ValueError):
        _parse(constraint=[c, "x", c])
    with pytest.raises(ValueError):
        _parse(constraint="(A)")
    with pytest.raises(ValueError, match="prefix_allowed_tokens_fn"):
        _parse(prefix_allowed_tokens_fn=lambda b, ids: [1])


def test_constrained_entry_points_validate_on_the_host():
    """Null pointers, n_states and states_ld are refused with an error code before anything is launched."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from aki_amd import _lib as L
    lib = L.load()
    for name in ("aki_logits_process_constrained", "aki_greedy_pick_constrained", "aki_sample_pick_constrained"):
        assert name in L.SIGNATURES
    P = C.c_void_p(4096)                                           # never dereferenced on the host

    def process(table=P, table_ld=64, n_states=3, states=P, states_ld=5):
        return lib.aki_logits_process_constrained(P, L.AKI_DT_BF16, 2, 64, 64, P, 64, None, 0, None, None, 0, None, 1.0, 0, 0, None, 0, None, 0,
                                                  None, 0, None, None, 0, 0, table, table_ld, n_states, states, states_ld, None)

    def greedy(table=P, table_ld=64, n_states=3, states=P, states_ld=5):
        return lib.aki_greedy_pick_constrained(P, 2, 64, 64, None, 0, 0, None, P, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, P, 64,
                                               1.0, 0, 0, None, 0, None, 0, None, None, 0, 0, table, table_ld, n_states, states, states_ld, None)

    def sample(table=P, table_ld=64, n_states=3, states=P, states_ld=5):
        return lib.aki_sample_pick_constrained(P, 2, 64, 64, None, 0, 0, None, P, None, 0, None, None, 0, None, None, None, 0, 0, 0, None, P, 64,
                                               1.0, 0, 0, None, 0, None, 0, None, None, 0, 0, 0, 1.0, 0, 1.0, 1, 0, None, 0, table, table_ld,
                                               n_states, states, states_ld, None)

    for call in (process, greedy, sample):
        for kw in (dict(table=None), dict(states=None), dict(n_states=0), dict(n_states=32768), dict(states_ld=0), dict(table_ld=63)):
            assert call(**kw) == -1, (call.__name__, kw)
